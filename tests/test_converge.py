"""Converged rendering on the GPU (pt_render_converge, csrc/device/pt_converge.h).

The acceptance criterion is exact: an entry that stops after n samples holds,
bit for bit, what pt_render(spp = n) returns for its pixel, and which entries
stop where -- with what error estimate -- is what the numpy model of the rule
(tests/converge_model.py) gives on the same block sums.  The block sums come
from the CPU oracle's per-sample values (case A) or from the existing
pt_render(sample_begin = 32 b, spp = 32, sum_only) (cases B, F).
"""
import numpy as np
import pytest

import converge_model as M
import pathtrace as pt
from pathtrace import scenes
from pathtrace.scene import to_text
from test_zero_child import SKIES, sky_scene

pytestmark = pytest.mark.gpu

W, H, DEPTH = 24, 16, 8
MIN, CAP, REL = 64, 256, 0.05


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(a, b, nan_ok=False):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape
    same = bits(a) == bits(b)
    if nan_ok:  # a NaN's sign and payload are the adder's, not the renderer's
        same |= np.isnan(a) & np.isnan(b)
    assert same.all(), "%d of %d values differ" % (int((~same).sum()), same.size)


def info_counts(info):
    return {k: info[k] for k in ("rounds", "samples", "capped")}


def gpu_blocks(ds, w, h, depth, cap):
    """[w * h, cap / 32, 3]: every pixel's 32-sample block sums, from the existing pt_render"""
    return np.stack([pt.render(ds, w, h, 32, depth, sample_begin=32 * b, sum_only=True).reshape(-1, 3)
                     for b in range(cap // 32)], axis=1)


def assert_groups_match_render(ds, w, h, depth, rgb, spp, nan_ok=False):
    """for every distinct stop count n, pt_render(pixels = that group, spp = n) is the group's rgb"""
    for n in np.unique(spp):
        group = np.flatnonzero(spp == n).astype(np.int32)
        assert_same_bits(pt.render(ds, w, h, int(n), depth, pixels=group), rgb[group], nan_ok)


@pytest.fixture(scope="module")
def p1(built):
    return pt.DeviceScene(scenes.scene_p1())


@pytest.fixture(scope="module")
def oracle_blocks(built, tmp_path_factory):
    """case A's block sums from the CPU oracle's per-sample values (24 x 16 x 256 samples)"""
    import oracle_py as O
    text = to_text(scenes.scene_p1(), str(tmp_path_factory.mktemp("converge_img")))
    vals = O.render(text, W, H, CAP, DEPTH, order=O.ORDER_FAST, per_sample=True)
    assert vals.shape == (W * H, CAP, 3)
    blocks = M.tree32(vals)
    blocks.setflags(write=False)
    return blocks


@pytest.fixture(scope="module")
def case_a(p1):
    rgb, spp, err, info = pt.render_converged(p1, W, H, CAP, DEPTH, min_spp=MIN, rel_tol=REL, abs_tol=0.0)
    out = (rgb.reshape(-1, 3), spp.reshape(-1), err.reshape(-1), info)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def test_a_against_the_oracle(case_a, oracle_blocks):
    rgb, spp, err, info = case_a
    m_rgb, m_spp, m_err, m_info = M.converge(oracle_blocks, MIN, CAP, REL, 0.0)
    groups = {n: int((m_spp == n).sum()) for n in (64, 128, 256)}
    print("stop groups", groups, "gpu", info_counts(info), "model", m_info)
    assert all(groups.values()) and sum(groups.values()) == W * H, groups
    np.testing.assert_array_equal(spp, m_spp)
    assert_same_bits(err, m_err)
    assert_same_bits(rgb, m_rgb)
    assert info_counts(info) == m_info
    assert info["launches"] == 3 and info["kernel_ms"] > 0 and info["reduce_ms"] > 0


def test_b_against_pt_render_across_many_workgroups(p1):
    w, h, cap, rel = 96, 64, 512, 0.01
    rgb, spp, err, info = pt.render_converged(p1, w, h, cap, DEPTH, min_spp=64, rel_tol=rel)
    rgb, spp, err = rgb.reshape(-1, 3), spp.reshape(-1), err.reshape(-1)
    groups = {n: int((spp == n).sum()) for n in (64, 128, 256, 512)}
    print("stop groups", groups, info_counts(info))
    assert all(groups.values()) and sum(groups.values()) == w * h, groups
    assert (spp > 64).sum() >= 256
    assert_groups_match_render(p1, w, h, DEPTH, rgb, spp)
    m_rgb, m_spp, m_err, m_info = M.converge(gpu_blocks(p1, w, h, DEPTH, cap), 64, cap, rel, 0.0)
    np.testing.assert_array_equal(spp, m_spp)
    assert_same_bits(err, m_err)
    assert info_counts(info) == m_info


def test_c_pass_splitting(p1, case_a):
    """a staging budget of one byte forces passes of 64 samples: round 2 (128 samples) takes two"""
    rgb, spp, err, info = pt.render_converged(p1, W, H, CAP, DEPTH, min_spp=MIN, rel_tol=REL, max_buffer_bytes=1)
    assert_same_bits(rgb.reshape(-1, 3), case_a[0])
    np.testing.assert_array_equal(spp.reshape(-1), case_a[1])
    assert_same_bits(err.reshape(-1), case_a[2])
    assert info_counts(info) == info_counts(case_a[3])
    assert info["launches"] == case_a[3]["launches"] + 1


def test_d_no_early_stop_is_pt_render(p1):
    rgb, spp, err, info = pt.render_converged(p1, W, H, 128, DEPTH, min_spp=128, rel_tol=REL)
    assert_same_bits(rgb, pt.render(p1, W, H, 128, DEPTH))
    assert (spp == 128).all()
    assert info["rounds"] == 1 and info["samples"] == W * H * 128


@pytest.mark.parametrize("pixels", [
    [200, 5, 383, 5, 17, 100, 5],                     # unsorted, one pixel three times
    [123],
    [int(v) for v in (np.arange(65) * 7 + 3) % (W * H)],  # one entry past a wave
], ids=["duplicates", "one", "sixty-five"])
def test_e_pixel_lists(p1, case_a, pixels):
    rgb, spp, err, info = pt.render_converged(p1, W, H, CAP, DEPTH, min_spp=MIN, rel_tol=REL, pixels=pixels)
    assert rgb.shape == (len(pixels), 3) and spp.shape == err.shape == (len(pixels),)
    assert_same_bits(rgb, case_a[0][pixels])
    np.testing.assert_array_equal(spp, case_a[1][pixels])
    assert_same_bits(err, case_a[2][pixels])
    assert info["samples"] == int(spp.sum())
    first = {}
    for k, px in enumerate(pixels):  # duplicates give identical results
        j = first.setdefault(px, k)
        assert bits(rgb[k]).tolist() == bits(rgb[j]).tolist() and spp[k] == spp[j]


def test_f_non_finite_pixels(built):
    w, h, depth, cap = 40, 24, 5, 128
    ds = pt.DeviceScene(sky_scene(SKIES["inf"]()))
    rgb, spp, err, info = pt.render_converged(ds, w, h, cap, depth, min_spp=64, rel_tol=REL)
    rgb, spp, err = rgb.reshape(-1, 3), spp.reshape(-1), err.reshape(-1)
    blocks = gpu_blocks(ds, w, h, depth, cap)
    with np.errstate(all="ignore"):
        y = ((blocks[:, :2, 0] + blocks[:, :2, 1]) + blocks[:, :2, 2]).astype(np.float64)
        bad = ~np.isfinite(y.sum(axis=1)) | ~np.isfinite((y * y).sum(axis=1))
    print("non-finite entries", int(bad.sum()), "of", w * h, info_counts(info))
    assert bad.any()  # inside an infinite sky every pixel sees it: all of them, on this frame
    assert (spp[bad] == 64).all() and np.isnan(err[bad]).all()
    assert not np.isnan(err[~bad & (spp == 64)]).any()
    m_rgb, m_spp, m_err, m_info = M.converge(blocks, 64, cap, REL, 0.0)
    np.testing.assert_array_equal(spp, m_spp)
    assert_same_bits(err, m_err, nan_ok=True)
    assert info_counts(info) == m_info
    assert_groups_match_render(ds, w, h, depth, rgb, spp, nan_ok=True)


def test_g_extremes(p1, case_a, oracle_blocks):
    rgb, spp, err, info = pt.render_converged(p1, W, H, CAP, DEPTH, min_spp=MIN, rel_tol=1e30)
    assert (spp == 64).all()
    assert info["samples"] == W * H * 64 and info["rounds"] == 1 and info["capped"] == 0
    assert_same_bits(rgb, pt.render(p1, W, H, 64, DEPTH))
    # no tolerance at all: only zero-variance entries stop early, every other one is capped
    rgb, spp, err, info = pt.render_converged(p1, W, H, CAP, DEPTH, min_spp=MIN, rel_tol=0.0, abs_tol=0.0)
    rgb, spp, err = rgb.reshape(-1, 3), spp.reshape(-1), err.reshape(-1)
    m_rgb, m_spp, m_err, m_info = M.converge(oracle_blocks, MIN, CAP, 0.0, 0.0)
    np.testing.assert_array_equal(spp, m_spp)
    assert_same_bits(err, m_err)
    assert_same_bits(rgb, m_rgb)
    assert info_counts(info) == m_info
    assert (err[spp < CAP] == 0).all()
    assert info["capped"] == int((err > 0).sum()) > 0 and (spp[err > 0] == CAP).all()
