"""Converged rendering without a GPU: pt_render_converge checks every argument
before it touches a device (a late check would surface as PT_ERR_DEVICE here),
its scene-independent module compiles for gfx950 into the code-object cache,
and the numpy model of the stopping rule (tests/converge_model.py) behaves as
include/pt/pt.h states on synthetic block sums."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import converge_model as M
import pathtrace as pt
import zoo
from pathtrace import _lib

PT_ERR_ARG = -1


def call(cp_kw=None, null=(), **kw):
    """pt_render_converge on scene_p1 with one bad argument; returns (status, pt_last_error())"""
    L = _lib.lib()
    ds = pt.DeviceScene(zoo.build("scene_p1"))
    args = dict(width=8, height=4, spp=128, depth=8)
    args.update(kw)
    p, keep = pt.make_params(args.pop("width"), args.pop("height"), args.pop("spp"), args.pop("depth"), **args)
    cp = _lib.ConvergeParams()
    cp.min_spp, cp.rel_tol, cp.abs_tol = 64, 0.05, 0.0
    for k, v in (cp_kw or {}).items():
        setattr(cp, k, v)
    n = len(keep) if keep is not None else p.width * p.height
    rgb = np.zeros((max(n, 1), 3), dtype=np.float32)
    spp = np.zeros(max(n, 1), dtype=np.int32)
    err = np.zeros(max(n, 1), dtype=np.float32)
    rc = L.pt_render_converge(ds.handle, None if "p" in null else ctypes.byref(p),
                              None if "cp" in null else ctypes.byref(cp),
                              None if "rgb_out" in null else rgb.ctypes.data, spp.ctypes.data, err.ctypes.data, None)
    return rc, L.pt_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(null=("p",)), "p is null"),
    (dict(null=("cp",)), "cp is null"),
    (dict(null=("rgb_out",)), "rgb_out"),
    (dict(spp=100), "p->spp"),                               # the cap is no multiple of 32
    (dict(order="reference"), "p->order"),
    (dict(sample_begin=32), "p->sample_begin"),
    (dict(sum_only=True), "p->sum_only"),
    (dict(cp_kw=dict(min_spp=32)), "cp->min_spp"),           # below 64
    (dict(cp_kw=dict(min_spp=80)), "cp->min_spp"),           # no multiple of 32
    (dict(cp_kw=dict(min_spp=256)), "cp->min_spp"),          # above the cap
    (dict(cp_kw=dict(rel_tol=-1.0)), "cp->rel_tol"),
    (dict(cp_kw=dict(rel_tol=float("nan"))), "cp->rel_tol"),
    (dict(cp_kw=dict(abs_tol=-0.5)), "cp->abs_tol"),
    (dict(cp_kw=dict(abs_tol=float("nan"))), "cp->abs_tol"),
    (dict(pixels=[0, 32]), "out of range"),                  # 8 x 4 frame: pt_render's own check
    (dict(grid_width=4), "grid_width"),
    (dict(depth=65), "depth"),
])
def test_arguments_are_checked_before_the_device(built, kw, name):
    rc, msg = call(**kw)
    assert rc == PT_ERR_ARG, (rc, msg)
    assert name in msg, msg


def test_good_arguments_reach_the_device(built):
    """the control of the test above: with nothing wrong the call gets past its checks (and, on a
    machine without a GPU, fails at the device)"""
    rc, msg = call()
    assert rc != PT_ERR_ARG, msg


def test_empty_list_touches_no_device(built):
    rc, msg = call(pixels=[])
    assert rc == 0, msg


def test_module_compiles_without_a_device(built, tmp_path):
    """pt_converge_compile in a fresh process with an empty cache and no visible device: one code
    object appears, beside the text it was compiled from -- pt_converge.h itself.  (This process
    may hold the module in memory already, so it cannot show the compile.)"""
    assert _lib.lib().pt_converge_compile() == 0, _lib.lib().pt_last_error()
    env = dict(os.environ, PT_JIT_CACHE=str(tmp_path), HIP_VISIBLE_DEVICES="")
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); rc = L.pt_converge_compile(); "
            "L.pt_last_error.restype = ctypes.c_char_p; print(L.pt_last_error()); sys.exit(0 if rc == 0 else 1)")
    r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    objs = [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]
    assert len(objs) == 1 and os.path.getsize(tmp_path / objs[0]) > 1000, os.listdir(tmp_path)
    header = open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), "csrc", "device",
                               "pt_converge.h")).read()
    assert open(tmp_path / (objs[0][:-6] + ".hip")).read() == header
    for kernel in ("pt_converge_reduce", "pt_converge_scan", "pt_converge_scatter"):
        assert kernel in header


def test_existing_device_headers_are_not_part_of_the_module(built):
    """the module is pt_converge.h alone, so no scene module's text -- and key -- depends on it"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "path-trace_amd", "csrc", "device", "pt_converge.h")).read()
    assert "#include" not in text


# ---------------------------------------------------------------- the model --
def blocks(rows):
    """[n, nb] luminance-like block values -> [n, nb, 3] with the value in each channel"""
    b = np.asarray(rows, dtype=np.float32)
    return np.repeat(b[:, :, None], 3, axis=2)


def test_model_constant_pixel_stops_at_min_spp():
    rgb, spp, err, info = M.converge(blocks([[16.0] * 8]), 64, 256, rel_tol=0.0, abs_tol=0.0)
    assert spp.tolist() == [64] and err.tolist() == [0.0]
    assert rgb.tolist() == [[0.5, 0.5, 0.5]]                       # 2 * 16 / 64
    assert info == dict(rounds=1, samples=64, capped=0)


def test_model_non_finite_pixel_stops_at_once():
    rows = [[1.0, np.inf, 1.0, 1.0], [np.nan, 1.0, 1.0, 1.0], [1.0, 2.0, np.inf, 1.0]]
    rgb, spp, err, info = M.converge(blocks(rows), 64, 128, rel_tol=0.0)
    # the third entry is finite through its first round and varies: it goes on, then hits the cap non-finite
    assert spp.tolist() == [64, 64, 128]
    assert np.isnan(err).all()
    assert np.isinf(rgb[0]).all() and np.isnan(rgb[1]).all() and np.isinf(rgb[2]).all()
    assert info == dict(rounds=2, samples=3 * 64 + 64, capped=0)


def test_model_rounds_64_128_160():
    assert M.schedule(64, 160) == [64, 128, 160]
    assert M.schedule(64, 1024) == [64, 128, 256, 512, 1024]
    assert M.schedule(128, 128) == [128]
    # entry 0 varies throughout; entry 1 settles once its mean is known to 10 %; entry 2 is constant
    rows = [[1.0, 3.0, 1.0, 3.0, 2.0], [10.0, 11.0, 10.0, 11.0, 10.0], [5.0] * 5]
    rgb, spp, err, info = M.converge(blocks(rows), 64, 160, rel_tol=0.0)
    assert spp.tolist() == [160, 160, 64]
    assert info == dict(rounds=3, samples=64 * 3 + 64 * 2 + 32 * 2, capped=2)
    rgb, spp, err, info = M.converge(blocks(rows), 64, 160, rel_tol=0.1)
    assert spp.tolist() == [160, 64, 64]
    assert info == dict(rounds=3, samples=64 * 3 + 64 + 32, capped=1)
    # entry 1 at 64: s1 = 63, s2 = 30^2 + 33^2, d = 4.5, e2 = 2.25, err = 1.5 / 32
    assert err[1] == np.float32(1.5 / 32) and err[2] == 0
    np.testing.assert_array_equal(rgb[1], np.float32(21.0) / np.float32(64))


def test_model_tree32_is_the_pairwise_tree():
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((3, 64, 3)) * 10 ** rng.uniform(-3, 3, (3, 64, 1))).astype(np.float32)
    got = M.tree32(v)
    for e in range(3):
        for b in range(2):
            for c in range(3):
                x = [np.float32(t) for t in v[e, 32 * b:32 * b + 32, c]]
                w = 1
                while w < 32:
                    for k in range(0, 32, 2 * w):
                        x[k] = np.float32(x[k] + x[k + w])
                    w *= 2
                assert got[e, b, c] == x[0]
