"""CPU: tests/hits_model.py's scan over the committed reference span lists.  Every outcome -- a hit at a
span's start, a hit at its end, no hit -- must be present in each fixture family the GPU tests of
pt_query_hits use (tests/test_hits_gpu.py), so that a broken fixture cannot make them vacuous; the counts
are those of the fixtures as they stand."""
import os

import numpy as np
import pytest

import fastcheck as C
import hits_model as HM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIN_OUTCOME = 5
# fixture: (entries, exits, misses)
COUNTS = {"spans_csg": (2338, 5, 657), "spans_p1": (2987, 13, 0), "fastcheck_seam": (3193, 2073, 1646)}


def check(name, got):
    print(name, "enter %d, exit %d, no hit %d" % got)
    assert got == COUNTS[name]
    for want, have in zip(COUNTS[name], got):
        assert want == 0 or have >= MIN_OUTCOME


@pytest.mark.parametrize("name", ["spans_csg", "spans_p1"])
def test_scan_outcomes_of_the_span_goldens(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    w = HM.expected_hits(z["rays"], z["counts"], z["data"])
    check(name, HM.outcomes(w["hit"] != 0, w["exit"] != 0))
    # the vectorised scan is tests/fastcheck.py's scan of the list of tuples
    t = z["data"][:, [0, 5]].view(np.float32)
    m = z["data"][:, [4, 9]].view(np.int32)
    for i, sp in enumerate(C.span_lists(z["counts"], t, m)[:256]):
        h, ts, ms = C.scan(sp)
        assert (bool(w["hit"][i]), int(w["material"][i])) == (h, ms)
        assert HM.u32(w["t"][i:i + 1])[0] == HM.u32(np.array([ts]))[0]
    # a miss is all +0, an exit's normal the negated end normal
    miss = w["hit"] == 0
    assert not HM.u32(w["normal"][miss]).any() and not HM.u32(w["pos"][miss]).any() and not HM.u32(w["t"][miss]).any()
    assert (w["material"][miss] == -1).all() and (w["exit"][miss] == 0).all()


def test_scan_outcomes_of_the_seam_trees():
    z = np.load(os.path.join(GOLD, "fastcheck_seam.npz"))
    tot, rays = np.zeros(3, np.int64), 0
    for name in C.seam_names():
        hit, ex, row, t = HM.scan(z["cnt_" + name], z["t_" + name])
        tot += HM.outcomes(hit, ex)
        rays += len(hit)
        h, ts, ms = C.scan_arrays(z["cnt_" + name].astype(np.int32), z["t_" + name], z["m_" + name].astype(np.int16))
        np.testing.assert_array_equal(h, hit)
        np.testing.assert_array_equal(HM.u32(ts), HM.u32(t))
    assert rays == 6912 and len(C.seam_names()) == 18
    check("fastcheck_seam", tuple(int(v) for v in tot))


def test_camera_rays_are_the_engines():
    """u = float32(uint32) / 2^32 of the engine's first two draws, then camera_dir's arithmetic"""
    r = HM.camera_rays([0, 5 * 33 + 20], 16, 12, 33, (16.0, 12.0, 24.0), 0x5EED, 7, 2)
    assert r.shape == (2, 2, 6) and not r[..., :3].any() and (r[..., 5] == -24).all()
    a, b = HM.engine_draws(0x5EED, 5 * 33 + 20, 8, 2)
    f = np.float32
    x = f(2) * (f(20) + f(np.uint32(a)) / f(4294967296.0)) / f(16) - f(1)
    y = f(1) - f(2) * (f(5) + f(np.uint32(b)) / f(4294967296.0)) / f(12)
    assert r[1, 1, 3] == x * f(16) and r[1, 1, 4] == y * f(12)
    assert x > 1  # a pixel past the right edge looks outside the screen
    assert HM.guide_mean(np.array([[1, 2, 4, 0]], f), 4)[0] == f(1.75)
