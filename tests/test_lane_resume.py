"""pt_scene_set_lane_resume: a lane keeps its sample, walks the whole ray tree
and asks the wave for each scatter burst (pt_device.h lane_walk_rs and
render_chunk's service loop); the wave walks no spine.

Every comparison is bit for bit and includes the counters: against the CPU
oracle the frame, `queries` and `shaded`; against the same scene with the
form off also the burst counters the oracle has no counterpart of (`leaf`
counts burst children only, `dark` and the pass counters are the kernel's
own), which must not move because the bursts are the same bursts.

The scenes here are scene_p1, a forcing scene and one sheared sphere: two
Difference nodes, no Intersection, one transform, no span tie.  The
adversarial CSG of tests/csgfuzz.py (ties, Intersections, transforms over
Differences), the strengths on the edges of traceRay's arithmetic, the census
of suspended lanes and full chunks over that geometry are in
tests/test_lane_resume_csg.py, which shares COUNTERS and ORDERS.

The modules are listed in tests/precompile_lane_resume.py.
"""
import os

import numpy as np
import pytest

import csgfuzz as F
import oracle_py as O
import pathtrace as pt
from pathtrace import scenes
from pathtrace.scene import ColorTexture, Material, MultiplyTexture, Plane, Sphere, Union, to_text

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H, SPP, DEPTH = 32, 20, 2, 8
ORDERS = {"fast": O.ORDER_FAST, "reference": O.ORDER_REFERENCE}
# the kernel's counters that no order of service may change
COUNTERS = ["samples", "queries", "shaded", "leaf_queries", "dark_queries", "attempts", "rounds", "slow_queries",
            "mid_queries"]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3).view(np.uint32)


def force_scene():
    """A glass sphere in front of a diffuse sphere, a mirror sphere beside them, an emissive sky plane.
    Behind the glass a refraction child lands on the diffuse sphere while its node's frame waits for the
    mirror child (a lane suspends at stack depth >= 1, and again in the same sample); the mirror sphere
    sends strength 0.99 sqrt(3) = 1.71 to the diffuse one: a burst of N = 17 146 children.  The diffuse
    reflectance is the demo's 0.8 under a MultiplyTexture of (1, 1, 1) -- the same values, and the only
    MultiplyTexture of the scene, evaluated once per scatter loop: the oracle's tex_multiply counts bursts."""
    m = scenes.materials()
    diffuse = Material(MultiplyTexture((1, 1, 1), ColorTexture(0.8)), ColorTexture(1))
    return Union(Union(Sphere((0, 0, -3), .5, m["glass"]), Sphere((0, 0, -5.2), 1.5, diffuse)),
                 Union(Sphere((1.5, 0, -3.6), .6, m["mirror"]), Plane((0, 0, 1), 200, m["sky"])))


def bright_scene():
    """matBrightDiffuseWhite on one sphere: its bursts' children recurse (not all-leaf)"""
    m = scenes.materials()
    return Union(Sphere((0, 0, -4), 1.0, m["brightDiffuse"]), Plane((0, 0, 1), 200, m["sky"]))


def cap_scene_leaf(shift=(0.0, 0.0, 0.0)):
    """csgfuzz's cap scene -- the glossy sphere (scatter coefficient 0.3) under a shear, whose rejection
    loops run into the 1000-attempt cap -- with the sphere's reflectance lowered from 0.9 to 0.5.  At 0.9
    the scene is not all-leaf (a burst of N = 1 child: strength x add in [1/3000, 2/3000) gives the child
    up to 6.67e-4 x 0.9 sqrt(3) = 1.04e-3 >= eps), so the form would not be built; at 0.5 that bound is
    5.8e-4 and the facts hold.  The cap depends on the sheared normals only, not on the reflectance."""
    root = F.cap_scene(shift)

    def spheres(o):
        return [o] if isinstance(o, Sphere) else [s for c in o.children() for s in spheres(c)]
    ball, = spheres(root)
    ball.material = Material(ColorTexture(0.5), ColorTexture(0.3))
    return root


BRIGHT = dict(W=16, H=12, spp=1, depth=3)
# launch shapes of the on-against-off test: (pixels, spp)
SHAPES = {"1px": (1, 2), "7px": (7, 2), "70px": (70, 2), "4spp": (70, 4), "96spp_3px": (3, 96), "128spp_2px": (2, 128)}


def p1_pixels(n):
    """n pixels of the 32 x 20 frame across the glass / mirror group, the diffuse group and the sky"""
    return (np.arange(n, dtype=np.int64) * 37 % (W * H)).astype(np.int32) if n > 3 else \
        np.array([10 * W + 24, 10 * W + 8, 2 * W + 2][:n], dtype=np.int32)


def check_vs_oracle(root, tmp, w, h, spp, depth, order, **opts):
    g, st = pt.render(pt.DeviceScene(root, **opts), w, h, spp, depth, order=order, stats=True)
    o, ost = O.render(to_text(root, str(tmp)), w, h, spp, depth, order=ORDERS[order], stats=True)
    print("queries %d / %d, shaded %d / %d" % (st["queries"], ost["queries"], st["shaded"], ost["shaded"]))
    np.testing.assert_array_equal(u32(g), u32(o))
    assert st["queries"] == ost["queries"] and st["shaded"] == ost["shaded"], (st, ost)
    return g, st


def test_force_scene_facts_and_bursts(built, tmp_path):
    """CPU: the forcing scene is all-leaf (the form applies), some sample runs two or more bursts, and
    some burst has more than 10^4 children"""
    root = force_scene()
    assert pt.DeviceScene(root).reach_facts["bursts_all_leaf"]
    text = to_text(root, str(tmp_path))
    most, biggest = 0, 0
    for p in range(W * H):
        _, st = O.render(text, W, H, 1, DEPTH, pixels=[p], stats=True, threads=1)
        most = max(most, st["tex_multiply"])
        if st["tex_multiply"] == 1:
            biggest = max(biggest, st["scatter_children"] - (st["shaded"] - 1))
    print("most bursts in one sample: %d, largest single burst: %d children" % (most, biggest))
    assert most >= 2
    assert biggest > 10000


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
def test_p1_matches_oracle(built, tmp_path, order):
    check_vs_oracle(scenes.scene_p1(), tmp_path, W, H, SPP, DEPTH, order, lane_resume=1)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
@pytest.mark.parametrize("depth", [DEPTH, 2])
def test_force_scene_matches_oracle(built, tmp_path, order, depth):
    """several suspensions per sample, bursts of more than 10^4 children; depth 2: the shallow stack"""
    root = force_scene()
    _, st = check_vs_oracle(root, tmp_path, W, H, SPP, depth, order, lane_resume=1)
    _, off = pt.render(pt.DeviceScene(root, lane_resume=0), W, H, SPP, depth, order=order, stats=True)
    assert [st[k] for k in COUNTERS] == [off[k] for k in COUNTERS], (st, off)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_on_equals_off(built, order, shape):
    """partial chunks, invalid lanes, chunks mixing finished, suspended and running lanes; sample-major
    with the slot permutation (4 spp), slot-major chunks of 32 (96 spp), chunks of 64 with block sums (128)"""
    n, spp = SHAPES[shape]
    pix = p1_pixels(n)
    out = []
    for on in (1, 0):
        g, st = pt.render(pt.DeviceScene(scenes.scene_p1(), lane_resume=on), W, H, spp, DEPTH, order=order,
                          pixels=pix, stats=True)
        out.append((g, [st[k] for k in COUNTERS]))
    np.testing.assert_array_equal(u32(out[0][0]), u32(out[1][0]))
    assert out[0][1] == out[1][1], (COUNTERS, out[0][1], out[1][1])


# Launches large enough for full chunks: the runtime halves a launch's chunk until every resident wave
# has four (runtime.cpp: n_items / chunk >= 4 x waves, 81 920 chunks on an MI355X), so the launches above
# run one or two lanes per chunk.  These give every wave chunks of 32 and 64 lanes, many of them
# suspended at once: (width, height, spp) -> sample-major with the slot permutation, slot-major chunks
# of 32 with block sums, slot-major chunks of 64 with block sums, chunks that straddle two pixels.
FULL_SHAPES = {"64spp_sample_major": (320, 256, 64), "128spp_chunk32": (256, 160, 128),
               "384spp_chunk64": (160, 100, 384), "330spp_straddle": (160, 100, 330)}


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["p1", "force"])
@pytest.mark.parametrize("shape", list(FULL_SHAPES))
def test_full_chunks_on_equals_off(built, scene, shape):
    """up to 64 lanes of a chunk walking, suspended and served in one round"""
    w, h, spp = FULL_SHAPES[shape]
    root = scenes.scene_p1() if scene == "p1" else force_scene()
    out = []
    for on in (1, 0):
        g, st = pt.render(pt.DeviceScene(root, lane_resume=on), w, h, spp, DEPTH, order="fast", stats=True)
        out.append((g, [st[k] for k in COUNTERS]))
    print(dict(zip(COUNTERS, out[0][1])))
    np.testing.assert_array_equal(u32(out[0][0]), u32(out[1][0]))
    assert out[0][1] == out[1][1], (COUNTERS, out[0][1], out[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
def test_cap_trace_rays(built, order):
    """the reference's count > 1000 early return inside a served burst (B_ABORT) unwinds through the
    lane's PH_RETURN like B_DONE: the frozen cap rays (tests/golden/csgfuzz_cap.npz) against the oracle"""
    with np.load(os.path.join(GOLD, "csgfuzz_cap.npz")) as z:
        rays, (spp, depth, seed) = z["rays"], [int(v) for v in z["meta"]]
    root = cap_scene_leaf()
    ds = pt.DeviceScene(root, lane_resume=1)
    assert ds.reach_facts["bursts_all_leaf"]
    got, st = pt.trace_rays(ds, rays, depth, spp=spp, seed=seed, order=order, stats=True)
    want, ost = O.trace_rays(to_text(root), rays, spp, depth, seed=seed, stats=True, order=ORDERS[order])
    assert ost["cap_returns"] > 0
    np.testing.assert_array_equal(u32(got), u32(want))
    assert st["queries"] == ost["queries"], (st["queries"], ost["queries"])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
def test_cap_render(built, tmp_path, order):
    c = F.CAP_RENDER
    root = cap_scene_leaf(c["shift"])
    assert pt.DeviceScene(root).reach_facts["bursts_all_leaf"]
    _, ost = O.render(to_text(root, str(tmp_path)), c["W"], c["H"], c["spp"], c["depth"], stats=True,
                      order=ORDERS[order])
    assert ost["cap_returns"] > 0
    check_vs_oracle(root, tmp_path, c["W"], c["H"], c["spp"], c["depth"], order, lane_resume=1)


def test_not_all_leaf_builds_without_the_form(built):
    """asked for on a scene whose bursts can recurse, the module is the one built without the form"""
    root = bright_scene()
    assert not pt.DeviceScene(root).reach_facts["bursts_all_leaf"]
    keys = [pt.DeviceScene(root, lane_resume=on).kernel_key(BRIGHT["depth"]) for on in (1, 0)]
    assert keys[0] == keys[1]
    p1 = [pt.DeviceScene(scenes.scene_p1(), lane_resume=on).kernel_key(DEPTH) for on in (1, 0)]
    assert p1[0] != p1[1]


@pytest.mark.gpu
def test_not_all_leaf_matches_oracle(built, tmp_path):
    b = BRIGHT
    check_vs_oracle(bright_scene(), tmp_path, b["W"], b["H"], b["spp"], b["depth"], "fast", lane_resume=1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["1px", "7px", "70px"])
def test_poisoned_lds(built, tmp_path, monkeypatch, shape):
    """every LDS word starts as all-ones (PT_POISON_LDS): the served burst reads nothing of the wave's
    frame that the request did not write"""
    monkeypatch.setenv("PT_DEVICE_DEFINES", "PT_POISON_LDS=1")
    n, spp = SHAPES[shape]
    pix = p1_pixels(n)
    root = scenes.scene_p1()
    g = pt.render(pt.DeviceScene(root, lane_resume=1), W, H, spp, DEPTH, order="fast", pixels=pix)
    o = O.render(to_text(root, str(tmp_path)), W, H, spp, DEPTH, order=O.ORDER_FAST, pixels=pix)
    np.testing.assert_array_equal(u32(g), u32(o))
