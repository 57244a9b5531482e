"""The lane-resume form (pt_device.h lane_walk_rs) over adversarial CSG.

tests/test_lane_resume.py holds the form to scene_p1, the forcing scene and
one sheared sphere: two Difference nodes, no Intersection, one transform and
no span tie.  The trace scenes of tests/csgfuzz.py have all of these, but their
glossy material (reflectance 0.9) makes them not all-leaf, so their modules
are built without the form.  With that one reflectance lowered to 0.5
(csgfuzz.trace_scene(s, leaf=True)) every burst ends in leaves and the form is
the scene's default module; tests/golden/csgfuzz_trace_leaf.npz holds what the
unmodified reference computes for them (tests/golden/make_csgfuzz_golden.py),
on the scenes' rays and on the same rays with strengths on the edges of
traceRay's arithmetic (csgfuzz.EDGE_STRENGTHS).

Every comparison is bit for bit.  CPU: the facts hold and the form is built,
the oracle equals the reference, and the census -- scatter loops entered, and
those entered below a waiting parent frame -- shows that lanes do suspend, at
stack depth >= 1 too.  GPU: reference order against the reference, fast order
against the oracle, the form on against off with every counter, the same over
launches large enough for chunks of 64 lanes walking 64 different rays, and the
camera path.

The modules are listed in tests/precompile_lane_resume.py.
"""
import os

import numpy as np
import pytest

import csgfuzz as F
import oracle_py as O
import pathtrace as pt
from pathtrace.scene import to_text
from test_lane_resume import COUNTERS, ORDERS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = range(F.N_TRACE_SCENES)
FAMILIES = ["", "edge_"]
FAMILY_IDS = ["rays", "edge_strengths"]
TRACE_SPP, TRACE_DEPTH = 2, 3
# census floors (bursts, nested_bursts).  Measured with the fixture's parameters (seed 0x5EED, reference
# order, spp 2, depth 3, all 512 rays), per scene: 532 / 136, 400 / 106, 630 / 82, 562 / 138, 672 / 134,
# 462 / 150.  The floors leave room for a counter defined slightly differently, not for an empty test.
MIN_BURSTS, MIN_NESTED = 300, 60
# the full-chunk launch: 160 copies of a scene's 512 rays at 64 spp = 5 242 880 items, the count at
# which the runtime keeps chunks of 64 (runtime.cpp: n_items / chunk >= 4 x waves, 81 920 chunks on an
# MI355X); sample-major with the slot permutation, so a chunk's 64 lanes hold 64 different rays
FULL_COPIES, FULL_SPP = 160, 64
# scene 3: a transform, two Differences and five Intersections.  Measured on an MI355X: 10.0 s for its
# two renders (32.7 G queries each); scene 4 (five Differences) passed the same comparison in 5.2 s and
# is left out to keep the suite short; test_full_chunks_on_equals_off[64spp_sample_major-p1] takes 2.0 s.
FULL_SCENES = [3]
# the camera path: 48 x 32 pixels over a screen that sees every assembly whole (centres at x = -15 .. 15,
# z = -8, radii up to 1.5: the outermost silhouette is at x / z = tan(atan(15 / 8) + asin(1.5 / 17)) =
# 2.35 < 20 / 8, and |y / z| <= 2 / 6 < 3 / 8; the default screen sees ground and wall only)
CAM = dict(W=48, H=32, spp=2, depth=6, screen=(20.0, 3.0, 8.0))
# the two scenes with a transform, and scene 5 for its glass: in scene 3 the one glass sphere is the
# outer operand of Intersection(z, Difference(x, y)) over the touching-spheres tie set, where x lies
# inside z, so no ray from outside meets a glass surface and the view cannot have refraction children
# (the oracle counts 0 on any screen).  There the lanes suspend below a mirror's frame instead; scenes
# 0 and 5 show their glass.
CAM_SCENES = [0, 3, 5]
CAM_GLASS = [0, 5]
_cache = {}


def gold():
    if "z" not in _cache:
        with np.load(os.path.join(GOLD, "csgfuzz_trace_leaf.npz")) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def meta():
    return [int(v) for v in gold()["meta"]]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3).view(np.uint32)


def assert_same_bits(got, want):
    np.testing.assert_array_equal(u32(got), u32(want))


def all_rays(s, family):
    return F.edge_strength_rays(s) if family else F.trace_rays(s)


def leaf_text(s):
    if ("text", s) not in _cache:
        _cache["text", s] = to_text(F.trace_scene(s, leaf=True))
    return _cache["text", s]


def oracle_trace(s, rays, order, spp, **kw):
    """the oracle's means and stats over the fixture's rays of a family ("" / "edge_") or over an
    array of rays, computed once per launch"""
    key = (s, rays if isinstance(rays, str) else rays.tobytes(), order, spp, tuple(sorted(kw.items())))
    if key not in _cache:
        r = gold()["%srays_%d" % (rays, s)] if isinstance(rays, str) else rays
        _cache[key] = O.trace_rays(leaf_text(s), r, spp, TRACE_DEPTH, order=ORDERS[order], stats=True, **kw)
    return _cache[key]


def oracle_camera(s, order):
    key = ("cam", s, order)
    if key not in _cache:
        c = CAM
        _cache[key] = O.render(leaf_text(s), c["W"], c["H"], c["spp"], c["depth"], screen=c["screen"],
                               order=ORDERS[order], stats=True)
    return _cache[key]


def gpu_trace(s, on, rays, order, **kw):
    got, st = pt.trace_rays(pt.DeviceScene(F.trace_scene(s, leaf=True), lane_resume=on), rays, TRACE_DEPTH,
                            order=order, stats=True, **kw)
    return got, [st[k] for k in COUNTERS]


# --------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("s", SCENES)
def test_leaf_facts_and_code_object_keys(built, s):
    """the leaf variant is all-leaf and its module with the form differs from the one without; the
    default scene is not all-leaf and asking for the form changes nothing"""
    leaf, plain = F.trace_scene(s, leaf=True), F.trace_scene(s)
    assert pt.DeviceScene(leaf).reach_facts["bursts_all_leaf"]
    assert not pt.DeviceScene(plain).reach_facts["bursts_all_leaf"]
    on, off = [pt.DeviceScene(leaf, lane_resume=v).kernel_key(TRACE_DEPTH) for v in (1, 0)]
    assert on != off
    assert pt.DeviceScene(leaf).kernel_key(TRACE_DEPTH) == on  # the default path
    on, off = [pt.DeviceScene(plain, lane_resume=v).kernel_key(TRACE_DEPTH) for v in (1, 0)]
    assert on == off


def test_leaf_changes_one_material_only():
    """leaf=True is the glossy reflectance 0.9 -> 0.5 and nothing else; the rays do not depend on it"""
    for s in SCENES:
        a, b = to_text(F.trace_scene(s)).splitlines(), leaf_text(s).splitlines()
        assert len(a) == len(b)
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        assert len(diff) == 1, diff
        x, y = (ln.split() for ln in diff[0])
        assert x[:2] == y[:2] and x[0] == "tex", diff
        assert [np.float32(float.fromhex(v)) for v in x[3:]] == [np.float32(0.9)] * 3, diff
        assert [float.fromhex(v) for v in y[3:]] == [0.5] * 3, diff


def test_fixture_is_the_generators_input():
    z = gold()
    assert meta()[:2] == [TRACE_SPP, TRACE_DEPTH]
    for s in SCENES:
        assert str(z["text_%d" % s]) == leaf_text(s)
        for fam in FAMILIES:
            rays, moved = all_rays(s, fam), z["%smoved_index_%d" % (fam, s)]
            assert len(moved) <= 0.02 * len(rays)  # only rays the reference itself asserts on, at most 2 %
            np.testing.assert_array_equal(z["%srays_%d" % (fam, s)].view(np.uint32),
                                          np.delete(rays, moved, axis=0).view(np.uint32))
            assert z["%smean_%d" % (fam, s)].shape == (len(rays) - len(moved), 3)
            assert not np.isnan(z["%smean_%d" % (fam, s)]).any()
        base, edge = all_rays(s, ""), all_rays(s, "edge_")
        np.testing.assert_array_equal(base[:, :6].view(np.uint32), edge[:, :6].view(np.uint32))
        want = np.array(F.EDGE_STRENGTHS, dtype=np.float32)
        np.testing.assert_array_equal(edge[:len(want), 6].view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(edge[len(want):, 6].view(np.uint32), edge[:-len(want), 6].view(np.uint32))
    eps = np.float32(1e-3)
    e = np.array(F.EDGE_STRENGTHS, dtype=np.float32)
    assert np.isnan(e[0]) and np.isposinf(e[1]) and e[4] == eps and 0 < e[5] < eps
    root, rays = F.regress_resume_negative_count()
    assert str(z["regress_text"]) == to_text(root)
    np.testing.assert_array_equal(z["regress_rays"].view(np.uint32), rays.view(np.uint32))
    assert os.path.getsize(os.path.join(GOLD, "csgfuzz_trace_leaf.npz")) <= 500 * 1000


def test_oracle_on_the_regression_rays(built):
    z = gold()
    spp, depth, seed = meta()
    got, st = O.trace_rays(str(z["regress_text"]), z["regress_rays"], spp, depth, seed=seed, stats=True)
    assert_same_bits(got, z["regress_mean"])
    assert st["bursts"] == spp  # the control's two samples; the three edge strengths run no loop
    assert not u32(got)[:3].any() and u32(got)[3].all()


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("s", SCENES)
def test_oracle_matches_reference(built, s, family):
    spp, _, seed = meta()
    got, _ = oracle_trace(s, family, "reference", spp, seed=seed)
    assert_same_bits(got, gold()["%smean_%d" % (family, s)])


@pytest.mark.parametrize("s", SCENES)
def test_census(built, s):
    """a guard against a vacuous test: with the fixture's parameters hundreds of samples of every scene
    enter a scatter loop (the lane suspends), dozens of them from a refraction or mirror child (it
    suspends with a parent frame waiting).  Counted by the oracle: `bursts` are the scatter loops with
    sc > eps that run, `nested_bursts` those entered by a traceRay call at recursion level >= 2."""
    spp, _, seed = meta()
    _, st = oracle_trace(s, "", "reference", spp, seed=seed)
    print("leaf scene %d: bursts %d, nested_bursts %d, queries %d" % (s, st["bursts"], st["nested_bursts"],
                                                                      st["queries"]))
    assert st["bursts"] >= MIN_BURSTS and st["nested_bursts"] >= MIN_NESTED, st
    assert st["cap_returns"] == 0


@pytest.mark.parametrize("s", CAM_SCENES)
def test_camera_view_hits_the_glass(built, s):
    """the camera test's screen has the assemblies in view: the glass is hit (at least 100 refraction
    children) and lanes suspend below a waiting frame, at the census's own floor; in scene 3, whose
    glass no outside ray can meet, below a mirror's frame only"""
    out, st = oracle_camera(s, "fast")
    print("leaf scene %d camera: refract_children %d, bursts %d, nested_bursts %d" % (
        s, st["refract_children"], st["bursts"], st["nested_bursts"]))
    if s in CAM_GLASS:
        assert st["refract_children"] >= 100
    else:
        assert st["refract_children"] == 0
    assert st["bursts"] >= MIN_BURSTS and st["nested_bursts"] >= MIN_NESTED, st
    assert np.isfinite(out).all()


# --------------------------------------------------------------------- GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("on", [1, 0], ids=["on", "off"])
@pytest.mark.parametrize("s", SCENES)
def test_gpu_reference_order_matches_reference(built, s, on, family):
    spp, depth, seed = meta()
    z = gold()
    got = pt.trace_rays(pt.DeviceScene(F.trace_scene(s, leaf=True), lane_resume=on), z["%srays_%d" % (family, s)],
                        depth, spp=spp, seed=seed, order="reference")
    assert_same_bits(got, z["%smean_%d" % (family, s)])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
@pytest.mark.parametrize("on", [1, 0], ids=["on", "off"])
def test_gpu_regress_resume_negative_count(built, on, order):
    """a strength that makes the scatter count INT_MIN: no child runs, the emission alone comes back"""
    spp, depth, seed = meta()
    z = gold()
    root, rays = F.regress_resume_negative_count()
    ds = pt.DeviceScene(root, lane_resume=on)
    assert ds.reach_facts["bursts_all_leaf"]
    got, st = pt.trace_rays(ds, rays, depth, spp=spp, seed=seed, order=order, stats=True)
    want, ost = O.trace_rays(to_text(root), rays, spp, depth, seed=seed, order=ORDERS[order], stats=True)
    if order == "reference":
        assert_same_bits(want, z["regress_mean"])
    assert_same_bits(got, want)
    assert not u32(got)[:3].any() and u32(got)[3].all()
    assert st["queries"] == ost["queries"]
    assert st["leaf_queries"] == st["queries"] - len(rays) * spp  # the control's children, nothing else


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCENES)
def test_gpu_fast_order_matches_oracle(built, s):
    """all 512 rays, other engine keys than the fixture's (sample_begin 5, ray_begin 1000)"""
    kw = dict(sample_begin=5, ray_begin=1000)
    ds = pt.DeviceScene(F.trace_scene(s, leaf=True), lane_resume=1)
    got, st = pt.trace_rays(ds, all_rays(s, ""), TRACE_DEPTH, spp=3, order="fast", stats=True, **kw)
    want, ost = oracle_trace(s, all_rays(s, ""), "fast", 3, **kw)
    assert_same_bits(got, want)
    assert st["queries"] == ost["queries"], (st["queries"], ost["queries"])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("s", SCENES)
def test_gpu_on_equals_off(built, s, family, order):
    """the same bursts served per lane and by the wave: frames and every counter"""
    spp, _, seed = meta()
    rays = gold()["%srays_%d" % (family, s)]
    on, off = [gpu_trace(s, v, rays, order, spp=spp, seed=seed) for v in (1, 0)]
    assert_same_bits(on[0], off[0])
    assert on[1] == off[1], (COUNTERS, on[1], off[1])


@pytest.mark.gpu
@pytest.mark.parametrize("s", FULL_SCENES)
def test_gpu_full_chunks_on_equals_off(built, s):
    """64 lanes of a chunk walking 64 different rays through transforms, Differences and
    Intersections, suspended and served in one round.  GPU against GPU (the oracle needs about 1 ms
    per sample and core): the off path is the one the small launches pin to the reference."""
    rays = np.tile(all_rays(s, ""), (FULL_COPIES, 1))
    assert len(rays) * FULL_SPP == 5242880
    on, off = [gpu_trace(s, v, rays, "fast", spp=FULL_SPP) for v in (1, 0)]
    print(dict(zip(COUNTERS, on[1])))
    assert_same_bits(on[0], off[0])
    assert on[1] == off[1], (COUNTERS, on[1], off[1])
    # copies of one ray have their own engine keys: their means differ somewhere
    per_copy = u32(on[0]).reshape(FULL_COPIES, -1)
    assert (per_copy != per_copy[0]).any(axis=1)[1:].all()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
@pytest.mark.parametrize("s", CAM_SCENES)
def test_gpu_camera_path_matches_oracle(built, s, order):
    c = CAM
    ds = pt.DeviceScene(F.trace_scene(s, leaf=True), lane_resume=1)
    got, st = pt.render(ds, c["W"], c["H"], c["spp"], c["depth"], screen=c["screen"], order=order, stats=True)
    want, ost = oracle_camera(s, order)
    print("queries %d / %d, shaded %d / %d" % (st["queries"], ost["queries"], st["shaded"], ost["shaded"]))
    assert_same_bits(got, want)
    assert st["queries"] == ost["queries"] and st["shaded"] == ost["shaded"], (st, ost)
