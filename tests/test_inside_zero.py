"""Kept children that end inside a solid (pt_device.h Inside, PT_INSIDE_ZERO).

The first pass settles a kept leaf child with a zero term when a non-emissive sphere X, reached
through Unions and A sides of Differences, is still open just below its exit and every subtractor on
its path is a sphere that is dead or lies strictly between X's running span start and X's exit.  The
proof is in pt_device.h; these tests hold the rule to the unmodified reference.

CPU: tests/inside_zero.py restates the per-lane predicate and the burst gates in float32.  Over the
sphere-only assemblies of tests/csgfuzz.py and the lattice cases, each under union_array([part, ground,
wall]), every ray the predicate fires on must stop traceRay's scan on a non-emissive material or return
black in the reference's own root span list (tests/golden/inside_zero.npz, frozen from oracle/_ref/ptref
by tests/golden/make_inside_zero_golden.py).  The rule as first proposed -- subtractors only had to exit
before X -- fails this test on 27 rays: src/difference.cpp:126-130 sets the END of an A span that starts
inside a B span to B's start, so X is lost when the origin is inside both.

GPU, fast order: the lattice scenes through pt_trace_rays, C3 at 48 x 27 x 64 spp and the Difference
trace scenes of csgfuzz on their frozen rays: bits equal to the oracle's and to the build without the
rule (PT_INSIDE_ZERO=0), equal query counts, no more mid and slow children than without it; on C3 at
most half the mid children.  Measured on an MI355X: C3 mid_queries 2 594 445 with the rule, 5 719 464
without (45 %); slow_queries 478 236 / 487 513.  The csgfuzz trace scenes are here because they are
Difference-bearing scenes the suite already freezes, not as evidence for the rule: it is compiled out or
never fires in them (mid 2 550 966 / 2 550 966 for s = 1, 0 / 0 for s = 2, 4, 5), and of the lattice scenes
lat1 moves by only 283 of 932 462 mid children.  At 1920 x 1080 x 1024 spp 8 pixels of C3's frame differ
between the arms, through the mid pass's fast check and not through the rule
(profiles/round10/frame_diff_passes.txt); no render here is large enough to reach such a child
(tests/test_fastcheck.py renders those pixels, since the fix of that check).

The modules are listed in tests/precompile_inside_zero.py."""
import os

import numpy as np
import pytest

import csgfuzz as F
import inside_zero as Z
import oracle_py as O
import pathtrace as pt
from pathtrace import scenes
from pathtrace.scene import Difference, Sphere, to_text

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OFF = "PT_INSIDE_ZERO=0"
TRACE_DEPTH = 3
LATTICE_RAYS = 384
C3 = dict(W=48, H=27, spp=64, depth=8)
FUZZ_SCENES = [1, 2, 4, 5]  # the Difference-bearing leaf variants without a transform
COUNTS = ["queries", "leaf_queries", "dark_queries"]
_cache = {}


def gold():
    if "z" not in _cache:
        with np.load(os.path.join(GOLD, "inside_zero.npz")) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3).view(np.uint32)


def verdicts(name):
    """the material index traceRay's scan stops on (-1: black) for each of the case's rays"""
    z = gold()
    cnt, t, m = z["cnt_" + name], z["t_" + name], z["m_" + name]
    pos = np.concatenate([[0], np.cumsum(cnt)])
    return np.array([Z.scan([(t[j, 0], m[j, 0], t[j, 1], m[j, 1]) for j in range(pos[i], pos[i + 1])])
                     for i in range(len(cnt))])


def sides(n, on_b=False):
    """(sphere, whether it lies below the B side of some Difference) for every sphere of the tree"""
    if isinstance(n, Sphere):
        return [(n, on_b)]
    if isinstance(n, Difference):
        return sides(n.a, on_b) + sides(n.b, True)
    return [x for c in n.children() for x in sides(c, on_b)]


# --------------------------------------------------------------------- CPU ---
def test_fixture_is_the_generators_input():
    z = gold()
    for k, (name, root) in enumerate(Z.cpu_cases()):
        assert str(z["text_" + name]) == to_text(root), name
        np.testing.assert_array_equal(z["rays_" + name].view(np.uint32), Z.case_rays(root, k).view(np.uint32))
        a = Z.dot(z["rays_" + name][:, 3:6], z["rays_" + name][:, 3:6])
        assert np.all(np.abs(a - 1) <= 2.0 ** -20), name  # unit child rays
    assert os.path.getsize(os.path.join(GOLD, "inside_zero.npz")) <= 500 * 1000


def test_predicate_is_sound_on_the_reference_span_lists():
    z = gold()
    fam = dict(outside=0, cavity=0, nested=0, refused_wall=0)
    for name, root in Z.cpu_cases():
        rays = z["rays_" + name]
        emis = Z.emissive_ids(str(z["text_" + name]))
        f = Z.fires(root, rays)
        v = verdicts(name)
        wall = np.isin(v, list(emis))
        assert not np.any(f & wall), (name, np.nonzero(f & wall)[0])
        cc = np.array([Z._sphere(s, rays[:, :3])[1] for s in Z.spheres(root)])
        outside = (cc > 1e-3).all(axis=0)
        fam["outside"] += int((f & outside).sum())
        # a cavity origin: on the surface of a subtractor (a sphere below some Difference's B side) and
        # strictly inside a sphere that is below none
        none = np.zeros(len(rays), bool)
        on_b = np.array([np.abs(Z._sphere(s, rays[:, :3])[1]) <= 1e-3 for s, b in sides(root) if b] + [none])
        in_a = np.array([Z._sphere(s, rays[:, :3])[1] < -1e-3 for s, b in sides(root) if not b] + [none])
        fam["cavity"] += int((f & on_b.any(axis=0) & in_a.any(axis=0)).sum())
        fam["nested"] += int(f.sum()) if name in Z.NESTED else 0
        fam["refused_wall"] += int((wall & ~f).sum())
    print(fam)
    # a guard against a vacuous test
    assert all(n >= 20 for n in fam.values()), fam


@pytest.mark.parametrize("name", ["x_on_b", "under_isect", "behind_wall", "emis_sphere", "xf", "dif_uni_b_overlap",
                                  "int_dif_a_overlap", "diff_chain_b"])
def test_rule_is_off_where_its_conditions_fail(name):
    """X on a B side, X under an Intersection, a sphere whose far bound reaches T_E, an emissive
    sphere, a transformed node: no ray fires"""
    root = dict(Z.cpu_cases())[name]
    assert not Z.fires(root, gold()["rays_" + name]).any()


def test_lattice_cases():
    cases = dict(Z.cpu_cases())
    ax = np.array([[0, 0, 0, 0, 0, -1], [0, 0, -3, 0, 0, -1], [0, 0, -4, 0, 0, -1]], np.float32)
    # the subtractor's exit equals X's exit exactly on the axis (both at z = -5): refused
    assert not Z.fires(cases["exit_tie"], ax).any()
    # a subtractor covering X's exit: refused on the axis, from outside and from inside X
    assert not Z.fires(cases["cover"], ax).any()
    # the cavity's origin (0, 0, -3.5) on B inside X; along -z the A exit (1.5) precedes the B exit (2)
    cav = np.array([[0, 0, -3.5, 0, 0, -1]], np.float32)
    assert not Z.fires(cases["cavity_short"], cav).any()
    # (A - B1) - B2 along -z from outside: B1 lies before X's exit, B2 (z = -4.5 .. -5.5) past it
    assert not Z.fires(cases["two_subs"], ax[:1]).any()
    # the same tree seen from the side, where both subtractors are missed: X occludes
    side = np.array([[-3, 0.875, -4, 1, 0, 0]], np.float32)
    assert Z.fires(cases["two_subs"], side).all()
    # an origin inside the wall's solid: T_E = 0
    behind = np.array([[0, 0, -17, 0, 0, 1]], np.float32)
    assert not Z.fires(cases["cavity_short"], behind).any()
    # weights that overflow: the burst keeps every child
    assert Z.wfin([0.8, 0.7, 0.6]) and not Z.wfin([3e37, 0.5, 0.5]) and not Z.wfin([np.nan, 0, 0])


# --------------------------------------------------------------------- GPU ---
def lattice_rays(name, n=LATTICE_RAYS):
    """n x 7 caller rays: from in front of, beside and above each assembly at points on and around
    it, so that bursts start on outer surfaces and on the cavities; in `behind` a tenth start behind the
    wall and aim at the sphere there (burst origins inside the wall's solid)"""
    rng = np.random.default_rng(4100 + len(name))
    parts = Z.lattice_parts(name)
    rays = []
    for k in range(n):
        _, c = parts[k % len(parts)]
        c = np.array(c, np.float32)
        o = c + np.array([(0, 0, 4), (0, 1.5, 3), (-2, 0, 3), (2, 1, 2), (0, 0, -3)][(k // len(parts)) % 5], np.float32)
        tgt = c + rng.uniform(-0.8, 0.8, size=3).astype(np.float32)
        if name == "behind" and k % 10 == 9:
            o, tgt = np.array([0, 0, -64], np.float32), np.array([0, 0, -70], np.float32) + rng.uniform(-1, 1, 3)
        rays.append(np.concatenate([o, tgt - o, [1.0]]))
    return np.array(rays, np.float32)


def gpu(make, fn, monkeypatch, off):
    if off:
        monkeypatch.setenv("PT_DEVICE_DEFINES", OFF)
    else:
        monkeypatch.delenv("PT_DEVICE_DEFINES", raising=False)
    return fn(make())


def check_arms(on, off, want, wst, half=False):
    (g1, s1), (g0, s0) = on, off
    np.testing.assert_array_equal(u32(g1), u32(want))
    np.testing.assert_array_equal(u32(g1), u32(g0))
    assert s1["queries"] == wst["queries"]
    assert [s1[k] for k in COUNTS] == [s0[k] for k in COUNTS]
    print("mid %d / %d, slow %d / %d" % (s1["mid_queries"], s0["mid_queries"], s1["slow_queries"], s0["slow_queries"]))
    assert s1["mid_queries"] <= s0["mid_queries"] and s1["slow_queries"] <= s0["slow_queries"]
    if half:
        assert 2 * s1["mid_queries"] <= s0["mid_queries"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", Z.GPU_SCENES)
def test_gpu_lattice_scenes(built, monkeypatch, name):
    root, rays = Z.lattice_scene(name), lattice_rays(name)
    depth = 1 if name == "overflow" else TRACE_DEPTH
    want, wst = O.trace_rays(to_text(root), rays, 1, depth, order=O.ORDER_FAST, stats=True)
    arms = [gpu(lambda: pt.DeviceScene(Z.lattice_scene(name)),
                lambda ds: pt.trace_rays(ds, rays, depth, spp=1, order="fast", stats=True), monkeypatch, off)
            for off in (False, True)]
    check_arms(arms[0], arms[1], want, wst)
    if name in ("behind", "xf", "emis_sphere", "overflow"):  # gated off, compiled out, refused by wfin: the same passes
        assert arms[0][1]["mid_queries"] == arms[1][1]["mid_queries"]
    if name in ("lat0", "lat1"):
        assert arms[0][1]["mid_queries"] < arms[1][1]["mid_queries"]


@pytest.mark.gpu
@pytest.mark.parametrize("s", FUZZ_SCENES)
def test_gpu_csgfuzz_leaf_scenes(built, monkeypatch, s):
    import test_lane_resume_csg as L
    spp, _, seed = L.meta()
    rays = L.gold()["rays_%d" % s]
    want, wst = L.oracle_trace(s, "", "fast", spp, seed=seed)
    arms = [gpu(lambda: pt.DeviceScene(F.trace_scene(s, leaf=True)),
                lambda ds: pt.trace_rays(ds, rays, L.TRACE_DEPTH, spp=spp, seed=seed, order="fast", stats=True),
                monkeypatch, off) for off in (False, True)]
    check_arms(arms[0], arms[1], want, wst)


def c3_render(monkeypatch, off, order):
    c = C3
    return gpu(lambda: scenes.CONFIGS["C3"].device_scene(),
               lambda ds: pt.render(ds, c["W"], c["H"], c["spp"], c["depth"], stats=True, order=order), monkeypatch, off)


@pytest.mark.gpu
def test_gpu_c3_fast_order(built, monkeypatch, tmp_path):
    c = C3
    want, wst = O.render(to_text(scenes.scene_p1(), str(tmp_path)), c["W"], c["H"], c["spp"], c["depth"],
                         order=O.ORDER_FAST, stats=True)
    check_arms(c3_render(monkeypatch, False, "fast"), c3_render(monkeypatch, True, "fast"), want, wst, half=True)


@pytest.mark.gpu
def test_gpu_c3_reference_order_does_not_take_the_rule(built, monkeypatch):
    (g1, s1), (g0, s0) = c3_render(monkeypatch, False, "reference"), c3_render(monkeypatch, True, "reference")
    np.testing.assert_array_equal(u32(g1), u32(g0))
    assert s1["mid_queries"] == s0["mid_queries"] and s1["slow_queries"] == s0["slow_queries"]
