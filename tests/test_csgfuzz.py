"""Adversarial CSG and the rejection cap against the unmodified reference.

The fast first-hit code (pt_device.h span_first_hit) skips the lazy CSG merges
whenever comparisons of span ends allow it; whether those comparisons are sound
is decided at exact ties -- a1 == b0, a0 == b0, B covering A, the Difference
quirk's inverted span -- which random rays almost never produce.  The inputs
of tests/csgfuzz.py sit on a float32-exact lattice so that they do, for every
(outer operator, inner operator, side) nesting, under transforms and in deep
Difference chains; tests/golden/make_csgfuzz_golden.py froze what the reference
computes for them, together with a census of the ties its own span lists show.

The second subject is the reference's `count > 1000` early return
(include/path-trace.h:144-157; pt_device.h replay() B_ABORT and the lane walks):
a glossy sphere under a sheared TransformedObject reaches it, and
csgfuzz_cap.npz holds rays on which the reference build's assertion fires.

Every comparison is bit for bit.  CPU: the fixtures are what the generator
makes today, the census conditions hold, and the oracle equals the reference.
GPU: pt_query_spans, pt_trace_rays (both orders, every walk option) and
pt_render against the fixtures and the oracle.
"""
import os

import numpy as np
import pytest

import csgfuzz as F
import oracle_py as O
import pathtrace as pt
from pathtrace.scene import TransformedObject, _Binary, to_text

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TREES = F.span_trees()
TREE_NAMES = [n for n, _ in TREES]
TRACE_SPP, TRACE_DEPTH = 2, 3
# scene options of the cap scene's ray-list modules (tests/precompile_modules.py builds them)
CAP_OPTS = [{}, {"lane_walk": 2}, {"lane_scatter": True}]
_cache = {}


def gold(name):
    if name not in _cache:
        with np.load(os.path.join(GOLD, "csgfuzz_%s.npz" % name)) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def span_rows(spans):
    """(counts, n x 10 words) of a list of span lists, the fixtures' layout"""
    counts = np.array([len(s) for s in spans], dtype=np.int32)
    rows = [np.concatenate([u32(a), [np.uint32(m0 & 0xFFFFFFFF)], u32(b), [np.uint32(m1 & 0xFFFFFFFF)]])
            for s in spans for (a, m0, b, m1) in s]
    return counts, np.array(rows, dtype=np.uint32).reshape(-1, 10)


def all_trace_rays(s):
    """the scene's rays before the ones the reference asserts on were taken out"""
    return F.trace_rays(s)


# --------------------------------------------------------------------- CPU ---
def test_fixtures_are_the_generators_inputs():
    """a numpy or seed drift would leave the fixtures describing other inputs than the tests build"""
    z = gold("spans")
    assert [str(n) for n in z["names"]] == TREE_NAMES and 40 <= len(TREES) <= 60
    for k, (name, builder) in enumerate(TREES):
        root = builder()
        assert str(z["text_%d" % k]) == to_text(root), name
        np.testing.assert_array_equal(u32(z["rays_%d" % k]), u32(F.span_rays(root, seed=k)), err_msg=name)
    t, c = gold("trace"), gold("cap")
    assert [int(v) for v in t["meta"]][:2] == [TRACE_SPP, TRACE_DEPTH]
    for s in range(F.N_TRACE_SCENES):
        assert str(t["text_%d" % s]) == to_text(F.trace_scene(s))
        rays = all_trace_rays(s)
        moved = c["moved_index_%d" % s]
        assert len(moved) <= 0.02 * len(rays)  # only rays the reference itself asserts on, at most 2 %
        np.testing.assert_array_equal(u32(t["rays_%d" % s]), u32(np.delete(rays, moved, axis=0)))
        np.testing.assert_array_equal(u32(c["moved_rays_%d" % s]), u32(rays[moved]))
    assert str(c["text"]) == to_text(F.cap_scene())
    np.testing.assert_array_equal(u32(c["rays"]), u32(F.cap_candidates()[c["index"]]))
    assert [int(v) for v in c["meta"]][:2] == [F.CAP_SPP, F.CAP_DEPTH]


def test_inputs_are_valid_scenes_and_rays():
    """lattice geometry, invertible transforms, finite rays with a direction; at most 14 primitives"""
    from pathtrace.scene import Plane, Sphere, count_primitives

    def walk(o):
        if isinstance(o, Sphere):
            assert float(o.r) in (0.5, 1.0, 1.5) and all(float(v) * 2 == int(float(v) * 2) for v in o.center)
        elif isinstance(o, Plane):
            assert float(o.d) * 2 == int(float(o.d) * 2)
        elif isinstance(o, TransformedObject):
            m = np.array([float(v) for v in o.matrix.m]).reshape(3, 4)[:, :3]
            assert abs(np.linalg.det(m)) > 0.1
        for ch in o.children():
            walk(ch)
    for _, b in TREES:
        walk(b())
    dets = [np.linalg.det(np.array([float(v) for v in m.m]).reshape(3, 4)[:, :3]) for _, m in F.XFORMS]
    assert min(dets) < 0 < max(dets)
    for s in range(F.N_TRACE_SCENES):
        root = F.trace_scene(s)
        assert count_primitives(root) <= 14 and 3 <= len(F.assembly_centres(s)) <= 5
        r = all_trace_rays(s)
        assert r.shape == (F.TRACE_RAYS, 7) and np.isfinite(r).all() and np.any(r[:, 3:6] != 0, axis=1).all()
        assert (r[:, 6] < 1e-3).any() and (r[:, 6] == 1).any()
    assert len(set(F.mode_scenes())) == 2


def test_census_conditions():
    """the reference's own span lists show the ties: every (operator, kind) cell has at least 20 rays,
    every tree has a span on a quarter of its rays, some ray has three spans or more"""
    z = gold("spans")
    assert z["census"].shape == (3, 4) and z["census"].min() >= 20, z["census"]
    longest = 0
    for k, name in enumerate(TREE_NAMES):
        counts = z["counts_%d" % k]
        assert (counts > 0).mean() >= 0.25, (name, int((counts > 0).sum()))
        longest = max(longest, int(counts.max()))
    assert longest >= 3
    for name in ("spans", "trace", "cap"):
        assert os.path.getsize(os.path.join(GOLD, "csgfuzz_%s.npz" % name)) <= 500 * 1000


def _census(root, rays, cells):
    if isinstance(root, TransformedObject) or not isinstance(root, _Binary):
        return
    la, lb = O.spans(to_text(root.a), rays), O.spans(to_text(root.b), rays)
    op = F.OPS.index(type(root))
    for sa, sb in zip(la, lb):
        a0, a1 = {float(s[0][0]) for s in sa}, {float(s[2][0]) for s in sa}
        b0, b1 = {float(s[0][0]) for s in sb}, {float(s[2][0]) for s in sb}
        for k, hit in enumerate((a0 & b0, a1 & b1, a1 & b0, b1 & a0)):
            cells[op, k] += bool(hit)
    _census(root.a, rays, cells)
    _census(root.b, rays, cells)


def test_oracle_census_equals_the_references(built):
    """the same count from the oracle's child span lists: the stored census is reproducible here"""
    z = gold("spans")
    cells = np.zeros((3, 4), dtype=np.int64)
    for k, (_, builder) in enumerate(TREES):
        _census(builder(), z["rays_%d" % k], cells)
    np.testing.assert_array_equal(cells, z["census"])


@pytest.mark.parametrize("k", range(len(TREES)), ids=TREE_NAMES)
def test_oracle_spans_match_reference(built, k):
    z = gold("spans")
    counts, rows = span_rows(O.spans(str(z["text_%d" % k]), z["rays_%d" % k]))
    np.testing.assert_array_equal(counts, z["counts_%d" % k])
    np.testing.assert_array_equal(rows, z["data_%d" % k])


@pytest.mark.parametrize("s", range(F.N_TRACE_SCENES))
def test_oracle_trace_rays_match_reference(built, s):
    z = gold("trace")
    spp, depth, seed = [int(v) for v in z["meta"]]
    got = O.trace_rays(str(z["text_%d" % s]), z["rays_%d" % s], spp, depth, seed=seed, order=O.ORDER_REFERENCE)
    np.testing.assert_array_equal(u32(got), u32(z["mean_%d" % s]))


def test_oracle_on_the_cap_rays(built):
    """each ray alone, as the reference ran it: the oracle takes the early return exactly where the
    reference's assertion fired, stays finite there, and equals the reference everywhere else"""
    z = gold("cap")
    spp, depth, seed = [int(v) for v in z["meta"]]
    aborts = z["aborts"]
    assert aborts.sum() >= 32 and (~aborts).sum() >= 96
    txt = str(z["text"])
    for k, ray in enumerate(z["rays"]):
        got, st = O.trace_rays(txt, ray[None], spp, depth, seed=seed, order=O.ORDER_REFERENCE, threads=1,
                               stats=True)
        assert (st["cap_returns"] > 0) == bool(aborts[k]), (k, st)
        assert np.isfinite(got).all(), k
        if not aborts[k]:
            np.testing.assert_array_equal(u32(got[0]), u32(z["mean"][k]), err_msg=str(k))
    for s in range(F.N_TRACE_SCENES):  # the trace scenes' rays the reference asserted on
        got = O.trace_rays(to_text(F.trace_scene(s)), all_trace_rays(s), TRACE_SPP, TRACE_DEPTH, seed=seed)
        assert np.isfinite(got).all()


def test_cap_render_reaches_the_cap(built):
    """the frame the GPU test renders: early returns happen in it, inside scatter bursts"""
    c = F.CAP_RENDER
    out, st = O.render(to_text(F.cap_scene(c["shift"])), c["W"], c["H"], c["spp"], c["depth"], stats=True)
    assert st["cap_returns"] > 0 and np.isfinite(out).all()


# --------------------------------------------------------------------- GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(TREES)), ids=TREE_NAMES)
def test_gpu_query_spans_match_reference(built, k):
    z = gold("spans")
    ds = pt.DeviceScene.from_text(to_text(TREES[k][1]()))  # material ids = the text's
    ms = max(int(z["counts_%d" % j].max()) for j in range(len(TREES)))
    counts, spans = ds.query_spans(z["rays_%d" % k], max_spans=ms)
    np.testing.assert_array_equal(counts, z["counts_%d" % k])
    rows = np.concatenate([spans[i, :c] for i, c in enumerate(counts)]).view(np.uint32)
    np.testing.assert_array_equal(rows, z["data_%d" % k])


@pytest.mark.gpu
@pytest.mark.parametrize("s", range(F.N_TRACE_SCENES))
def test_gpu_trace_rays_reference_order_bitexact(built, s):
    z = gold("trace")
    spp, depth, seed = [int(v) for v in z["meta"]]
    got = pt.trace_rays(F.trace_scene(s), z["rays_%d" % s], depth, spp=spp, seed=seed, order="reference")
    np.testing.assert_array_equal(u32(got), u32(z["mean_%d" % s]))


FAST_CASES = [(s, o) for s in range(F.N_TRACE_SCENES) for o in [{}] + (F.MODE_OPTS if s in F.mode_scenes() else [])]


@pytest.mark.gpu
@pytest.mark.parametrize("s,opts", FAST_CASES)
def test_gpu_trace_rays_fast_order_matches_oracle(built, s, opts):
    """every ray of the scene, the ones the reference asserts on included"""
    rays = all_trace_rays(s)
    root = F.trace_scene(s)
    got, st = pt.trace_rays(pt.DeviceScene(root, **opts), rays, TRACE_DEPTH, spp=3, order="fast", sample_begin=5,
                            ray_begin=1000, stats=True)
    want, ost = O.trace_rays(to_text(root), rays, 3, TRACE_DEPTH, sample_begin=5, order=O.ORDER_FAST,
                             ray_begin=1000, stats=True)
    np.testing.assert_array_equal(u32(got), u32(want))
    assert st["queries"] == ost["queries"]


@pytest.mark.gpu
def test_gpu_both_first_hit_paths_run(built):
    """a guard against a vacuous test: over the trace scenes some leaf queries take the fast first-hit
    path and some need the full merge.  Observed on an MI355X (reference order, spp 2, depth 3; queries /
    slow_queries per scene): 5 527 414 / 1 322 055, 5 565 324 / 1 525 744, 7 915 008 / 4 123 237,
    6 387 148 / 3 402 249, 8 405 166 / 3 335 644, 5 768 526 / 1 038 579 -- 39 568 586 / 14 747 508 in all."""
    q = slow = 0
    for s in range(F.N_TRACE_SCENES):
        z = gold("trace")
        _, st = pt.trace_rays(F.trace_scene(s), z["rays_%d" % s], TRACE_DEPTH, spp=TRACE_SPP, order="reference",
                              stats=True)
        q, slow = q + st["queries"], slow + st["slow_queries"]
        print("scene %d: queries %d, slow_queries %d" % (s, st["queries"], st["slow_queries"]))
    assert 0 < slow < q, (slow, q)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
@pytest.mark.parametrize("opts", CAP_OPTS, ids=["default", "lane_walk2", "lane_scatter"])
def test_gpu_cap_trace_rays_match_oracle(built, opts, order):
    z = gold("cap")
    spp, depth, seed = [int(v) for v in z["meta"]]
    root = F.cap_scene()
    got, st = pt.trace_rays(pt.DeviceScene(root, **opts), z["rays"], depth, spp=spp, seed=seed, order=order,
                            stats=True)
    want, ost = O.trace_rays(to_text(root), z["rays"], spp, depth, seed=seed, stats=True,
                             order=O.ORDER_FAST if order == "fast" else O.ORDER_REFERENCE)
    assert ost["cap_returns"] > 0
    np.testing.assert_array_equal(u32(got), u32(want))
    assert st["queries"] == ost["queries"], (st["queries"], ost["queries"])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
def test_gpu_cap_render_matches_oracle(built, order):
    """the early returns of this frame happen inside a parent's burst (test_cap_render_reaches_the_cap)"""
    c = F.CAP_RENDER
    root = F.cap_scene(c["shift"])
    got, st = pt.render(root, c["W"], c["H"], c["spp"], c["depth"], order=order, stats=True)
    want, ost = O.render(to_text(root), c["W"], c["H"], c["spp"], c["depth"], stats=True,
                         order=O.ORDER_FAST if order == "fast" else O.ORDER_REFERENCE)
    np.testing.assert_array_equal(u32(got.reshape(-1, 3)), u32(want))
    assert st["queries"] == ost["queries"], (st["queries"], ost["queries"])
