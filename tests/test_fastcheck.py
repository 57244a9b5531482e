"""The CSG fast check (pt_device.h fast_ok / pair_ok / fast_first_hit) on the seam of two spheres.

Where every pair of positive primitive spans passes pair_ok, the burst passes and the spine and lane
queries take fast_first_hit over the primitives' own spans in place of the lazy merges.  An origin on the
circle where two overlapping spheres meet is where that goes wrong most easily: one sphere's span ends at
the origin (inert), the other's straddles it, and under Difference(Union(x1, x2), y) a subtractor y wholly
behind the origin still reaches the merged span [x1.t0, x2.t1] and inverts it (src/difference.cpp:124-130)
while every pair passed.  8 pixels of the C3 bench frame lost terms to it
(profiles/round10/frame_diff_passes.txt).  The lens of an Intersection that ends before EPS does the same
harm below a Difference -- as the B span of Difference(y, Intersection(x1, x2)) it inverts a y that starts
inside it -- and no pair check sees it, since an Intersection's primitives are not positive.  With the
header's rule as it stood (fastcheck's "inert_everywhere") the property test below fails on 17 of
dif_uni_a's 384 rays, 3 of dif_int_b's and 16 of c3_seam_rays' 4096 (the 5 found rays among them), and on
no other tree; tools/fastcheck_model.py counts the variants over 10^6 rays.  pair_ok now takes no inert
span at a Union below a Difference, and an Intersection below a Difference must be empty.

CPU: tests/fastcheck.py restates the check in float32.  On every ray where its fast_ok holds,
fast_first_hit must equal traceRay's scan of the root span list in hit / miss, t bits and material -- over
the seam trees against the unmodified reference's lists (tests/golden/fastcheck_seam.npz, frozen by
tests/golden/make_fastcheck_golden.py; the CPU oracle's lists equal them bit for bit) and over
fastcheck.c3_seam_rays against the oracle's.  The census keeps the test from being vacuous; for the
Difference-outer trees it counts rays whose reference list holds an inverted span while the own span of a
primitive below no B side reaches EPS (an inner Intersection has no positive primitive, so the census
takes its operands).  pair_ok's text in the header is pinned to the string the model was written from.

GPU, bit for bit against the oracle: every seam scene through pt.trace_rays with rays aimed from outside
at the seam (depth 3, spp 4, both orders, the lane-resume form on and off), a 48 x 27 frame of the
minimal-case scene, and the 8 pixels of the C3 frame with their x-neighbours at 1024 spp against
tests/golden/render_c3_seam.npz.

The modules are listed in tests/precompile_fastcheck.py."""
import os
import re

import numpy as np
import pytest

import fastcheck as C
import oracle_py as O
import pathtrace as pt
from pathtrace import scenes
from pathtrace.scene import to_text

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
HEADER = os.path.join(os.path.dirname(HERE), "path-trace_amd", "csrc", "device", "pt_device.h")
SEAM_RAYS = 384
MIN_CENSUS = 20
TRACE_DEPTH, TRACE_SPP = 3, 4
ORDERS = {"reference": O.ORDER_REFERENCE, "fast": O.ORDER_FAST}
NAMES = C.seam_names()
DIFF_OUTER = [n for n in NAMES if n.startswith("dif_")]
_cache = {}


def gold(name="fastcheck_seam.npz"):
    if name not in _cache:
        with np.load(os.path.join(GOLD, name)) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def trees():
    if "trees" not in _cache:
        _cache["trees"] = {name: root for name, _, root in C.seam_trees()}
    return _cache["trees"]


def lists(name):
    z = gold()
    return z["cnt_" + name].astype(np.int32), z["t_" + name], z["m_" + name].astype(np.int16)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# --------------------------------------------------------------------- CPU ---
def test_fixture_is_the_generators_input():
    z = gold()
    for k, name in enumerate(NAMES):
        assert str(z["text_" + name]) == to_text(trees()[name]), name
        rays = C.seam_rays(trees()[name], k, SEAM_RAYS)
        np.testing.assert_array_equal(u32(z["rays_" + name]), u32(rays))
        a = C.dot(rays[1:, 3:6], rays[1:, 3:6])
        assert np.all(np.abs(a - 1) <= 2.0 ** -20), name  # unit child rays
    np.testing.assert_array_equal(z["rays_" + C.MINIMAL][0], C.MINIMAL_RAY[0])
    assert os.path.getsize(os.path.join(GOLD, "fastcheck_seam.npz")) <= 500 * 1000


@pytest.mark.parametrize("name", NAMES)
def test_oracle_spans_equal_the_reference(built, name):
    z = gold()
    cnt, t, m = C.span_arrays(O.spans(str(z["text_" + name]), z["rays_" + name]))
    wc, wt, wm = lists(name)
    np.testing.assert_array_equal(cnt, wc)
    np.testing.assert_array_equal(u32(t), u32(wt))
    np.testing.assert_array_equal(m, wm)


def test_minimal_case():
    """Difference(Union(x1, x2), y), spans [-2, 0], [-0.5, 1.5], [-3, -1]: the reference's root list is the
    one inverted span [-2, -3]; with inert at every Union every pair passes and the exit at 1.5 is reported"""
    root = trees()[C.MINIMAL]
    cnt, t, m = lists(C.MINIMAL)
    assert cnt[0] == 1 and t[0].tolist() == [-2.0, -3.0]
    assert C.scan(C.span_lists(cnt[:1], t, m)[0]) == (False, 0.0, -1)
    ps = C.PrimSpans(root, C.MINIMAL_RAY)
    assert ps.t0[:3, 0].tolist() == [-2.0, -0.5, -3.0] and ps.t1[:3, 0].tolist() == [0.0, 1.5, -1.0]
    assert ps.live[:3, 0].all() and not ps.live[3:, 0].any()  # the ray is parallel to ground and wall
    hit, tf, mf = C.fast_first_hit(root, ps)
    assert hit[0] and tf[0] == 1.5 and mf[0] == 1
    assert C.fast_ok(root, ps, "inert_everywhere")[0] and C.fast_ok(root, ps, "no_diff_inert")[0]
    assert not C.fast_ok(root, ps)[0] and not C.fast_ok(root, ps, "no_union_inert")[0]


@pytest.mark.parametrize("name", NAMES)
def test_fast_first_hit_is_the_scan_on_the_seam_trees(name):
    root, rays = trees()[name], gold()["rays_" + name]
    cnt, t, m = lists(name)
    bad, ok = C.disagreements(root, rays, cnt, t, m)
    quirk = C.inverted(cnt, t) & C.reaches(root, C.PrimSpans(root, rays))
    print("%s: %d pass fast_ok, %d fail, %d inverted with a span reaching EPS, %d disagree" % (
        name, ok.sum(), (~ok).sum(), quirk.sum(), bad.sum()))
    assert not bad.any(), np.flatnonzero(bad)
    # not vacuous
    assert ok.sum() >= MIN_CENSUS and (~ok).sum() >= MIN_CENSUS
    if name in DIFF_OUTER:
        assert quirk.sum() >= MIN_CENSUS
    # the scan of the list of tuples is the scan of the arrays
    h, ts, ms = C.scan_arrays(cnt, t, m)
    for i, sp in enumerate(C.span_lists(cnt, t, m)[:64]):
        assert C.scan(sp) == (bool(h[i]), ts[i], int(ms[i]))


def c3_lists():
    if "c3" not in _cache:
        root, rays = scenes.scene_p1(), C.c3_seam_rays(0)
        _cache["c3"] = (root, rays) + C.span_arrays(O.spans(to_text(root), rays))
    return _cache["c3"]


def test_fast_first_hit_is_the_scan_on_c3(built):
    root, rays, cnt, t, m = c3_lists()
    bad, ok = C.disagreements(root, rays, cnt, t, m)
    print("C3: %d pass fast_ok, %d fail, %d disagree" % (ok.sum(), (~ok).sum(), bad.sum()))
    assert not bad.any(), rays[bad]
    assert ok.sum() >= MIN_CENSUS and (~ok).sum() >= MIN_CENSUS
    assert not ok[:len(C.C3_FOUND)].any()  # the found rays take the merge


def test_inert_at_every_union_is_unsound(built):
    """the rule before the fix: the model must see what the device did"""
    root, rays = trees()[C.MINIMAL], gold()["rays_" + C.MINIMAL]
    bad, _ = C.disagreements(root, rays, *lists(C.MINIMAL), rule="inert_everywhere")
    assert bad[0] and bad.sum() >= 10
    name = "dif_int_b"  # the lens that ends before EPS, as a B span
    for rule in ("inert_everywhere", "no_union_inert", "lens_before_eps"):
        assert C.disagreements(trees()[name], gold()["rays_" + name], *lists(name), rule=rule)[0].any(), rule
    root, rays, cnt, t, m = c3_lists()
    bad, _ = C.disagreements(root, rays, cnt, t, m, rule="inert_everywhere")
    assert bad[:len(C.C3_FOUND)].all() and bad[len(C.C3_FOUND):].any()
    h, ts, _ = C.scan_arrays(cnt, t, m)
    # the oracle's list of the first found ray: an inverted span, then the sky wall, where the scan stops
    assert cnt[0] == 2 and t[0, 1] < t[0, 0] and h[0] and ts[0] > 200


def test_pair_ok_text_is_the_models():
    """a later edit of the rule fails here until tests/fastcheck.py follows"""
    text = open(HEADER).read()
    m = re.search(r"__device__ __forceinline__ int pair_ok\(const PS &ps, int x, int y\)\s*\{(.*?)\n\}", text, re.S)
    assert m, "pair_ok not found"
    assert " ".join(m.group(1).split()) == C.PAIR_OK_BODY
    assert "template <int KIND, bool D = false, class PS>\n__device__ __forceinline__ int pair_ok" in text
    # D is set on both sides of a Difference and handed down unchanged everywhere else
    assert ("A::template fast_ok<PS, D || KIND == NODE_DIFF>(ps) & "
            "B::template fast_ok<PS, D || KIND == NODE_DIFF>(ps)") in text
    assert "pair_ok<KIND, D>(ps, decltype(x)::value, decltype(y)::value)" in text
    assert "int fast_ok(const PS &ps) { return C::template fast_ok<PS, D>(ps); }" in text  # transforms
    apart = re.search(r"int apart\(const PS &ps, int x, int y\)\s*\{(.*?)\n\}", text, re.S)
    assert " ".join(apart.group(1).split()) == (
        "return (!ps.live[x]) | (!ps.live[y]) | (ps.t1[x] < ps.t0[y]) | (ps.t1[y] < ps.t0[x]);")
    sep = re.search(r"int sep\(const PS &ps, int x, int y\)\s*\{(.*?)\n\}", text, re.S)
    assert " ".join(sep.group(1).split()) == "return apart(ps, x, y) | ((ps.t1[x] < EPS) & (ps.t1[y] < EPS));"
    ine = re.search(r"int inert\(const PS &ps, int x\)\s*\{(.*?)\n\}", text, re.S)
    assert " ".join(ine.group(1).split()) == "return ps.live[x] & (ps.t1[x] < EPS);"


def test_c3_fixture_pixel_from_the_oracle(built):
    z = gold("render_c3_seam.npz")
    cfg = scenes.CONFIGS["C3"]
    assert z["pixels"].tolist() == C.C3_PIXELS and len(C.C3_PIXELS) == 24
    assert z["meta"].tolist() == [cfg.width, cfg.height, C.C3_SPP, C.C3_DEPTH]
    k = C.C3_PIXELS.index(C.C3_BAD[1])
    got = O.render(to_text(cfg.scene()), cfg.width, cfg.height, C.C3_SPP, C.C3_DEPTH, pixels=[C.C3_BAD[1]],
                   order=O.ORDER_FAST)
    np.testing.assert_array_equal(u32(got[0]), u32(z["mean"][k]))
    assert abs(float(z["mean"][k, 0]) - 0.00049044343) < 1e-9  # the profile's oracle value of pixel 1081685


# --------------------------------------------------------------------- GPU ---
def oracle_trace(name, order):
    key = ("trace", name, order)
    if key not in _cache:
        rays = C.aimed_rays(trees()[name], NAMES.index(name))
        _cache[key] = (rays,) + O.trace_rays(to_text(trees()[name]), rays, TRACE_SPP, TRACE_DEPTH,
                                             order=ORDERS[order], stats=True)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("resume", [1, 0], ids=["lane_resume", "no_lane_resume"])
@pytest.mark.parametrize("order", ["reference", "fast"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_seam_scene_rays(built, name, order, resume):
    rays, want, wst = oracle_trace(name, order)
    got, st = pt.trace_rays(pt.DeviceScene(C.seam_trees_scene(name), lane_resume=resume), rays, TRACE_DEPTH,
                            spp=TRACE_SPP, order=order, stats=True)
    np.testing.assert_array_equal(u32(got), u32(want))
    assert st["queries"] == wst["queries"]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["reference", "fast"])
def test_gpu_seam_frame(built, order):
    c = C.SEAM_FRAME
    root = C.seam_trees_scene(C.MINIMAL)
    want, wst = O.render(to_text(root), c["W"], c["H"], c["spp"], c["depth"], screen=c["screen"],
                         order=ORDERS[order], stats=True)
    got, st = pt.render(root, c["W"], c["H"], c["spp"], c["depth"], screen=c["screen"], order=order, stats=True)
    np.testing.assert_array_equal(u32(got).reshape(-1, 3), u32(want).reshape(-1, 3))
    assert st["queries"] == wst["queries"]


@pytest.mark.gpu
def test_gpu_c3_seam_pixels(built):
    """the 8 pixels of the bench frame that were not the oracle's, and their x-neighbours"""
    z = gold("render_c3_seam.npz")
    cfg = scenes.CONFIGS["C3"]
    got, st = pt.render(cfg.device_scene(), cfg.width, cfg.height, C.C3_SPP, C.C3_DEPTH, pixels=C.C3_PIXELS,
                        order="fast", stats=True)
    print("mid_queries %d, slow_queries %d" % (st["mid_queries"], st["slow_queries"]))
    # the fast check ran, and so did the merge
    assert st["mid_queries"] > st["slow_queries"] > 0
    differ = np.flatnonzero((u32(got).reshape(-1, 3) != u32(z["mean"])).any(axis=1))
    assert differ.size == 0, [C.C3_PIXELS[i] for i in differ]
    assert st["queries"] == int(z["queries"])
