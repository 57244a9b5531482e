"""User-defined Object subclasses with several spans per ray on the device
(reference include/object.h:14-20: makeSpanIterator returns any SpanIterator).
A caller gives up to PT_OBJECT_MAX_SPANS ordered, strictly separated spans and
their normals as device source through pt_object_device_spans; the node
(path-trace_amd/csrc/device/pt_user_object_n.h) takes one primitive slot per
span and joins every CSG node and transform like that many built-in
primitives.  The oracle cannot host such a node, so each user object has a
built-in twin whose arithmetic its bodies restate (tests/multispan.py): the
user scene must give the twin's bits on the GPU and the oracle's bits of the
twin's to_text -- frames in both summation orders, with the select-form pull
(lane_walk) and the spine's fast checks (fast_spine) over the K slots, with
slack slots, span by span through pt_query_spans, and on caller rays through
pt_trace_rays."""
import os
import subprocess

import numpy as np
import pytest

import pathtrace as pt
from pathtrace.scene import DeviceSpansObject, Plane, Union, to_text

import multispan as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "path-trace_amd", "lib")
W, H, SPP, DEPTH = 48, 32, 4, 6
OPTIONS = [{"lane_walk": 1}, {"fast_spine": True}]
MAX_SPANS = 8  # PT_OBJECT_MAX_SPANS (include/pt/pt.h)

# one span through the span-list signatures: src/sphere.cpp:31-49 (prm: center, r*r)
ONE_SPANS = """
    const V3 oc = mk(o.x - prm[0], o.y - prm[1], o.z - prm[2]);
    const float a = dot(d, d);
    const float b = dot(oc, d);
    const float disc = b * b - a * (dot(oc, oc) - prm[3]);
    if (disc <= 1e-3f)
        return 0;
    const float s = sqrtf(disc);
    t0[0] = (-b - s) / a, t1[0] = (-b + s) / a;
    return 1;
"""
ONE_NORMAL = """
    const V3 q = mk(p.x - prm[0], p.y - prm[1], p.z - prm[2]);
    float m = sqrtf(dot(q, q));
    if (m == 0.0f)
        m = 1.0f;
    return mk(q.x / m, q.y / m, q.z / m);
"""


def one_span_scene():
    m = M.mats()
    return Union(DeviceSpansObject(ONE_SPANS, ONE_NORMAL, (0, 0, -4, 0.25), m["diffuse"], 1),
                 Plane((0, 1, 0), .5, m["emitW"]))


def _floor(obj):
    return Union(obj, Plane((0, 1, 0), .5, M.mats()["emitW"]))


# ------------------------------------------------------------------ CPU ---
def test_multi_zoo_compiles_into_its_own_module(built):
    user = pt.DeviceScene(M.multi_zoo(True)).compile(DEPTH)
    assert user != pt.DeviceScene(M.multi_zoo(False)).compile(DEPTH)


def test_query_and_ray_modules_compile(built):
    pt.DeviceScene(M.multi_zoo(True)).compile_queries()
    pt.DeviceScene(M.multi_zoo(True)).compile_rays(DEPTH)


def test_body_error_is_a_compile_error(built):
    bad = DeviceSpansObject("return nope;", M.SHELL_NORMAL, (0, 0, -4, 0.25, 0.09, 0.5, 0.3), M.mats()["diffuse"], 2)
    with pytest.raises(pt.PtError, match="nope"):
        pt.DeviceScene(_floor(bad)).compile(4)


@pytest.mark.parametrize("spans,normal", [("", M.SHELL_NORMAL), (M.SHELL_SPANS, "")])
def test_rejects_empty_bodies(built, spans, normal):
    with pytest.raises(pt.PtError, match="pt_object_device_spans"):
        pt.DeviceScene(DeviceSpansObject(spans, normal, (), M.mats()["diffuse"], 2))


@pytest.mark.parametrize("k", [0, MAX_SPANS + 1])
def test_rejects_max_spans_out_of_range(built, k):
    with pytest.raises(pt.PtError, match="pt_object_device_spans"):
        pt.DeviceScene(DeviceSpansObject(M.SHELL_SPANS, M.SHELL_NORMAL, (0, 0, -4, 0.25, 0.09, 0.5, 0.3),
                                         M.mats()["diffuse"], k))


@pytest.mark.parametrize("nparams,mat", [(3, 0), (0, 99)], ids=["null-parameter-block", "bad-material"])
def test_c_abi_rejects_bad_block_and_material(built, nparams, mat):
    L = pt._lib.lib()
    h = L.pt_scene_create()
    try:
        with pytest.raises(pt.PtError, match="pt_object_device_spans"):
            pt._lib.check(L.pt_object_device_spans(h, M.SHELL_SPANS.encode(), M.SHELL_NORMAL.encode(), None, nparams,
                                                   2, mat))
    finally:
        L.pt_scene_destroy(h)


def test_max_spans_in_range_is_accepted(built):
    """1 and PT_OBJECT_MAX_SPANS flatten; one span through the new signatures compiles"""
    pt.DeviceScene(M.shell_scene(True, MAX_SPANS))
    pt.DeviceScene(one_span_scene()).compile(DEPTH)


def test_to_text_names_the_class():
    with pytest.raises(ValueError, match="DeviceSpansObject"):
        to_text(M.multi_zoo(True))


def test_duplicate_keeps_every_field():
    a = M.shell(M.GLASS_C, 0.5, 0.3, M.mats()["glass"], True, 4)
    b = a.duplicate()
    assert b is not a and isinstance(b, DeviceSpansObject)
    assert (b.spans_body, b.normal_body, b.params, b.material, b.max_spans) == \
        (a.spans_body, a.normal_body, a.params, a.material, 4)


@pytest.fixture(scope="module")
def facade_bin(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("facade_ms") / "facade_multispan")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "facade_multispan.cpp"),
                    "-L" + LIBDIR, "-lpt", "-Wl,-rpath," + LIBDIR, "-o", out], check=True)
    return out


def test_facade_flattens_like_python_mirror(facade_bin):
    """Object subclasses overriding deviceSpans generate the Python mirror's module"""
    r = subprocess.run([facade_bin, "key", str(DEPTH)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == pt.DeviceScene(M.multi_zoo(True)).compile(DEPTH)


# ------------------------------------------------------------------ GPU ---
@pytest.fixture(scope="module")
def oracle_frames(built, tmp_path_factory):
    """the oracle's frames of multi_zoo's built-in twin, by summation order"""
    import oracle_py as O
    txt = to_text(M.multi_zoo(False), str(tmp_path_factory.mktemp("ms_img")))
    return {"fast": O.render(txt, W, H, SPP, DEPTH, order=O.ORDER_FAST),
            "reference": O.render(txt, W, H, SPP, DEPTH, order=O.ORDER_REFERENCE)}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3)).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
def test_multi_zoo_frame_is_the_twins(oracle_frames, order):
    user = pt.render(pt.DeviceScene(M.multi_zoo(True)), W, H, SPP, DEPTH, order=order)
    twin = pt.render(pt.DeviceScene(M.multi_zoo(False)), W, H, SPP, DEPTH, order=order)
    assert np.any(np.asarray(user) != 0)
    np.testing.assert_array_equal(_bits(user), _bits(twin))
    np.testing.assert_array_equal(_bits(user), _bits(oracle_frames[order]))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["fast", "reference"])
@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "-".join(o))
def test_multi_zoo_options_same_frame(oracle_frames, opts, order):
    """lane_walk: the select-form pulls walk the K slots; fast_spine: the spine's fast checks see them"""
    user = pt.render(pt.DeviceScene(M.multi_zoo(True), **opts), W, H, SPP, DEPTH, order=order)
    assert np.any(np.asarray(user) != 0)
    np.testing.assert_array_equal(_bits(user), _bits(oracle_frames[order]))


@pytest.mark.gpu
def test_slack_slots_change_nothing(built):
    """the shell declared with max_spans=4 (two slots never live) renders the max_spans=2 frame"""
    a = pt.render(pt.DeviceScene(M.shell_scene(True, 4)), W, H, SPP, DEPTH)
    b = pt.render(pt.DeviceScene(M.shell_scene(True, 2)), W, H, SPP, DEPTH)
    assert np.any(np.asarray(a) != 0)
    np.testing.assert_array_equal(_bits(a), _bits(b))


@pytest.mark.gpu
def test_multi_zoo_span_queries(built, tmp_path):
    """Object::makeSpanIterator over multi_zoo on the device (pt_query_spans)
    against the oracle's span lists of the twin: counts, start / end t and
    normals; the rays must leave the single-span case often"""
    import oracle_py as O
    rays = M.query_rays(256)
    want = O.spans(to_text(M.multi_zoo(False), str(tmp_path)), rays)
    n = np.array([len(w) for w in want])
    assert (n >= 2).sum() >= 32 and (n >= 3).sum() >= 1
    counts, spans = pt.DeviceScene(M.multi_zoo(True)).query_spans(rays)
    np.testing.assert_array_equal(counts, n)
    for k, w in enumerate(want):
        for j, (a, _, b, _) in enumerate(w):  # start t + normal, end t + normal (material ids aside)
            np.testing.assert_array_equal(spans[k, j, 0:4].view(np.uint32), a.view(np.uint32))
            np.testing.assert_array_equal(spans[k, j, 5:9].view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_trace_rays_same_as_twin(built):
    """traceRay on caller rays (pt_trace_rays) through the span lists: the twin's means bit for bit"""
    rays = M.query_rays(256)
    user = pt.trace_rays(pt.DeviceScene(M.multi_zoo(True)), rays, DEPTH, spp=SPP)
    twin = pt.trace_rays(pt.DeviceScene(M.multi_zoo(False)), rays, DEPTH, spp=SPP)
    assert np.any(user != 0)
    np.testing.assert_array_equal(_bits(user), _bits(twin))


@pytest.mark.gpu
def test_facade_render_bitexact(facade_bin, tmp_path):
    out = str(tmp_path / "img.bin")
    r = subprocess.run([facade_bin, "render", str(W), str(H), str(SPP), str(DEPTH), out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.float32).reshape(-1, 3)
    want = pt.render(M.multi_zoo(True), W, H, SPP, DEPTH)
    assert np.any(got != 0)
    np.testing.assert_array_equal(got.view(np.uint32), _bits(want))
