"""Chained rendering without a GPU: the chained modules compile for gfx950 and
have code-object keys of their own, the render modules keep the keys they had
before the chained kind existed, and pt_trace_chains checks its arguments
before it touches a device."""
import ctypes

import numpy as np
import pytest

import pathtrace as pt
import zoo
from pathtrace import _lib

PT_ERR_ARG = -1
# pt_scene_kernel_key of the two fixture scenes, generated from the header without its PT_CHAIN regions:
# the chained module kind does not change the text a render module is generated from.  (At the commit
# before that kind the keys were db0f1a47f6cdbf02 / 9071001ab7d9e4bb; the header's pair rules changed
# since -- tests/test_fastcheck.py -- and the keys with them.)
PARENT_KEYS = {("scene_p1", 8): "0d42b82b4b012bac", ("csg_zoo", 6): "fddc84e561b76751"}


@pytest.mark.parametrize("builder,depth,rays", [("scene_p1", 8, False), ("scene_p1", 8, True), ("csg_zoo", 6, False)])
def test_chain_modules_compile_without_a_device(built, builder, depth, rays):
    ds = pt.DeviceScene(zoo.build(builder))
    ds.compile_chain(depth, rays)
    keys = {ds.kernel_key(depth), ds.module_key(depth, rays=True), ds.module_key(depth, chain=True),
            ds.module_key(depth, rays=True, chain=True)}
    assert len(keys) == 4, keys  # render, ray-list, chained pixels, chained rays: four code objects
    assert ds.module_key(depth) == ds.kernel_key(depth)


@pytest.mark.parametrize("builder,depth", sorted(PARENT_KEYS))
def test_render_keys_are_the_parents(built, builder, depth):
    assert pt.DeviceScene(zoo.build(builder)).kernel_key(depth) == PARENT_KEYS[(builder, depth)]


def test_chain_module_ignores_lane_walk_options(built):
    """a scene that asks for a lane walk, the scatter walk or unsplit launches gets the chained module
    of the plain scene (pt_scene_set_lane_resume's rule)"""
    root = zoo.build("scene_p1")
    plain = pt.DeviceScene(root).module_key(8, chain=True)
    for kw in (dict(lane_walk=4), dict(lane_scatter=True), dict(split=False)):
        assert pt.DeviceScene(root, **kw).module_key(8, chain=True) == plain, kw


RAYS = np.array([[0, 0, 0, 0, 0, -1, 1], [0, 0, 0, 0.1, 0, -1, 1]], dtype=np.float32)


def bad_ray(row, col, value):
    r = RAYS.copy()
    r[row, col] = value
    return r


def call(pixels=None, rays=None, begin=(0, 2), nchains=1, **kw):
    """pt_trace_chains with one bad argument; returns (status, pt_last_error())"""
    L = _lib.lib()
    ds = pt.DeviceScene(zoo.build("scene_p1"))
    p = _lib.ChainParams()
    p.width, p.height, p.spp, p.depth = kw.get("width", 8), kw.get("height", 4), kw.get("spp", 2), kw.get("depth", 8)
    p.screen_w, p.screen_h, p.screen_dist, p.device = 8.0, 4.0, 8.0, 0
    pix = None if pixels is None else np.ascontiguousarray(pixels, dtype=np.int32)
    ray = None if rays is None else np.ascontiguousarray(rays, dtype=np.float32)
    b = np.ascontiguousarray(begin, dtype=np.int64)
    states = np.zeros(max(1, nchains), dtype=np.uint64)
    out, after = np.zeros((16, 3), dtype=np.float32), np.zeros(16, dtype=np.uint64)
    rc = L.pt_trace_chains(ds.handle, ctypes.byref(p), None if pix is None else pix.ctypes.data,
                           None if ray is None else ray.ctypes.data, b.ctypes.data, nchains, states.ctypes.data,
                           out.ctypes.data, after.ctypes.data, None)
    return rc, L.pt_last_error().decode()


@pytest.mark.parametrize("kw,names", [
    (dict(pixels=[0, 1], rays=RAYS), ("pixels", "rays")),                    # both
    (dict(), ("pixels", "rays")),                                            # neither
    (dict(pixels=[0, 1], begin=(1, 2)), ("begin[0]",)),
    (dict(pixels=[0, 1, 2], begin=(0, 2, 1, 3), nchains=3), ("begin", "chain 1")),
    (dict(pixels=[0, 32]), ("pixels[1]",)),                                  # 8 x 4 frame
    (dict(pixels=[-1, 0]), ("pixels[0]",)),
    (dict(rays=bad_ray(1, 3, np.inf)), ("rays[1]", "non-finite")),           # a direction component
    (dict(rays=bad_ray(0, 1, np.nan)), ("rays[0]", "non-finite")),           # an origin component
    (dict(pixels=[0, 1], spp=0), ("spp",)),
    (dict(pixels=[0, 1], depth=-1), ("depth",)),
])
def test_arguments_are_checked_before_the_device(built, kw, names):
    rc, msg = call(**kw)
    assert rc == PT_ERR_ARG, (rc, msg)
    for n in names:
        assert n in msg, msg


def test_empty_chains_touch_no_device(built):
    """nothing to run: PT_OK without a device, the states as given"""
    L = _lib.lib()
    ds = pt.DeviceScene(zoo.build("scene_p1"))
    p = _lib.ChainParams()
    p.width, p.height, p.spp, p.depth = 8, 4, 2, 8
    begin = np.zeros(4, dtype=np.int64)
    states = np.array([5, 6, 7], dtype=np.uint64)
    pix = np.zeros(1, dtype=np.int32)
    rc = L.pt_trace_chains(ds.handle, ctypes.byref(p), pix.ctypes.data, None, begin.ctypes.data, 3,
                           states.ctypes.data, None, None, None)
    assert rc == 0, L.pt_last_error()
    assert list(states) == [5, 6, 7]
