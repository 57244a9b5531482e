"""First-hit queries and guide buffers without a GPU: pt_query_hits and pt_render_guides check every
argument before they touch a device (a late check would surface as PT_ERR_DEVICE here) and name it in
pt_last_error(); the guides module compiles for gfx950 into the code-object cache; and compiling it
leaves the keys of the scene's render, ray-list and chained modules what they were -- it is a module kind
of its own (path-trace_amd/csrc/device/pt_guides.h), so no profile bound to those keys loses its code."""
import ctypes

import numpy as np
import pytest

import multispan as M
import pathtrace as pt
import zoo
from pathtrace import _lib

PT_ERR_ARG = -1
DEPTH = 8
RAY = [0, 0, 0, 0.1, 0.2, -1]


def p1():
    return pt.DeviceScene(zoo.build("scene_p1"))


def query(rays=RAY, n=None, path=_lib.PT_HIT_FAST, null=()):
    """pt_query_hits on scene_p1 with one bad argument; returns (status, pt_last_error())"""
    L, ds = _lib.lib(), p1()
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = len(r) if n is None else n
    out = np.zeros(max(n, 1), dtype=_lib.HIT_DTYPE)
    rc = L.pt_query_hits(ds.handle, None if "rays" in null else r.ctypes.data, n, path,
                         None if "out" in null else out.ctypes.data, None, None, 0)
    return rc, L.pt_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(null=("rays",)), "rays is null"),
    (dict(null=("out",)), "out is null"),
    (dict(n=-1), "n must be"),
    (dict(path=2), "path"),
    (dict(path=-1), "path"),
    (dict(rays=[RAY, [0, float("nan"), 0, 0, 0, -1]]), "rays[1]"),
    (dict(rays=[[float("inf"), 0, 0, 0, 0, -1]]), "rays[0]"),
    (dict(rays=[RAY, RAY, [0, 0, 0, 0, float("-inf"), -1]]), "rays[2]"),
    (dict(rays=[RAY, [1, 2, 3, 0, -0.0, 0]]), "rays[1] has a zero direction"),
])
def test_query_arguments_are_checked_before_the_device(built, kw, name):
    rc, msg = query(**kw)
    assert rc == PT_ERR_ARG, (rc, msg)
    assert "pt_query_hits" in msg and name in msg, msg


def guides(null=(), planes=("emission", "t"), **kw):
    """pt_render_guides on scene_p1 with one bad argument; returns (status, pt_last_error())"""
    L, ds = _lib.lib(), p1()
    args = dict(width=8, height=4, spp=2)
    args.update(kw)
    p, keep = pt.make_params(args.pop("width"), args.pop("height"), args.pop("spp"), 0, **args)
    n = max(1, len(keep) if keep is not None else max(p.width, 1) * max(p.height, 1))
    gb, hold = _lib.GuideBuffers(), []
    for name in planes:
        hold.append(np.zeros((n, 3), dtype=np.float32))
        setattr(gb, name, hold[-1].ctypes.data)
    rc = L.pt_render_guides(ds.handle, None if "p" in null else ctypes.byref(p),
                            None if "out" in null else ctypes.byref(gb))
    return rc, L.pt_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(null=("p",)), "p is null"),
    (dict(null=("out",)), "out is null"),
    (dict(planes=()), "out has every plane null"),
    (dict(pixels=[0, 32]), "p->pixels[1]"),                  # 8 x 4 frame
    (dict(pixels=[3, 4, -1]), "p->pixels[2]"),
    (dict(pixels=[-5], grid_width=9), "p->pixels[0]"),
    (dict(width=0), "width"),
    (dict(spp=0), "spp"),
    (dict(grid_width=4), "grid_width"),
])
def test_guides_arguments_are_checked_before_the_device(built, kw, name):
    rc, msg = guides(**kw)
    assert rc == PT_ERR_ARG, (rc, msg)
    assert "pt_render_guides" in msg and name in msg, msg


def test_good_arguments_reach_the_device(built):
    """the control of the tests above: with nothing wrong the calls get past their checks (and, on a
    machine without a GPU, fail at the device); the arguments pt_render_guides ignores are not checked"""
    rc, msg = query()
    assert rc != PT_ERR_ARG, msg
    rc, msg = guides(order=7, max_buffer_bytes=-1, sum_only=True, pixels=[40], grid_width=9)
    assert rc != PT_ERR_ARG, msg


def test_empty_inputs_touch_no_device(built):
    assert query(rays=np.zeros((0, 6)))[0] == 0
    assert guides(pixels=[])[0] == 0


SCENES = {"p1": lambda: zoo.build("scene_p1"), "csg": zoo.csg_zoo, "shell": lambda: M.shell_scene(True)}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_guides_module_compiles_and_moves_no_key(built, name):
    ds = pt.DeviceScene(SCENES[name]())
    kinds = [dict(), dict(rays=True), dict(chain=True)]
    before = [ds.module_key(DEPTH, **k) for k in kinds]
    key = ds.compile_guides()
    assert len(key) == 16 and key == ds.guides_key() and key not in before
    assert [ds.module_key(DEPTH, **k) for k in kinds] == before
