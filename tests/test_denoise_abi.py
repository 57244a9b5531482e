"""pt_denoise without a GPU: every argument is checked before a device is touched (a late check would
surface as PT_ERR_DEVICE here) and named in pt_last_error(), for the host and the device variant alike;
the module compiles for gfx950 into the code-object cache; and it is a module kind of its own
(path-trace_amd/csrc/device/pt_denoise.h), so the keys of the scenes' render and guides modules are what
they were before it was compiled."""
import ctypes

import numpy as np
import pytest

import pathtrace as pt
import zoo
from pathtrace import _lib

PT_ERR_ARG = -1
W, H = 6, 4
PLANES = ("rgb", "err", "normal", "t", "material", "albedo", "emission", "out", "var_out")


def call(null=(), device_variant=False, no_p=False, no_b=False, **kw):
    """pt_denoise on a 6 x 4 frame of zeros with one bad argument; returns (status, pt_last_error())"""
    L = _lib.lib()
    args = dict(width=W, height=H, device=0)
    args.update({k: kw.pop(k) for k in ("width", "height", "device") if k in kw})
    p = pt.denoise_params(args["width"], args["height"], args["device"])
    for k, v in kw.items():
        setattr(p, k, v)
    n = W * H
    hold = {k: np.zeros((n, 3), dtype=np.int32 if k == "material" else np.float32) for k in PLANES}
    b = _lib.DenoiseBuffers()
    for k in PLANES:
        setattr(b, k, None if k in null else hold[k].ctypes.data)
    pp, bp = (None if no_p else ctypes.byref(p)), (None if no_b else ctypes.byref(b))
    rc = L.pt_denoise_device(pp, bp, None) if device_variant else L.pt_denoise(pp, bp)
    return rc, L.pt_last_error().decode()


BAD = [
    (dict(no_p=True), "p is null"),
    (dict(no_b=True), "b is null"),
    (dict(null=("rgb",)), "b->rgb is null"),
    (dict(null=("normal",)), "b->normal is null"),
    (dict(null=("t",)), "b->t is null"),
    (dict(null=("material",)), "b->material is null"),
    (dict(null=("out",)), "b->out is null"),
    (dict(null=("albedo",)), "b->albedo is null"),
    (dict(null=("emission",)), "b->emission is null"),
    (dict(width=0), "p->width"),
    (dict(height=0), "p->height"),
    (dict(height=-3), "p->height"),
    (dict(width=1 << 16, height=1 << 15), "p->width * p->height"),
    (dict(iterations=-1), "p->iterations"),
    (dict(iterations=9), "p->iterations"),
    (dict(sigma_l=0.0), "p->sigma_l"),
    (dict(sigma_l=-1.0), "p->sigma_l"),
    (dict(sigma_l=float("nan")), "p->sigma_l"),
    (dict(sigma_z=0.0), "p->sigma_z"),
    (dict(sigma_z=float("nan")), "p->sigma_z"),
    (dict(normal_power_log2=-1), "p->normal_power_log2"),
    (dict(normal_power_log2=9), "p->normal_power_log2"),
    (dict(demodulate=2), "p->demodulate"),
    (dict(device=-1), "p->device"),
]


@pytest.mark.parametrize("device_variant", [False, True])
@pytest.mark.parametrize("kw,name", BAD)
def test_arguments_are_checked_before_the_device(built, kw, name, device_variant):
    rc, msg = call(device_variant=device_variant, **kw)
    assert rc == PT_ERR_ARG, (rc, msg)
    assert "pt_denoise" in msg and name in msg, msg


@pytest.mark.parametrize("kw", [dict(), dict(null=("err", "var_out")), dict(sigma_l=float("inf")),
                                dict(null=("albedo", "emission"), demodulate=0), dict(iterations=0),
                                dict(iterations=8, normal_power_log2=8)])
def test_good_arguments_get_past_the_checks(built, kw):
    """the control: with nothing wrong the call gets past its checks (and, without a GPU, fails at the
    device); err, var_out and -- without demodulate -- albedo and emission may be null"""
    rc, msg = call(**kw)
    assert rc != PT_ERR_ARG, msg


def test_module_compiles_without_a_device_and_moves_no_key(built):
    L = _lib.lib()
    scenes = {"scene_p1": 8, "csg_zoo": 6}
    ds = {name: pt.DeviceScene(zoo.build(name)) for name in scenes}
    before = {name: (ds[name].module_key(d), ds[name].guides_key()) for name, d in scenes.items()}
    assert L.pt_denoise_compile() == 0, L.pt_last_error().decode()
    key = L.pt_denoise_key().decode()
    assert len(key) == 16 and all(key not in pair for pair in before.values())
    assert {name: (ds[name].module_key(d), ds[name].guides_key()) for name, d in scenes.items()} == before
    # tests/test_chain_abi.py pins these render keys by value; the denoiser is in none of them
    from test_chain_abi import PARENT_KEYS
    for (name, depth), want in PARENT_KEYS.items():
        assert pt.DeviceScene(zoo.build(name)).module_key(depth) == want


def test_python_entry_points_check_their_planes(built):
    rgb = np.zeros((H, W, 3), np.float32)
    g = dict(normal=rgb, t=rgb[..., 0], material=np.zeros((H, W), np.int32), albedo=rgb, emission=rgb)
    with pytest.raises(ValueError, match="guides\\['t'\\]"):
        pt.denoise(rgb, dict(g, t=np.zeros(3)))
    with pytest.raises(ValueError, match="err has"):
        pt.denoise(rgb, g, err=np.zeros(5))
    with pytest.raises(TypeError, match="sigma"):
        pt.denoise(rgb, g, sigma=3)
    with pytest.raises(KeyError):
        pt.denoise(rgb, {k: v for k, v in g.items() if k != "albedo"})
    assert pt.DENOISE_DEFAULTS == dict(iterations=5, sigma_l=2.0, sigma_z=0.1, normal_power_log2=5, demodulate=True)
