"""pt_denoise on the GPU, bit for bit against its numpy model (tests/denoise_model.py): the device's own
converged frames and guide buffers of scene_p1 and the CSG zoo, synthetic frames at the sizes and
parameters where the kernels take another path, the device variant on a stream of its own with the output
over the input, and the Python chain.  A NaN counts as equal to a NaN (its payload is the adder's).
The render and guides modules are the ones tests/precompile_modules.py and tests/precompile_guides.py list."""
import ctypes

import numpy as np
import pytest

import denoise_model as DM
import pathtrace as pt
import zoo
from pathtrace import _lib

pytestmark = pytest.mark.gpu
f32 = np.float32


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = ~DM.same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size,
                                                                      np.argwhere(bad)[:4].tolist())


def check(rgb, g, err, **params):
    """pt.denoise against the model, image and variance; returns the image"""
    out, var = pt.denoise(rgb, g, err, return_var=True, **params)
    m_out, m_var = DM.denoise(rgb, g["normal"], g["t"], g["material"], err, g.get("albedo"), g.get("emission"),
                              **params)
    assert_same(out, m_out, "image %r" % (params,))
    assert_same(var, m_var, "variance %r" % (params,))
    return out


# ------------------------------------------------------- rendered frames ---
FRAMES = {"scene_p1": (37, 23, 8), "csg_zoo": (64, 36, 6)}  # 37 x 23: no multiple of any tile
_frames = {}


def rendered(name):
    """the device's own inputs: render_converged with a cap of 128 and render_guides at 16 samples"""
    if name not in _frames:
        w, h, depth = FRAMES[name]
        ds = pt.DeviceScene(zoo.build(name))
        rgb, spp, err, _ = pt.render_converged(ds, w, h, 128, depth, rel_tol=0.05)
        g = pt.render_guides(ds, w, h, 16)
        for a in [rgb, err] + list(g.values()):
            a.setflags(write=False)
        _frames[name] = (ds, rgb, err, g)
    return _frames[name]


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_rendered_frames(built, name, demodulate):
    """5 iterations: the step 16 taps leave a 23-row image for most pixels"""
    _, rgb, err, g = rendered(name)
    assert len(np.unique(g["material"])) >= 3 and (err > 0).any()
    out = check(rgb, g, err, demodulate=demodulate)
    assert (out != rgb).any()


def test_render_denoised_is_the_three_calls(built):
    ds, rgb, err, g = rendered("scene_p1")
    w, h, depth = FRAMES["scene_p1"]
    out, raw, spp, err2, info = pt.render_denoised(ds, w, h, 128, depth, rel_tol=0.05, guide_spp=16, sigma_l=4.0)
    assert_same(raw, rgb, "raw")
    assert_same(err2, err, "err")
    assert spp.shape == (h, w) and info["rounds"] >= 1
    assert_same(out, pt.denoise(rgb, g, err, sigma_l=4.0), "denoised")


# ------------------------------------------------------ synthetic frames ---
def synthetic(w, h, seed=7):
    """a noisy frame over three materials and a region of misses, curved normals, a depth ramp"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    x, y = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    rgb = (0.4 + 0.3 * np.sin(0.3 * x + 0.2 * y)[..., None] + 0.08 * rng.standard_normal((h, w, 3))).astype(f32)
    err = (0.03 + 0.1 * rng.random((h, w))).astype(f32)
    material = ((x // 5 + y // 3) % 3).astype(np.int32)
    material[: (h + 1) // 2, w // 2:] = -1
    normal = np.stack([np.sin(0.15 * x), np.cos(0.2 * y) * 0.5, 1.5 + 0 * x], axis=-1).astype(f32)
    normal[material == -1] = 0
    t = (3 + 0.05 * x + 0.02 * y).astype(f32)
    t[material == -1] = 0
    g = dict(normal=normal, t=t, material=material, albedo=(0.05 + 0.9 * rng.random((h, w, 3))).astype(f32),
             emission=(0.05 * rng.random((h, w, 3))).astype(f32))
    g["albedo"][0, 0] = 0  # below the floor of 0.01
    return rgb, err, g


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (5, 1), (130, 3), (65, 2), (64, 5)])
def test_synthetic_sizes(built, w, h):
    """one pixel, one column, one row; 130 x 3 needs three waves per row, 65 x 2 a wave with one live lane"""
    rgb, err, g = synthetic(w, h)
    check(rgb, g, err)
    check(rgb, g, None, demodulate=False, iterations=2)


@pytest.mark.parametrize("params", [dict(iterations=0), dict(iterations=8), dict(iterations=0, demodulate=False),
                                    dict(normal_power_log2=0), dict(normal_power_log2=8),
                                    dict(sigma_l=float("inf")), dict(sigma_l=8.0, sigma_z=0.01, iterations=3)],
                         ids=lambda p: "-".join("%s=%s" % kv for kv in p.items()))
def test_synthetic_parameters(built, params):
    rgb, err, g = synthetic(70, 9)
    out = check(rgb, g, err, **params)
    if params.get("iterations") == 0 and not params.get("demodulate", True):
        assert_same(out, rgb, "identity")


@pytest.mark.parametrize("with_err", [True, False])
def test_synthetic_non_finite_pixels(built, with_err):
    rgb, err, g = synthetic(40, 11)
    rgb[3, 4], rgb[8, 30, 1], rgb[5, 5, 2] = np.nan, np.inf, -np.inf
    err[3, 4], err[2, 2] = np.nan, np.inf
    g["normal"][6, 6], g["t"][7, 7] = np.nan, np.nan
    bad = ~np.isfinite(rgb).all(axis=-1)
    for params in (dict(), dict(sigma_l=float("inf")), dict(demodulate=False)):
        out = check(rgb, g, err if with_err else None, **params)
        assert np.isfinite(out[~bad]).all() and not np.isfinite(out[bad]).all(axis=-1).any()


def test_synthetic_variance_from_the_neighbourhood(built):
    """err = None on a frame of one material, of many, and with fewer than two usable neighbours"""
    rgb, _, g = synthetic(33, 10)
    check(rgb, g, None)
    g["material"][:] = np.arange(33 * 10, dtype=np.int32).reshape(10, 33)  # every pixel alone: n = 1, v = 0
    out, var = pt.denoise(rgb, g, None, return_var=True, demodulate=False)
    assert (var == 0).all()
    check(rgb, g, None, demodulate=False)


# --------------------------------------------------------------- variants ---
def test_device_variant_on_a_stream_with_the_output_over_the_input(built):
    import torch
    _, rgb, err, g = rendered("csg_zoo")
    h, w = rgb.shape[:2]
    want, want_var = pt.denoise(rgb, g, err, return_var=True)
    again = pt.denoise(rgb, g, err)
    assert_same(again, want, "two runs")
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)  # a copy: the fixtures are read-only
    d = {k: up(g[k]) for k in ("normal", "t", "material", "albedo", "emission")}
    d_rgb, d_err = up(rgb), up(err)
    d_var = torch.zeros((h, w), dtype=torch.float32, device=dev)
    p = pt.denoise_params(w, h, 0)
    b = _lib.DenoiseBuffers()
    b.rgb = b.out = d_rgb.data_ptr()  # in place
    b.err, b.var_out = d_err.data_ptr(), d_var.data_ptr()
    for k, a in d.items():
        setattr(b, k, a.data_ptr())
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().pt_denoise_device(ctypes.byref(p), ctypes.byref(b), ctypes.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert_same(d_rgb.cpu().numpy(), want, "device variant, in place")
    assert_same(d_var.cpu().numpy(), want_var, "device variant, variance")
    # the timed variant: the same bits (not in place), and a device time for each of its 7 launches
    d_in, d_out = up(rgb), torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    b.rgb, b.out = d_in.data_ptr(), d_out.data_ptr()
    ms = (ctypes.c_float * 7)()
    _lib.check(_lib.lib().pt_denoise_device_timed(ctypes.byref(p), ctypes.byref(b),
                                                  ctypes.c_void_p(stream.cuda_stream), ms))
    assert_same(d_out.cpu().numpy(), want, "timed device variant")
    assert all(0 < v < 1000 for v in ms), list(ms)
    prof = (ctypes.c_double * 7)()
    pt.denoise(rgb, g, err)
    assert _lib.lib().pt_call_profile(prof, 7) == 0
    assert prof[0] > 0 and 0 < prof[5] < prof[0]  # PT_PROF_TOTAL and PT_PROF_KERNEL, microseconds
