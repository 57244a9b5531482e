"""The numpy model of pt_denoise (tests/denoise_model.py) on the CPU: the properties the filter is built
to have -- the device is held to them through the bit comparison of tests/test_denoise_gpu.py -- and its
effect on a real frame: scene_p1 at 32 x 18, 64 samples from the CPU oracle in the fast order, the error
estimate of tests/converge_model.py, the guides of tests/hits_model.py at 16 samples, against the oracle's
1024-sample frame of another seed."""
import numpy as np
import pytest

import converge_model as CM
import denoise_model as DM
import guide_scenes as G
import hits_model as HM

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def flat_guides(h, w, material=0):
    normal = np.zeros((h, w, 3), f32)
    normal[..., 2] = 1
    return dict(normal=normal, t=np.full((h, w), 4, f32), material=np.full((h, w), material, np.int32))


def noisy(rng, h, w):
    """a frame with structure and noise, its error estimate, and demodulation planes"""
    x = np.linspace(0, 1, w, dtype=f32)[None, :, None]
    rgb = (0.3 + 0.4 * x + 0.05 * rng.standard_normal((h, w, 3))).astype(f32)
    err = (0.02 + 0.05 * rng.random((h, w))).astype(f32)
    albedo = (0.2 + 0.7 * rng.random((h, w, 3))).astype(f32)
    emission = (0.1 * rng.random((h, w, 3))).astype(f32)
    return rgb, err, albedo, emission


# ------------------------------------------------------------ properties ---
@pytest.mark.parametrize("demodulate", [False, True])
def test_flat_dyadic_image_comes_back(demodulate):
    """all weights and sums are dyadic, so a flat image is returned bit for bit, at the borders too, where
    taps fall off the image (the step 4, 8 and 16 taps leave a 9 x 5 image for most pixels)"""
    h, w = 5, 9
    rgb = np.full((h, w, 3), 0.5, f32)
    out, var = DM.denoise(rgb, err=np.zeros((h, w), f32), albedo=np.full((h, w, 3), 0.5, f32),
                          emission=np.full((h, w, 3), 0.25, f32), iterations=5, demodulate=demodulate,
                          **flat_guides(h, w))
    assert (bits(out) == bits(rgb)).all()
    assert (bits(var) == 0).all()


def test_no_iterations_without_demodulation_is_the_identity():
    rng = np.random.default_rng(1)
    rgb, err, _, _ = noisy(rng, 6, 7)
    rgb[0, 0], rgb[1, 1, 1], rgb[2, 2, 0] = -0.0, np.nan, np.inf
    out, var = DM.denoise(rgb, err=err, iterations=0, demodulate=False, **flat_guides(6, 7))
    assert (bits(out) == bits(rgb)).all()
    assert (bits(var) == bits(err * err)).all()


@pytest.mark.parametrize("with_err", [True, False])
def test_nothing_crosses_a_material_edge(with_err):
    rng = np.random.default_rng(2)
    h, w = 12, 21
    rgb, err, albedo, emission = noisy(rng, h, w)
    g = flat_guides(h, w)
    g["material"][:, 9:] = 3
    other = rgb.copy()
    other[:, 9:] = (5 * rng.random((h, w - 9, 3))).astype(f32)
    kw = dict(err=err if with_err else None, albedo=albedo, emission=emission, iterations=5, **g)
    a, va = DM.denoise(rgb, **kw)
    b, vb = DM.denoise(other, **kw)
    assert (bits(a[:, :9]) == bits(b[:, :9])).all() and (bits(va[:, :9]) == bits(vb[:, :9])).all()
    assert (bits(a[:, 9:]) != bits(b[:, 9:])).any()
    assert (bits(a[:, :9]) != bits(rgb[:, :9])).any()  # and the filter did something there


@pytest.mark.parametrize("sigma_l", [8.0, np.inf])
def test_non_finite_pixels_do_not_spread(sigma_l):
    """a NaN and an inf pixel: every other output is finite and is what it is when those two pixels hold a
    finite colour so far away that every tap on them weighs nothing; the two stay non-finite"""
    rng = np.random.default_rng(3)
    h, w = 11, 13
    rgb, err, albedo, emission = noisy(rng, h, w)
    bad = np.zeros((h, w), bool)
    bad[4, 5] = bad[7, 9] = True
    poisoned, removed = rgb.copy(), rgb.copy()
    poisoned[4, 5], poisoned[7, 9, 1] = np.nan, np.inf
    kw = dict(err=err, albedo=albedo, emission=emission, iterations=4, sigma_l=sigma_l, **flat_guides(h, w))
    a, va = DM.denoise(poisoned, **kw)
    assert np.isfinite(a[~bad]).all() and np.isfinite(va).all()
    assert not np.isfinite(a[4, 5]).any() and not np.isfinite(a[7, 9, 1])
    if sigma_l != np.inf:  # with the luminance weight off only a non-finite pixel is left out
        removed[4, 5] = removed[7, 9] = 1e30
        b, vb = DM.denoise(removed, **kw)
        assert (bits(a[~bad]) == bits(b[~bad])).all() and (bits(va[~bad]) == bits(vb[~bad])).all()


def test_variance_of_one_pass_without_the_luminance_weight():
    """sigma_l = +inf, flat guides, a dyadic variance: Sw = 1 and v' = v * sum h^2 = v * 4900 / 65536
    exactly for the pixels whose 25 taps are all in the image, whatever the colours"""
    rng = np.random.default_rng(4)
    h, w = 7, 9
    rgb, _, _, _ = noisy(rng, h, w)
    err = np.full((h, w), 0.25, f32)
    out, var = DM.denoise(rgb, err=err, iterations=1, sigma_l=np.inf, demodulate=False, **flat_guides(h, w))
    want = f32(0.0625) * f32(4900) / f32(65536)
    assert (bits(var[2:-2, 2:-2]) == bits(want)).all()
    assert (bits(var[0]) != bits(want)).all()
    assert (bits(out) != bits(rgb)).any()


def test_miss_pixels_ignore_normal_and_depth():
    """material -1: wn = wz = 1, so a region of misses with zero normals and zero depth is still filtered"""
    rng = np.random.default_rng(5)
    h, w = 6, 8
    rgb, err, _, _ = noisy(rng, h, w)
    g = dict(normal=np.zeros((h, w, 3), f32), t=np.zeros((h, w), f32), material=np.full((h, w), -1, np.int32))
    out, _ = DM.denoise(rgb, err=err, iterations=2, demodulate=False, **g)
    assert (np.abs(out - rgb) > 1e-3).mean() > 0.5
    g["material"][:] = 0  # a hit with a zero normal has wn = 0: only the centre tap is left
    out, _ = DM.denoise(rgb, err=err, iterations=2, demodulate=False, **g)
    assert np.allclose(out, rgb, rtol=1e-6, atol=0)


def test_noise_on_a_smooth_interior_is_reduced():
    """a colour ramp with Gaussian noise and an honest, or a one-degree-of-freedom, error estimate: the
    filter brings the frame closer to the ramp, and a wider luminance tolerance brings it closer still"""
    rng = np.random.default_rng(6)
    h, w, sigma = 32, 48, 0.05
    truth = np.broadcast_to(0.3 + 0.4 * np.linspace(0, 1, w, dtype=f32)[None, :, None], (h, w, 3)).astype(f32)
    rgb = (truth + sigma * rng.standard_normal((h, w, 3))).astype(f32)
    honest = np.full((h, w), sigma * np.sqrt(3), f32)  # the standard error of r + g + b
    rough = (honest * np.abs(rng.standard_normal((h, w)))).astype(f32)  # as two batch means estimate it
    err_of = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
    for err in (honest, rough):
        at = {s: err_of(DM.denoise(rgb, err=err, demodulate=False, sigma_l=s, **flat_guides(h, w))[0])
              for s in (2.0, 8.0)}
        print("raw %.4f, sigma_l 2: %.4f, 8: %.4f" % (err_of(rgb), at[2.0], at[8.0]))
        assert at[8.0] < at[2.0] < err_of(rgb)


# ------------------------------------------------------- a rendered frame ---
W, H, DEPTH, SPP, GUIDE_SPP, TRUTH_SPP = 32, 18, 8, 64, 16, 1024
SEED, TRUTH_SEED = 0x5EED, 0xBEEF
SCREEN = (float(W), float(H), float(2 * min(W, H)))


def cpu_guides(text, spp):
    """pt_render_guides' planes of the whole frame from the CPU alone (as tests/test_guides_gpu.py's model)"""
    import oracle_py as O
    n = W * H
    rays = HM.camera_rays(list(range(n)), W, H, W, SCREEN, SEED, 0, spp).reshape(-1, 6)
    cnt, rows = HM.rows_from_oracle(O.spans(text, rays))
    w = HM.expected_hits(rays, cnt, rows)
    sh, _ = HM.expected_shade(text, O.tex_eval(text, w["pos"]), w["material"], w["hit"] != 0)
    per = lambda a: np.asarray(a, f32).reshape((n, spp) + np.shape(a)[1:])
    frame = lambda a: a.reshape((H, W) + a.shape[1:])
    return dict(emission=frame(HM.guide_mean(per(sh[:, 0:3]), spp)), albedo=frame(HM.guide_mean(per(sh[:, 3:6]), spp)),
                normal=frame(HM.guide_mean(per(w["normal"]), spp)), t=frame(HM.guide_mean(per(w["t"]), spp)),
                material=frame(w["material"].reshape(n, spp)[:, 0].astype(np.int32)))


@pytest.fixture(scope="module")
def frame(built, tmp_path_factory):
    import oracle_py as O
    text = G.text("scene_p1", str(tmp_path_factory.mktemp("denoise_img")))
    vals = O.render(text, W, H, SPP, DEPTH, order=O.ORDER_FAST, per_sample=True, seed=SEED)
    rgb, spp, err, _ = CM.converge(CM.tree32(vals), SPP, SPP, 0.0)
    assert (spp == SPP).all()
    truth = O.render(text, W, H, TRUTH_SPP, DEPTH, order=O.ORDER_FAST, seed=TRUTH_SEED)
    return dict(rgb=rgb.reshape(H, W, 3), err=err.reshape(H, W), truth=truth.reshape(H, W, 3),
                guides=cpu_guides(text, GUIDE_SPP))


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_quality_on_scene_p1(frame):
    """the defaults reduce the error of a 64-sample frame against the 1024-sample truth; the sweep is
    printed (and recorded in DESIGN.md s7e), the condition is only that the ratio is below 1"""
    g = frame["guides"]
    raw = rmse(frame["rgb"], frame["truth"])
    ratios = {}
    for sigma_l in (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 8.0, 16.0, np.inf):
        out, _ = DM.denoise(frame["rgb"], g["normal"], g["t"], g["material"], frame["err"], g["albedo"],
                            g["emission"], sigma_l=sigma_l)
        ratios[sigma_l] = rmse(out, frame["truth"]) / raw
    out, _ = DM.denoise(frame["rgb"], g["normal"], g["t"], g["material"], frame["err"], g["albedo"], g["emission"])
    ratio = rmse(out, frame["truth"]) / raw
    print("raw rmse %.5f, denoised/raw at the defaults %.3f; sigma_l sweep %s"
          % (raw, ratio, ", ".join("%g: %.3f" % kv for kv in ratios.items())))
    for name, kw in (("no demodulation", dict(demodulate=False)), ("err = None", None), ("3 iterations", dict(iterations=3))):
        o, _ = DM.denoise(frame["rgb"], g["normal"], g["t"], g["material"], None if kw is None else frame["err"],
                          g["albedo"], g["emission"], **(kw or {}))
        print("  %s: %.3f" % (name, rmse(o, frame["truth"]) / raw))
    assert ratio == ratios[DM.DEFAULTS["sigma_l"]]
    assert ratio < 1.0
