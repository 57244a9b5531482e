"""What the denoiser costs and buys on C3 (one MI355X, one process).
usage: python tools/denoise_probe.py [--scale K] [--arms 0,1] [--config C3]   (K divides width and height)

(i)  Cost: pt_denoise_device_timed on the frame's own planes in device memory -- the device time of
     prepare, of every pass and of finalise by HIP events, the median of five runs after a warm-up, for
     each arm of csrc/device/pt_denoise.h (0 packed 16-byte records, the form that ships; 1 the same with
     an LDS tile and its halo for the step 1 and 2 passes, PT_DENOISE_LDS_TILE), the arms taking turns
     within every round.  (A third arm, the records as eight planes of floats, lost on every pass and was
     retired: profiles/round15/denoise_probe.txt has its figures as arm 1, the LDS tile's as arm 2.)
     Beside each pass, the bytes per second its time means against the traffic model of 25 taps x 36 B read
     and 16 B written per pixel.  Every arm's output is compared with arm 0's, bit for bit.
(ii) Effect: render_converged(rel_tol 0.05) + guides at 16 spp + denoise against render_converged(rel_tol
     0.01) alone: each one's device time and RMSE against the uniform frame of the same seed at C3's sample
     count, over the frame and over the pixels whose first hit is glass or mirror (no scatter, a reflect
     colour) and the others apart; the noise floor (two uniform frames of different seeds) beside them;
     and a sweep of sigma_l.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "path-trace_amd"))
import pathtrace as pt  # noqa: E402
from pathtrace import _lib, scenes  # noqa: E402

SEED, OTHER_SEED = 0x5EED, 0xC0FFEE
RUNS = 5
ARM_NAMES = {0: "packed records", 1: "LDS tile (steps 1, 2)"}


def rmse(a, b, mask=None):
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask])))


def kernel_us():
    prof = (ctypes.c_double * 7)()
    _lib.lib().pt_call_profile(prof, 7)
    return prof[5]


def specular_materials(ds, w, h):
    """the pt_ids whose material does not scatter and has a reflect colour: glass and mirror"""
    ys, xs = np.meshgrid(np.linspace(-1, 1, 54), np.linspace(-1, 1, 96), indexing="ij")
    rays = np.zeros((ys.size, 6), np.float32)  # through the frame: (x W, y H, -2 min(W, H)), the default screen
    rays[:, 3], rays[:, 4], rays[:, 5] = xs.ravel() * w, ys.ravel() * h, -2.0 * min(w, h)
    q = ds.query_hits(rays, shade=True)
    ids = set()
    for m in np.unique(q["material"][q["hit"] != 0]):
        sh = q["shade"][q["material"] == m][0]
        if sh[9] == 0 and sh[3:6].max() > 0:
            ids.add(int(m))
    return sorted(ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--arms", default="0,1")
    args = ap.parse_args()
    arms = [int(a) for a in args.arms.split(",")]
    import torch
    cfg = scenes.CONFIGS[args.config]
    W, H, spp, depth = cfg.width // args.scale, cfg.height // args.scale, cfg.spp, cfg.depth
    ds = cfg.device_scene()
    L = _lib.lib()
    print("%s %dx%d, cap %d spp, depth %d, render module %s, guides module %s, denoise module %s" %
          (cfg.name, W, H, spp, depth, ds.kernel_key(depth), ds.guides_key(), L.pt_denoise_key().decode()))

    # ---- the inputs
    pt.render(ds, W, H, 64, depth)  # warm-up: code objects loaded, buffers grown
    img5, n5, err5, info5 = pt.render_converged(ds, W, H, spp, depth, min_spp=64, rel_tol=0.05, seed=SEED)
    img5, n5, err5, info5 = pt.render_converged(ds, W, H, spp, depth, min_spp=64, rel_tol=0.05, seed=SEED)
    img1, n1, err1, info1 = pt.render_converged(ds, W, H, spp, depth, min_spp=64, rel_tol=0.01, seed=SEED)
    pt.render_guides(ds, W, H, 16, seed=SEED)
    g = pt.render_guides(ds, W, H, 16, seed=SEED)
    guides_ms = kernel_us() / 1e3
    t5 = info5["kernel_ms"] + info5["reduce_ms"]
    t1 = info1["kernel_ms"] + info1["reduce_ms"]

    # ---- (i) cost
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)
    d = {k: up(g[k]) for k in ("normal", "t", "material", "albedo", "emission")}
    d_rgb, d_err = up(img5), up(err5)
    d_out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    p = pt.denoise_params(W, H, 0)
    b = _lib.DenoiseBuffers()
    b.rgb, b.err, b.out = d_rgb.data_ptr(), d_err.data_ptr(), d_out.data_ptr()
    for k, a in d.items():
        setattr(b, k, a.data_ptr())
    nk = p.iterations + 2
    ms = (ctypes.c_float * nk)()
    times = {a: [] for a in arms}
    outs = {}
    torch.cuda.synchronize()
    for run in range(RUNS + 1):  # run 0 is the warm-up
        for a in arms:
            os.environ["PT_DENOISE_LDS_TILE"] = str(a)
            _lib.check(L.pt_denoise_device_timed(ctypes.byref(p), ctypes.byref(b), None, ms))  # the module's load
            _lib.check(L.pt_denoise_device_timed(ctypes.byref(p), ctypes.byref(b), None, ms))
            if run:
                times[a].append(list(ms))
            else:
                outs[a] = d_out.cpu().numpy()
    os.environ.pop("PT_DENOISE_LDS_TILE")
    model_bytes = W * H * (25 * 36 + 16)
    names = ["prepare"] + ["pass %d (step %d)" % (i, 1 << i) for i in range(p.iterations)] + ["finalise"]
    print("(i) cost at the defaults %s: device ms by HIP events, median of %d runs after a warm-up, arms interleaved"
          % (pt.DENOISE_DEFAULTS, RUNS))
    print("    traffic model of a pass: %.1f MB (25 taps x 36 B read + 16 B written per pixel)" % (model_bytes / 1e6))
    med = {a: np.median(np.array(times[a]), axis=0) for a in arms}
    spread = {a: (np.array(times[a]).sum(axis=1).min(), np.array(times[a]).sum(axis=1).max()) for a in arms}
    for k, name in enumerate(names):
        cells = []
        for a in arms:
            c = "%8.4f" % med[a][k]
            if name.startswith("pass"):
                c += " (%5.2f TB/s)" % (model_bytes / (med[a][k] * 1e-3) / 1e12)
            cells.append("arm %d %s" % (a, c))
        print("    %-18s %s" % (name, "   ".join(cells)))
    for a in arms:
        same = bool(np.array_equal(outs[a].view(np.uint32), outs[arms[0]].view(np.uint32)))
        print("    arm %d (%s): sum of medians %.4f ms, whole calls %.4f .. %.4f ms, same bits as arm %d: %s" %
              (a, ARM_NAMES[a], float(med[a].sum()), spread[a][0], spread[a][1], arms[0], same))
    denoise_ms = float(med[0].sum()) if 0 in med else float(med[arms[0]].sum())

    # ---- (ii) effect
    ref, st = pt.render(ds, W, H, spp, depth, seed=SEED, stats=True)
    other = pt.render(ds, W, H, spp, depth, seed=OTHER_SEED)
    spec_ids = specular_materials(ds, W, H)
    spec = np.isin(g["material"], spec_ids)
    out = pt.denoise(img5, g, err5)
    assert np.array_equal(out.view(np.uint32), outs[arms[0]].view(np.uint32))
    print("(ii) effect: RMSE against the uniform %d-spp frame of the same seed (%.1f ms device time)" %
          (spp, st["kernel_ms"] + st["reduce_ms"]))
    print("    noise floor (uniform frames of seeds %#x and %#x): %.6f; glass and mirror pixels (ids %s, %.2f %% of "
          "the frame) %.6f, the others %.6f" % (SEED, OTHER_SEED, rmse(ref, other), spec_ids, 100 * spec.mean(),
                                                rmse(ref, other, spec), rmse(ref, other, ~spec)))
    rows = [("converged rel_tol 0.05", t5, img5), ("  + guides 16 spp + denoise", t5 + guides_ms + denoise_ms, out),
            ("converged rel_tol 0.01", t1, img1)]
    for name, t, img in rows:
        print("    %-28s %9.2f ms   RMSE %.6f   glass and mirror %.6f   others %.6f" %
              (name, t, rmse(img, ref), rmse(img, ref, spec), rmse(img, ref, ~spec)))
    print("    of which guides %.3f ms, denoise %.3f ms; mean spp %.1f (0.05) and %.1f (0.01)" %
          (guides_ms, denoise_ms, info5["samples"] / (W * H), info1["samples"] / (W * H)))
    print("    sigma_l sweep on the rel_tol 0.05 frame (RMSE, glass and mirror, others):")
    for sl in (1.0, 2.0, 4.0, 8.0, float("inf")):
        o = pt.denoise(img5, g, err5, sigma_l=sl)
        print("      sigma_l %4g: %.6f  %.6f  %.6f" % (sl, rmse(o, ref), rmse(o, ref, spec), rmse(o, ref, ~spec)))
    for name, kw in (("no demodulation", dict(demodulate=False)), ("3 iterations", dict(iterations=3))):
        o = pt.denoise(img5, g, err5, **kw)
        print("      %-14s %.6f  %.6f  %.6f" % (name + ":", rmse(o, ref), rmse(o, ref, spec), rmse(o, ref, ~spec)))
    o = pt.denoise(img5, g, None)
    print("      %-14s %.6f  %.6f  %.6f" % ("err = None:", rmse(o, ref), rmse(o, ref, spec), rmse(o, ref, ~spec)))
    o = pt.denoise(img1, g, err1)
    print("    the rel_tol 0.01 frame denoised: %.6f  %.6f  %.6f" % (rmse(o, ref), rmse(o, ref, spec), rmse(o, ref, ~spec)))


if __name__ == "__main__":
    main()
