"""What converged rendering costs and saves on C3 (one MI355X, one process).
usage: python tools/converge_probe.py [--scale K]      (K divides width and height; 1 = C3 itself)

(a) Overhead: pt_render_converge with min_spp = spp = C3's 1024 -- one round,
    nothing stops early, the moments reduce, the decision and the scan run --
    against pt_render at 1024 spp, in interleaved pairs after a warm-up of
    each.  Device time = kernel_ms + reduce_ms of the call's stats.  No
    threshold: the yardstick is pt_render's time in the same process, with the
    spread of the pairs beside the ratio.
(b) Effect: min_spp 64, cap 1024, rel_tol 0.05 / 0.02 / 0.01: device time, mean
    samples per pixel, entries per stop count, and RMSE against the uniform
    1024-spp frame of the same seed; beside it the RMSE between two uniform
    1024-spp frames of different seeds -- the noise floor.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "path-trace_amd"))
import pathtrace as pt  # noqa: E402
from pathtrace import scenes  # noqa: E402

PAIRS = 3
SEED, OTHER_SEED = 0x5EED, 0xC0FFEE


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    args = ap.parse_args()
    cfg = scenes.CONFIGS["C3"]
    W, H, spp, depth = cfg.width // args.scale, cfg.height // args.scale, cfg.spp, cfg.depth
    ds = cfg.device_scene()
    print("C3 %dx%d, cap %d spp, depth %d, module %s" % (W, H, spp, depth, ds.kernel_key(depth)))

    def uniform(seed=SEED):
        t = time.perf_counter()
        img, st = pt.render(ds, W, H, spp, depth, seed=seed, stats=True)
        return img, st["kernel_ms"] + st["reduce_ms"], st["reduce_ms"], (time.perf_counter() - t) * 1e3

    def converged(min_spp, rel_tol):
        t = time.perf_counter()
        img, n, err, info = pt.render_converged(ds, W, H, spp, depth, min_spp=min_spp, rel_tol=rel_tol, seed=SEED)
        return img, n, info, info["kernel_ms"] + info["reduce_ms"], (time.perf_counter() - t) * 1e3

    # warm-up: code objects loaded, buffers grown
    pt.render(ds, W, H, 64, depth)
    pt.render_converged(ds, W, H, 128, depth, min_spp=64, rel_tol=0.05)

    print("(a) overhead: converge(min_spp = spp = %d) against pt_render(%d), %d interleaved pairs" %
          (spp, spp, PAIRS))
    ratios, u_times, ref = [], [], None
    for k in range(PAIRS):
        ref, u_ms, u_red, u_host = uniform()
        img, n, info, c_ms, c_host = converged(spp, 0.01)
        same = bool(np.array_equal(img.view(np.uint32), ref.view(np.uint32)))
        ratios.append(c_ms / u_ms)
        u_times.append(u_ms)
        print("  pair %d: pt_render %9.2f ms (reduce %6.3f, host %9.2f)  converge %9.2f ms (reduce %6.3f, host %9.2f)"
              "  ratio %.4f  same bits %s  rounds %d" %
              (k, u_ms, u_red, u_host, c_ms, info["reduce_ms"], c_host, ratios[-1], same, info["rounds"]))
    print("  ratio converge / pt_render: median %.4f, pairs %.4f .. %.4f" %
          (float(np.median(ratios)), min(ratios), max(ratios)))

    print("(b) effect: min_spp 64, cap %d" % spp)
    other, o_ms, _, _ = uniform(OTHER_SEED)
    print("  noise floor: RMSE between uniform %d-spp frames of seeds %#x and %#x: %.6f   (mean %.4f)" %
          (spp, SEED, OTHER_SEED, rmse(ref, other), float(ref.mean())))
    u_ms = float(np.median(u_times))
    print("  uniform %d spp: %.2f ms (median of (a)'s pairs)" % (spp, u_ms))
    for rel in (0.05, 0.02, 0.01):
        img, n, info, c_ms, c_host = converged(64, rel)
        counts = {int(v): int(c) for v, c in zip(*np.unique(n, return_counts=True))}
        print("  rel_tol %.2f: %9.2f ms (host %9.2f, reduce %6.3f) = %.3f of uniform, mean spp %7.2f, rounds %d, "
              "capped %d, RMSE vs uniform %.6f, vs the other seed %.6f" %
              (rel, c_ms, c_host, info["reduce_ms"], c_ms / u_ms, info["samples"] / (W * H), info["rounds"],
               info["capped"], rmse(img, ref), rmse(img, other)))
        print("    entries per stop count: %s" % counts)


if __name__ == "__main__":
    main()
