"""What the guide buffers and the first-hit queries cost (one MI355X, one process).
usage: python tools/guides_probe.py [--scale K] [--rays N]   (K divides C3's width and height; 1 = C3 itself)

(a) pt_render_guides with all six planes on C3's scene at C3's frame, 16 spp, against pt_render at
    depth 0, PT_ORDER_REFERENCE, 16 spp with stats -- the only way to get one of these planes (the
    emission) without the guides module -- in 3 interleaved pairs after a warm-up of each.  Device time:
    the guides kernel by HIP events (pt_call_profile's PT_PROF_KERNEL), pt_render's kernel_ms +
    reduce_ms; host time beside both (the guides call copies six planes back, pt_render one).  The
    emission plane must be pt_render's frame bit for bit.  Then the guides kernel with one plane at a
    time, to see which part costs what.  No threshold.
(b) pt_query_hits on both paths over N = 2^20 hashed camera rays of C3 and of C2: ms per path (device
    and host), the share of rays the fast check decided, and the number of rays on which the two paths
    differ in any field, which must be 0 -- any such ray is printed, and the exit status is 1.

The same pt_render call on another build of the library (the parent commit's) is --only-render: it
prints the render module's key and the pairs' pt_render times alone."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "path-trace_amd"))
import pathtrace as pt  # noqa: E402
from pathtrace import _lib, scenes  # noqa: E402

PAIRS, SPP, SEED = 3, 16, 0x5EED
FIELDS = ("hit", "exit", "material", "t", "normal", "pos", "ior")


def kernel_us():
    out = (ctypes.c_double * 7)()
    _lib.lib().pt_call_profile(out, 7)
    return out[5]


def splitmix(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def camera_rays(cfg, n):
    """n rays from the origin through hashed points of cfg's screen (make_params' camera convention)"""
    with np.errstate(over="ignore"):
        h = splitmix(np.arange(n, dtype=np.uint64) + np.uint64(SEED))
        u = (h >> np.uint64(40)).astype(np.float64) / float(1 << 24)
        v = (splitmix(h) >> np.uint64(40)).astype(np.float64) / float(1 << 24)
    W, H = cfg.width, cfg.height
    r = np.zeros((n, 6), np.float32)
    r[:, 3], r[:, 4], r[:, 5] = (2 * u - 1) * W, (1 - 2 * v) * H, -2.0 * min(W, H)
    return r


def render0(ds, W, H):
    t = time.perf_counter()
    img, st = pt.render(ds, W, H, SPP, 0, seed=SEED, order="reference", stats=True)
    return img, st["kernel_ms"] + st["reduce_ms"], st["kernel_ms"], (time.perf_counter() - t) * 1e3


def guides(ds, W, H, planes=None):
    t = time.perf_counter()
    g = pt.render_guides(ds, W, H, SPP, seed=SEED, planes=planes)
    return g, kernel_us() / 1e3, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--only-render", action="store_true")
    args = ap.parse_args()
    cfg = scenes.CONFIGS["C3"]
    W, H = cfg.width // args.scale, cfg.height // args.scale
    ds = cfg.device_scene()
    print("C3 %dx%d, %d spp; render module (depth 0) %s" % (W, H, SPP, ds.kernel_key(0)))
    render0(ds, W, H)
    if args.only_render:
        for k in range(PAIRS):
            _, r_ms, r_k, r_host = render0(ds, W, H)
            print("  run %d: pt_render(depth 0, reference) %8.3f ms (kernel %8.3f, host %8.2f)" % (k, r_ms, r_k, r_host))
        return 0
    print("guides module %s" % ds.guides_key())
    guides(ds, W, H)
    print("(a) pt_render_guides (six planes) against pt_render(depth 0, reference), %d interleaved pairs" % PAIRS)
    ratios = []
    for k in range(PAIRS):
        img, r_ms, r_k, r_host = render0(ds, W, H)
        g, g_ms, g_host = guides(ds, W, H)
        same = bool(np.array_equal(g["emission"].view(np.uint32), img.view(np.uint32)))
        ratios.append(g_ms / r_ms)
        print("  pair %d: pt_render %8.3f ms (kernel %8.3f, host %8.2f)  guides kernel %8.3f ms (host %8.2f)"
              "  ratio %.4f  emission same bits %s" % (k, r_ms, r_k, r_host, g_ms, g_host, ratios[-1], same))
    print("  ratio guides / pt_render (device): median %.4f, pairs %.4f .. %.4f" %
          (float(np.median(ratios)), min(ratios), max(ratios)))
    for planes in (["coverage"], ["t"], ["material"], ["normal"], ["emission"], ["albedo"]):
        ms = sorted(guides(ds, W, H, planes)[1] for _ in range(PAIRS))
        print("  one plane %-9s kernel %8.3f ms (median of %d, %.3f .. %.3f)" % (planes[0], ms[1], PAIRS, ms[0], ms[-1]))

    print("(b) pt_query_hits, %d hashed camera rays" % args.rays)
    bad = 0
    for name in ("C3", "C2"):
        c = scenes.CONFIGS[name]
        sc = c.device_scene()
        rays = camera_rays(c, args.rays)
        sc.query_hits(rays[:4096])
        res = {}
        for path in ("fast", "merge", "fast", "merge"):
            t = time.perf_counter()
            res[path] = sc.query_hits(rays, path=path)
            host = (time.perf_counter() - t) * 1e3
            print("  %s %-5s kernel %8.3f ms, host %8.2f ms" % (name, path, kernel_us() / 1e3, host))
        f, m = res["fast"], res["merge"]
        differ = np.zeros(len(rays), bool)
        for k in FIELDS:
            a, b = np.ascontiguousarray(f[k]), np.ascontiguousarray(m[k])
            a, b = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
            differ |= (a != b).reshape(len(rays), -1).any(axis=1)
        print("  %s guides module %s: decided %.4f of the rays, hits %.4f, exits %d, rays on which the paths differ: %d"
              % (name, sc.guides_key(), f["decided"].mean(), f["hit"].mean(), int(f["exit"].sum()), int(differ.sum())))
        for i in np.flatnonzero(differ)[:32]:
            print("    ray %d: %s" % (i, [float(v).hex() for v in rays[i]]))
        bad += int(differ.sum())
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
