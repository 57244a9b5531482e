"""What chained rendering costs (one MI355X).  usage: python tools/chain_probe.py

scene_p1, 64 x 36, depth 8, in one process:
  - 4 096 chains x 8 hashed pixels x 4 spp through pt_trace_chains (32 launches
    of up to 4 096 items, one per step);
  - the same 32 768 pixels through the strict-order pt_render at 4 spp (one
    launch and its reduce): the yardstick, not a target;
  - one chain of one pixel at 64 spp, 64 launches of one item: the per-step cost,
    for the sky pixel (0, 0), whose sample its lane finishes with two draws -- the
    step is the launch -- and for the frame's centre pixel, a diffuse hit whose
    sample is a burst of some 10^4 children served by one wave.
Device events (pt_render_stats.kernel_ms: for a chained call the first launch's
start to the last launch's end, the gaps between launches included; for the
render, its launch plus its reduce), the median of five after a warm-up.  The
host clock around the one-pixel calls gives their latency."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "path-trace_amd"))
import pathtrace as pt  # noqa: E402
from pathtrace import scenes  # noqa: E402

W, H, DEPTH, SPP, NCHAINS, LEN, REPS = 64, 36, 8, 4, 4096, 8, 5
M64 = (1 << 64) - 1


def splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def median_of(fn):
    fn()  # warm-up: code object loaded, buffers grown
    return statistics.median(fn() for _ in range(REPS))


def main():
    ds = pt.DeviceScene(scenes.scene_p1())
    pixels = np.array([splitmix(977 + k) % (W * H) for k in range(NCHAINS * LEN)], dtype=np.int32)
    begin = np.arange(NCHAINS + 1, dtype=np.int64) * LEN
    states = np.array([pt.lcg_state(k) for k in range(NCHAINS)], dtype=np.uint64)
    samples = len(pixels) * SPP

    def chained():
        return pt.trace_pixels_chained(ds, pixels, begin, states, W, H, SPP, DEPTH, stats=True)[3]["kernel_ms"]

    def render():
        st = pt.render(ds, W, H, SPP, DEPTH, order="reference", pixels=pixels, stats=True)[1]
        return st["kernel_ms"] + st["reduce_ms"]

    where = {"sky": np.array([0], dtype=np.int32), "centre": np.array([W * (H // 2) + W // 2], dtype=np.int32)}

    def one_pixel(name, spp, clock):
        def call():
            t = time.perf_counter()
            st = pt.trace_pixels_chained(ds, where[name], [0, 1], [pt.lcg_state(1)], W, H, spp, DEPTH,
                                         stats=clock == "device")
            return st[3]["kernel_ms"] if clock == "device" else (time.perf_counter() - t) * 1e3
        return call

    c_ms, r_ms = median_of(chained), median_of(render)
    print("scene_p1 %dx%d depth %d, %d samples (%d chains x %d pixels x %d spp), median of %d" %
          (W, H, DEPTH, samples, NCHAINS, LEN, SPP, REPS))
    print("chained   pt_trace_chains  %8.3f ms  %8.2f Msamples/s  (%d launches)" %
          (c_ms, samples / c_ms / 1e3, LEN * SPP))
    print("unchained pt_render strict %8.3f ms  %8.2f Msamples/s  (1 launch + reduce)" % (r_ms, samples / r_ms / 1e3))
    print("chained / unchained throughput: %.3f" % (r_ms / c_ms))
    for name in ("sky", "centre"):
        s_ms = median_of(one_pixel(name, 64, "device"))
        print("one chain, the %s pixel, 64 spp: %.3f ms on the device = %.2f us per step" %
              (name, s_ms, s_ms / 64 * 1e3))
        for spp in (1, 4, 64):
            h_ms = median_of(one_pixel(name, spp, "host"))
            print("one chain, the %s pixel, %2d spp: %.1f us per call on the host clock (%.2f us per step)" %
                  (name, spp, h_ms * 1e3, h_ms / spp * 1e3))


if __name__ == "__main__":
    main()
