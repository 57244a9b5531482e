"""Freezes the fixtures of tests/test_fastcheck.py:

  fastcheck_seam.npz    the unmodified reference's root span lists (oracle/_ref/ptref, O.ref_spans) for
                        fastcheck.seam_rays of every seam tree under ground and wall.  Per tree:
                        rays_<name> (n x 6 float32), cnt_<name> (spans per ray), t_<name> (start, end per
                        span), m_<name> (start and end material per span), text_<name> (the scene);
  render_c3_seam.npz    the CPU oracle's values (O.render, ORDER_FAST) of fastcheck.C3_PIXELS of the C3
                        frame at 1024 spp, depth 8: pixels, mean (n x 3) and the oracle's query count.

usage: python tests/golden/make_fastcheck_golden.py [seam] [c3]   (after __graft_entry__.build())"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in ("path-trace_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import fastcheck as C  # noqa: E402
import oracle_py as O  # noqa: E402
from pathtrace import scenes  # noqa: E402
from pathtrace.scene import to_text  # noqa: E402

SEAM_RAYS = 384


def make_seam():
    if not O.ref_available():
        sys.exit("needs `make -C oracle ref` (the reference tree)")
    out = {}
    for k, (name, _, root) in enumerate(C.seam_trees()):
        rays = C.seam_rays(root, k, SEAM_RAYS)
        text = to_text(root)
        cnt, t, m = C.span_arrays(O.ref_spans(text, rays))
        out["rays_" + name], out["text_" + name] = rays, np.array(text)
        out["cnt_" + name], out["t_" + name], out["m_" + name] = cnt.astype(np.int8), t, m.astype(np.int8)
    path = os.path.join(HERE, "fastcheck_seam.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(C.seam_trees()), "trees")


def make_c3():
    cfg = scenes.CONFIGS["C3"]
    mean, st = O.render(to_text(cfg.scene()), cfg.width, cfg.height, C.C3_SPP, C.C3_DEPTH, pixels=C.C3_PIXELS,
                        order=O.ORDER_FAST, stats=True)
    path = os.path.join(HERE, "render_c3_seam.npz")
    np.savez_compressed(path, pixels=np.array(C.C3_PIXELS, np.int32), mean=mean,
                        queries=np.array(st["queries"], np.int64),
                        meta=np.array([cfg.width, cfg.height, C.C3_SPP, C.C3_DEPTH], np.int64))
    print(path, os.path.getsize(path), "bytes,", len(C.C3_PIXELS), "pixels,", st["queries"], "queries")


if __name__ == "__main__":
    what = sys.argv[1:] or ["seam", "c3"]
    assert set(what) <= {"seam", "c3"}, what
    if "seam" in what:
        make_seam()
    if "c3" in what:
        make_c3()
