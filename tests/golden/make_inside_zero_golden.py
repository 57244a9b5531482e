"""Freezes tests/golden/inside_zero.npz: the unmodified reference's root span lists
(oracle/_ref/ptref, O.ref_spans) for the rays of tests/inside_zero.cpu_cases().
Per case: rays_<name> (n x 6 float32), cnt_<name> (spans per ray), t_<name> (start, end per span)
and m_<name> (start and end material per span), text_<name> (the scene).
usage: python tests/golden/make_inside_zero_golden.py   (after __graft_entry__.build())"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in ("path-trace_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import inside_zero as Z  # noqa: E402
import oracle_py as O  # noqa: E402
from pathtrace.scene import to_text  # noqa: E402

out = {}
for k, (name, root) in enumerate(Z.cpu_cases()):
    rays = Z.case_rays(root, k)
    text = to_text(root)
    spans = O.ref_spans(text, rays)
    out["rays_" + name] = rays
    out["text_" + name] = np.array(text)
    out["cnt_" + name] = np.array([len(s) for s in spans], np.int8)
    out["t_" + name] = np.array([[s[0][0], s[2][0]] for sp in spans for s in sp], np.float32).reshape(-1, 2)
    out["m_" + name] = np.array([[s[1], s[3]] for sp in spans for s in sp], np.int8).reshape(-1, 2)
path = os.path.join(HERE, "inside_zero.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes,", len(Z.cpu_cases()), "cases")
