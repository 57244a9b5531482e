"""Counts where the CSG fast check, as tests/fastcheck.py restates it, disagrees with the lazy merges.  (no GPU)

usage: python tools/fastcheck_model.py [RAYS] [--find N]

Over at least RAYS rays (default 1 000 000) -- fastcheck.seam_rays of every seam tree, bare and under
ground and wall, and fastcheck.c3_seam_rays for the rest -- and for each pair rule of fastcheck.RULES:
the rays that pass fast_ok, and those of them on which fast_first_hit is not what traceRay's scan finds
in the CPU oracle's root span list (hit / miss, t bits, material).  "header" is the rule pt_device.h has;
it must show 0.  Exit status 1 if it does not.  --find N prints up to N C3 rays on which the rule with
inert at every Union disagrees (the constants fastcheck.C3_FOUND were taken from such a list).

A model of the device code, not a run of it: tests/test_fastcheck.py holds the device to the oracle."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("path-trace_amd", "oracle", "tests")]

import fastcheck as C  # noqa: E402
import oracle_py as O  # noqa: E402
from pathtrace import scenes  # noqa: E402
from pathtrace.scene import to_text  # noqa: E402

CHUNK = 40000


def count(root, rays, tally, found=None):
    text = to_text(root)
    for k in range(0, len(rays), CHUNK):
        r = rays[k:k + CHUNK]
        cnt, t, m = C.span_arrays(O.spans(text, r))
        for rule in C.RULES:
            bad, ok = C.disagreements(root, r, cnt, t, m, rule)
            tally[rule] += np.array([bad.sum(), ok.sum(), len(r)])
            if found is not None and rule == "inert_everywhere":
                found.extend(r[bad])


def main(argv):
    find = 0
    if "--find" in argv:
        k = argv.index("--find")
        find = int(argv[k + 1])
        argv = argv[:k] + argv[k + 2:]
    total = int(argv[0]) if argv else 1000000
    O.build()
    tally = {rule: np.zeros(3, np.int64) for rule in C.RULES}
    seam = {rule: np.zeros(3, np.int64) for rule in C.RULES}
    trees = C.seam_trees()
    per = max(704, total // (4 * 2 * len(trees)))
    for k, (name, part, root) in enumerate(trees):
        for j, r in enumerate((part, root)):
            count(r, C.seam_rays(r, 100 + 2 * k + j, per), seam)
    for rule in C.RULES:
        tally[rule] += seam[rule]
    found = []
    c3 = max(4096, total - int(seam["header"][2]))
    count(scenes.scene_p1(), C.c3_seam_rays(100, c3), tally, found)
    print("%-18s %22s %14s %10s" % ("rule", "disagree with the scan", "pass fast_ok", "rays"))
    for label, tab in (("seam trees", seam), ("seam trees + C3", tally)):
        print(label)
        for rule in C.RULES:
            print("  %-16s %22d %14d %10d" % ((rule,) + tuple(tab[rule])))
    for r in found[:find]:
        print("    [%s]," % ", ".join(repr(float(v)) for v in r))
    return 0 if tally["header"][0] == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
