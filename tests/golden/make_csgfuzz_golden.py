"""Freezes what the UNMODIFIED reference (oracle/_ref/ptref) computes for the
adversarial CSG inputs of tests/csgfuzz.py, for tests/test_csgfuzz.py:

  csgfuzz_spans.npz  per span tree its text, rays and full span lists (the layout of
                     spans_csg.npz), plus the tie census: for every binary node
                     with no transform above it, the reference's span lists of
                     its two children for the same rays, and the number of rays
                     with an A span end exactly equal to a B span end, per
                     operator and kind (csgfuzz.TIE_KINDS);
  csgfuzz_trace.npz  per trace scene its rays and traceRay means (spp 2, depth 3,
                     reference order).  The reference build asserts
                     count <= 1000 in its rejection loop (include/path-trace.h:147)
                     and takes the whole run down with it; such rays are located by
                     bisection, removed (at most 2 % of a scene's rays) and
                     the final list is run again, since a ray's engine key is its index;
  csgfuzz_trace_leaf.npz  the same for the all-leaf variants of the trace scenes
                     (csgfuzz.trace_scene(s, leaf=True): the scenes whose default
                     module is the lane-resume form) and, per scene, for the
                     edge-strength family (csgfuzz.edge_strength_rays), with
                     the indices of the rays removed from either family, and
                     csgfuzz.regress_resume_negative_count's rays and means;
  csgfuzz_cap.npz    rays through the cap scene: those on which that assertion
                     fires when the ray runs alone (index 0) at depth 2 -- the
                     reference's own proof that the cap is reached -- and rays it
                     completes, with its values.

Runs only where the reference tree exists.

    python tests/golden/make_csgfuzz_golden.py [spans] [trace] [trace_leaf]

Without arguments every fixture is written; `trace` writes csgfuzz_trace.npz and
csgfuzz_cap.npz (which holds the rays make_trace removed), `trace_leaf` only
csgfuzz_trace_leaf.npz.
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "path-trace_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import csgfuzz as F  # noqa: E402
import oracle_py as O  # noqa: E402
from make_golden import spans_to_arrays  # noqa: E402
from pathtrace.scene import TransformedObject, to_text  # noqa: E402
from pathtrace.scene import _Binary  # noqa: E402

SEED = 0x5EED
TRACE_SPP, TRACE_DEPTH = 2, 3
MAX_REMOVED = 0.02
CAP_ABORTS, CAP_COMPLETES = 40, 96
# a ray that leaves every scene here untouched: up and away from above the ground
MISS = np.array([0, 50, 0, 0, 1, 0.5, 1], np.float32)


def census(root, rays, cells, ref_spans=None):
    """adds to cells[op][kind] the rays whose child span lists tie at this node, then descends (not
    below a transform: its children see other rays)"""
    ref_spans = ref_spans or O.ref_spans
    if isinstance(root, TransformedObject) or not isinstance(root, _Binary):
        return
    la, lb = ref_spans(to_text(root.a), rays), ref_spans(to_text(root.b), rays)
    op = F.OPS.index(type(root))
    for sa, sb in zip(la, lb):
        a0, a1 = {float(s[0][0]) for s in sa}, {float(s[2][0]) for s in sa}
        b0, b1 = {float(s[0][0]) for s in sb}, {float(s[2][0]) for s in sb}
        for k, hit in enumerate((a0 & b0, a1 & b1, a1 & b0, b1 & a0)):
            cells[op, k] += bool(hit)
    census(root.a, rays, cells, ref_spans)
    census(root.b, rays, cells, ref_spans)


def make_spans():
    out = {}
    cells = np.zeros((3, 4), dtype=np.int64)
    names = []
    for k, (name, builder) in enumerate(F.span_trees()):
        root = builder()
        txt = to_text(root)
        rays = F.span_rays(root, seed=k)
        spans = O.ref_spans(txt, rays)
        counts, data = spans_to_arrays(spans)
        assert np.all(np.isfinite(data.view(np.float32)[:, [0, 5]])), name
        census(root, rays, cells)
        names.append(name)
        out["text_%d" % k], out["rays_%d" % k], out["counts_%d" % k] = np.array(txt), rays, counts
        out["data_%d" % k] = data
        print("%-28s non-empty %3d / %d, longest %d" % (name, int((counts > 0).sum()), len(rays), counts.max()))
    print("census (rows union / intersection / difference, columns %s):\n%s" % (" ".join(F.TIE_KINDS), cells))
    np.savez_compressed(os.path.join(HERE, "csgfuzz_spans.npz"), names=np.array(names), census=cells, **out)


def ref_completes(txt, rays, depth, spp=TRACE_SPP, threads=0):
    """the reference's means, or None where its assert(count <= 1000) ended the run"""
    try:
        return O.ref_trace_rays(txt, rays, spp, depth, seed=SEED, threads=threads)
    except RuntimeError as e:
        if "count <= 1000" not in str(e):
            raise
        return None


def find_abort(txt, rays, lo, hi):
    """the first ray of rays[lo:hi] on which the reference asserts, every other ray replaced by MISS so
    that each keeps its index"""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probe = np.tile(MISS, (len(rays), 1))
        probe[lo:mid] = rays[lo:mid]
        if ref_completes(txt, probe, TRACE_DEPTH) is None:
            hi = mid
        else:
            lo = mid
    return lo


def freeze(txt, all_rays, what):
    """(keep, rays, mean): the reference's means of all_rays[keep], keep dropping the rays it asserts on"""
    keep = np.ones(len(all_rays), dtype=bool)
    while True:
        rays = all_rays[keep]
        mean = ref_completes(txt, rays, TRACE_DEPTH)
        if mean is not None:
            break
        k = find_abort(txt, rays, 0, len(rays))
        keep[np.flatnonzero(keep)[k]] = False
    removed = int((~keep).sum())
    assert removed <= MAX_REMOVED * len(all_rays), "%s: the reference asserts on %d rays" % (what, removed)
    return keep, rays, mean


def make_trace():
    out = {}
    moved = []
    for s in range(F.N_TRACE_SCENES):
        txt = to_text(F.trace_scene(s))
        all_rays = F.trace_rays(s)
        keep, rays, mean = freeze(txt, all_rays, "scene %d" % s)
        removed = int((~keep).sum())
        moved.append((np.flatnonzero(~keep).astype(np.int32), all_rays[~keep]))
        out["text_%d" % s], out["rays_%d" % s], out["mean_%d" % s] = np.array(txt), rays, mean
        print("trace scene %d: %d rays, %d removed, mean %s" % (s, len(rays), removed, mean.mean(axis=0)))
    np.savez_compressed(os.path.join(HERE, "csgfuzz_trace.npz"),
                        meta=np.array([TRACE_SPP, TRACE_DEPTH, SEED], dtype=np.int64), **out)
    return moved


def make_trace_leaf():
    """csgfuzz_trace_leaf.npz; touches no other fixture"""
    out = {}
    for s in range(F.N_TRACE_SCENES):
        txt = to_text(F.trace_scene(s, leaf=True))
        out["text_%d" % s] = np.array(txt)
        for tag, all_rays in (("", F.trace_rays(s)), ("edge_", F.edge_strength_rays(s))):
            keep, rays, mean = freeze(txt, all_rays, "leaf scene %d %srays" % (s, tag))
            assert not np.isnan(mean).any(), (s, tag)
            out["%srays_%d" % (tag, s)], out["%smean_%d" % (tag, s)] = rays, mean
            out["%smoved_index_%d" % (tag, s)] = np.flatnonzero(~keep).astype(np.int32)
            print("leaf trace scene %d %srays: %d rays, %d removed, mean %s" % (s, tag, len(rays), int((~keep).sum()),
                                                                              mean.mean(axis=0)))
    root, rays = F.regress_resume_negative_count()
    out["regress_text"], out["regress_rays"] = np.array(to_text(root)), rays
    out["regress_mean"] = O.ref_trace_rays(to_text(root), rays, TRACE_SPP, TRACE_DEPTH, seed=SEED)
    print("regress_resume_negative_count: %s" % out["regress_mean"])
    np.savez_compressed(os.path.join(HERE, "csgfuzz_trace_leaf.npz"),
                        meta=np.array([TRACE_SPP, TRACE_DEPTH, SEED], dtype=np.int64), **out)


def make_cap(moved):
    txt = to_text(F.cap_scene())
    cand = F.cap_candidates()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda r: ref_completes(txt, r[None], F.CAP_DEPTH, F.CAP_SPP, threads=1), cand))
    res = [None if r is None else r[0] for r in res]
    aborts = np.array([r is None for r in res])
    ia, ic = np.flatnonzero(aborts)[:CAP_ABORTS], np.flatnonzero(~aborts)[:CAP_COMPLETES]
    assert len(ia) >= 32 and len(ic) >= 96, (len(ia), len(ic))
    idx = np.sort(np.concatenate([ia, ic]))
    mean = np.array([res[i] if res[i] is not None else np.zeros(3, np.float32) for i in idx], np.float32)
    np.savez_compressed(os.path.join(HERE, "csgfuzz_cap.npz"), text=np.array(txt), rays=cand[idx], index=idx.astype(np.int32),
                        aborts=aborts[idx], mean=mean,
                        # the trace scenes' rays the reference asserted on (original indices, rays)
                        **{"moved_index_%d" % s: m[0] for s, m in enumerate(moved)},
                        **{"moved_rays_%d" % s: m[1] for s, m in enumerate(moved)},
                        meta=np.array([F.CAP_SPP, F.CAP_DEPTH, SEED], dtype=np.int64))
    print("cap: %d of %d candidates abort; kept %d aborting, %d completing" % (aborts.sum(), len(cand), len(ia),
                                                                               len(ic)))


def main():
    if not O.ref_available():
        sys.exit("needs `make -C oracle ref` (the reference tree)")
    what = sys.argv[1:] or ["spans", "trace", "trace_leaf"]
    assert set(what) <= {"spans", "trace", "trace_leaf"}, what
    if "spans" in what:
        make_spans()
    if "trace" in what:
        make_cap(make_trace())
    if "trace_leaf" in what:
        make_trace_leaf()


if __name__ == "__main__":
    main()
