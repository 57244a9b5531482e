"""pt_render_converge (include/pt/pt.h, csrc/device/pt_converge.h) restated in
numpy: f32 exactly where the device uses f32, f64 elsewhere, one operation per
statement so that nothing is contracted or reassociated.

An entry's input is its sequence of 32-sample block sums B_0, B_1, ... (f32
rgb) up to the cap; the model reads only the blocks the entry would have
traced.
"""
import numpy as np


def tree32(vals):
    """pt_tree32 per channel: vals [..., 32 * nb, 3] f32 per-sample values ->
    [..., nb, 3] block sums, each the 32-leaf pairwise tree of its samples."""
    v = np.ascontiguousarray(vals, dtype=np.float32)
    nb = v.shape[-2] // 32
    assert v.shape[-2] == 32 * nb
    b = v.reshape(v.shape[:-2] + (nb, 32, 3))
    for _ in range(5):
        b = b[..., 0::2, :] + b[..., 1::2, :]
        assert b.dtype == np.float32
    return b[..., 0, :]


def schedule(min_spp, cap):
    """the sample count at the end of each possible round: min_spp, then doubling, cut at the cap"""
    ends, n = [], min_spp
    while True:
        ends.append(n)
        if n >= cap:
            return ends
        n = min(2 * n, cap)


def converge(blocks, min_spp, cap, rel_tol, abs_tol=0.0):
    """blocks [n, cap / 32, 3] f32.  Returns rgb [n, 3] f32, spp [n] int32,
    err [n] f32 and info = {rounds, samples, capped}."""
    B = np.ascontiguousarray(blocks, dtype=np.float32)
    n = B.shape[0]
    assert min_spp % 32 == 0 and cap % 32 == 0 and 64 <= min_spp <= cap and B.shape[1] >= cap // 32
    rel, ab = np.float64(np.float32(rel_tol)), np.float64(np.float32(abs_tol))
    acc = np.zeros((n, 3), dtype=np.float32)
    s1 = np.zeros(n, dtype=np.float64)
    s2 = np.zeros(n, dtype=np.float64)
    rgb = np.zeros((n, 3), dtype=np.float32)
    spp = np.zeros(n, dtype=np.int32)
    err = np.zeros(n, dtype=np.float32)
    active = np.ones(n, dtype=bool)
    rounds = samples = capped = 0
    done = 0
    with np.errstate(all="ignore"):
        for end in schedule(min_spp, cap):
            if not active.any():
                break
            rounds += 1
            samples += int(active.sum()) * (end - done)
            for j in range(done // 32, end // 32):
                b = B[:, j, :]
                acc = np.where(active[:, None], acc + b, acc).astype(np.float32)
                y = (b[:, 0] + b[:, 1]) + b[:, 2]
                assert y.dtype == np.float32
                yd = y.astype(np.float64)
                sq = yd * yd
                s1 = np.where(active, s1 + yd, s1)
                s2 = np.where(active, s2 + sq, s2)
            m = np.float64(end // 32)
            bad = ~np.isfinite(s1) | ~np.isfinite(s2)
            sq1 = s1 * s1
            d = s2 - sq1 / m
            v = np.where(d > 0, d, 0.0)
            e2 = v / (m * (m - 1.0))
            ta = 32.0 * ab
            tr = rel * np.abs(s1 / m)
            t = np.where(ta > tr, ta, tr)
            met = e2 <= t * t
            stop = active & (bad | met | (end == cap))
            capped += int(np.sum(active & ~bad & ~met & (end == cap)))
            e = (np.sqrt(e2) / 32.0).astype(np.float32)
            e = np.where(bad, np.float32(np.nan), e).astype(np.float32)
            rgb[stop] = (acc / np.float32(end))[stop]
            spp[stop] = end
            err[stop] = e[stop]
            active &= ~stop
            done = end
    assert not active.any()
    return rgb, spp, err, dict(rounds=rounds, samples=samples, capped=capped)
