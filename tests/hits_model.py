"""What pt_query_hits and pt_render_guides must return, restated in numpy float32 from data the CPU already
has (tests/test_hits_model.py, tests/test_hits_gpu.py, tests/test_guides_gpu.py):

  scan()          traceRay's scan over a root span list (include/path-trace.h:66-100): the first span whose
                  start reaches EPS is an entry, else whose end reaches EPS an exit; a start or an end at or
                  beyond MAXV, and a list that runs out, are misses
  scan_rows()     the same over pt_query_spans' ten-word rows (tests/golden/spans_*.npz "data"), with the
                  normal traceRay shades with: the span's, negated on an exit (:84-96)
  position()      pos = o + t * d, each operation rounded to float32
  camera_rays()   tracePixel's jittered camera ray of (seed, key, sample) (:190-198) from
                  include/pt/pt_engine.h's recurrence: u = float32(uint32) / 2^32, 2 * (px + u) / W - 1
  guide_mean()    a guide plane's rule: the samples summed in float32 from +0 in sample order, / float32(spp)
"""
import re

import numpy as np

f32 = np.float32
EPS, MAXV = f32(1e-3), f32(1e20)
M64 = (1 << 64) - 1


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ scan ---
def scan(cnt, t):
    """cnt: spans per ray; t: (all spans x 2) start, end.  Returns (hit, exit, row, t): row is the index of
    the span hit among all spans (0 on a miss), t is +0 on a miss."""
    cnt = np.asarray(cnt, np.int64)
    t = np.asarray(t, f32).reshape(-1, 2)
    n = len(cnt)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    open_ = np.ones(n, bool)
    hit, ex = np.zeros(n, bool), np.zeros(n, bool)
    row, tt = np.zeros(n, np.int64), np.zeros(n, f32)
    for j in range(int(cnt.max()) if n else 0):
        i = np.flatnonzero(open_ & (cnt > j))
        s, e = t[first[i] + j, 0], t[first[i] + j, 1]
        with np.errstate(invalid="ignore"):
            far_s = s >= MAXV
            at_s = ~far_s & (s >= EPS)
            far_e = ~far_s & ~at_s & (e >= MAXV)
            at_e = ~far_s & ~at_s & ~far_e & (e >= EPS)
        hit[i], ex[i] = at_s | at_e, at_e
        row[i] = np.where(at_s | at_e, first[i] + j, 0)
        tt[i] = np.where(at_s, s, np.where(at_e, e, f32(0))).astype(f32)
        open_[i] = ~(far_s | at_s | far_e | at_e)
    return hit, ex, row, tt


def outcomes(hit, ex):
    """(entries, exits, misses)"""
    return int((hit & ~ex).sum()), int((hit & ex).sum()), int((~hit).sum())


def scan_rows(cnt, data):
    """cnt and the ten-word rows (t, normal, material for the start, then for the end; uint32 views) of
    pt_query_spans / oracle_py.spans.  Returns a dict of the hit record's fields: hit, exit (int32), t,
    normal (n x 3), material (-1 on a miss); every float +0 on a miss."""
    data = np.asarray(data, np.uint32).reshape(-1, 10)
    hit, ex, row, tt = scan(cnt, data[:, [0, 5]].view(f32))
    n = len(hit)
    nrm, mat = np.zeros((n, 3), f32), np.full(n, -1, np.int32)
    if len(data):
        r = data[row]
        start_n, end_n = r[:, 1:4].view(f32), r[:, 6:9].view(f32)
        nrm = np.where(ex[:, None], -end_n, start_n).astype(f32)  # traceRay flips the end normal
        nrm[~hit] = f32(0)
        mat = np.where(hit, np.where(ex, r[:, 9], r[:, 4]).view(np.int32), -1).astype(np.int32)
    return {"hit": hit.astype(np.int32), "exit": ex.astype(np.int32), "t": tt, "normal": nrm, "material": mat}


def rows_from_oracle(spans):
    """oracle_py.spans' records [(t n3, m0, t n3, m1)] per ray as (cnt, ten-word rows)"""
    cnt = np.array([len(sp) for sp in spans], np.int32)
    rows = np.zeros((int(cnt.sum()), 10), np.uint32)
    k = 0
    for sp in spans:
        for (a, m0, b, m1) in sp:
            rows[k, 0:4], rows[k, 4] = u32(a), np.int32(m0).view(np.uint32)
            rows[k, 5:9], rows[k, 9] = u32(b), np.int32(m1).view(np.uint32)
            k += 1
    return cnt, rows


def position(rays, t, hit):
    """o + t * d in float32, +0 on a miss"""
    rays = np.asarray(rays, f32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        pos = (rays[:, :3] + (np.asarray(t, f32)[:, None] * rays[:, 3:6]).astype(f32)).astype(f32)
    pos[~np.asarray(hit, bool)] = f32(0)
    return pos


def expected_hits(rays, cnt, data):
    """the whole record of scan_rows plus pos"""
    w = scan_rows(cnt, data)
    w["pos"] = position(rays, w["t"], w["hit"] != 0)
    return w


# --------------------------------------------------------------- engine ---
def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def engine_draws(seed, key, sample, n):
    """the first n outputs of the engine keyed (seed, key, sample): pt_engine.h"""
    v = splitmix64(splitmix64(seed) ^ ((key << 20) & M64) ^ sample)
    out = []
    for _ in range(n):
        v = (v * 214013 + 2531011) & M64
        out.append(v >> 32)
    return out


def camera_rays(pixels, W, H, gw, screen, seed, sample_begin, spp):
    """(entries x spp x 6) float32: origin 0, direction (x sw, y sh, -dist) with camera_dir's arithmetic"""
    sw, sh, dist = (f32(v) for v in screen)
    rays = np.zeros((len(pixels), spp, 6), f32)
    for k, pix in enumerate(pixels):
        px, py = int(pix) % gw, int(pix) // gw
        for s in range(spp):
            a, b = engine_draws(seed, int(pix), sample_begin + s, 2)
            ux = np.array(a, np.uint32).astype(f32) / f32(4294967296.0)
            uy = np.array(b, np.uint32).astype(f32) / f32(4294967296.0)
            x = f32(2.0) * (f32(px) + ux) / f32(W) - f32(1.0)
            y = f32(1.0) - f32(2.0) * (f32(py) + uy) / f32(H)
            rays[k, s, 3:6] = (x * sw, y * sh, -dist)
    return rays


def guide_mean(x, spp):
    """x: (entries x spp [x c]) per-sample values, +0 on a miss: ((0 + x_0) + x_1) + ... / float32(spp)"""
    x = np.asarray(x, f32)
    acc = np.zeros(x.shape[:1] + x.shape[2:], f32)
    with np.errstate(all="ignore"):
        for s in range(x.shape[1]):
            acc = (acc + x[:, s]).astype(f32)
        return (acc / f32(spp)).astype(f32)


# ------------------------------------------------------------ scene text ---
def materials(scene_text):
    """{material id: (reflect, scatter, emissive, transmit texture ids, ior float32, trc texture id)} of
    the text scene's `mat` lines"""
    out = {}
    for m in re.finditer(r"^mat (\d+) (\d+) (\d+) (\d+) (\d+) (\S+) (\d+)\s*$", scene_text, flags=re.M):
        g = m.groups()
        out[int(g[0])] = (int(g[1]), int(g[2]), int(g[3]), int(g[4]), f32(float.fromhex(g[5])), int(g[6]))
    return out


def expected_shade(scene_text, tex, material, hit):
    """pt_query_hits' shade_out (n x 11) and ior (n) from oracle_py.tex_eval(scene_text, pos) = tex
    (textures x n x 4): emissive, reflect, transmit rgb, scatter and trc values of each hit's material"""
    n = len(material)
    sh, ior = np.zeros((n, 11), f32), np.zeros(n, f32)
    mats = materials(scene_text)
    for i in np.flatnonzero(np.asarray(hit, bool)):
        refl, scat, emis, trans, mi, trc = mats[int(material[i])]
        sh[i, 0:3], sh[i, 3:6], sh[i, 6:9] = tex[emis, i, :3], tex[refl, i, :3], tex[trans, i, :3]
        sh[i, 9], sh[i, 10], ior[i] = tex[scat, i, 3], tex[trc, i, 3], mi
    return sh, ior
