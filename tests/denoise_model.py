"""pt_denoise (include/pt/pt.h, csrc/device/pt_denoise.h) restated in numpy float32: one operation per
statement, in the device's order, so that nothing is contracted or reassociated and the bits agree.

    denoise(rgb, normal, t, material, err=None, albedo=None, emission=None, **params) -> (out, var)

All planes are H x W (x 3).  params: iterations, sigma_l, sigma_z, normal_power_log2, demodulate.
`passes` returns the (signal, variance) buffers after prepare and after every pass as well.
"""
import numpy as np

f32 = np.float32
DEFAULTS = dict(iterations=5, sigma_l=2.0, sigma_z=0.1, normal_power_log2=5, demodulate=True)
K = (f32(0.375), f32(0.25), f32(0.0625))
INF = f32(np.inf)


def _f(a):
    return np.ascontiguousarray(a, dtype=f32)


def lum(s):
    y = (s[..., 0] + s[..., 1]) + s[..., 2]
    assert y.dtype == f32
    return y


def edge(x):
    """E(x) = (1 - x)^2 below 1, else 0; 0 for a NaN"""
    u = f32(1.0) - x
    return np.where(x < f32(1.0), u * u, f32(0.0)).astype(f32)


def shifted(a, dy, dx):
    """a[clamp(y + dy), clamp(x + dx)] and the mask of the (y, x) whose (y + dy, x + dx) is in the image"""
    h, w = a.shape[:2]
    yy, xx = np.arange(h) + dy, np.arange(w) + dx
    inside = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
    return a[np.clip(yy, 0, h - 1)][:, np.clip(xx, 0, w - 1)], inside


def albedo_of(albedo, demodulate, shape):
    if not demodulate:
        a = np.ones(shape + (3,), f32)
        return a, np.ones(shape, f32)
    al = _f(albedo)
    a = np.where(al > f32(0.01), al, f32(0.01)).astype(f32)
    abar = ((a[..., 0] + a[..., 1]) + a[..., 2]) / f32(3.0)
    assert abar.dtype == f32
    return a, abar


def prepare(rgb, normal, t, material, err, albedo, emission, demodulate):
    """(s [H, W, 3], v [H, W], nhat [H, W, 3])"""
    rgb, normal = _f(rgb), _f(normal)
    shape = rgb.shape[:2]
    a, abar = albedo_of(albedo, demodulate, shape)
    s = ((rgb - _f(emission)) / a).astype(f32) if demodulate else rgb.copy()
    if err is not None:
        e = _f(err)
        v = np.where(np.isfinite(e), (e * e) / (abar * abar), f32(0.0)).astype(f32)
    else:
        y = lum(s)
        n, s1 = np.zeros(shape, f32), np.zeros(shape, f32)
        taps = []
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                yq, inside = shifted(y, dy, dx)
                mq, _ = shifted(material, dy, dx)
                ok = inside & (mq == material) & np.isfinite(yq)
                n = np.where(ok, n + f32(1.0), n).astype(f32)
                s1 = np.where(ok, s1 + yq, s1).astype(f32)
                taps.append((yq, ok))
        mean = s1 / n
        s2 = np.zeros(shape, f32)
        for yq, ok in taps:
            d = yq - mean
            s2 = np.where(ok, s2 + d * d, s2).astype(f32)
        v = np.where(n >= f32(2.0), s2 / (n - f32(1.0)), f32(0.0)).astype(f32)
    nx, ny, nz = normal[..., 0], normal[..., 1], normal[..., 2]
    n2 = (nx * nx + ny * ny) + nz * nz
    ln = np.sqrt(n2)
    nhat = np.where((n2 > 0)[..., None], normal / ln[..., None], f32(0.0)).astype(f32)
    assert s.dtype == f32 and v.dtype == f32 and n2.dtype == f32
    return s, v, nhat


def atrous(s, v, nhat, t, material, step, sigma_l, sigma_z, npow):
    """one pass: (s', v')"""
    shape = v.shape
    sigma_l, sigma_z = f32(sigma_l), f32(sigma_z)
    vt = np.zeros(shape, f32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            g = f32(0.5 if dy == 0 else 0.25) * f32(0.5 if dx == 0 else 0.25)
            vq, _ = shifted(v, dy, dx)
            mq, _ = shifted(material, dy, dx)
            vt = vt + g * np.where(mq == material, vq, v)
    den = sigma_l * np.sqrt(np.where(vt > 0, vt, f32(0.0)).astype(f32)) + f32(1e-4)
    assert vt.dtype == f32 and den.dtype == f32
    lum_off = sigma_l == INF
    yp = lum(s)
    miss = material == -1
    sc, sv, sw = np.zeros(shape + (3,), f32), np.zeros(shape, f32), np.zeros(shape, f32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            h = K[abs(dy)] * K[abs(dx)]
            if dy == 0 and dx == 0:
                w, sq, vq = np.full(shape, h, f32), s, v
            else:
                sq, inside = shifted(s, step * dy, step * dx)
                vq, _ = shifted(v, step * dy, step * dx)
                nq, _ = shifted(nhat, step * dy, step * dx)
                tq, _ = shifted(t, step * dy, step * dx)
                mq, _ = shifted(material, step * dy, step * dx)
                dot = (nhat[..., 0] * nq[..., 0] + nhat[..., 1] * nq[..., 1]) + nhat[..., 2] * nq[..., 2]
                wn = np.where(dot > 0, dot, f32(0.0)).astype(f32)
                for _ in range(npow):
                    wn = wn * wn
                d = np.abs(t - tq)
                tm = np.where(t > tq, t, tq)
                wz = np.where(d > 0, edge(d / (sigma_z * tm)), f32(1.0)).astype(f32)
                wn = np.where(miss, f32(1.0), wn).astype(f32)
                wz = np.where(miss, f32(1.0), wz).astype(f32)
                dl = np.abs(yp - lum(sq))
                if lum_off:
                    wl = np.where(dl < INF, f32(1.0), f32(0.0)).astype(f32)
                else:
                    wl = edge(dl / den)
                w = ((h * wn) * wz) * wl
                w = np.where(inside & (mq == material), w, f32(0.0)).astype(f32)
            assert w.dtype == f32
            take = w > 0
            sc = np.where(take[..., None], sc + w[..., None] * sq, sc).astype(f32)
            sv = np.where(take, sv + (w * w) * vq, sv).astype(f32)
            sw = np.where(take, sw + w, sw).astype(f32)
    return (sc / sw[..., None]).astype(f32), (sv / (sw * sw)).astype(f32)


def passes(rgb, normal, t, material, err=None, albedo=None, emission=None, **params):
    """[(s, v) after prepare, after pass 0, ...] and (a, abar, e) for finalise"""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **params)
    t, material = _f(t), np.ascontiguousarray(material, dtype=np.int32)
    with np.errstate(all="ignore"):
        s, v, nhat = prepare(rgb, normal, t, material, err, albedo, emission, p["demodulate"])
        out = [(s, v)]
        for i in range(p["iterations"]):
            s, v = atrous(s, v, nhat, t, material, 1 << i, p["sigma_l"], p["sigma_z"], p["normal_power_log2"])
            out.append((s, v))
    return out, p


def denoise(rgb, normal, t, material, err=None, albedo=None, emission=None, **params):
    """(out [H, W, 3], var [H, W])"""
    bufs, p = passes(rgb, normal, t, material, err, albedo, emission, **params)
    s, v = bufs[-1]
    if not p["demodulate"]:
        return s.copy(), v.copy()
    with np.errstate(all="ignore"):
        a, abar = albedo_of(albedo, True, v.shape)
        out = _f(emission) + s * a
        var = v * (abar * abar)
    assert out.dtype == f32 and var.dtype == f32
    return out, var


def same_bits(a, b):
    """elementwise: the same bits, or both NaN (a NaN's payload is the hardware's business)"""
    a, b = _f(a), _f(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
