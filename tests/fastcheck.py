"""The CSG fast check (pt_device.h sep / inert / pair_ok / fast_ok / fast_first_hit) restated in numpy,
float32, operation for operation, with the scenes and rays that put it on the seam of two spheres, for
tests/test_fastcheck.py, tests/golden/make_fastcheck_golden.py and tools/fastcheck_model.py.

The check runs over the primitives' own spans (Sph::init, Pln::init): where fast_ok holds on a ray,
fast_first_hit over the positive primitives must be what traceRay's scan (include/path-trace.h:66-100)
finds in the root span list of the lazy merges.  It works over trees of Sphere, Plane, Union, Difference
and Intersection; any other node makes fast_ok false.

RULE selects the pair rule: "header" is pair_ok as pt_device.h has it (PAIR_OK_BODY below is the text it
was written from; tests/test_fastcheck.py pins the header to it), the others are the variants
tools/fastcheck_model.py counts:
  "inert_everywhere"  the rule before the seam fix: inert passes a pair at every Union node, and an
                      Intersection's pairs may both end before EPS anywhere.  Unsound under
                      Difference(Union(x1, x2), y) and under Difference(y, Intersection(x1, x2))
  "no_union_inert"    that rule without the inert clause at any Union node
  "no_diff_inert"     that rule without the inert clause at a Difference
  "lens_before_eps"   the header's rule, but an Intersection below a Difference may still hold a span
                      that ends before EPS
"""
import numpy as np

import csgfuzz as F
from inside_zero import _scene, dot, unit
from pathtrace import scenes
from pathtrace.scene import Difference, Intersection, Plane, Sphere, Union

f32 = np.float32
EPS, MAXV = f32(1e-3), f32(1e20)
EPS2 = EPS * EPS
CENTRE = (0.0, 0.0, -4.0)
RULES = ("header", "inert_everywhere", "no_union_inert", "no_diff_inert", "lens_before_eps")
NODE_ISECT, NODE_UNION, NODE_DIFF = 0, 1, 2

# pair_ok's body in pt_device.h, whitespace collapsed: what pair_ok() below restates under RULE "header"
PAIR_OK_BODY = (
    "int ok = (KIND == NODE_ISECT && D) ? apart(ps, x, y) : sep(ps, x, y); "
    "if (KIND == NODE_UNION) "
    "ok |= ((ps.t0[x] >= EPS) & (ps.t0[y] >= EPS) & (ps.t0[x] != ps.t0[y])) | (!D & (inert(ps, x) | inert(ps, y))); "
    "if (KIND == NODE_DIFF) "
    "ok |= ((ps.t0[x] >= EPS) & (ps.t0[y] > ps.t0[x])) | inert(ps, x); "
    "return ok;")


# ------------------------------------------------------- primitive spans ---
def primitives(root):
    """the tree's spheres and planes in the device's order (A before B)"""
    if isinstance(root, (Sphere, Plane)):
        return [root]
    return [p for ch in root.children() for p in primitives(ch)]


def material_ids(root):
    """material index per primitive as the text scene numbers them: by first use, A before B"""
    ids, out = {}, []
    for p in primitives(root):
        out.append(ids.setdefault(id(p.material), len(ids)))
    return out


def sphere_span(n, o, d, a):
    """Sph::init: (t0, t1, live)"""
    omc = o - np.array(n.center, f32)
    c = dot(omc, omc) - f32(n.r) * f32(n.r)
    b = dot(omc, d)
    disc = b * b - a * c
    live = ~(disc <= EPS)
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
    return ((-b - sq) / a).astype(f32), ((-b + sq) / a).astype(f32), live


def plane_span(n, o, d):
    """Pln::init: (t0, t1, live)"""
    nv = np.array(n.normal, f32)[None, :]
    num = -f32(n.d) - dot(o, nv)
    div = dot(d, nv)
    small = np.abs(div) < EPS2
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (num / div).astype(f32)
    with np.errstate(invalid="ignore"):
        deg = small | (np.abs(t) >= MAXV)
    neg = div < 0
    live = ~deg | (np.abs(num) < EPS2)
    return (np.where(~deg & neg, t, -MAXV).astype(f32), np.where(~deg & ~neg, t, MAXV).astype(f32), live)


class PrimSpans:
    """t0, t1, live (primitives x rays) and each primitive's material index"""

    def __init__(self, root, rays):
        rays = np.asarray(rays, f32)
        o, d = rays[:, :3], rays[:, 3:6]
        a = dot(d, d)
        sp = [sphere_span(p, o, d, a) if isinstance(p, Sphere) else plane_span(p, o, d) for p in primitives(root)]
        self.t0, self.t1 = np.array([s[0] for s in sp], f32), np.array([s[1] for s in sp], f32)
        self.live = np.array([s[2] for s in sp], bool)
        self.mat = material_ids(root)
        self.n = len(rays)


# ----------------------------------------------------------------- rules ---
def apart(ps, x, y):
    with np.errstate(invalid="ignore"):
        return (~ps.live[x]) | (~ps.live[y]) | (ps.t1[x] < ps.t0[y]) | (ps.t1[y] < ps.t0[x])


def sep(ps, x, y):
    with np.errstate(invalid="ignore"):
        return apart(ps, x, y) | ((ps.t1[x] < EPS) & (ps.t1[y] < EPS))


def inert(ps, x):
    with np.errstate(invalid="ignore"):
        return ps.live[x] & (ps.t1[x] < EPS)


def pair_ok(kind, ps, x, y, d, rule="header"):
    """pair_ok<KIND, D>; d: the node lies below some Difference"""
    ok = apart(ps, x, y) if kind == NODE_ISECT and d and rule == "header" else sep(ps, x, y)
    with np.errstate(invalid="ignore"):
        if kind == NODE_UNION:
            ok = ok | ((ps.t0[x] >= EPS) & (ps.t0[y] >= EPS) & (ps.t0[x] != ps.t0[y]))
            if (rule in ("header", "lens_before_eps") and not d) or rule in ("inert_everywhere", "no_diff_inert"):
                ok = ok | inert(ps, x) | inert(ps, y)
        if kind == NODE_DIFF:
            ok = ok | ((ps.t0[x] >= EPS) & (ps.t0[y] > ps.t0[x]))
            if rule != "no_diff_inert":
                ok = ok | inert(ps, x)
    return ok


def _walk(n, ps, k, d, rule):
    """(ok per ray, positive primitive indices, next primitive index) of the subtree whose first primitive is k"""
    if isinstance(n, (Sphere, Plane)):
        return np.ones(ps.n, bool), [k], k + 1
    if not isinstance(n, (Union, Difference, Intersection)):
        return np.zeros(ps.n, bool), [], k + len(primitives(n))
    kind = NODE_UNION if isinstance(n, Union) else NODE_DIFF if isinstance(n, Difference) else NODE_ISECT
    oka, pa, k = _walk(n.a, ps, k, d or kind == NODE_DIFF, rule)
    okb, pb, k = _walk(n.b, ps, k, d or kind == NODE_DIFF, rule)
    ok = oka & okb
    for x in pa:
        for y in pb:
            ok = ok & pair_ok(kind, ps, x, y, d, rule)
    pos = pa + pb if kind == NODE_UNION else pa if kind == NODE_DIFF else []
    return ok, pos, k


def supported(n):
    if isinstance(n, (Sphere, Plane)):
        return True
    return isinstance(n, (Union, Difference, Intersection)) and supported(n.a) and supported(n.b)


def positives(root):
    """each_pos: primitives reached through Unions and Difference A sides, not through an Intersection"""
    return _walk(root, PrimSpans(root, np.zeros((0, 6), f32)), 0, False, "header")[1] if supported(root) else []


def fast_ok(root, ps, rule="header"):
    if not supported(root):
        return np.zeros(ps.n, bool)
    return _walk(root, ps, 0, False, rule)[0]


def fast_first_hit(root, ps):
    """(hit, t, material) per ray; valid where fast_ok holds"""
    found = np.zeros(ps.n, bool)
    b0, b1 = np.zeros(ps.n, f32), np.zeros(ps.n, f32)
    bm = np.zeros(ps.n, np.int64)
    with np.errstate(invalid="ignore"):
        for x in positives(root):
            cand = ps.live[x] & (ps.t1[x] >= EPS)
            better = cand & (~found | (ps.t0[x] < b0))
            b0, b1 = np.where(better, ps.t0[x], b0), np.where(better, ps.t1[x], b1)
            bm = np.where(better, ps.mat[x], bm)
            found |= cand
        near = found & ~(b0 >= MAXV)
        entry = near & (b0 >= EPS)
        leave = near & ~(b0 >= EPS) & ~(b1 >= MAXV)
    return entry | leave, np.where(entry, b0, b1).astype(f32), bm


def scan(spans):
    """traceRay's scan over a root span list [(start, m0, end, m1)]: (hit, t, material)"""
    for (s, m0, e, m1) in spans:
        if s >= MAXV:
            return False, f32(0), -1
        if s >= EPS:
            return True, f32(s), int(m0)
        if e >= MAXV:
            return False, f32(0), -1
        if e >= EPS:
            return True, f32(e), int(m1)
    return False, f32(0), -1


def span_arrays(spans):
    """oracle_py's span records as (cnt per ray, t (spans x 2: start, end), m (spans x 2: their materials))"""
    cnt = np.array([len(sp) for sp in spans], np.int32)
    t = np.array([[s[0][0], s[2][0]] for sp in spans for s in sp], f32).reshape(-1, 2)
    m = np.array([[s[1], s[3]] for sp in spans for s in sp], np.int16).reshape(-1, 2)
    return cnt, t, m


def span_lists(cnt, t, m):
    """the same as [(start, m0, end, m1)] per ray"""
    pos = np.concatenate([[0], np.cumsum(cnt)])
    return [[(t[j, 0], m[j, 0], t[j, 1], m[j, 1]) for j in range(pos[i], pos[i + 1])] for i in range(len(cnt))]


def scan_arrays(cnt, t, m):
    """scan() over every ray's list at once: (hit, t, material) arrays"""
    n = len(cnt)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    open_ = np.ones(n, bool)
    hit, tt, mm = np.zeros(n, bool), np.zeros(n, f32), np.full(n, -1, np.int64)
    for j in range(int(cnt.max()) if n else 0):
        i = np.flatnonzero(open_ & (cnt > j))
        s, e = t[first[i] + j, 0], t[first[i] + j, 1]
        with np.errstate(invalid="ignore"):
            far_s = s >= MAXV
            at_s = ~far_s & (s >= EPS)
            far_e = ~far_s & ~at_s & (e >= MAXV)
            at_e = ~far_s & ~at_s & ~far_e & (e >= EPS)
        hit[i] = at_s | at_e
        tt[i] = np.where(at_s, s, np.where(at_e, e, 0)).astype(f32)
        mm[i] = np.where(at_s, m[first[i] + j, 0], np.where(at_e, m[first[i] + j, 1], -1))
        open_[i] = ~(far_s | at_s | far_e | at_e)
    return hit, tt, mm


def disagreements(root, rays, cnt, t, m, rule="header"):
    """(the rays where fast_ok holds and fast_first_hit is not the scan's answer in hit / miss, t bits and
    material, the rays where fast_ok holds): two masks"""
    ps = PrimSpans(root, rays)
    ok = fast_ok(root, ps, rule)
    hit, tf, mf = fast_first_hit(root, ps)
    h, ts, ms = scan_arrays(cnt, t, m)
    bad = (h != hit) | (h & ((ts.view(np.uint32) != tf.view(np.uint32)) | (ms != mf)))
    return ok & bad, ok


def inverted(cnt, t):
    """rays whose root list holds a span that ends before it starts"""
    ray = np.repeat(np.arange(len(cnt)), cnt)
    out = np.zeros(len(cnt), bool)
    out[ray[t[:, 1] < t[:, 0]]] = True
    return out


def a_side(n, k=0, on_b=False):
    """(indices of the primitives below no Difference's B side, next index): the positives, and the
    primitives an Intersection keeps from being positive"""
    if isinstance(n, (Sphere, Plane)):
        return ([] if on_b else [k]), k + 1
    out = []
    for j, ch in enumerate(n.children()):
        idx, k = a_side(ch, k, on_b or (isinstance(n, Difference) and j == 1))
        out += idx
    return out, k


def reaches(root, ps):
    """rays on which the own span of some primitive below no B side reaches EPS"""
    out = np.zeros(ps.n, bool)
    with np.errstate(invalid="ignore"):
        for x in a_side(root)[0]:
            out |= ps.live[x] & (ps.t1[x] >= EPS)
    return out


# ------------------------------------------------------------ seam trees ---
# x1 and x2 overlap; y lies behind x1 on their common centre line (along x), overlapping x1 and clear
# of x2.  Around c, the ray from c along +x has the spans x1 [-2, 0], x2 [-0.5, 1.5], y [-3, -1]: under
# Difference(Union(x1, x2), y) the reference's root list is the one inverted span [-2, -3].
SEAM_LEAVES = [("s", -1, 0, 0, 1), ("s", 0.5, 0, 0, 1), ("s", -2, 0, 0, 1)]
# under an inner Intersection the solid is the lens of x1 and x2 (x in -0.5 .. 0 around c), which that y
# does not reach: there y overlaps the lens from the side
SEAM_LEAVES_LENS = [("s", -1, 0, 0, 1), ("s", 0.5, 0, 0, 1), ("s", -1, 0.5, 0, 1)]
MINIMAL = "dif_uni_a"
MINIMAL_RAY = np.array([[CENTRE[0], CENTRE[1], CENTRE[2], 1, 0, 0]], f32)
DISPLACE = (0.0, 1e-6, -1e-6, 1e-4, -1e-4, 5e-4, -5e-4, 1e-3, -1e-3, 2e-3, -2e-3)


def seam_part(name, c=CENTRE, M=None):
    """outer(inner(x1, x2), y) (side a) or outer(y, inner(x1, x2)) (side b) of a tree name like dif_uni_a"""
    M = F.materials(leaf=True) if M is None else M
    o, i, side = name.split("_")
    short = [n[:3] for n in F.OP_NAMES]
    leaves = SEAM_LEAVES_LENS if i == "int" else SEAM_LEAVES
    return F.nest(short.index(o), short.index(i), side, leaves, c, M[:4], 0)


def seam_names():
    return ["%s_%s_%s" % (o[:3], i[:3], s) for o in F.OP_NAMES for i in F.OP_NAMES for s in "ab"]


def seam_trees():
    """[(name, bare assembly, the assembly under union_array([part, ground, emissive wall]))]"""
    out = []
    for name in seam_names():
        M = F.materials(leaf=True)
        out.append((name, seam_part(name, M=M), _scene([seam_part(name, M=M)], M)))
    return out


def seam_trees_scene(name):
    """the scene of one seam tree, built anew"""
    M = F.materials(leaf=True)
    return _scene([seam_part(name, M=M)], M)


def spheres(root):
    return [p for p in primitives(root) if isinstance(p, Sphere)]


def seam_circles(root):
    """[(centre m, axis w, orthonormal e1, e2, radius)] of every pair of spheres whose surfaces meet"""
    out = []
    sph = spheres(root)
    for i in range(len(sph)):
        for j in range(i + 1, len(sph)):
            c1, c2 = np.array(sph[i].center, np.float64), np.array(sph[j].center, np.float64)
            r1, r2 = float(sph[i].r), float(sph[j].r)
            dist = np.linalg.norm(c2 - c1)
            if dist == 0 or dist >= r1 + r2 or dist <= abs(r1 - r2):
                continue
            w = (c2 - c1) / dist
            h = (dist * dist + r1 * r1 - r2 * r2) / (2 * dist)
            e1 = np.cross(w, [0.0, 1.0, 0.0] if abs(w[1]) < 0.9 else [1.0, 0.0, 0.0])
            e1 /= np.linalg.norm(e1)
            out.append((c1 + h * w, w, e1, np.cross(w, e1), np.sqrt(r1 * r1 - h * h)))
    return out


def seam_points(root, rng, n, upper=False):
    """n x (point, axis, outward radial): points of the seam circles moved across them by DISPLACE, in
    turn along the centre line and along the circle's radius; upper: on the circles' upper halves"""
    circ = seam_circles(root)
    out = []
    for k in range(n):
        m, w, e1, e2, rho = circ[k % len(circ)]
        th = rng.uniform(0, 2 * np.pi)
        u = np.cos(th) * e1 + np.sin(th) * e2
        u = -u if upper and u[1] < 0 else u
        dv = DISPLACE[(k // len(circ)) % len(DISPLACE)]
        p = m + rho * u + dv * (w if (k // (len(circ) * len(DISPLACE))) % 2 == 0 else u)
        out.append((p, w, u))
    return out


def _directions(rng, w, u, k):
    """lattice directions along the centre line, then random ones"""
    if k % 4 == 0:
        return w * (1 if (k // 4) % 2 else -1)
    if k % 4 == 1:
        s = rng.choice([-1.0, -0.5, 0.5, 1.0], size=2)
        return s[0] * w + s[1] * u
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def rays_at(root, n, rng):
    rays = []
    for k, (p, w, u) in enumerate(seam_points(root, rng, n)):
        rays.append(np.concatenate([p, _directions(rng, w, u, k)]))
    return unit(np.array(rays))


def seam_rays(root, seed, n=704):
    """unit rays (n x 6) whose origins lie on and beside the seam circles of the tree's spheres; for the
    seam trees the first is MINIMAL_RAY"""
    return np.concatenate([MINIMAL_RAY, rays_at(root, n - 1, np.random.default_rng(8100 + seed))])


# rays of the C3 scene on which the rule with inert at every Union passes every pair and
# fast_first_hit is not the scan's answer (found with tools/fastcheck_model.py); the first is a child
# of the bench frame's pixel column x = 725
C3_FOUND = np.array([
    [1.1081421, 0.16922468, -4.6035752, 0.029953545, 0.32189399, -0.94630182],
    [1.4175101518630981, 0.3239549398422241, -3.716024398803711, 0.8164966702461243, 0.4082483649253845, -0.4082479774951935],
    [1.0639042854309082, 0.1789098083972931, -4.568282127380371, -0.10831774026155472, -0.01236496027559042, -0.9940394163131714],
    [1.2937073707580566, 0.4843079745769501, -3.803277015686035, 0.1705353558063507, 0.8709198832511902, -0.4608863294124603],
    [-0.7480000257492065, -0.4618385434150696, -3.7098186016082764, 0.27555567026138306, -0.8719694018363953, -0.404646098613739],
], f32)


def c3_seam_rays(seed, n=4096):
    root = scenes.scene_p1()
    return np.concatenate([C3_FOUND, rays_at(root, n - len(C3_FOUND), np.random.default_rng(8200 + seed))])


# ------------------------------------------------------------- GPU inputs ---
def aimed_rays(root, seed, n=264):
    """n x 7 caller rays from outside the assembly at the seam points and beside them: the primary hit,
    the bursts' origin, is then on the seam.  Strength 1."""
    rng = np.random.default_rng(8300 + seed)
    rays = []
    for k, (p, w, u) in enumerate(seam_points(root, rng, n, upper=True)):
        o = p + 3.0 * u + (0.5 * rng.uniform(-1, 1)) * w
        rays.append(np.concatenate([o, p - o, [1.0]]))
    return np.array(rays, f32)


SEAM_FRAME = dict(W=48, H=27, spp=4, depth=3, screen=(48.0, 27.0, 40.0))
# the 8 pixels of the C3 bench frame that differed from the oracle (profiles/round10/frame_diff_passes.txt),
# each with its two neighbours in x
C3_BAD = [1079765, 1081685, 1083605, 1085525, 1091286, 1098966, 1102806, 1104726]
C3_PIXELS = sorted(p + dx for p in C3_BAD for dx in (-1, 0, 1))
C3_SPP, C3_DEPTH = 1024, 8
