"""Scenes, rays and the numpy restatement of the inside-solid probe (pt_device.h Inside,
PT_INSIDE_ZERO) for tests/test_inside_zero.py and tests/golden/make_inside_zero_golden.py.

fires(root, rays) restates the kernel's per-lane predicate and its burst-uniform gates in float32,
operation for operation (each ray is its own burst: the ray's origin is the burst origin, its unit
direction the child's).  scan(spans, emissive) is traceRay's scan (include/path-trace.h:66-96) over a
root span list."""
import numpy as np

import csgfuzz as F
from pathtrace.scene import (ColorTexture, Difference, Intersection, Material, Plane, Sphere, TransformedObject,
                             Union, union_array)

f32 = np.float32
EPS, MAXV = f32(1e-3), f32(1e20)
INF = f32(np.inf)
CENTRE = (0.0, 0.0, -4.0)


def is_emissive(mat):
    e = mat.emissive
    return not (isinstance(e, ColorTexture) and all(float(c) == 0.0 for c in e.color))


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ------------------------------------------------------------- predicate ---
def ok(n):
    """Inside<N>::ok: every plane under Unions only, no emissive sphere, no transform"""
    if isinstance(n, Sphere):
        return not is_emissive(n.material)
    if isinstance(n, Plane):
        return True
    if isinstance(n, Union):
        return ok(n.a) and ok(n.b)
    if isinstance(n, (Difference, Intersection)):
        return sph_only(n)
    return False


def sph_only(n):
    if isinstance(n, Sphere):
        return not is_emissive(n.material)
    if isinstance(n, (Union, Difference, Intersection)):
        return sph_only(n.a) and sph_only(n.b)
    return False


def has_diff_or_isect(n):
    """the clear pass exists (CLEAR: not a union-only tree)"""
    return isinstance(n, (Difference, Intersection)) or any(has_diff_or_isect(c) for c in n.children())


def _sphere(n, o):
    omc = o - np.array(n.center, f32)
    rr = f32(n.r) * f32(n.r)
    return omc, dot(omc, omc) - rr, rr


def emis_lb(n, o):
    if isinstance(n, Sphere):
        return np.full(len(o), INF, f32)
    if isinstance(n, Plane):
        if not is_emissive(n.material):
            return np.full(len(o), INF, f32)
        nv = np.array(n.normal, f32)
        num = -f32(n.d) - dot(o, nv[None, :])
        nn = np.sqrt(dot(nv, nv))
        return np.where(num <= f32(-1e-3), (-num / nn) * f32(0.999), f32(0.0)).astype(f32)
    return np.minimum(emis_lb(n.a, o), emis_lb(n.b, o))


def far2(n, o):
    if isinstance(n, Sphere):
        _, c, rr = _sphere(n, o)
        return c + f32(2.0) * rr
    if isinstance(n, Plane):
        return np.zeros(len(o), f32)
    return np.maximum(far2(n.a, o), far2(n.b, o))


def evaluate(n, o, d, a, mg, xmin):
    """(bmin, bmax, xbest, xlo) per ray"""
    k = len(o)
    none = (np.full(k, -INF, f32), np.full(k, INF, f32), np.full(k, -INF, f32), np.zeros(k, f32))
    if isinstance(n, Sphere):
        omc, c, _ = _sphere(n, o)
        b = dot(omc, d)
        disc = b * b - a * c
        with np.errstate(invalid="ignore"):
            sq = np.sqrt(disc)
        dead = disc <= EPS
        bmin = np.where(dead, INF, -b - sq).astype(f32)
        bmax = np.where(dead, -INF, -b + sq).astype(f32)
        return bmin, bmax, np.where(bmax > xmin, bmax, -INF).astype(f32), bmin
    if isinstance(n, Union):
        A, B = evaluate(n.a, o, d, a, mg, xmin), evaluate(n.b, o, d, a, mg, xmin)
        ta = A[2] >= B[2]
        return none[0], none[1], np.where(ta, A[2], B[2]), np.where(ta, A[3], B[3])
    if isinstance(n, Difference):
        A, B = evaluate(n.a, o, d, a, mg, xmin), evaluate(n.b, o, d, a, mg, xmin)
        with np.errstate(invalid="ignore"):
            passed = (A[2] > B[1] + mg) & (B[0] > A[3] + mg)
        return none[0], none[1], np.where(passed, A[2], -INF).astype(f32), np.maximum(A[3], B[1])
    return none


def gates(root, o):
    """(on, mg, xmin) per origin: T_E > 0 and every sphere's far bound below it"""
    te = np.minimum(emis_lb(root, o), f32(1e15))
    g2 = f32(2.02) * far2(root, o)
    g = np.sqrt(g2)
    return (te > 0) & (g2 < te * te), f32(1e-5) * g, EPS * f32(1.001) + f32(1e-5) * g


def fires(root, rays):
    """the rays (n x 6, unit directions) the first pass would settle with a zero term"""
    rays = np.asarray(rays, f32)
    if not (ok(root) and has_diff_or_isect(root)):
        return np.zeros(len(rays), bool)
    o, d = rays[:, :3], rays[:, 3:6]
    on, mg, xmin = gates(root, o)
    v = evaluate(root, o, d, dot(d, d), mg, xmin)
    return on & (v[2] > 0)


def wfin(rc):
    rc = np.asarray(rc, f32)
    return bool(np.all(np.abs(rc) < f32(1e37)))


# ------------------------------------------------------------------ scan ---
def scan(spans):
    """traceRay's scan: the material index the scan stops on, or -1 for black"""
    for (s, m0, e, m1) in spans:
        if s >= MAXV:
            return -1
        if s >= EPS:
            return int(m0)
        if e >= MAXV:
            return -1
        if e >= EPS:
            return int(m1)
    return -1


def emissive_ids(text):
    """material indices of a text scene whose emissive texture is not black"""
    tex, out = {}, set()
    for ln in text.splitlines():
        w = ln.split()
        if w and w[0] == "tex" and w[2] == "color":
            tex[int(w[1])] = any(float.fromhex(v) != 0.0 for v in w[3:6])
        if w and w[0] == "mat" and tex.get(int(w[4]), True):
            out.add(int(w[1]))
    return out


# ---------------------------------------------------------------- scenes ---
def _mats(leaf=True):
    return F.materials(leaf)


def _scene(parts, M, wall_z=-16.0):
    return union_array(list(parts) + [Plane((0, 1, 0), (0, -2, 0), M[0]), Plane((0, 0, 1), (0, 0, wall_z), M[4])])


def _at(c, dx, dy, dz):
    return (c[0] + dx, c[1] + dy, c[2] + dz)


# the lattice assemblies, float32-exact, around a centre c: name -> builder(c, M)
LATTICE = {
    # a subtractor whose exit equals X's exit exactly on the axis rays: the rule must not fire there
    "exit_tie": lambda c, M: Difference(Sphere(c, 1, M[0]), Sphere(_at(c, 0, 0, -0.5), 0.5, M[1])),
    # a subtractor covering X's exit
    "cover": lambda c, M: Difference(Sphere(c, 1, M[0]), Sphere(_at(c, 0, 0, -1), 1, M[1])),
    # an origin on the cavity whose A exit comes before the B exit: the ray leaves for the wall
    "cavity_short": lambda c, M: Difference(Sphere(c, 1, M[0]), Sphere(_at(c, 0, 0, -0.5), 1, M[0])),
    # (A - B1) - B2 with only B2 past X's exit (for rays along -z)
    "two_subs": lambda c, M: Difference(Difference(Sphere(c, 1, M[0]), Sphere(_at(c, 0, 0, 0.5), 0.75, M[1])),
                                        Sphere(_at(c, 0, 0, -1), 0.5, M[0])),
    # X on a B side
    "x_on_b": lambda c, M: Difference(Sphere(c, 1.5, M[0]), Union(Sphere(_at(c, 0, 0, 1), 1, M[0]),
                                                                  Sphere(_at(c, 0.5, 0, 1), 1, M[1]))),
    # X under an Intersection
    "under_isect": lambda c, M: Intersection(Sphere(c, 1, M[0]), Sphere(_at(c, 0.5, 0, 0), 1, M[0])),
}
GPU_SCENES = ["lat0", "lat1", "behind", "xf", "emis_sphere", "overflow"]
GPU_WALL_Z = -60.0  # the assemblies stand up to 19 apart: every far bound stays below T_E = 56
SPACING = 6.0


def lattice_parts(name):
    """[(assembly name, centre)] of a GPU lattice scene"""
    names = {"lat0": ["exit_tie", "cover", "cavity_short", "two_subs"], "lat1": ["x_on_b", "under_isect", "cavity_short"],
             "behind": ["cavity_short"], "xf": ["cavity_short"], "emis_sphere": ["cavity_short"], "overflow": ["cavity_short"]}[name]
    k = len(names)
    return [(n, ((j - (k - 1) / 2.0) * SPACING, 0.0, -4.0)) for j, n in enumerate(names)]


def lattice_scene(name):
    """the GPU lattice scenes.  behind also has a non-emissive sphere behind the wall (far bound >= T_E:
    no burst takes the rule); xf a transformed sphere and emis_sphere an emissive one (the rule is
    compiled out); overflow a reflectance of 3e37, whose rc fails wfin."""
    M = _mats()
    if name == "overflow":
        M[0] = Material(ColorTexture(3e37), ColorTexture(1))
    parts = [LATTICE[n](c, M) for n, c in lattice_parts(name)]
    if name == "behind":
        parts.append(Sphere((0, 0, -70), 2, M[1]))
    if name == "xf":
        parts.append(TransformedObject(F._about(F.SHEAR, (5.0, 0.0, -4.0)), Sphere((0, 0, 0), 1, M[0])))
    if name == "emis_sphere":
        parts.append(Sphere((5, 0, -4), 0.5, M[4]))
    return _scene(parts, M, GPU_WALL_Z)


def cpu_cases():
    """[(name, root, family)]: every sphere-only assembly of csgfuzz and every lattice case under
    union_array([part, ground, wall]); the spheres take the four non-emissive materials"""
    out = []
    k = 0
    for o in range(3):
        for i in range(3):
            for side in "ab":
                for tag, leaves in (("overlap", F.OVERLAP_LEAVES[F.OVERLAP_PICK[k]]),
                                    ("tie", F.SPHERE_TIE_LEAVES[k % len(F.SPHERE_TIE_LEAVES)])):
                    M = _mats()
                    name = "%s_%s_%s_%s" % (F.OP_NAMES[o][:3], F.OP_NAMES[i][:3], side, tag)
                    out.append((name, _scene([F.nest(o, i, side, leaves, CENTRE, M[:4], k)], M)))
                k += 1
    for side in "ab":
        M = _mats()
        out.append(("diff_chain_" + side, _scene([F.diff_chain(side, CENTRE, M)], M)))
    for n, b in LATTICE.items():
        M = _mats()
        out.append((n, _scene([b(CENTRE, M)], M)))
    M = _mats()
    out.append(("behind_wall", _scene([LATTICE["cavity_short"](CENTRE, M), Sphere((0, 0, -30), 2, M[1])], M)))
    M = _mats()
    out.append(("emis_sphere", _scene([LATTICE["cavity_short"](CENTRE, M), Sphere((3, 0, -4), 0.5, M[4])], M)))
    M = _mats()
    out.append(("xf", _scene([LATTICE["cavity_short"](CENTRE, M),
                              TransformedObject(F._about(F.SHEAR, (5.0, 0.0, -4.0)), Sphere((0, 0, 0), 1, M[0]))], M)))
    return out


NESTED = ("diff_chain_a", "two_subs", "dif_dif_a_overlap", "dif_dif_a_tie")  # a Difference on an A side


def spheres(root):
    return [root] if isinstance(root, Sphere) else [s for ch in root.children() for s in spheres(ch)]


def unit(rays):
    r = np.array(rays, np.float64)
    r[:, 3:6] /= np.linalg.norm(r[:, 3:6], axis=1)[:, None]
    return r.astype(f32)


def case_rays(root, seed, n_span=128, n_surf=96):
    """unit rays: the span_rays families (origins on surfaces, inside solids, at centres, tangents),
    origins on every sphere's surface with directions into and out of it (cavity origins among them),
    and a few origins inside the wall's solid"""
    rng = np.random.default_rng(9000 + seed)
    part = root.a if isinstance(root, Union) else root
    rays = [F.span_rays(part, n=n_span, seed=seed, centre=CENTRE)]
    sph = [s for s in spheres(part) if abs(float(s.center[2])) < 20]
    surf = []
    for k in range(n_surf):
        s = sph[k % len(sph)]
        u = rng.choice(np.array([-1, -0.5, 0, 0.5, 1], f32), size=3)
        if not u.any():
            u[2] = 1
        u = (u.astype(np.float64) / np.linalg.norm(u)).astype(f32)
        o = np.array(s.center, f32) + f32(s.r) * u
        d = rng.uniform(-1, 1, size=3).astype(f32)
        if k % 4 != 3:  # mostly into the sphere: the cavity's children
            d = d - u * f32(1.0 + np.dot(d, u))
        surf.append(np.concatenate([o, d]))
    for k in range(8):
        surf.append(np.array([k - 4.0, 0.5, -17.0 - k, 0.25 * (k - 4), 0.0, 1.0], f32))
    return unit(np.concatenate([rays[0], np.array(surf, f32)]))
