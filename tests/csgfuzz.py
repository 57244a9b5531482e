"""Adversarial CSG inputs: span trees whose span ends tie exactly, the rays that
reach the ties, small trace scenes made of the same assemblies, and the scene
that reaches the reference's `count > 1000` early return
(include/path-trace.h:144-157).

Everything is deterministic (fixed seeds, numpy default_rng, float32) and sits
on a lattice float32 represents exactly -- centres and plane points on
multiples of 0.5, radii 0.5 / 1 / 1.5 -- so a tie between two span ends is an
equality of floats, not a near miss.  Shared by tests/golden/make_csgfuzz_golden.py
(which freezes the unmodified reference's outputs), tests/test_csgfuzz.py and
tests/precompile_modules.py."""
import numpy as np

from pathtrace.scene import (ColorTexture, Difference, Intersection, Material, Matrix, Plane, Sphere,
                             TransformedObject, Union, union_array)

OPS = (Union, Intersection, Difference)
OP_NAMES = ("union", "intersection", "difference")
# census kinds: an A span end equal to a B span end (tests/golden/make_csgfuzz_golden.py)
TIE_KINDS = ("a0==b0", "a1==b1", "a1==b0", "b1==a0")

# negative determinant + anisotropic scale; shear + translation (constructor order x00 x10 x20 x30 ...)
FLIP_SCALE = Matrix(-1.0, 0.0, 0.0, 0.5, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.5, -2.0)
SHEAR = Matrix(1.0, 0.5, 0.0, 0.0, 0.0, 1.0, 0.25, 0.5, 0.0, 0.0, 1.0, 0.0)
XFORMS = (("flip", FLIP_SCALE), ("shear", SHEAR))


def materials(leaf=False):
    """the five materials of zoo.csg_zoo: diffuse, glossy, glass, mirror, emitter.  `leaf` lowers the
    glossy reflectance from 0.9 to 0.5 and changes nothing else: a burst's child then carries at most
    0.5 sqrt(3) (2e-4 / 0.3) 1.01 = 5.8e-4 < eps of strength, every burst of the scene ends in leaves
    (reach_facts["bursts_all_leaf"]) and the lane-resume form is built (tests/test_lane_resume_csg.py)."""
    diffuse = Material(ColorTexture(0.8, 0.7, 0.6), ColorTexture(1))
    glossy = Material(ColorTexture(0.5 if leaf else 0.9), ColorTexture(0.3))
    glass = Material(ColorTexture(0.7), ColorTexture(0), ColorTexture(0), ColorTexture(0.9, 0.95, 1.0), 1.45,
                     ColorTexture(0.8))
    mirror = Material(ColorTexture(0.99), ColorTexture(0))
    emit = Material(ColorTexture(0), ColorTexture(0), ColorTexture(1.5, 1.2, 0.9))
    return [diffuse, glossy, glass, mirror, emit]


# ------------------------------------------------------------------ leaves ---
# A leaf set is three primitives (x, y: the inner node's operands; z: the outer
# node's other operand) around `c`, each given as ("s", dx, dy, dz, r) or
# ("p", nx, ny, nz, px, py, pz) relative to c.
OVERLAP_LEAVES = [
    [("s", 0, 0, 0, 1), ("s", 0.5, 0, 0, 1), ("s", 0, 0.5, -0.5, 1)],
    [("s", -0.5, 0, 0, 1.5), ("s", 0.5, 0.5, 0, 1), ("s", 0, -0.5, 0.5, 1)],
    [("s", 0, 0, 0, 1.5), ("s", 1, 0, 0, 1), ("s", -1, 0, 0.5, 1)],
]
TIE_LEAVES = [
    # coincident spheres; z touches them at (+1, 0, 0)
    [("s", 0, 0, 0, 1), ("s", 0, 0, 0, 1), ("s", 2, 0, 0, 1)],
    # touching spheres (at the centre); z shares x's far end and covers the contact
    [("s", -1, 0, 0, 1), ("s", 1, 0, 0, 1), ("s", -0.5, 0, 0, 1.5)],
    # nested spheres, tangent from inside at (+1.5, 0, 0); z tangent from inside at (-1.5, 0, 0)
    [("s", 0, 0, 0, 1.5), ("s", 0.5, 0, 0, 1), ("s", -1, 0, 0, 0.5)],
    # duplicate planes (y < 0.5 twice); z the abutting half-space y > 0.5
    [("p", 0, 1, 0, 0, 0.5, 0), ("p", 0, 1, 0, 0, 0.5, 0), ("p", 0, -1, 0, 0, 0.5, 0)],
    # abutting half-spaces x < 0 | x > 0; z a sphere centred on the contact plane
    [("p", 1, 0, 0, 0, 0, 0), ("p", -1, 0, 0, 0, 0, 0), ("s", 0, 0, 0, 1.5)],
    # a sphere B covers (concentric), z coincident with the cover
    [("s", 0, 0, 0, 1), ("s", 0, 0, 0, 1.5), ("s", 0, 0, 0, 1.5)],
]
# sphere-only sets (trace scenes: planes would reach the neighbouring assemblies)
SPHERE_TIE_LEAVES = [t for t in TIE_LEAVES if all(p[0] == "s" for p in t)]

CENTRE = (0.0, 0.0, -4.0)


def _leaf(spec, c, mat):
    if spec[0] == "s":
        return Sphere((c[0] + spec[1], c[1] + spec[2], c[2] + spec[3]), spec[4], mat)
    return Plane(spec[1:4], (c[0] + spec[4], c[1] + spec[5], c[2] + spec[6]), mat)


def nest(outer, inner, side, leaves, c, M, m0=0):
    """outer(inner(x, y), z) for side "a", outer(z, inner(x, y)) for side "b" """
    x, y, z = (_leaf(s, c, M[(m0 + k) % len(M)]) for k, s in enumerate(leaves))
    node = OPS[inner](x, y)
    return OPS[outer](node, z) if side == "a" else OPS[outer](z, node)


def diff_chain(side, c, M):
    """Difference chains three deep on one side, four spheres along x"""
    s = [Sphere((c[0] + dx, c[1], c[2]), r, M[k]) for k, (dx, r) in
         enumerate([(0, 1.5), (1, 1), (-1, 1), (0, 0.5)])]
    if side == "a":
        return Difference(Difference(Difference(s[0], s[1]), s[2]), s[3])
    return Difference(s[0], Difference(s[1], Difference(s[2], s[3])))


def slab(k, c, M):
    """two planes whose half-spaces overlap (Plane(n, p) is n.p + d < 0), cut by a sphere"""
    if k == 0:  # -1 < y < 1
        sl = Intersection(Plane((0, 1, 0), (0, c[1] + 1, 0), M[0]), Plane((0, -1, 0), (0, c[1] - 1, 0), M[1]))
        return Intersection(Sphere(c, 1.5, M[2]), sl)
    # c.x - 0.5 < x < c.x + 0.5, taken out of a sphere
    sl = Intersection(Plane((1, 0, 0), (c[0] + 0.5, 0, 0), M[3]), Plane((-1, 0, 0), (c[0] - 0.5, 0, 0), M[0]))
    return Difference(Sphere(c, 1.5, M[1]), sl)


def random_tree(rng, depth, c, M, planes=True):
    if depth == 0:
        if planes and rng.random() < 0.2:
            n = [0.0, 0.0, 0.0]
            n[int(rng.integers(3))] = float(rng.choice([-1.0, 1.0]))
            p = [c[k] + 0.5 * float(rng.integers(-2, 3)) for k in range(3)]
            return Plane(n, p, M[int(rng.integers(len(M)))])
        ctr = [c[k] + 0.5 * float(rng.integers(-2, 3)) for k in range(3)]
        return Sphere(ctr, float(rng.choice([0.5, 1.0, 1.5])), M[int(rng.integers(len(M)))])
    op = OPS[int(rng.choice([0, 0, 1, 2, 2]))]
    # unbalanced now and then, so that leaves sit at every depth
    da = depth - 1 if rng.random() < 0.7 else 0
    db = depth - 1 if rng.random() < 0.7 else 0
    return op(random_tree(rng, da, c, M, planes), random_tree(rng, db, c, M, planes))


# the leaf set of each (outer, inner, side) nesting, chosen so that no tree is empty for most rays
# (an Intersection of touching spheres is) and every tie set is used three times
OVERLAP_PICK = [0, 1, 2, 0, 1, 2, 0, 1, 0, 1, 1, 1, 2, 0, 0, 2, 1, 0]
TIE_PICK = [0, 1, 2, 3, 4, 5, 3, 1, 4, 5, 1, 4, 0, 3, 2, 5, 2, 0]
RANDOM_SEEDS = [1000, 1003, 1004, 1006, 1008, 1009, 1011, 1012, 1013, 1015]


def span_trees():
    """[(name, builder)]: builder() makes the tree (fresh materials each call)"""
    trees = []
    k = 0
    for o in range(3):
        for i in range(3):
            for side in "ab":
                ov, ti = OVERLAP_LEAVES[OVERLAP_PICK[k]], TIE_LEAVES[TIE_PICK[k]]
                tag = "%s_%s_%s" % (OP_NAMES[o][:3], OP_NAMES[i][:3], side)
                trees.append((tag + "_overlap", lambda o=o, i=i, side=side, ov=ov, k=k:
                              nest(o, i, side, ov, CENTRE, materials(), k)))
                trees.append((tag + "_tie", lambda o=o, i=i, side=side, ti=ti, k=k:
                              nest(o, i, side, ti, CENTRE, materials(), k + 1)))
                k += 1
    trees += [("slab_%d" % j, lambda j=j: slab(j, CENTRE, materials())) for j in range(2)]
    trees += [("diff_chain_" + s, lambda s=s: diff_chain(s, CENTRE, materials())) for s in "ab"]
    for o in range(3):
        for j, (xn, m) in enumerate(XFORMS):
            leaves = TIE_LEAVES[(1, 1, 2)[o]] if j == 0 else OVERLAP_LEAVES[o]
            trees.append(("xf_%s_%s" % (xn, OP_NAMES[o][:3]), lambda o=o, m=m, leaves=leaves, j=j:
                          TransformedObject(m, nest(o, (o + 1 + j) % 3, "ab"[j], leaves, CENTRE, materials(), o))))
    for s in RANDOM_SEEDS:
        trees.append(("random_%d" % s, lambda s=s: random_tree(np.random.default_rng(s), 4, CENTRE, materials())))
    trees.append(("regress_xf_diff_zero_sign", regress_xf_diff_zero_sign))
    return trees


def regress_xf_diff_zero_sign():
    """Regression: a Difference below a transform.  The boundary taken from B has its normal negated
    before the transform maps it back (span.h:100-112, object.h:41); negating after the mapping gives
    the other sign wherever a component's sum is zero, as on these axis-parallel rays."""
    M = materials()
    c = CENTRE
    return TransformedObject(FLIP_SCALE, Difference(Sphere(c, 1.5, M[0]), Sphere((c[0] + 1, c[1], c[2]), 1, M[1])))


# -------------------------------------------------------------------- rays ---
AXES = np.eye(3, dtype=np.float32)


def primitives(root, out=None):
    """the tree's spheres (centre, r) and planes (normal, point) in their own frame"""
    out = {"s": [], "p": []} if out is None else out
    if isinstance(root, Sphere):
        out["s"].append((np.array(root.center, np.float32), np.float32(root.r)))
    elif isinstance(root, Plane):
        n = np.array(root.normal, np.float32)
        out["p"].append((n, n * np.float32(-root.d)))
    else:
        for ch in root.children():
            primitives(ch, out)
    return out


def span_rays(root, n=256, seed=0, centre=CENTRE):
    """n x 6 float32 rays for one tree: the tie families, then a random remainder"""
    rng = np.random.default_rng(7000 + seed)
    prim = primitives(root)
    c0 = np.array(centre, np.float32)
    sph = prim["s"] or [(c0, np.float32(1.0))]
    pla = prim["p"] or [(AXES[1].copy(), c0 + np.float32(0.5) * AXES[1])]
    rays = []

    def add(o, d):
        rays.append(np.concatenate([np.asarray(o, np.float32), np.asarray(d, np.float32)]))

    # 1. axis-parallel rays along the line of centres (x through `centre`): origins before, on, inside and
    #    past every solid, both ways, three lengths
    for j, off in enumerate(np.arange(-4.0, 4.5, 0.5, dtype=np.float32)):
        for sgn in (1.0, -1.0):
            add(c0 + off * AXES[0], sgn * AXES[0] * np.float32((1.0, 2.0, 0.5)[j % 3]))
    # 2. axis-parallel rays through each sphere's centre along y and z, from lattice origins
    for (c, r) in sph[:4]:
        for ax in (1, 2):
            for off in (-3.0, -1.0, 1.5):
                add(c + np.float32(off) * AXES[ax], -np.sign(off) * AXES[ax])
    # 3. rays through sphere centres from lattice origins (direction = lattice difference)
    for k in range(24):
        c, r = sph[k % len(sph)]
        o = c0 + np.float32(0.5) * rng.integers(-6, 7, size=3).astype(np.float32)
        if np.all(o == c):
            o = o + AXES[2] * np.float32(3)
        add(o, c - o)
    # 4. silhouette tangents: origin r off the centre line, direction along another axis
    for k in range(24):
        c, r = sph[k % len(sph)]
        u, v = AXES[k % 3], AXES[(k + 1 + (k // 3) % 2) % 3]
        sgn = np.float32(1 if (k // 6) % 2 == 0 else -1)
        add(c + sgn * r * u - np.float32(3) * v, v * np.float32((1.0, 0.5)[k % 2]))
    # 5. origins on a surface, inside a solid, at a centre; lattice directions without zero components
    for k in range(36):
        c, r = sph[k % len(sph)]
        o = c + np.float32((1.0, 0.5, 0.0)[k % 3]) * r * AXES[(k // 3) % 3] * np.float32(1 if k % 2 else -1)
        add(o, rng.choice(np.array([-1, -0.5, 0.5, 1], np.float32), size=3))
    # 6. parallel to a plane, origin on it and off it
    for k in range(16):
        nrm, p = pla[k % len(pla)]
        ax = int(np.argmax(np.abs(nrm)))
        t = AXES[(ax + 1 + k % 2) % 3]
        o = p + np.float32(0.5) * rng.integers(-4, 5) * AXES[(ax + 2 - k % 2) % 3]
        o = np.where(nrm != 0, p, o + c0 * (nrm == 0))
        if (k // 2) % 2:
            o = o + nrm * np.float32(0.5 if (k // 4) % 2 else -0.5)
        add(o, t * np.float32(1 if k % 3 else -1))
    # 7. long and short directions of the families above
    m = len(rays)
    for k in range(24):
        r = rays[(k * 7) % m].copy()
        r[3:] *= np.float32(1024.0 if k % 2 == 0 else 1.0 / 1024.0)
        rays.append(r)
    # 8. random remainder, aimed into the box around the tree
    while len(rays) < n:
        o = c0 + rng.uniform(-4, 4, size=3).astype(np.float32)
        tgt = c0 + rng.uniform(-1.5, 1.5, size=3).astype(np.float32)
        d = (tgt - o) * np.float32(rng.choice([0.25, 1.0, 300.0]))
        add(o, d)
    rays = np.array(rays[:n], dtype=np.float32)
    assert rays.shape == (n, 6) and np.all(np.isfinite(rays)) and np.all(np.any(rays[:, 3:] != 0, axis=1))
    return rays


# ------------------------------------------------------------ trace scenes ---
N_TRACE_SCENES = 6
TRACE_RAYS = 512
SPACING = 10.0


def _assemblies(s):
    """[(kind, builder(c, M))] of trace scene s: sphere-only assemblies"""
    combos = [(o, i, side) for o in range(3) for i in range(3) for side in "ab"]
    out = []
    for j in range(3):
        o, i, side = combos[3 * s + j]
        tie = (s + j) % 2 == 1
        leaves = (SPHERE_TIE_LEAVES[(s + j) % len(SPHERE_TIE_LEAVES)] if tie
                  else OVERLAP_LEAVES[(s + j) % len(OVERLAP_LEAVES)])
        out.append(("tie" if tie else "overlap",
                    lambda c, M, o=o, i=i, side=side, leaves=leaves, j=j: nest(o, i, side, leaves, c, M, s + j)))
    if s in (1, 4):  # a Difference chain replaces the third assembly (14 primitives at most)
        out[2] = ("chain", lambda c, M, side="ab"[s // 4]: diff_chain(side, c, M))
    elif s in (0, 3):  # a Difference (flipped and scaled) / an Intersection (sheared) of two overlapping spheres
        xf = XFORMS[s // 3][1]
        out.append(("xf", lambda c, M, xf=xf: TransformedObject(
            _about(xf, c), OPS[2 - s // 3](Sphere((0, 0, 0), 1, M[1]), Sphere((0.5, 0, 0), 1, M[3])))))
    else:  # a glass lens of two spheres through each other's centres, a mirror sphere touching it
        out.append(("tie", lambda c, M: Union(Intersection(Sphere(c, 1, M[2]), Sphere((c[0], c[1], c[2] - 1), 1, M[2])),
                                              Sphere((c[0] + 2, c[1], c[2]), 1, M[3]))))
    return out


def _about(m, c):
    """m's linear part L about the point c.  A TransformedObject applies its matrix to the ray (world to
    object, include/object.h:66), so an object built around the origin stands at c under x -> L (x - c)"""
    v = [np.float32(x) for x in m.m]
    c = [np.float32(x) for x in c]
    t = [-((v[4 * k] * c[0] + v[4 * k + 1] * c[1]) + v[4 * k + 2] * c[2]) for k in range(3)]
    return Matrix(v[0], v[1], v[2], t[0], v[4], v[5], v[6], t[1], v[8], v[9], v[10], t[2])


def assembly_centres(s):
    k = len(_assemblies(s))
    return [((j - (k - 1) / 2.0) * SPACING, 0.0, -8.0) for j in range(k)]


def trace_scene(s, leaf=False):
    M = materials(leaf)
    parts = [b(c, M) for (_, b), c in zip(_assemblies(s), assembly_centres(s))]
    ground = Plane((0, 1, 0), (0, -2, 0), M[0])
    wall = Plane((0, 0, 1), (0, 0, -16), M[4])
    return union_array(parts + [ground, wall])


def count_nodes(root, cls):
    return int(isinstance(root, cls)) + sum(count_nodes(ch, cls) for ch in root.children())


def mode_scenes():
    """the two trace scenes that also run under fast_spine / lane_walk=2 / lane_scatter: the one with
    the most Difference nodes and, of the others, the one with the most tie assemblies"""
    diffs = [count_nodes(trace_scene(s), Difference) for s in range(N_TRACE_SCENES)]
    a = int(np.argmax(diffs))
    ties = [sum(k == "tie" for k, _ in _assemblies(s)) if s != a else -1 for s in range(N_TRACE_SCENES)]
    return [a, int(np.argmax(ties))]


MODE_OPTS = [{"fast_spine": True}, {"lane_walk": 2}, {"lane_scatter": True}]


def strengths(rng, n):
    """zoo.trace_rays_input's mix: uniform 0..3, 15 % below eps, 25 % exactly 1"""
    s = rng.uniform(0.0, 3.0, size=(n, 1)).astype(np.float32)
    s[rng.random(n) < 0.15] = np.float32(0.0005)
    s[rng.random(n) < 0.25] = np.float32(1.0)
    return s


def trace_rays(s, n=TRACE_RAYS):
    """n x 7 caller rays of trace scene s: the span families aimed at each assembly"""
    M = materials()
    cs = assembly_centres(s)
    per = n // len(cs)
    parts = []
    for j, ((_, b), c) in enumerate(zip(_assemblies(s), cs)):
        root = b(c, M)
        if isinstance(root, TransformedObject):  # aim at where the transform puts it
            root = Sphere(c, 1, M[0])
        k = per if j < len(cs) - 1 else n - per * (len(cs) - 1)
        r = span_rays(root, 256, seed=100 * (s + 1) + j, centre=c)
        # every family, thinned evenly, then the random remainder
        idx = np.linspace(0, 255, k).astype(int)
        parts.append(r[idx])
    r = np.concatenate(parts)
    rng = np.random.default_rng(9000 + s)
    # unit-length directions except the long / short families: eps applies to t
    ln = np.linalg.norm(r[:, 3:], axis=1, keepdims=True)
    keep = (ln > 100) | (ln < 0.01) | (rng.random((len(r), 1)) < 0.3)
    r[:, 3:] = np.where(keep, r[:, 3:], r[:, 3:] / ln).astype(np.float32)
    return np.concatenate([r, strengths(rng, len(r))], axis=1).astype(np.float32)


# the strengths a caller can pass that sit on an edge of traceRay's arithmetic: NaN and +inf (10000 x
# strength converts to INT_MIN on x86: no scatter loop runs), a finite value past INT_MAX, a negative
# one, eps itself (shaded: the test is strength < eps) and a value just below it (not shaded).
# No large finite strength that leaves N positive: a refraction child scales it into bursts of 1e8 children.
EDGE_STRENGTHS = (float("nan"), float("inf"), 1e30, -1.0, float(np.float32(1e-3)), 0.00099999)


def edge_strength_rays(s, n=TRACE_RAYS):
    """trace_rays(s) with the strength column cycled through EDGE_STRENGTHS"""
    r = trace_rays(s, n)
    r[:, 6] = np.resize(np.array(EDGE_STRENGTHS, dtype=np.float32), len(r))
    return r


def regress_resume_negative_count():
    """Regression (scene, rays): a scatter loop whose count is negative.  10000 x strength x addFactor x sc
    converts to INT_MIN where it is NaN, infinite or past INT_MAX (x86's cvttss2si), the reference's
    `for (i = 0; i < N; i++)` runs no child and traceRay returns the emission alone (path-trace.h:128-160).
    The lane-resume walk asked the wave for that burst without the loop's own test, and the burst, which
    relies on i < N, ran a round of children with weights add / N.  One diffuse sphere (sc = 1) lit by an
    emissive half-space behind the caller (z > 4); the last ray is the control (strength 1)."""
    M = materials()
    root = Union(Sphere((0, 0, -4), 1, M[0]), Plane((0, 0, -1), (0, 0, 4), M[4]))
    rays = np.array([[0, 0, 0, 0, 0, -1, st] for st in EDGE_STRENGTHS[:3] + (1.0,)], dtype=np.float32)
    return root, rays


# --------------------------------------------------------------- cap scene ---
CAP_SHEAR = 2.0
CAP_DEPTH = 2
CAP_SPP = 2


def cap_scene(shift=(0.0, 0.0, 0.0)):
    """a glossy sphere (scatter coefficient 0.3) under a sheared TransformedObject: the reference maps
    normals with inv.applyNoTranslate, not the inverse transpose, so reflected directions can point
    into the surface and the rejection loop runs into its 1000-attempt cap.  The matrix maps world to
    object space: the world solid is the ellipsoid of points (x - 4 y, 2 y, z) over the sphere's.
    `shift` moves the whole scene (the camera of a render stays at the origin)."""
    M = materials()
    dx, dy, dz = (np.float32(v) for v in shift)
    s = np.float32(CAP_SHEAR)
    # object = L (world - shift)
    ball = TransformedObject(Matrix(1, s, 0, -(dx + s * dy), 0, 0.5, 0, -np.float32(0.5) * dy, 0, 0, 1, -dz),
                             Sphere((0, 0, -4.5), 1.5, M[1]))
    floor = Plane((0, 1, 0), (0, -3.5 + dy, 0), M[0])
    wall = Plane((0, 0, 1), (0, 0, -12 + dz), M[4])
    return union_array([ball, floor, wall])


def cap_candidates(n=5000, seed=77):
    """rays aimed at the sheared sphere, strength 1"""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-6, -3, -1], [6, 5, 1], size=(n, 3)).astype(np.float32)
    u = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    u = u / np.maximum(1, np.linalg.norm(u, axis=1, keepdims=True)) * np.float32(1.5)
    tgt = np.stack([u[:, 0] - 2 * CAP_SHEAR * u[:, 1], 2 * u[:, 1], u[:, 2] - 4.5], axis=1).astype(np.float32)
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([o, d, np.ones((n, 1), np.float32)], axis=1).astype(np.float32)


# the cap render: camera at the origin, the scene shifted so that it stands half a unit above the
# floor beside the sphere
CAP_RENDER = dict(W=24, H=16, spp=2, depth=3, shift=(3.0, 3.0, 0.0))
