"""Fixtures of the multi-span user objects (pt_object_device_spans,
pathtrace.DeviceSpansObject; tests/test_multispan.py, tests/precompile_multispan.py).

The CPU oracle cannot host a user node with several spans, so every user
object here has a built-in twin whose arithmetic its bodies restate: a shell is
Difference(Sphere(c, R), Sphere(c, r)), a dumbbell is Union(Sphere, Sphere) and
an onion (a shell around a ball, three spans) is a nested Difference, each
sphere by src/sphere.cpp:31-49 (live iff disc > 1e-3), the span lists as
src/difference.cpp:84-135 and src/union.cpp:84-134 emit them.  A scene built
with user=True must render its user=False twin's frame bit for bit, and the
twin's to_text goes to the oracle.  The same body text stands in
tests/cpp/facade_multispan.cpp (the kernel keys are compared)."""
import numpy as np

from pathtrace.scene import (ColorTexture, DeviceSpansObject, Difference, Intersection, Material, Matrix, Plane,
                             Sphere, TransformedObject, Union)

# prm: center, R*R, r*r, R, r.  The radii are well apart, so a ray through the
# inner sphere has outer.t0 < inner.t0 < inner.t1 < outer.t1 strictly and the
# Difference emits [outer.t0, inner.t0], [inner.t1, outer.t1].
SHELL_SPANS = """
    const V3 oc = mk(o.x - prm[0], o.y - prm[1], o.z - prm[2]);
    const float a = dot(d, d);
    const float b = dot(oc, d);
    const float cc = dot(oc, oc);
    const float disco = b * b - a * (cc - prm[3]);
    if (disco <= 1e-3f)
        return 0;
    const float so = sqrtf(disco);
    const float o0 = (-b - so) / a, o1 = (-b + so) / a;
    const float disci = b * b - a * (cc - prm[4]);
    if (disci <= 1e-3f) {
        t0[0] = o0, t1[0] = o1;
        return 1;
    }
    const float si = sqrtf(disci);
    t0[0] = o0, t1[0] = (-b - si) / a;
    t0[1] = (-b + si) / a, t1[1] = o1;
    return 2;
"""
# q / |q| on the outer surface, its exact negation on the inner one (the
# Difference's flipped normal), by the radius |q| is nearer to
SHELL_NORMAL = """
    const V3 q = mk(p.x - prm[0], p.y - prm[1], p.z - prm[2]);
    float m = sqrtf(dot(q, q));
    const float eo = m > prm[5] ? m - prm[5] : prm[5] - m;
    const float ei = m > prm[6] ? m - prm[6] : prm[6] - m;
    if (m == 0.0f)
        m = 1.0f;
    const V3 n = mk(q.x / m, q.y / m, q.z / m);
    return ei < eo ? mk(-n.x, -n.y, -n.z) : n;
"""
# prm: center, R1*R1, R2*R2, R3*R3, R1, R2, R3 with R1 > R2 > R3 well apart: a
# shell around a ball, Difference(Sphere(c, R1), Difference(Sphere(c, R2),
# Sphere(c, R3))), up to three spans: [s1.t0, s2.t0], [s3.t0, s3.t1], [s2.t1, s1.t1]
ONION_SPANS = """
    const V3 oc = mk(o.x - prm[0], o.y - prm[1], o.z - prm[2]);
    const float a = dot(d, d);
    const float b = dot(oc, d);
    const float cc = dot(oc, oc);
    const float d1 = b * b - a * (cc - prm[3]);
    if (d1 <= 1e-3f)
        return 0;
    const float s1 = sqrtf(d1);
    const float o0 = (-b - s1) / a, o1 = (-b + s1) / a;
    const float d2 = b * b - a * (cc - prm[4]);
    if (d2 <= 1e-3f) {
        t0[0] = o0, t1[0] = o1;
        return 1;
    }
    const float s2 = sqrtf(d2);
    const float m0 = (-b - s2) / a, m1 = (-b + s2) / a;
    const float d3 = b * b - a * (cc - prm[5]);
    if (d3 <= 1e-3f) {
        t0[0] = o0, t1[0] = m0;
        t0[1] = m1, t1[1] = o1;
        return 2;
    }
    const float s3 = sqrtf(d3);
    t0[0] = o0, t1[0] = m0;
    t0[1] = (-b - s3) / a, t1[1] = (-b + s3) / a;
    t0[2] = m1, t1[2] = o1;
    return 3;
"""
# q / |q| on the outer sphere and on the ball, its exact negation on the
# shell's inner surface (radius R2)
ONION_NORMAL = """
    const V3 q = mk(p.x - prm[0], p.y - prm[1], p.z - prm[2]);
    float m = sqrtf(dot(q, q));
    const float e1 = m > prm[6] ? m - prm[6] : prm[6] - m;
    const float e2 = m > prm[7] ? m - prm[7] : prm[7] - m;
    const float e3 = m > prm[8] ? m - prm[8] : prm[8] - m;
    if (m == 0.0f)
        m = 1.0f;
    const V3 n = mk(q.x / m, q.y / m, q.z / m);
    return e2 < e1 && e2 < e3 ? mk(-n.x, -n.y, -n.z) : n;
"""
# prm: center A, rA*rA, center B, rB*rB, rA, rB: two disjoint balls, ordered by
# the union's own test a.t1 < b.t0 (src/union.cpp:96)
DUMBBELL_SPANS = """
    const float a = dot(d, d);
    const V3 pa = mk(o.x - prm[0], o.y - prm[1], o.z - prm[2]);
    const float ba = dot(pa, d);
    const float da = ba * ba - a * (dot(pa, pa) - prm[3]);
    const V3 pb = mk(o.x - prm[4], o.y - prm[5], o.z - prm[6]);
    const float bb = dot(pb, d);
    const float db = bb * bb - a * (dot(pb, pb) - prm[7]);
    const bool la = !(da <= 1e-3f), lb = !(db <= 1e-3f);
    float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
    if (la) {
        const float s = sqrtf(da);
        a0 = (-ba - s) / a, a1 = (-ba + s) / a;
    }
    if (lb) {
        const float s = sqrtf(db);
        b0 = (-bb - s) / a, b1 = (-bb + s) / a;
    }
    if (la && lb) {
        const bool af = a1 < b0;
        t0[0] = af ? a0 : b0, t1[0] = af ? a1 : b1;
        t0[1] = af ? b0 : a0, t1[1] = af ? b1 : a1;
        return 2;
    }
    if (la) {
        t0[0] = a0, t1[0] = a1;
        return 1;
    }
    if (lb) {
        t0[0] = b0, t1[0] = b1;
        return 1;
    }
    return 0;
"""
# the normal of the ball whose surface p is nearer to
DUMBBELL_NORMAL = """
    const V3 qa = mk(p.x - prm[0], p.y - prm[1], p.z - prm[2]);
    const V3 qb = mk(p.x - prm[4], p.y - prm[5], p.z - prm[6]);
    const float ma = sqrtf(dot(qa, qa)), mb = sqrtf(dot(qb, qb));
    const float ea = ma > prm[8] ? ma - prm[8] : prm[8] - ma;
    const float eb = mb > prm[9] ? mb - prm[9] : prm[9] - mb;
    const V3 q = eb < ea ? qb : qa;
    float m = eb < ea ? mb : ma;
    if (m == 0.0f)
        m = 1.0f;
    return mk(q.x / m, q.y / m, q.z / m);
"""


def _sq(r):
    return float(np.float32(r) * np.float32(r))  # r_squared = r * r in float (src/sphere.cpp:10)


def shell(c, R, r, m, user, max_spans=2):
    if not user:
        return Difference(Sphere(c, R, m), Sphere(c, r, m))
    return DeviceSpansObject(SHELL_SPANS, SHELL_NORMAL, (c[0], c[1], c[2], _sq(R), _sq(r), R, r), m, max_spans)


def onion(c, r1, r2, r3, m, user):
    if not user:
        return Difference(Sphere(c, r1, m), Difference(Sphere(c, r2, m), Sphere(c, r3, m)))
    return DeviceSpansObject(ONION_SPANS, ONION_NORMAL,
                             (c[0], c[1], c[2], _sq(r1), _sq(r2), _sq(r3), r1, r2, r3), m, 3)


def dumbbell(ca, ra, cb, rb, m, user):
    if not user:
        return Union(Sphere(ca, ra, m), Sphere(cb, rb, m))
    return DeviceSpansObject(DUMBBELL_SPANS, DUMBBELL_NORMAL,
                             (ca[0], ca[1], ca[2], _sq(ra), cb[0], cb[1], cb[2], _sq(rb), ra, rb), m, 2)


def mats():
    return {"diffuse": Material(ColorTexture(0.8), ColorTexture(1)),
            "mirror": Material(ColorTexture(0.99), ColorTexture(0)),
            "glass": Material(ColorTexture(0.7), ColorTexture(0), ColorTexture(0), ColorTexture(0.9), 1.3,
                              ColorTexture(1)),
            "emitW": Material(ColorTexture(0), ColorTexture(0), ColorTexture(2))}


GLASS_C, DIFF_C = (0.9, 0.1, -3.2), (-1.0, 0.05, -3.4)
ROT_T = (-0.2, 0.9, -4.5)  # where the rotated dumbbell stands
BIG_C = (0.0, -0.1, -5.5)
CAP_A, CAP_B = (-1.9, 0.6, -4.5), (-1.3, 0.6, -4.5)
ONION_C = (1.6, 0.3, -4.8)


def multi_zoo(user=True, shell_slots=2):
    """Every merge over a span list, over the emissive floor: a glass and a
    diffuse shell at the root union, a rotated dumbbell carved by a sphere that
    cuts both balls (Difference A side under a transform), a big sphere dented
    by a dumbbell (Difference B side), a dumbbell cut by a plane (Intersection)
    and a glass onion, whose rays through the centre have three spans."""
    m = mats()
    glass = shell(GLASS_C, 0.5, 0.3, m["glass"], user, shell_slots)
    matte = shell(DIFF_C, 0.5, 0.3, m["diffuse"], user, shell_slots)
    rot = Matrix.rotateY(0.5).concat(Matrix.rotateX(0.2)).concat(Matrix.translate(*ROT_T))
    carved = Difference(TransformedObject(rot, dumbbell((-0.35, 0, 0), 0.25, (0.35, 0, 0), 0.25, m["diffuse"], user)),
                        Sphere((ROT_T[0], ROT_T[1] + 0.25, ROT_T[2] + 0.1), 0.4, m["mirror"]))
    dented = Difference(Sphere(BIG_C, 0.7, m["diffuse"]),
                        dumbbell((-0.3, -0.1, -5.0), 0.25, (0.3, -0.1, -5.0), 0.25, m["mirror"], user))
    capped = Intersection(dumbbell(CAP_A, 0.25, CAP_B, 0.25, m["diffuse"], user), Plane((0, 1, 0), -0.6, m["diffuse"]))
    layers = onion(ONION_C, 0.5, 0.38, 0.2, m["glass"], user)
    return Union(Union(Union(glass, matte), Union(carved, dented)),
                 Union(Union(capped, layers), Plane((0, 1, 0), .5, m["emitW"])))


def shell_scene(user=True, max_spans=2):
    """the glass shell alone over the floor (the slack test: max_spans above what the body returns)"""
    m = mats()
    return Union(shell(GLASS_C, 0.5, 0.3, m["glass"], user, max_spans), Plane((0, 1, 0), .5, m["emitW"]))


def query_rays(n=256, seed=7):
    """rays from above the scene aimed at the objects' centres with jitter: they
    run down through the shells and dumbbells into the floor's half-space"""
    rng = np.random.default_rng(seed)
    o = np.array([0.0, 1.6, 0.0], np.float32)
    aims = np.array([GLASS_C, DIFF_C, ROT_T, BIG_C, CAP_A, CAP_B, (-0.3, -0.1, -5.0), ONION_C], np.float32)
    tgt = aims[rng.integers(0, len(aims), n)] + rng.normal(scale=0.15, size=(n, 3)).astype(np.float32)
    return np.concatenate([np.tile(o, (n, 1)), (tgt - o).astype(np.float32)], axis=1).astype(np.float32)
