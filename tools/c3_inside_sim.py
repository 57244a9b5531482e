"""CPU estimate (not the renderer): how many of C3's kept burst children the inside-solid probe
(pt_device.h Inside, PT_INSIDE_ZERO) settles in the first pass, and that it fires on no child whose
term is not zero.  float64; primary-ray diffuse hits on C3's geometry, uniform-ball children, the
kernel's definitions of dark (the child recedes from the sky wall), clear (every sphere dead or ended
before eps) and mid (kept, not clear).  First hits come from the reference's own merges restated on
span lists (src/union.cpp:84-134, src/difference.cpp:84-135 with the branch of :126-130 that sets a
span's END to the subtractor's start), so surfaces that branch makes visible inside a cavity are
burst origins here as they are in the renderer.  Two rules are counted: the one first proposed
(subtractors dead or exiting before X's exit) and the one built (each subtractor also starts after X's
running span start).  Output of this script: profiles/round10/c3_inside_sim.txt."""
import math

import numpy as np

EPS, MAXV = 1e-3, 1e20
rng = np.random.default_rng(0)
S = [((-1, 0, -4), .6, "d"), ((-.5, 0, -4), .6, "d"), ((-.7, .3, -3.6), .4, "d"),
     ((1, 0, -4), .6, "g"), ((1.4, .2, -4.2), .5, "m"), ((1, 0, -3.4), .3, "g")]
C = np.array([s[0] for s in S], float)
R = np.array([s[1] for s in S])
W, H = 1920, 1080


def sph(i, o, d):
    oc = o - C[i]
    b = oc @ d
    disc = b * b - (oc @ oc - R[i] ** 2)
    if disc <= EPS:
        return []
    s = math.sqrt(disc)
    return [[-b - s, -b + s, i, i]]  # start, end, start primitive, end primitive


def union(A, B):
    A, B, out = [list(x) for x in A], [list(x) for x in B], []
    while A or B:
        if not A:
            out.append(B.pop(0))
        elif not B:
            out.append(A.pop(0))
        elif A[0][1] < B[0][0]:
            out.append(A.pop(0))
        elif B[0][1] < A[0][0]:
            out.append(B.pop(0))
        elif A[0][0] < B[0][0]:
            if A[0][1] < B[0][1]:
                A[0][1], A[0][3] = B[0][1], B[0][3]
            B.pop(0)
        else:
            if A[0][1] > B[0][1]:
                B[0][1], B[0][3] = A[0][1], A[0][3]
            A.pop(0)
    return out


def difference(A, B):
    A, B, out = [list(x) for x in A], [list(x) for x in B], []
    while A:
        if not B or A[0][1] < B[0][0]:
            out.append(A.pop(0))
        elif B[0][1] < A[0][0]:
            B.pop(0)
        elif A[0][0] < B[0][0]:
            if A[0][1] < B[0][1]:
                A[0][1], A[0][3] = B[0][0], B[0][2]
                out.append(A.pop(0))
            else:
                out.append([A[0][0], B[0][0], A[0][2], B[0][2]])
                A[0][0], A[0][2] = B[0][1], B[0][3]
                B.pop(0)
        elif A[0][1] > B[0][1]:
            A[0][1], A[0][3] = B[0][0], B[0][2]  # :128, the end from B's start
            B.pop(0)
        else:
            A.pop(0)
    return out


def spans(o, d):
    left = difference(union(sph(0, o, d), sph(1, o, d)), sph(2, o, d))
    right = difference(union(sph(3, o, d), sph(4, o, d)), sph(5, o, d))
    wall = [[(-200 - o[2]) / d[2], MAXV, 6, 6]] if d[2] < 0 else ([[-MAXV, (-200 - o[2]) / d[2], 6, 6]] if d[2] > 0 else [])
    return union(left, union(right, wall))


def first_hit(o, d):
    """traceRay's scan: (t, primitive) or None"""
    for s0, s1, p0, p1 in spans(o, d):
        if s0 >= MAXV:
            return None
        if s0 >= EPS:
            return s0, p0
        if s1 >= MAXV:
            return None
        if s1 >= EPS:
            return s1, p1
    return None


def rule(o, d, bound):
    """the probe on C3's tree: X in {S0, S1} less S2, X in {S3, S4} less S5"""
    G = math.sqrt(2.02 * max((o - C[i]) @ (o - C[i]) + R[i] ** 2 for i in range(6)))
    mg, xmin = 1e-5 * G, EPS * 1.001 + 1e-5 * G
    for xs, b in (((0, 1), 2), ((3, 4), 5)):
        sb = sph(b, o, d)
        best = max((sph(x, o, d) for x in xs), key=lambda s: s[0][1] if s and s[0][1] > xmin else -math.inf)
        if not best or best[0][1] <= xmin:
            continue
        if not sb or (best[0][1] > sb[0][1] + mg and (not bound or sb[0][0] > best[0][0] + mg)):
            return True
    return False


n = dict(children=0, kept=0, clear=0, mid=0, mid_zero=0, proposed=0, proposed_wrong=0, built=0, built_wrong=0,
         built_missed=0)
origins = 0
dist = 2 * min(W, H)
while origins < 400:
    px, py = rng.uniform(0, W), rng.uniform(0, H)
    d = np.array([(2 * px / W - 1) * W, (1 - 2 * py / H) * H, -dist])
    d /= np.linalg.norm(d)
    h = first_hit(np.zeros(3), d)
    if h is None or h[1] > 2:
        continue  # only the left solid scatters
    origins += 1
    o = h[0] * d
    nrm = (o - C[h[1]]) / R[h[1]]
    if h[1] == 2:
        nrm = -nrm  # a boundary taken from the subtractor faces into it (span.h:100-112)
    v = rng.uniform(-1, 1, (2400, 3))
    v = v[(v * v).sum(1) < 1]
    v = v[v @ nrm > EPS]
    for w in v:
        c = w / np.linalg.norm(w)
        n["children"] += 1
        if c[2] >= 0:
            continue
        n["kept"] += 1
        sp = [sph(i, o, c) for i in range(6)]
        if all(not s or s[0][1] < EPS for s in sp):
            n["clear"] += 1
            continue
        n["mid"] += 1
        hit = first_hit(o, c)
        zero = hit is None or hit[1] != 6
        n["mid_zero"] += zero
        for name, bound in (("proposed", False), ("built", True)):
            f = rule(o, c, bound)
            n[name] += f
            n[name + "_wrong"] += f and not zero
        n["built_missed"] += zero and not rule(o, c, True)
print("origins", origins)
for k, x in n.items():
    print("%-16s %8d" % (k, x))
print("kept / children %.3f, mid / kept %.3f, zero / mid %.3f, proposed / mid %.3f, built / mid %.3f" % (
    n["kept"] / n["children"], n["mid"] / n["kept"], n["mid_zero"] / n["mid"], n["proposed"] / n["mid"],
    n["built"] / n["mid"]))
