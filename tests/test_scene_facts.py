"""Scene reachability facts (codegen.cpp reach_facts, pt_device.h PT_REACH_PRUNE).

Code generation decides from a scene's materials which burst_t variants its
scatter bursts can reach -- kr_reach (bit 0: sc == 1, bit 1: sc != 1) and
bursts_all_leaf (burst()'s `deferred` test holds for every burst) -- and the
kernel instantiates only those.  Here: the facts of the zoo scenes; a float32
restatement of the device arithmetic swept over strengths, addFactors and
adversarial points, which must find `deferred` wherever the fact is claimed
and a counterexample just outside the proven region; the pruned kernel's size;
and on the GPU the variants no other scene isolates, bit for bit against the
oracle.
"""
import os
import sys

import numpy as np
import pytest

import pathtrace as pt
import zoo
from pathtrace import scenes
from pathtrace.scene import (ColorTexture, Difference, Intersection, Material, Plane, Sphere, TransformedObject,
                             Union, to_text, union_array)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPS = F(1e-3)

# ---------------------------------------------------------------- the facts

ZOO_FACTS = [("scene_p1", 1, True),      # sc == 1 only
             ("occlude_box", 3, True),   # sc 1 and 0.5, reflect 0.8 and 0.7
             ("csg_zoo", 3, False),      # sc 1 and 0.3: 0.9 sqrt(3) / 0.3 = 5.2
             ("union_zoo", 3, False),
             ("scatter_zoo", 3, False),  # reflect 8, sc 0.0064
             ("texture_zoo", 3, False)]  # image / alpha scatter coefficients: nothing known


@pytest.mark.parametrize("name,kr,leaf", ZOO_FACTS)
def test_zoo_facts(built, name, kr, leaf):
    assert pt.DeviceScene(zoo.build(name)).reach_facts == {"kr_reach": kr, "bursts_all_leaf": leaf}


def one_sphere(reflect, sc):
    """a scattering sphere over an emissive ground (whose sc = 0: one mirror child, no burst)"""
    return Union(Sphere((0, 0, -4), 0.9, Material(ColorTexture(reflect), ColorTexture(sc))),
                 Plane((0, 1, 0), 1.0, Material(ColorTexture(0), ColorTexture(0), ColorTexture(2))))


def test_facts_follow_the_materials(built):
    assert pt.DeviceScene(one_sphere(0.8, 0.5)).reach_facts == {"kr_reach": 2, "bursts_all_leaf": True}
    # no material scatters: no burst at all
    assert pt.DeviceScene(one_sphere(0.8, 0.0)).reach_facts == {"kr_reach": 0, "bursts_all_leaf": True}
    # a coefficient above 1 clamps to 1; NaN reflectance is unbounded
    assert pt.DeviceScene(one_sphere(0.8, 3.0)).reach_facts["kr_reach"] == 1
    assert pt.DeviceScene(one_sphere(float("nan"), 1.0)).reach_facts == {"kr_reach": 1, "bursts_all_leaf": False}
    # the facts are part of the source, hence of the code-object key
    assert pt.DeviceScene(one_sphere(0.8, 1.0)).kernel_key(4) != pt.DeviceScene(one_sphere(0.8, 0.5)).kernel_key(4)


# ------------------------------------------------- the soundness sweep (CPU)

def length32(rc):
    """pt_device.h length(): sqrt(dot), every step rounded to float32"""
    x, y, z = (F(v) for v in rc)
    return np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z)))


def burst_tests(strength, add, sc, abs_rc):
    """PH_SETUP's N (pt_device.h:4217-4222 of the parent) and burst()'s `deferred`
    strength test (:3740-3742) in float32: returns (is a burst with N >= 1, deferred)."""
    strength, add, sc = F(strength), F(add), F(sc)
    with np.errstate(over="ignore", invalid="ignore"):
        x = ((F(10000.0) * strength) * add) * sc
        in_range = x < F(2147483648.0)  # cvt_x86: otherwise INT_MIN, and i >= N ends the loop at once
        n = np.where(in_range, x, F(0)).astype(np.int64)
        n = np.where(n == 0, 1, n)
        sna = (strength / n.astype(np.float32)) * add
        deferred = (sna * F(abs_rc)) * F(1.01) < EPS
    assert x.dtype == np.float32 and sna.dtype == np.float32
    return in_range, deferred


def sweep(sc, abs_rc):
    """every (strength, add) point of the grid and the adversarial points: (points that are bursts, deferred there)"""
    strength = np.concatenate([np.geomspace(1e-3, 3e7, 6000), [1e-3, 1.0, 8.0, 1e6, 2.5e6]]).astype(np.float32)
    add = np.concatenate([np.geomspace(1e-3, 1.0, 300), np.linspace(1e-3, 1.0, 200), [1e-3, 1.0]]).astype(np.float32)
    s, a = np.meshgrid(strength, add, indexing="ij")
    ok, d = burst_tests(s.ravel(), a.ravel(), sc, abs_rc)
    # adversarial: 10000 str add sc within a few ulps of an integer k (below it N = k - 1, the
    # largest str / N), above all of 1 and 2, where N stays 1 for the largest sNa of all
    ks = np.array([1, 2, 3, 4, 5, 8, 16, 64, 65, 100, 1000, 10000, 1 << 20, (1 << 24) + 2], dtype=np.float64)
    a2 = np.concatenate([np.geomspace(1e-3, 1.0, 40), [1.0]]).astype(np.float32)
    k2, aa = np.meshgrid(ks, a2.astype(np.float64), indexing="ij")
    s0 = (k2 / (1e4 * aa * float(F(sc)))).astype(np.float32).ravel()
    aa = aa.astype(np.float32).ravel()
    for _ in range(12):
        s0 = np.nextafter(s0, F(0))
    for _ in range(24):
        ok2, d2 = burst_tests(s0, aa, sc, abs_rc)
        ok, d = np.concatenate([ok, ok2]), np.concatenate([d, d2])
        s0 = np.nextafter(s0, F(np.inf))
    return ok, d


def materials(o, out):
    if isinstance(o, (Union, Intersection, Difference)):
        materials(o.a, out), materials(o.b, out)
    elif isinstance(o, TransformedObject):
        materials(o.o, out)
    else:
        out.append(o.material)
    return out


def burst_materials(root):
    """(sc, |reflect|) of the materials that can burst: clamp01(mean3(scatter)) > EPS, in float32"""
    res = set()
    for m in materials(root, []):
        refl, scat = m.textures()[:2]
        c = [F(v) for v in scat.color]
        sc = min(F(1), max(F(0), F(F(F(c[0] + c[1]) + c[2]) * F(F(1) / F(3)))))
        if sc > EPS:
            res.add((float(sc), float(length32(refl.color))))
    return sorted(res)


# grey reflectances at the edge of what the facts can claim, from the restatement's own
# arithmetic: the largest sNa is str add at x just below 2 (N = 1), i.e. 2e-4 / sc, so with
# sc = 1 the strength test can fail once g sqrt(3) 2e-4 1.01 reaches EPS
G_EDGE = 1e-3 / (2e-4 * 1.01 * np.sqrt(3.0))
G_IN, G_OUT = float(F(G_EDGE * (1 - 1e-4))), float(F(G_EDGE * (1 + 1e-4)))


@pytest.mark.parametrize("name", [n for n, _, leaf in ZOO_FACTS if leaf] + ["C2", "C3", "C5"])
def test_all_leaf_claims_hold_in_float32(built, name):
    root = scenes.CONFIGS[name].scene() if name in scenes.CONFIGS else zoo.build(name)
    assert pt.DeviceScene(root).reach_facts["bursts_all_leaf"]
    mats = burst_materials(root)
    assert mats
    for sc, abs_rc in mats:
        ok, d = sweep(sc, abs_rc)
        assert ok.sum() > 1e6 and np.all(d[ok]), (name, sc, abs_rc, int((~d[ok]).sum()))


def test_proof_boundary_is_not_vacuous(built):
    """just inside the proven region every burst is deferred and the fact is
    claimed; just outside, the sweep finds a burst that is not, and it is not"""
    ok, d = sweep(1.0, length32((G_IN,) * 3))
    assert np.all(d[ok])
    ok, d = sweep(1.0, length32((G_OUT,) * 3))
    assert np.any(~d[ok])
    assert pt.DeviceScene(one_sphere(G_IN, 1.0)).reach_facts == {"kr_reach": 1, "bursts_all_leaf": True}
    assert pt.DeviceScene(one_sphere(G_OUT, 1.0)).reach_facts == {"kr_reach": 1, "bursts_all_leaf": False}


# --------------------------------------------------- the pruned kernel (CPU)

def test_pruning_shrinks_the_kernel(built, monkeypatch):
    """scene_p1 at depth 8: one lane-major round instance instead of two, and
    under 0.6 of the unpruned pt_render_fast's bytes (0.50 when written)"""
    sys.path.insert(0, os.path.join(ROOT, "tools", "ab"))
    try:
        import isa_stat
    finally:
        sys.path.pop(0)
    cache = os.path.join(ROOT, "path-trace_amd", "_jit_cache")
    pruned = isa_stat.kernel_stats(os.path.join(cache, pt.DeviceScene(scenes.scene_p1()).compile(8) + ".hsaco"))
    monkeypatch.setenv("PT_DEVICE_DEFINES", "PT_REACH_PRUNE=0")
    full = isa_stat.kernel_stats(os.path.join(cache, pt.DeviceScene(scenes.scene_p1()).compile(8) + ".hsaco"))
    print("pruned %d bytes, %d rounds; unpruned %d bytes, %d rounds" % (
        pruned["code_bytes"], len(pruned["rounds"]), full["code_bytes"], len(full["rounds"])))
    assert len(full["rounds"]) >= 2 and {r["variant"][:9] for r in full["rounds"]} == {"KR0=false", "KR0=true "}
    assert len(pruned["rounds"]) == 1 and pruned["rounds"][0]["variant"].startswith("KR0=true")
    assert pruned["code_bytes"] < 0.6 * full["code_bytes"], (pruned["code_bytes"], full["code_bytes"])


def test_retired_knob_is_a_compile_error(built):
    """a retired value knob and a retired hook of pt_device.h: defining either
    fails the compile with an error that names it, instead of building the
    default under a variant's name; with nothing defined the module compiles"""
    assert "PT_DEVICE_DEFINES" not in os.environ
    for defs, knob in [("PT_LM_BITS=0", "PT_LM_BITS"), ("PT_PAD_VALU=4", "PT_PAD_VALU")]:
        os.environ["PT_DEVICE_DEFINES"] = defs
        try:
            with pytest.raises(pt.PtError) as err:
                pt.DeviceScene(scenes.scene_p1()).compile(4)
        finally:
            del os.environ["PT_DEVICE_DEFINES"]
        assert "retired build-time knob" in str(err.value) and knob in str(err.value), str(err.value)
    assert pt.DeviceScene(scenes.scene_p1()).compile(4)


# ------------------------------------------------------------------- GPU

def against_oracle(root, tmp_path, w, h, spp, depth):
    import oracle_py as O
    gpu, st = pt.render(pt.DeviceScene(root), w, h, spp, depth, stats=True)
    ref, rst = O.render(to_text(root, str(tmp_path)), w, h, spp, depth, order=O.ORDER_FAST, stats=True)
    gpu = gpu.reshape(-1, 3)
    np.testing.assert_array_equal(gpu.view(np.uint32), ref.view(np.uint32))
    assert st["queries"] == rst["queries"], (st["queries"], rst["queries"])
    assert np.all(np.isfinite(gpu)) and np.any(gpu > 0)


@pytest.mark.gpu
def test_kr0_false_only_bitexact(built, tmp_path):
    """the only scene whose kernel holds the KR0 = false variant alone"""
    root = one_sphere(0.8, 0.5)
    assert pt.DeviceScene(root).reach_facts == {"kr_reach": 2, "bursts_all_leaf": True}
    against_oracle(root, tmp_path, 16, 12, 2, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("g,leaf", [(G_IN, True), (G_OUT, False), (8.0, False)])
def test_proof_boundary_bitexact(built, tmp_path, g, leaf):
    """either side of the proof's boundary (the non-deferred variant pruned /
    kept), and a reflectance far outside it, whose children do recurse"""
    root = one_sphere(g, 1.0)
    assert pt.DeviceScene(root).reach_facts == {"kr_reach": 1, "bursts_all_leaf": leaf}
    against_oracle(root, tmp_path, 8, 6, 1, 3)
