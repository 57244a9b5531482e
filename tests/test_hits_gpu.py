"""pt_query_hits (DeviceScene.query_hits) on the GPU: what traceRay sees at the first surface, on both
query paths -- the lazy merge, and the fast check with the merge as its fallback -- bit for bit against the
CPU and against each other.

  span goldens   tests/golden/spans_csg.npz and spans_p1.npz, the unmodified reference's span lists: hit,
                 exit, t, normal, material and pos are tests/hits_model.py's scan of them
  seam trees     the 18 trees of tests/golden/fastcheck_seam.npz, origins on the seam of two spheres: hit,
                 exit, t and material against the reference lists, and a census of the fast check's
                 verdicts -- at least MIN_CENSUS rays it decided, and as many that it sent to the merge and
                 that still hit.  tests/fastcheck.py's model predicts both classes far above the bound on
                 these rays (test_model_predicts_the_census, CPU), so no ray was added to the fixture's.
  shading        the five texture lookups at the hit point and the ior, against the CPU oracle's lookups
  multi-span     the shell user object of tests/multispan.py against Difference(Sphere, Sphere)

The modules are listed in tests/precompile_guides.py."""
import os

import numpy as np
import pytest

import fastcheck as C
import guide_scenes as G
import hits_model as HM
import multispan as M
import oracle_py as O
import pathtrace as pt
import zoo as T
from test_fastcheck import MIN_CENSUS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = ("fast", "merge")
FIELDS = ("hit", "exit", "material", "t", "normal", "pos", "ior")
_cache = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, fields, what):
    for k in fields:
        g, w = bits(got[k]), bits(np.asarray(want[k], dtype=got[k].dtype))
        assert g.shape == w.shape, (what, k)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs on %d rays, first %s" % (what, k, bad.size, bad[:8])


def both_paths(ds, rays, shade=False):
    """query_hits on both paths, which must agree in every field on every ray"""
    fast, merge = (ds.query_hits(rays, path=p, shade=shade) for p in PATHS)
    same(fast, merge, FIELDS + (("shade",) if shade else ()), "fast vs merge")
    assert not merge["decided"].any() and set(np.unique(fast["decided"])) <= {0, 1}
    return fast, merge


def seam():
    if "seam" not in _cache:
        with np.load(os.path.join(GOLD, "fastcheck_seam.npz")) as z:
            _cache["seam"] = {k: z[k] for k in z.files}
    return _cache["seam"]


# --------------------------------------------------------------------- CPU ---
def test_model_predicts_the_census():
    """tests/fastcheck.py's float32 model of the check on the fixture's rays: both classes the GPU census
    asks for lie far above MIN_CENSUS (the device may decide more rays than the model in Difference-free
    trees, where it tries the union rule first, never fewer than the bound allows)"""
    z, trees = seam(), {name: root for name, _, root in C.seam_trees()}
    decided = undecided_hit = 0
    for name in C.seam_names():
        rays = z["rays_" + name]
        ok = C.fast_ok(trees[name], C.PrimSpans(trees[name], rays))
        hit = HM.scan(z["cnt_" + name], z["t_" + name])[0]
        decided += int(ok.sum())
        undecided_hit += int((~ok & hit).sum())
    print("model: %d decided, %d undecided and hit" % (decided, undecided_hit))
    assert decided >= 10 * MIN_CENSUS and undecided_hit >= 10 * MIN_CENSUS


# --------------------------------------------------------------------- GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.SPAN_SCENES))
def test_gpu_hits_are_the_scan_of_the_reference_lists(built, tmp_path, name):
    z = np.load(os.path.join(GOLD, "spans_%s.npz" % name))
    ds = pt.DeviceScene.from_text(G.text(G.SPAN_SCENES[name], tmp_path))  # material ids = the text's
    want = HM.expected_hits(z["rays"], z["counts"], z["data"])
    for got in both_paths(ds, z["rays"]):
        same(got, want, ("hit", "exit", "t", "normal", "material", "pos"), name)


@pytest.mark.gpu
def test_gpu_seam_trees(built):
    z, texts = seam(), G.seam_texts()
    assert sorted(texts) == sorted(C.seam_names()) and len(texts) == 18
    decided = undecided_hit = 0
    for name in C.seam_names():
        ds = pt.DeviceScene.from_text(texts[name])
        rays, m = z["rays_" + name], z["m_" + name]
        hit, ex, row, t = HM.scan(z["cnt_" + name], z["t_" + name])
        want = {"hit": hit.astype(np.int32), "exit": ex.astype(np.int32), "t": t,
                "material": np.where(hit, m[row, ex.astype(np.int64)], -1).astype(np.int32)}
        fast, merge = both_paths(ds, rays)
        for got in (fast, merge):
            same(got, want, ("hit", "exit", "t", "material"), name)
        decided += int((fast["decided"] == 1).sum())
        undecided_hit += int(((fast["decided"] == 0) & (fast["hit"] == 1)).sum())
    print("device: %d decided, %d undecided and hit" % (decided, undecided_hit))
    assert decided >= MIN_CENSUS and undecided_hit >= MIN_CENSUS


def shade_rays(name):
    """caller rays of a shading scene: the reference list's for scene_p1, else zoo's traceRay inputs"""
    if name == "scene_p1":
        return np.load(os.path.join(GOLD, "spans_p1.npz"))["rays"][:1024]
    return T.trace_rays_input(1024)[:, :6]


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.SHADE_SCENES)
def test_gpu_shading_inputs_are_the_oracles_lookups(built, tmp_path, name):
    text, rays = G.text(name, tmp_path), shade_rays(name)
    ds = pt.DeviceScene.from_text(text)
    cnt, rows = HM.rows_from_oracle(O.spans(text, rays))
    want = HM.expected_hits(rays, cnt, rows)
    want["shade"], want["ior"] = HM.expected_shade(text, O.tex_eval(text, want["pos"]), want["material"],
                                                   want["hit"] != 0)
    used = np.unique(want["material"][want["hit"] != 0])
    print(name, "materials hit:", used.tolist())
    assert len(used) >= 3
    for got in both_paths(ds, rays, shade=True):
        same(got, want, FIELDS + ("shade",), name)
    # without shade_out the record is the same
    same(ds.query_hits(rays), want, FIELDS, name + " (no shade)")


def shell_rays(n=384, seed=11):
    """rays at the shell from above, from inside its cavity (the second span's entry) and from inside its
    wall (an exit)"""
    rng = np.random.default_rng(seed)
    c = np.array(M.GLASS_C, np.float32)
    o = np.tile(np.array([0.0, 1.6, 0.0], np.float32), (n, 1))
    d = (c + rng.normal(scale=0.25, size=(n, 3)) - o).astype(np.float32)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    inside = np.arange(n) % 3 == 1
    o[inside], d[inside] = c + 0.1 * u[inside], rng.normal(size=(int(inside.sum()), 3))
    wall = np.arange(n) % 3 == 2
    o[wall], d[wall] = c + 0.4 * u[wall], rng.normal(size=(int(wall.sum()), 3))
    return np.concatenate([o, d], axis=1).astype(np.float32)


@pytest.mark.gpu
def test_gpu_multispan_shell_is_its_builtin_twin(built):
    rays = shell_rays()
    user = both_paths(pt.DeviceScene(M.shell_scene(True)), rays)
    twin = both_paths(pt.DeviceScene(M.shell_scene(False)), rays)
    same(user[0], twin[0], FIELDS, "shell vs Difference(Sphere, Sphere)")
    h = twin[0]
    assert (h["hit"] == 1).sum() >= 100 and (h["exit"] == 1).sum() >= 20
