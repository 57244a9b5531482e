"""pt_render_guides (pathtrace.render_guides) on the GPU, bit for bit against the CPU.

The emission plane is by construction pt_render's frame at depth 0 in the reference order: it must equal
the CPU oracle's render and the device's own.  With every emissive texture a CoordTexture (p1_coord) the
emission of a hit is its position, so that identity pins the camera ray and t of every hit sample to the
oracle.  Every other plane is held to the model: camera rays from tests/hits_model.py, hits from the scan
of the oracle's span lists, textures from the oracle's lookups, each plane summed in float32 from +0 in
sample order and divided by spp.  The model itself is checked on the CPU: its emission plane is the
oracle's depth-0 render.

Frames are 16 x 12 at 4 spp.  The CSG zoo and scene_p1 are closed by a sky wall behind everything, which
every camera ray reaches (its z component is -screen_dist whatever the frame size), so no sample of theirs
misses and their coverage is 1 in every pixel at every frame size.  The frame whose pixels are partly
covered is csg_open's, the CSG zoo without that wall (tests/guide_scenes.py): the model counts its full,
partial and empty pixels on the CPU before the GPU test relies on them.

The modules are listed in tests/precompile_guides.py."""
import ctypes

import numpy as np
import pytest

import guide_scenes as G
import hits_model as HM
import oracle_py as O
import pathtrace as pt
from pathtrace import _lib

W, H, SPP, SEED = 16, 12, 4, 0x5EED
SCREEN = (float(W), float(H), float(2 * min(W, H)))  # make_params' default
PLANES = ["emission", "albedo", "normal", "t", "coverage", "material"]
# the pixel list: grid_width 33, a repeated entry, a pixel past the right edge (x = 20 >= 16)
GRID_W, SAMPLE_BEGIN = 33, 7
PIXEL_LIST = [5, 3 * GRID_W + 2, 5, 2 * GRID_W + 20, 11 * GRID_W + 15]
_cache = {}


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def scene_text(name, tmp_path_factory):
    if name not in _cache:
        _cache[name] = G.text(name, tmp_path_factory.mktemp("img_" + name))
    return _cache[name]


def model(text, pixels, gw, sample_begin):
    """the six planes of the entries `pixels`, from the CPU alone"""
    key = ("model", text, tuple(pixels), gw, sample_begin)
    if key in _cache:
        return _cache[key]
    n = len(pixels)
    rays = HM.camera_rays(pixels, W, H, gw, SCREEN, SEED, sample_begin, SPP).reshape(-1, 6)
    cnt, rows = HM.rows_from_oracle(O.spans(text, rays))
    w = HM.expected_hits(rays, cnt, rows)
    hit = w["hit"] != 0
    sh, _ = HM.expected_shade(text, O.tex_eval(text, w["pos"]), w["material"], hit)
    per = lambda a: np.asarray(a, np.float32).reshape((n, SPP) + np.shape(a)[1:])
    out = {"emission": HM.guide_mean(per(sh[:, 0:3]), SPP), "albedo": HM.guide_mean(per(sh[:, 3:6]), SPP),
           "normal": HM.guide_mean(per(w["normal"]), SPP), "t": HM.guide_mean(per(w["t"]), SPP),
           "coverage": HM.guide_mean(per(hit.astype(np.float32)), SPP),
           "material": w["material"].reshape(n, SPP)[:, 0].astype(np.int32)}
    _cache[key] = out
    return out


def same(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, name
    if name == "material":
        np.testing.assert_array_equal(got, want, err_msg=name)
    else:
        bad = np.flatnonzero((u32(got) != u32(want)).reshape(len(got), -1).any(axis=1))
        assert bad.size == 0, "%s: %d entries differ, first %s" % (name, bad.size, bad[:8])


# --------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("name", G.GUIDE_SCENES)
def test_model_emission_is_the_oracles_depth0_render(built, tmp_path_factory, name):
    text = scene_text(name, tmp_path_factory)
    m = model(text, list(range(W * H)), W, 0)
    want = O.render(text, W, H, SPP, 0, order=O.ORDER_REFERENCE)
    same(m["emission"], want, "emission")
    cov = m["coverage"]
    print(name, "coverage: %d full, %d partial, %d empty" % ((cov == 1).sum(), ((cov > 0) & (cov < 1)).sum(),
                                                              (cov == 0).sum()))
    if name == "p1_coord":  # the emission of a hit is its position: some sample's t is pinned in every pixel
        assert (cov > 0).all() and np.abs(m["emission"]).max() > 1
    if name == "csg_open":  # the sample loop is really exercised: hits and misses within one pixel
        assert ((cov > 0) & (cov < 1)).sum() >= 5 and (cov == 0).any() and (cov == 1).any()
        assert (m["material"] == -1).any()


def test_model_pixel_list_is_the_oracles(built, tmp_path_factory):
    """sample_begin 0: the oracle's grid render of the list (it has no sample offset)"""
    text = scene_text("scene_p1", tmp_path_factory)
    want = O.render_gw(text, W, H, GRID_W, PIXEL_LIST, SPP, 0, order=O.ORDER_REFERENCE)
    same(model(text, PIXEL_LIST, GRID_W, 0)["emission"], want, "emission")


# --------------------------------------------------------------------- GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("name", G.GUIDE_SCENES)
def test_gpu_guide_frames(built, tmp_path_factory, name):
    text = scene_text(name, tmp_path_factory)
    ds = pt.DeviceScene.from_text(text)
    g = pt.render_guides(ds, W, H, SPP)
    assert sorted(g) == sorted(PLANES) and g["emission"].shape == (H, W, 3) and g["t"].shape == (H, W)
    flat = {k: v.reshape((W * H,) + v.shape[2:]) for k, v in g.items()}
    # the identity: pt_render's frame at depth 0, reference order -- the oracle's and the device's own
    same(flat["emission"], O.render(text, W, H, SPP, 0, order=O.ORDER_REFERENCE), "emission vs oracle")
    same(flat["emission"], pt.render(ds, W, H, SPP, 0, order="reference").reshape(-1, 3), "emission vs pt.render")
    m = model(text, list(range(W * H)), W, 0)
    for k in PLANES:
        same(flat[k], m[k], k)


@pytest.mark.gpu
def test_gpu_guide_pixel_list(built, tmp_path_factory):
    text = scene_text("scene_p1", tmp_path_factory)
    ds = pt.DeviceScene.from_text(text)
    g = pt.render_guides(ds, W, H, SPP, pixels=PIXEL_LIST, grid_width=GRID_W, sample_begin=SAMPLE_BEGIN)
    m = model(text, PIXEL_LIST, GRID_W, SAMPLE_BEGIN)
    for k in PLANES:
        assert len(g[k]) == len(PIXEL_LIST)  # compact, one row per entry
        same(g[k], m[k], k)
    for k in PLANES:  # the repeated entry twice
        same(g[k][2:3], g[k][0:1], k)
    # pt_render with the same list, grid and sample offset at depth 0
    p, keep = pt.make_params(W, H, SPP, 0, None, SEED, "reference", 0, PIXEL_LIST, 0, GRID_W, SAMPLE_BEGIN)
    rgb = np.zeros((len(PIXEL_LIST), 3), dtype=np.float32)
    _lib.check(_lib.lib().pt_render(ds.handle, ctypes.byref(p), rgb.ctypes.data, None))
    same(g["emission"], rgb, "emission vs pt_render")


@pytest.mark.gpu
def test_gpu_null_planes_are_skipped(built, tmp_path_factory):
    text = scene_text("csg_zoo", tmp_path_factory)
    ds = pt.DeviceScene.from_text(text)
    full = pt.render_guides(ds, W, H, SPP)
    for names in (["normal"], ["t", "material"], ["albedo", "coverage"], ["emission"]):
        g = pt.render_guides(ds, W, H, SPP, planes=names)
        assert sorted(g) == sorted(names)
        for k in names:
            same(g[k].reshape(W * H, -1), full[k].reshape(W * H, -1), k)
