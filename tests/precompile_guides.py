"""The guides modules (pt_query_hits, pt_render_guides; device/pt_guides.h) tests/test_hits_gpu.py,
tests/test_guides_gpu.py, tests/test_hits_abi.py and tests/test_facade_guides.py use
(__graft_entry__.build() precompiles them after every render module): the span and shading scenes and the
guide frames' scenes from their texts (tests/guide_scenes.py), the 18 seam trees of
tests/golden/fastcheck_seam.npz, the multi-span shell with its built-in twin, and scene_p1 and the CSG zoo
built through the constructors; and the depth-0 render modules the guide frames are compared with."""


def _from_text(name):
    import tempfile
    import guide_scenes as G
    import pathtrace as pt
    with tempfile.TemporaryDirectory() as td:  # the scene copies its images when it loads the text
        return pt.DeviceScene.from_text(G.text(name, td))


def test_jobs():
    import guide_scenes as G
    import multispan as M
    import pathtrace as pt
    import zoo
    names = sorted(set(G.SPAN_SCENES.values()) | set(G.SHADE_SCENES) | set(G.GUIDE_SCENES))
    jobs = [((lambda n=n: _from_text(n).compile_guides()), None) for n in names]
    # pt_render at depth 0, the reference of the emission plane (tests/test_guides_gpu.py)
    jobs += [((lambda n=n: _from_text(n)), 0) for n in G.GUIDE_SCENES]
    jobs += [((lambda t=t: pt.DeviceScene.from_text(t).compile_guides()), None) for t in G.seam_texts().values()]
    jobs += [((lambda u=u: pt.DeviceScene(M.shell_scene(u)).compile_guides()), None) for u in (True, False)]
    jobs += [((lambda b=b: pt.DeviceScene(zoo.build(b)).compile_guides()), None) for b in ("scene_p1", "csg_zoo")]
    return jobs
