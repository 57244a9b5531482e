"""The device modules tests/test_fastcheck.py traces and renders (__graft_entry__.build() precompiles
them with tests/precompile_inside_zero.py's): the ray-list module of every seam scene with the lane-resume
form on and off, and the render module of the minimal-case scene.  C3's render module is the product's."""


def test_jobs():
    import pathtrace as pt
    import fastcheck as C
    from test_fastcheck import TRACE_DEPTH
    jobs = [((lambda name=name, on=on: pt.DeviceScene(C.seam_trees_scene(name), lane_resume=on)
              .compile_rays(TRACE_DEPTH)), None) for name in C.seam_names() for on in (1, 0)]
    jobs.append(((lambda: pt.DeviceScene(C.seam_trees_scene(C.MINIMAL))), C.SEAM_FRAME["depth"]))
    return jobs
