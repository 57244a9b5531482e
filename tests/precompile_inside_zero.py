"""The device modules tests/test_inside_zero.py renders and traces (__graft_entry__.build()
precompiles them after tests/precompile_lane_resume.py's): the lattice scenes' ray-list modules, the
csgfuzz Difference trace scenes' and C3's render module, each with the inside-solid probe and without
it (PT_INSIDE_ZERO=0)."""
import os


def _with_defines(defs, make):
    def job():
        if defs:
            os.environ["PT_DEVICE_DEFINES"] = defs
        try:
            make()
        finally:
            os.environ.pop("PT_DEVICE_DEFINES", None)  # pool workers are reused
    return job


def test_jobs():
    import pathtrace as pt
    import csgfuzz as F
    import inside_zero as Z
    from pathtrace import scenes
    from test_inside_zero import C3, FUZZ_SCENES, OFF, TRACE_DEPTH
    jobs = []
    for defs in ("", OFF):
        for name in Z.GPU_SCENES:
            depth = 1 if name == "overflow" else TRACE_DEPTH
            jobs.append((_with_defines(defs, lambda name=name, depth=depth:
                                       pt.DeviceScene(Z.lattice_scene(name)).compile_rays(depth)), None))
        for s in FUZZ_SCENES:
            jobs.append((_with_defines(defs, lambda s=s: pt.DeviceScene(F.trace_scene(s, leaf=True))
                                       .compile_rays(TRACE_DEPTH)), None))
        jobs.append((_with_defines(defs, lambda: scenes.CONFIGS["C3"].device_scene().compile(C3["depth"])), None))
    return jobs
