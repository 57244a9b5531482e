"""The device modules tests/test_lane_resume.py renders and traces
(__graft_entry__.build() precompiles them after tests/precompile_multispan.py's):
scene_p1 and the forcing scene with the lane-resume form on and off, the cap
scene's all-leaf variant (render and ray-list modules), the scene that is not all-leaf, and
scene_p1 with the form under PT_POISON_LDS; and the modules of
tests/test_lane_resume_csg.py: the ray-list modules of csgfuzz's six all-leaf
trace scenes and of its regression scene with the form on and off, and the
camera-path render modules."""
import os


def _poisoned():
    import pathtrace as pt
    from pathtrace import scenes
    from test_lane_resume import DEPTH
    os.environ["PT_DEVICE_DEFINES"] = "PT_POISON_LDS=1"
    try:
        pt.DeviceScene(scenes.scene_p1(), lane_resume=1).compile(DEPTH)
    finally:
        del os.environ["PT_DEVICE_DEFINES"]  # pool workers are reused


def test_jobs():
    import pathtrace as pt
    import csgfuzz as F
    from pathtrace import scenes
    from test_lane_resume import BRIGHT, DEPTH, bright_scene, cap_scene_leaf, force_scene
    jobs = [((lambda on=on: pt.DeviceScene(scenes.scene_p1(), lane_resume=on)), DEPTH) for on in (1, 0)]
    jobs += [((lambda on=on: pt.DeviceScene(force_scene(), lane_resume=on)), d) for on in (1, 0) for d in (DEPTH, 2)]
    jobs += [((lambda: pt.DeviceScene(cap_scene_leaf(), lane_resume=1).compile_rays(F.CAP_DEPTH)), None),
             ((lambda: pt.DeviceScene(cap_scene_leaf(F.CAP_RENDER["shift"]), lane_resume=1)), F.CAP_RENDER["depth"]),
             ((lambda: pt.DeviceScene(bright_scene(), lane_resume=1)), BRIGHT["depth"]),
             (_poisoned, None)]
    return jobs + csg_jobs()


def csg_jobs():
    import pathtrace as pt
    import csgfuzz as F
    from test_lane_resume_csg import CAM, CAM_SCENES, TRACE_DEPTH
    jobs = [((lambda s=s, on=on: pt.DeviceScene(F.trace_scene(s, leaf=True), lane_resume=on).compile_rays(TRACE_DEPTH)),
             None) for s in range(F.N_TRACE_SCENES) for on in (1, 0)]
    jobs += [((lambda s=s: pt.DeviceScene(F.trace_scene(s, leaf=True), lane_resume=1)), CAM["depth"])
             for s in CAM_SCENES]
    jobs += [((lambda on=on: pt.DeviceScene(F.regress_resume_negative_count()[0], lane_resume=on)
               .compile_rays(TRACE_DEPTH)), None) for on in (1, 0)]
    return jobs
