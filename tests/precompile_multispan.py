"""The device modules tests/test_multispan.py renders and queries
(__graft_entry__.build() precompiles them after tests/precompile_modules.py's):
multi_zoo and its built-in twin, the option variants, the shell with and
without slack slots, the query and ray-list modules."""


def test_jobs():
    import pathtrace as pt
    import multispan as M
    from test_multispan import DEPTH, OPTIONS, one_span_scene
    jobs = [((lambda u=u: pt.DeviceScene(M.multi_zoo(u))), DEPTH) for u in (True, False)]
    jobs += [((lambda o=o: pt.DeviceScene(M.multi_zoo(True), **o)), DEPTH) for o in OPTIONS]
    jobs += [((lambda k=k: pt.DeviceScene(M.shell_scene(True, k))), DEPTH) for k in (2, 4)]
    jobs += [((lambda: pt.DeviceScene(one_span_scene())), DEPTH)]
    jobs += [((lambda: pt.DeviceScene(M.multi_zoo(True)).compile_queries()), None),
             ((lambda: pt.DeviceScene(M.multi_zoo(True)).compile_rays(DEPTH)), None),
             ((lambda: pt.DeviceScene(M.multi_zoo(False)).compile_rays(DEPTH)), None)]
    return jobs
