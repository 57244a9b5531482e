"""The chained modules tests/test_chain_gpu.py and tests/test_chain_abi.py use
(__graft_entry__.build() precompiles them after tests/precompile_lane_resume.py's):
scene_p1 at depth 8 for chained pixels and chained rays, csg_zoo at depth 6 for
chained pixels -- tests/chain_cases.py's scenes and depths."""


def test_jobs():
    import pathtrace as pt
    import zoo
    from chain_cases import CASES
    kinds = sorted(set(CASES.values()))  # (builder, depth, rays)
    return [((lambda b=b, d=d, r=r: pt.DeviceScene(zoo.build(b)).compile_chain(d, r)), None) for b, d, r in kinds]
