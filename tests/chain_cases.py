"""The chained-rendering fixtures (tests/golden/chain_*.npz, frozen from the
unmodified reference by tests/golden/make_chain_golden.py): tracePixel<T> /
traceRay<T> with ONE engine threaded through every sample of every entry of a
chain, as a program that owns a DefaultRandomEngine runs them.  Their scenes
and loader, shared by the maker and tests/test_chain.py.  No device kernel
consumes them yet: they are the yardstick for one that runs a chain on a
caller's engine state."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fixture -> (scene builder (zoo.build), depth, rays)
CASES = {
    "mixed": ("scene_p1", 8, False),
    "uneven1": ("scene_p1", 8, False),
    "uneven5": ("scene_p1", 8, False),
    "many": ("scene_p1", 8, False),
    "csg": ("csg_zoo", 6, False),
    "rays1": ("scene_p1", 8, True),
    "rays8": ("scene_p1", 8, True),
}
LCG_MULT, LCG_INC, M64 = 214013, 2531011, (1 << 64) - 1


def lcg_discard(state: int, n: int) -> int:
    """DefaultRandomEngine's state after n more draws, by the O(log n) jump of
    include/pt/pt_engine.h (v' = A v + G c)."""
    a, g, m, h = 1, 0, LCG_MULT, 1
    while n:
        if n & 1:
            g = (g * m + h) & M64
            a = (a * m) & M64
        h = (h * (m + 1)) & M64
        m = (m * m) & M64
        n >>= 1
    return (a * state + g * LCG_INC) & M64


class Fixture:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, "chain_%s.npz" % name))
        self.name = name
        self.builder, self.depth, self.is_rays = CASES[name]
        self.W, self.H, self.spp, depth = [int(v) for v in z["meta"]]
        assert depth == self.depth
        self.screen = tuple(float(v) for v in z["screen"])
        self.entries = z["entries"]          # int32 pixel indices, or n x 7 float32 rays
        self.begin = z["begin"]              # nchains + 1 int64
        self.lengths = np.diff(self.begin)
        self.states0 = z["states0"]          # uint64, the chains' initial states
        self.colour = z["colour"]            # n x 3 float32
        self.state_after = z["state_after"]  # uint64 per entry
        self.draws = z["draws"]              # uint64 per entry, since its chain's start
        self.final_state = z["final_state"]  # uint64 per chain

    def scene(self):
        import zoo
        return zoo.build(self.builder)
