"""The reference's one-engine mode, host side: the chained fixtures' own
consistency (tests/golden/chain_*.npz) and the facade's DefaultRandomEngine
(tests/cpp/facade_engine.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import pathtrace as pt

import chain_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "path-trace_amd", "lib")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_fixture_self_consistent(name):
    """Every entry's recorded state is its chain's initial state advanced by the
    recorded draw count (the O(log n) jump of include/pt/pt_engine.h), draw
    counts never decrease along a chain, and a chain's final state is its last
    entry's (an empty chain's: its initial state)."""
    f = C.Fixture(name)
    assert f.begin[0] == 0 and f.begin[-1] == len(f.entries) == len(f.colour)
    assert len(f.states0) == len(f.final_state) == len(f.begin) - 1
    for c, s0 in enumerate(f.states0):
        prev, last = 0, int(s0)
        for k in range(f.begin[c], f.begin[c + 1]):
            assert int(f.draws[k]) >= prev
            prev = int(f.draws[k])
            last = int(f.state_after[k])
            assert C.lcg_discard(int(s0), prev) == last, (c, k)
        assert int(f.final_state[c]) == last
    if not f.is_rays:  # a pixel sample draws at least its two jitter numbers
        per = np.concatenate([np.diff(np.concatenate([[0], f.draws[a:b].astype(np.int64)]))
                              for a, b in zip(f.begin[:-1], f.begin[1:])])
        assert per.min() >= 2 * f.spp


def test_lcg_state_is_the_reference_seed():
    assert pt.lcg_state(0) == 0x12476242 and pt.lcg_state(7) == 7 ^ 0x12476242
    assert int(C.Fixture("mixed").states0[0]) == pt.lcg_state(7)


def test_facade_default_random_engine(built, tmp_path):
    """PathTrace::DefaultRandomEngine: SURVEY A.5's known answers (the first
    outputs for seeds 0, 1, 12345, frozen from the reference in
    tests/golden/kat.npy), discard(n) == n calls, the state() round trip."""
    exe = str(tmp_path / "facade_engine")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "facade_engine.cpp"),
                    "-L" + LIBDIR, "-lpt", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = np.array([int(v) for v in r.stdout.split()], dtype=np.uint32)
    assert list(got[:3]) == [15280, 3270311074, 2688171609]
    kat = np.load(os.path.join(ROOT, "tests", "golden", "kat.npy"))
    np.testing.assert_array_equal(got, kat[:15].view(np.uint32))
