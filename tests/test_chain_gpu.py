"""Chained rendering on the GPU (pt_trace_chains) against the unmodified
reference's frozen results (tests/golden/chain_*.npz, tests/chain_cases.py):
tracePixel<T> / traceRay<T> with ONE DefaultRandomEngine threaded through every
sample of every entry of a chain.  Every comparison is bit for bit, on the
uint32 view of the colours and on the uint64 engine states."""
import os
import subprocess

import numpy as np
import pytest

import pathtrace as pt

import chain_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "path-trace_amd", "lib")

pytestmark = pytest.mark.gpu

_fixtures, _scenes = {}, {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = C.Fixture(name)
    return _fixtures[name]


def device_scene(f):
    """one DeviceScene per scene builder: the calls of a module share its loaded code object"""
    if f.builder not in _scenes:
        _scenes[f.builder] = pt.DeviceScene(f.scene())
    return _scenes[f.builder]


def run(f, entries, begin, states):
    ds = device_scene(f)
    if f.is_rays:
        return pt.trace_rays_chained(ds, entries, begin, states, f.spp, f.depth)
    return pt.trace_pixels_chained(ds, entries, begin, states, f.W, f.H, f.spp, f.depth, screen=f.screen)


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d differ, first at %s" % (what, len(bad), got.size, bad[0])


def test_first_entry_csg(built):
    """One entry of one chain on csg_zoo: the narrowest chained run there is."""
    f = fixture("csg")
    colour, after, final = run(f, f.entries[:1], [0, 1], f.states0[:1])
    same(colour, f.colour[:1], "colour")
    same(after, f.state_after[:1], "state_after")
    same(final, f.state_after[:1], "final_state")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_fixture(built, name):
    f = fixture(name)
    colour, after, final = run(f, f.entries, f.begin, f.states0)
    same(colour, f.colour, "colour")
    same(after, f.state_after, "state_after")
    same(final, f.final_state, "final_state")


def test_continuation(built):
    """Every chain of uneven5 cut after half of its entries, the second call starting
    from the states the first returned: the results of one call."""
    f = fixture("uneven5")
    cut = f.begin[:-1] + f.lengths // 2
    halves = []
    states = f.states0
    for lo, hi in ((f.begin[:-1], cut), (cut, f.begin[1:])):
        idx = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]).astype(np.int64)
        begin = np.concatenate([[0], np.cumsum(hi - lo)])
        colour, after, states = run(f, f.entries[idx], begin, states)
        halves.append((idx, colour, after))
    colour, after = np.zeros_like(f.colour), np.zeros_like(f.state_after)
    for idx, c, a in halves:
        colour[idx], after[idx] = c, a
    same(colour, f.colour, "colour")
    same(after, f.state_after, "state_after")
    same(states, f.final_state, "final_state")


def test_batching_independent(built):
    """many's 300 chains in one call and as 3 calls of 100: the same bits."""
    f = fixture("many")
    one = run(f, f.entries, f.begin, f.states0)
    parts = []
    for a in range(0, 300, 100):
        lo, hi = f.begin[a], f.begin[a + 100]
        parts.append(run(f, f.entries[lo:hi], f.begin[a:a + 101] - lo, f.states0[a:a + 100]))
    for k, what in enumerate(("colour", "state_after", "final_state")):
        same(np.concatenate([p[k] for p in parts]), one[k], what)
    same(one[0], f.colour, "colour against the reference")


def test_facade_chain(built, tmp_path):
    """PathTrace::tracePixel with a DefaultRandomEngine over mixed's 36 pixels in
    order (tests/cpp/facade_chain.cpp): colours and the engine's state after each
    call are the reference's, and tracePixelsChained gives the same chain in one call."""
    f = fixture("mixed")
    exe, pix = str(tmp_path / "facade_chain"), str(tmp_path / "pixels.bin")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "facade_chain.cpp"),
                    "-L" + LIBDIR, "-lpt", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    f.entries.astype(np.int32).tofile(pix)
    r = subprocess.run([exe, str(f.W), str(f.H), str(f.spp), str(f.depth)] + [repr(v) for v in f.screen] +
                       ["7", pix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = [ln.split() for ln in r.stdout.splitlines()]
    single = np.array([[int(v) for v in row[1:]] for row in rows if row[0] == "P"], dtype=np.uint64)
    chained = np.array([[int(v) for v in row[1:]] for row in rows if row[0] == "C"], dtype=np.uint64)
    end = [int(row[1]) for row in rows if row[0] == "E"]
    want = f.colour.view(np.uint32).astype(np.uint64)
    same(single[:, :3], want, "tracePixel colours")
    same(single[:, 3], f.state_after, "engine state after each tracePixel")
    same(chained, want, "tracePixelsChained colours")
    assert end == [int(f.final_state[0])]
