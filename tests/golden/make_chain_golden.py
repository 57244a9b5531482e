"""Freezes the chained-rendering fixtures tests/golden/chain_*.npz from the
UNMODIFIED reference: tracePixel<T> / traceRay<T> (include/path-trace.h:58-165,
:187-201) driven by tests/golden/chain_driver.cpp with one engine threaded
through every sample of every entry of a chain, T stepping DefaultRandomEngine's
recurrence from the chain's initial state.  Per entry the colour, the engine
state after it and the draws since the chain's start are kept.

The driver is compiled into oracle/_ref/ (never committed) against the objects
`make -C oracle ref` leaves there.  Runs only where /root/reference exists,
never from build(), smoke() or a test.  The reference asserts at its rejection
cap (path-trace.h:148): the driver aborting is the check that no fixture sample
reaches it.

    python tests/golden/make_chain_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "path-trace_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import oracle_py as O  # noqa: E402
import zoo as T  # noqa: E402
from chain_cases import CASES  # noqa: E402
from pathtrace import lcg_state  # noqa: E402
from pathtrace.scene import to_text  # noqa: E402

REF = "/root/reference"
REFOUT = os.path.join(ROOT, "oracle", "_ref")
DRIVER = os.path.join(REFOUT, "chain_driver")
REF_OBJS = "sphere plane union intersection difference object path-trace image color span material transform vector3d"


def build_driver():
    """oracle/Makefile's flags and link line for ptref, with our driver in ref_driver.o's place."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fexceptions"]
    obj = os.path.join(REFOUT, "chain_driver.o")
    subprocess.check_call(["g++", "-std=c++17", *flags, "-w", "-I" + os.path.join(REF, "include"), "-c", "-o", obj,
                           os.path.join(HERE, "chain_driver.cpp")])
    subprocess.check_call(["g++", "-o", DRIVER, obj, *[os.path.join(REFOUT, n + ".o") for n in REF_OBJS.split()],
                           "-lpthread", "-Wl,--unresolved-symbols=ignore-in-object-files", "-Wl,-z,lazy", "-no-pie"])


def splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return x ^ (x >> 31)


def hashed_pixels(n, W, H, seed):
    return np.array([splitmix(seed * 1000003 + k) % (W * H) for k in range(n)], dtype=np.int32)


def seeds(v):
    return np.array([lcg_state(s) for s in v], dtype=np.uint64)


def cases():
    """name -> (W, H, spp, entries, chain lengths, initial states)"""
    c = {}
    mixed = np.array([y * 64 + x for y in (4, 14, 18, 22) for x in (8, 14, 20, 26, 32, 40, 44, 48, 52)],
                     dtype=np.int32)
    c["mixed"] = (64, 36, 3, mixed, [36], seeds([7]))
    # fewer chains than one workgroup's waves, an empty one, a repeated pixel inside one chain
    un = hashed_pixels(28, 64, 36, 11)
    un[5] = un[3]  # chain 3 = entries 3..9
    for spp in (1, 5):
        c["uneven%d" % spp] = (64, 36, spp, un, [0, 1, 2, 7, 17, 1], seeds(range(100, 106)))
    # more chains than one dequeue round; 32-bit seeds and full 64-bit states
    st = np.concatenate([seeds(range(150)), np.array([splitmix(0xC0FFEE + k) for k in range(150)], dtype=np.uint64)])
    c["many"] = (64, 36, 2, hashed_pixels(600, 64, 36, 23), [2] * 300, st)
    c["csg"] = (32, 24, 2, hashed_pixels(32, 32, 24, 31), [8] * 4, seeds(range(40, 44)))
    rays = T.trace_rays_input(48)
    c["rays1"] = (0, 0, 2, rays, [48], seeds([9]))
    c["rays8"] = (0, 0, 2, rays, [6] * 8, seeds(range(60, 68)))
    return c


def run(name, W, H, spp, entries, lengths, states0):
    builder, depth, is_rays = CASES[name]
    begin = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = len(entries)
    assert begin[-1] == n and len(states0) == len(lengths)
    screen = (float(W), float(H), float(2 * min(W, H)))  # pathtrace.make_params' default
    with tempfile.TemporaryDirectory() as d:
        f = lambda k: os.path.join(d, k)  # noqa: E731
        open(f("scene.txt"), "w").write(to_text(T.build(builder), f("img")))
        np.ascontiguousarray(entries).tofile(f("entries.bin"))
        begin.tofile(f("begin.bin"))
        np.ascontiguousarray(states0, dtype=np.uint64).tofile(f("states.bin"))
        if is_rays:
            cmd = [DRIVER, "rays", f("scene.txt"), str(spp), str(depth)]
        else:
            cmd = [DRIVER, "pixels", f("scene.txt"), str(W), str(H), str(spp), str(depth)] + [repr(v) for v in screen]
        subprocess.check_call(cmd + [f("entries.bin"), f("begin.bin"), f("states.bin"), f("out.bin")])
        raw = open(f("out.bin"), "rb").read()
    nc = len(lengths)
    assert len(raw) == 12 * n + 16 * n + 8 * nc
    colour = np.frombuffer(raw, dtype=np.float32, count=3 * n).reshape(n, 3)
    state_after = np.frombuffer(raw, dtype=np.uint64, count=n, offset=12 * n)
    draws = np.frombuffer(raw, dtype=np.uint64, count=n, offset=20 * n)
    final_state = np.frombuffer(raw, dtype=np.uint64, count=nc, offset=28 * n)
    np.savez_compressed(os.path.join(HERE, "chain_%s.npz" % name), entries=entries, begin=begin,
                        states0=np.asarray(states0, dtype=np.uint64), colour=colour, state_after=state_after,
                        draws=draws, final_state=final_state, meta=np.array([W, H, spp, depth], dtype=np.int64),
                        screen=np.array(screen, dtype=np.float64))
    per = np.diff(np.concatenate([[0], draws])) if nc == 1 else draws
    print("%-8s %4d entries %3d chains  draws/entry min %d max %d  mean colour %s" %
          (name, n, nc, per.min() if n else 0, per.max() if n else 0, colour.mean(axis=0)))


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference sources (%s)" % REF)
    build_driver()
    assert O.ref_available()
    for name, args in cases().items():
        run(name, *args)


if __name__ == "__main__":
    main()
