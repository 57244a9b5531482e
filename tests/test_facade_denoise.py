"""The denoiser through the C++ host facade (include/pt/PathTrace.hpp): Renderer::denoise and
renderDenoised compile with g++ against the facade + libpt.so and return the bits of the C calls they
delegate to (pt_denoise; pt_render_converge and pt_render_guides before it) for P1 at 37 x 23
(tests/cpp/facade_denoise.cpp checks the rest in the binary, exit codes 10-17)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "path-trace_amd", "lib")


@pytest.fixture(scope="module")
def denoise_bin(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("facade") / "facade_denoise")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "facade_denoise.cpp"),
                    "-L" + LIBDIR, "-lpt", "-Wl,-rpath," + LIBDIR, "-o", out], check=True)
    return out


def test_facade_denoise_compiles(denoise_bin):
    """the facade's new members build under -Wall -Wextra -Werror; without its arguments the binary does nothing"""
    assert subprocess.run([denoise_bin], capture_output=True, timeout=60).returncode == 2


@pytest.mark.gpu
def test_facade_denoise_is_the_c_call(denoise_bin):
    r = subprocess.run([denoise_bin, "37", "23", "128"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr)
    f = r.stdout.split()
    assert f[:3] == ["denoise", "ok", str(37 * 23)] and int(f[3]) > 0, r.stdout
