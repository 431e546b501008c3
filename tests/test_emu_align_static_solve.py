"""The static-order solve option and the Jacobian's reciprocal depth on the CPU: tests/test_gpu_align_static_solve.py run against the host
emulation build (its cases are small: every one of them runs here).  The emulator executes the wave intrinsics of
plsvo_wave.hpp::wave_solve6_core lane by lane, so both routes of the solve and the ballot that chooses between them
are checked for indexing, control flow and arithmetic before a GPU is involved."""
import os
import subprocess
import sys

import pytest

from test_emu_parity import CXX, ROOT, build_emu, emu_env

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="host emulation build needs clang++ (ext_vector_type, address spaces)")


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_static_solve"))


def test_static_solve_cases_pass_on_the_emulated_library(emu_lib):
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_align_static_solve.py"), "-m", "gpu", "-q", "-n", "4", "-s",
                          "-p", "no:cacheprovider"], env=emu_env(emu_lib), capture_output=True, text=True, cwd=ROOT)
    tail = out.stdout[-4000:] + out.stderr[-1000:]
    assert out.returncode == 0, tail
    last = [l for l in out.stdout.splitlines() if " passed" in l][-1]
    assert " failed" not in last and " skipped" not in last and int(last.split(" passed")[0].split()[-1]) == 10, tail
