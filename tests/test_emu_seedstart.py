"""Seeds started from a keyframe's corners on the CPU: tests/test_gpu_seedstart.py (less its 640 x 480 case) run against the host
emulation build -- the occupancy, detection and start kernels on the lock-step wave emulator, ballots, ranks and the slot table and all:
this checks the algorithm and its control flow on every case, not the compiled gfx950 code."""
import os
import subprocess
import sys

import pytest

from test_emu_parity import CXX, ROOT, build_emu, emu_env

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="host emulation build needs clang++ (ext_vector_type, address spaces)")


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_seedstart"))


def test_seedstart_cases_pass_on_the_emulated_library(emu_lib):
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_seedstart.py"), "-m", "gpu", "-q", "-n", "4", "-s",
                          "-p", "no:cacheprovider", "-k", "not full_size"], env=emu_env(emu_lib), capture_output=True, text=True, cwd=ROOT)
    tail = out.stdout[-4000:] + out.stderr[-1000:]
    assert out.returncode == 0, tail
    last = [l for l in out.stdout.splitlines() if " passed" in l][-1]
    assert " failed" not in last and " skipped" not in last and int(last.split(" passed")[0].split()[-1]) == 10, tail
