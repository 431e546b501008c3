"""The structure optimisation on the resident map tables on the CPU: tests/test_gpu_structsel.py run against the host emulation build --
the same device code on the lock-step wave emulator, ballots, the carried tie count, the wave-minimum walk over the keys and all: this
checks the algorithm and its control flow on every case, not the compiled gfx950 code."""
import os
import subprocess
import sys

import pytest

from test_emu_parity import CXX, ROOT, build_emu, emu_env

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="host emulation build needs clang++ (ext_vector_type, address spaces)")


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_structsel"))


def test_structsel_cases_pass_on_the_emulated_library(emu_lib):
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_structsel.py"), "-m", "gpu", "-q", "-n", "4", "-s",
                          "-p", "no:cacheprovider"], env=emu_env(emu_lib), capture_output=True, text=True, cwd=ROOT)
    tail = out.stdout[-4000:] + out.stderr[-1000:]
    assert out.returncode == 0, tail
    last = [l for l in out.stdout.splitlines() if " passed" in l][-1]
    assert " failed" not in last and " skipped" not in last and int(last.split(" passed")[0].split()[-1]) == 11, tail
