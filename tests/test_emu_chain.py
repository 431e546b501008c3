"""The resident frame step's directed cases on the CPU: tests/test_gpu_chain.py run against the host emulation build -- the same device
code on the lock-step wave emulator, the ballots and the carried total of the selection's compaction, the 256-stride loops, the
dynamic LDS and all: this checks the glue kernels' algorithm and the staging / readback around them on every case, not the compiled
gfx950 code (the contraction of the bearing arithmetic is the compiler's there)."""
import os
import subprocess
import sys

import pytest

from test_emu_parity import CXX, ROOT, build_emu, emu_env

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="host emulation build needs clang++ (ext_vector_type, address spaces)")


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_chain"))


def test_chain_cases_pass_on_the_emulated_library(emu_lib):
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_chain.py"), "-m", "gpu", "-q", "-n", "3", "-s",
                          "-p", "no:cacheprovider"], env=emu_env(emu_lib), capture_output=True, text=True, cwd=ROOT)
    tail = out.stdout[-4000:] + out.stderr[-1000:]
    assert out.returncode == 0, tail
    last = [l for l in out.stdout.splitlines() if " passed" in l][-1]
    assert " failed" not in last and " skipped" not in last and int(last.split(" passed")[0].split()[-1]) == 6, tail
