"""The bootstrap's KLT track on the CPU: tests/test_gpu_klt.py runs against the host emulation build -- the same klt_pyrdown_kernel /
klt_first_kernel / klt_track_kernel / klt_commit_kernel and the same argument checks of the C ABI, compiled for the host without fma
contraction like the device unit.  This checks the source's control flow and operation order on every case, not the compiled gfx950
code: the MI355X run of that file stays the gate."""
import os
import subprocess
import sys

import pytest

from test_emu_parity import CXX, ROOT, build_emu, emu_env

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="host emulation build needs clang++ (ext_vector_type, address spaces)")


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_klt"))


def test_klt_cases_pass_on_the_emulated_library(emu_lib):
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_klt.py"), "-m", "gpu", "-q", "-n", "4",
                          "-p", "no:cacheprovider"], env=emu_env(emu_lib), capture_output=True, text=True, cwd=ROOT)
    tail = out.stdout[-4000:] + out.stderr[-1000:]
    assert out.returncode == 0, tail
    last = [l for l in out.stdout.splitlines() if " passed" in l][-1]
    assert " failed" not in last and " skipped" not in last and int(last.split(" passed")[0].split()[-1]) == 20, tail
