"""The per-level set-up of the alignment kernel's throughput shapes on the CPU: the small cases of tests/test_gpu_align_setup.py run
against the host emulation build -- the slot table, the hand-pipelined record loop and plsvo_align_fetch_records compiled for the host,
lane by lane: indexing, clamping and control flow, not the overlap of the requests, which only the MI355X run and its phase table show."""
import os
import subprocess
import sys

import pytest

from test_emu_parity import CXX, ROOT, build_emu, emu_env

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="host emulation build needs clang++ (ext_vector_type, address spaces)")


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_setup"))


def test_align_setup_cases_pass_on_the_emulated_library(emu_lib):
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_align_setup.py"), "-m", "gpu", "-q", "-n", "4", "-s",
                          "-p", "no:cacheprovider", "-k", "not full_size"], env=emu_env(emu_lib), capture_output=True, text=True, cwd=ROOT)
    tail = out.stdout[-4000:] + out.stderr[-1000:]
    assert out.returncode == 0, tail
    last = [l for l in out.stdout.splitlines() if " passed" in l][-1]
    assert " failed" not in last and " skipped" not in last and int(last.split(" passed")[0].split()[-1]) == 6, tail
