"""The tail split of the alignment launch on the CPU: tests/test_gpu_tail_split.py run against the host emulation build (the emulator
runs the workgroups of a launch in blockIdx order, so a fine part always finds its coarse part's flag: this checks that the state
arrives whole through HBM -- indexing, control flow, every carried value -- not the cross-XCD visibility protocol, which only the
MI355X run exercises), and the one branch nothing may provoke on a GPU: the bounded poll that gives up."""
import os
import subprocess
import sys

import pytest

from test_emu_parity import CXX, ROOT, build_emu, emu_env

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="host emulation build needs clang++ (ext_vector_type, address spaces)")


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_tail"))


def test_tail_split_cases_pass_on_the_emulated_library(emu_lib):
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_tail_split.py"), "-m", "gpu", "-q", "-n", "4", "-s",
                          "-p", "no:cacheprovider", "-k", "not full_size"], env=emu_env(emu_lib), capture_output=True, text=True, cwd=ROOT)
    tail = out.stdout[-4000:] + out.stderr[-1000:]
    assert out.returncode == 0, tail
    last = [l for l in out.stdout.splitlines() if " passed" in l][-1]
    assert " failed" not in last and " skipped" not in last and int(last.split(" passed")[0].split()[-1]) == 4, tail


def test_a_fine_part_whose_flag_never_comes_gives_up_and_reports_it(emu_lib):
    """the coarse parts publish a wrong flag value (test hook of the emulation build): every fine part's bounded poll runs out, flags its
    frame with error 2 and ends; the fetch reports a hand-off time-out (not a capacity problem), the context stays usable, and with the
    right value the same batch runs through."""
    code = r'''
import ctypes as C, importlib, os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
P = importlib.import_module("pl-svo_amd")
import tail_split_cases as T
imgs, jobs = T.mixed_batch(P)
ctx = T.make_ctx(P, PLSVO_ALIGN_TAIL_MIN=4, PLSVO_ALIGN_TAIL_FRAMES=4)
T.load_images(ctx, imgs, 320, 240)
ctx.set_launch_shapes(align_threads=64)
hook = P.capi.lib().plsvo_emu_set_tail_flag_value
hook.argtypes = [C.c_uint]
hook.restype = None
ctx.align_stage(jobs)
ctx.align_run()
good = ctx.align_fetch()
hook(7)
ctx.align_run()
assert ctx.align_tail_frames() == 4
try:
    ctx.align_fetch()
    raise SystemExit("no error reported")
except P.capi.PlsvoError as e:
    assert e.code == P.abi.E_HIP and "timed out" in str(e) and "capacity" not in str(e), (e.code, str(e))
hook(1)
ctx.align_run()
again = ctx.align_fetch()
assert all(np.array_equal(a.T, b.T) and a.iters_per_level == b.iters_per_level for a, b in zip(good, again))
ctx.close()
print("ok")
'''
    out = subprocess.run([sys.executable, "-c", code, ROOT], env=emu_env(emu_lib), capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-1500:] + out.stderr[-3000:]
