"""Registers of the alignment kernel as shipped: the unit's gfx950 assembly through the Makefile's own target (`align_kernels.s`: the
flags of `align_kernels.o`), cross-compiled -- no GPU.  The four launch shapes keep nothing in scratch, the two throughput shapes stay
clear of the 256-register limit (every formulation that reached it spilled), and no packed-f32 arithmetic is left in the
unit, which is how `-fno-slp-vectorize` shows in the output."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-svo_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (cross-compiles for gfx950 without a GPU)")


@pytest.fixture(scope="module")
def asm():
    subprocess.run(["make", "-C", CSRC, "-s", "align_kernels.s"], check=True, capture_output=True)
    with open(os.path.join(CSRC, "align_kernels.s")) as f:
        return f.read()


@pytest.fixture(scope="module")
def kernels(asm):
    """{threads per frame: metadata block of align_fused_kernel<threads>}"""
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", asm, re.S):
        name = re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)
        t = re.search(r"align_fused_kernelILi(\d+)EE", name)
        if t:
            out[int(t.group(1))] = m.group(0)
    return out


def field(block, key):
    return int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))


def test_every_shape_is_built(kernels):
    assert sorted(kernels) == [64, 128, 256, 512]


@pytest.mark.parametrize("threads", [64, 128, 256, 512])
def test_no_scratch_and_no_spilled_vector_register(kernels, threads):
    blk = kernels[threads]
    assert field(blk, "private_segment_fixed_size") == 0
    assert field(blk, "vgpr_spill_count") == 0


@pytest.mark.parametrize("threads", [64, 128])
def test_throughput_shapes_stay_below_the_register_limit(kernels, threads):
    assert field(kernels[threads], "vgpr_count") <= 252


def test_no_packed_f32_arithmetic_in_the_unit(asm):
    assert "v_pk_mul_f32" not in asm and "v_pk_add_f32" not in asm
