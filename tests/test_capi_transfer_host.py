"""The staging and readback path of the C ABI's host layer (pl-svo_amd/csrc/capi_transfer.hpp: Blob, Carver, upload_blob, Readback) on
a plain context object against the emulated runtime, as a stand-alone program under AddressSanitizer and UBSan
(tests/host/capi_transfer_host_test.cpp): section offsets, zero-filled and empty sections, both pinned staging buffers and their
regrowth, the direct path above 8 MB, 1 / 4 / 9 readback ranges with empty ones, the pinned / fallback border at 4 MB."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staging_and_readback_helpers_under_sanitizers(tmp_path):
    exe = str(tmp_path / "capi_transfer_host_test")
    subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unknown-pragmas", "-Wno-attributes", "-I", os.path.join(ROOT, "tests", "host", "emu"), "-I", os.path.join(ROOT, "pl-svo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "capi_transfer_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stdout + out.stderr[-3000:]
    checks, bad = (int(t) for t in out.stdout.split())
    assert checks >= 150 and bad == 0, out.stdout + out.stderr[-3000:]
