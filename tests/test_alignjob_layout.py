"""The structs of plsvo_candidates_align_* in include/plsvo_hip.h against their ctypes mirrors, size and every offset, the constants
beside them, and the entry points in the built library (without the feature none of these exist)."""
import ctypes as C
import os
import subprocess

import np_alignjob as NA
import select_cases as Sc

A = Sc.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("plsvo_candidates_align_reserve", "plsvo_candidates_align_build", "plsvo_candidates_align_compose", "plsvo_candidates_align_poses_dev",
                "plsvo_candidates_align_fetch", "plsvo_candidates_align_fetch_job")


def test_ctypes_mirrors_have_the_c_layouts(tmp_path):
    header = os.path.join(ROOT, "include", "plsvo_hip.h")
    structs = {"plsvo_cand_align_cfg": A.CandAlignCfg, "plsvo_cand_align_job": A.CandAlignJob, "plsvo_cand_align_report": A.CandAlignReport,
               "plsvo_cand_align_job_out": A.CandAlignJobOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("K %d %d\\n", PLSVO_K_ALIGN_INIT, PLSVO_K_COUNT);')
    lines.append('printf("S %d %d\\n", PLSVO_ALIGN_JOB_OK, PLSVO_ALIGN_JOB_NO_ROOM);')
    lines.append('printf("L %d\\n", PLSVO_MAX_LEVELS);')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in out.strip().splitlines()}
    for cname, ct in structs.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(v) for v in got["K"]] == [A.K_ALIGN_INIT, A.K_COUNT] == [0, 12]        # timed under the alignment's set-up family: no new one
    assert [int(v) for v in got["S"]] == [A.ALIGN_JOB_OK, A.ALIGN_JOB_NO_ROOM] == [NA.OK, NA.NO_ROOM] == [0, 1]
    assert int(got["L"][0]) == A.MAX_LEVELS == NA.MAX_LEVELS
    assert C.sizeof(A.CandAlignReport) == 32 and C.sizeof(A.CandAlignCfg) == 32


def test_the_library_exports_the_entry_points():
    """the product library as build() leaves it (symbols only: no device is opened)"""
    lib = os.path.join(ROOT, "pl-svo_amd", "libplsvo_hip.so")
    assert os.path.exists(lib), "pl-svo_amd/libplsvo_hip.so is not built: run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert f" T {name}\n" in out, name
        assert name in Sc.P.capi.SYMBOLS, name
