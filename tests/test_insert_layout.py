"""The insertion's structs of include/plsvo_hip.h against their ctypes mirrors, size and every offset, the constants beside them, and
the entry points in the built library (without the feature none of these exist)."""
import ctypes as C
import os
import subprocess

import select_cases as Sc

A = Sc.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("plsvo_candidates_reserve", "plsvo_candidates_capacity", "plsvo_candidates_insert_keyframe", "plsvo_candidates_insert_fetch", "plsvo_candidates_fetch_map", "plsvo_candidates_set_positions")


def test_ctypes_mirrors_have_the_c_layouts(tmp_path):
    header = os.path.join(ROOT, "include", "plsvo_hip.h")
    structs = {"plsvo_cand_reserve": A.CandReserve, "plsvo_cand_insert": A.CandInsert, "plsvo_cand_insert_out": A.CandInsertOut, "plsvo_cand_map_out": A.CandMapOut,
               "plsvo_cand_positions": A.CandPositions}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("K %d %d %d\\n", PLSVO_K_SELECT, PLSVO_K_INSERT, PLSVO_K_COUNT);')
    lines.append('printf("E %d %d %d\\n", PLSVO_LM_EVENT_PROMOTED, PLSVO_LM_EVENT_DELETED, PLSVO_LM_EVENT_JOINED);')
    lines.append('printf("S %d %d %d\\n", PLSVO_INSERT_POSE_HOST, PLSVO_INSERT_POSE_DEV, PLSVO_INSERT_POSE_RESIDENT);')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in out.strip().splitlines()}
    for cname, ct in structs.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(v) for v in got["K"]] == [A.K_SELECT, A.K_INSERT, A.K_COUNT]
    assert [int(v) for v in got["E"]] == [A.LM_EVENT_PROMOTED, A.LM_EVENT_DELETED, A.LM_EVENT_JOINED]
    assert [int(v) for v in got["S"]] == [A.INSERT_POSE_HOST, A.INSERT_POSE_DEV, A.INSERT_POSE_RESIDENT]
    assert C.sizeof(A.CandInsert) <= 104                               # "a per-stream record of about 100 bytes"


def test_the_library_exports_the_entry_points():
    """the product library as build() leaves it (symbols only: no device is opened)"""
    lib = os.path.join(ROOT, "pl-svo_amd", "libplsvo_hip.so")
    assert os.path.exists(lib), "pl-svo_amd/libplsvo_hip.so is not built: run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert f" T {name}\n" in out, name
        assert name in Sc.P.capi.SYMBOLS, name

