"""The structs of plsvo_candidates_add / _reserve_landmarks in include/plsvo_hip.h against their ctypes mirrors, size and every offset,
the constants beside them, and the entry points in the built library (without the feature none of these exist)."""
import ctypes as C
import os
import subprocess

import select_cases as Sc

A = Sc.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("plsvo_candidates_reserve_landmarks", "plsvo_candidates_lm_capacity", "plsvo_candidates_add", "plsvo_candidates_add_fetch")


def test_ctypes_mirrors_have_the_c_layouts(tmp_path):
    header = os.path.join(ROOT, "include", "plsvo_hip.h")
    structs = {"plsvo_cand_lm_reserve": A.CandLmReserve, "plsvo_cand_new": A.CandNew, "plsvo_cand_add_out": A.CandAddOut, "plsvo_cand_reserve": A.CandReserve}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("K %d %d %d\\n", PLSVO_K_INSERT, PLSVO_K_NEWCAND, PLSVO_K_COUNT);')
    lines.append('printf("E %d %d %d %d\\n", PLSVO_LM_EVENT_PROMOTED, PLSVO_LM_EVENT_DELETED, PLSVO_LM_EVENT_JOINED, PLSVO_LM_EVENT_NEW);')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in out.strip().splitlines()}
    for cname, ct in structs.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(v) for v in got["K"]] == [A.K_INSERT, A.K_NEWCAND, A.K_COUNT] == [10, 11, 12]
    assert [int(v) for v in got["E"]] == [A.LM_EVENT_PROMOTED, A.LM_EVENT_DELETED, A.LM_EVENT_JOINED, A.LM_EVENT_NEW] == [1, 2, 4, 8]
    assert C.sizeof(A.CandReserve) == 24                               # plsvo_cand_reserve is what it was: the landmark room has a struct of its own
    assert [f for f, _ in A.CandNew._fields_][2:] == list(A._CAND_NEW_ORDER)


def test_the_library_exports_the_entry_points():
    """the product library as build() leaves it (symbols only: no device is opened)"""
    lib = os.path.join(ROOT, "pl-svo_amd", "libplsvo_hip.so")
    assert os.path.exists(lib), "pl-svo_amd/libplsvo_hip.so is not built: run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert f" T {name}\n" in out, name
        assert name in Sc.P.capi.SYMBOLS, name
