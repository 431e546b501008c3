"""The structs of plsvo_candidates_compact in include/plsvo_hip.h against their ctypes mirrors, size and every offset, the constants beside
them, and the entry points in the built library (without the feature none of these exist)."""
import ctypes as C
import os
import subprocess

import np_compact as NK
import select_cases as Sc

A = Sc.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("plsvo_candidates_compact", "plsvo_candidates_compact_fetch")


def test_ctypes_mirrors_have_the_c_layouts(tmp_path):
    header = os.path.join(ROOT, "include", "plsvo_hip.h")
    structs = {"plsvo_cand_compact": A.CandCompact, "plsvo_cand_compact_out": A.CandCompactOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("K %d %d\\n", PLSVO_K_INSERT, PLSVO_K_COUNT);')
    lines.append('printf("M %d %d %d\\n", PLSVO_COMPACT_STANDBY, PLSVO_COMPACT_ALWAYS, PLSVO_COMPACT_ROOM);')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in out.strip().splitlines()}
    for cname, ct in structs.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(v) for v in got["K"]] == [A.K_INSERT, A.K_COUNT] == [10, 12]          # timed under the insertion's family: no new one
    assert [int(v) for v in got["M"]] == [A.COMPACT_STANDBY, A.COMPACT_ALWAYS, A.COMPACT_ROOM] == [NK.STANDBY, NK.ALWAYS, NK.ROOM] == [0, 1, 2]
    assert C.sizeof(A.CandCompact) == 16 and C.sizeof(A.CandCompactOut) == 88
    assert tuple(f for f, _ in A.CandCompactOut._fields_)[:18] == A._CAND_COMPACT_COUNTS == NK.REPORT


def test_the_library_exports_the_entry_points():
    """the product library as build() leaves it (symbols only: no device is opened)"""
    lib = os.path.join(ROOT, "pl-svo_amd", "libplsvo_hip.so")
    assert os.path.exists(lib), "pl-svo_amd/libplsvo_hip.so is not built: run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert f" T {name}\n" in out, name
        assert name in Sc.P.capi.SYMBOLS, name
