"""The structs of the plsvo_seeds_* calls in include/plsvo_hip.h against their ctypes mirrors, size and every offset, the constants beside
them, and the entry points in the built library (without the feature none of these exist)."""
import ctypes as C
import os
import subprocess

import select_cases as Sc

A = Sc.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("plsvo_seeds_reserve", "plsvo_seeds_capacity", "plsvo_seeds_stage", "plsvo_seeds_update", "plsvo_seeds_update_fetch", "plsvo_seeds_keyframe",
                "plsvo_seeds_fetch_lists", "plsvo_seeds_fetch_rows", "plsvo_seeds_commit_rows")


def test_ctypes_mirrors_have_the_c_layouts(tmp_path):
    header = os.path.join(ROOT, "include", "plsvo_hip.h")
    structs = {"plsvo_seed_reserve": A.SeedReserve, "plsvo_seed_params": A.SeedParams, "plsvo_seed_list": A.SeedList, "plsvo_seed_frame": A.SeedFrame,
               "plsvo_seed_report": A.SeedReport, "plsvo_seed_kf": A.SeedKf, "plsvo_seed_rows": A.SeedRows}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("S %d %d %d %d %d %d %d\\n", PLSVO_SEED_NOT_VISIBLE, PLSVO_SEED_NO_MATCH, PLSVO_SEED_UPDATED, PLSVO_SEED_CONVERGED, PLSVO_SEED_NAN, PLSVO_SEED_AGED, PLSVO_SEEDS_NO_ROOM);')
    lines.append('printf("K %d %d %d\\n", PLSVO_K_SEEDS, PLSVO_K_NEWCAND, PLSVO_K_COUNT);')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in out.strip().splitlines()}
    for cname, ct in structs.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(v) for v in got["S"]] == [A.SEED_NOT_VISIBLE, A.SEED_NO_MATCH, A.SEED_UPDATED, A.SEED_CONVERGED, A.SEED_NAN, A.SEED_AGED, A.SEEDS_NO_ROOM] == [0, 1, 2, 3, 4, 5, 1]
    assert [int(v) for v in got["K"]] == [A.K_SEEDS, A.K_NEWCAND, A.K_COUNT]           # the seed calls time their launches under the existing families
    assert C.sizeof(A.SeedReport) == 96 and [f for f, _ in A.SeedList._fields_][4:] == [f for f, _, _ in A._SEED_LIST_FIELDS]


def test_the_library_exports_the_entry_points():
    """the product library as build() leaves it (symbols only: no device is opened)"""
    lib = os.path.join(ROOT, "pl-svo_amd", "libplsvo_hip.so")
    assert os.path.exists(lib), "pl-svo_amd/libplsvo_hip.so is not built: run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert f" T {name}\n" in out, name
        assert name in Sc.P.capi.SYMBOLS, name
