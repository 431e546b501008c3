"""The map-candidate stage without a device: the cases of tests/candidates_cases.py hold every path the kernel has (asserted as
conditions on the INPUTS, so a case cannot silently miss what it is there for), and the restatement tests/np_candidates.py has two
properties that need no kernel: each filed set equals a brute-force set computation, and the output order restricted to any grid cell
is a stable sort of that cell by descending type -- what cell.sort(pointQualityComparator) leaves (src/reprojector.cpp:239, :260)."""
import math

import numpy as np
import pytest

import candidates_cases as Cc
import np_candidates as N
import np_keyframe as K


def _all_streams():
    for name, fn in Cc.ALL.items():
        case = fn()
        for k, (st, T, ov) in enumerate(zip(case["streams"], case["T"], case["overlap"])):
            yield (name, k), st, T, ov


def _in_frame(T, pos, cell=Cc.CELL):
    return N.reproject(T, pos, Cc.CAM_T, cell, Cc.BOUNDARY)[1] >= 0


def _cosines(st, T, pos, obs):
    fp = K.se3_inv(T)[4:]
    a = N._normalized([fp[k] - pos[k] for k in range(3)])
    out = []
    for o in obs:
        kp = K.se3_inv(st["kf_T"][o["kf"]])[4:]
        d = N._normalized([kp[k] - pos[k] for k in range(3)])
        out.append((a[0] * d[0] + a[1] * d[1]) + a[2] * d[2])
    return out


def test_case_shapes():
    """320 x 240; batches of nine streams of unequal size; keyframes with 0, 1, 63, 64, 65 and 130 features; n_overlap 0, 1 and 10 with
    more keyframes in the table than in the list; observation lists of 1 to 12 entries"""
    assert Cc.CAM_T[4:] == (320, 240)
    case = Cc.sizes_case()
    assert len(case["streams"]) == 9 == len(Cc.edge_batch_case()["streams"])
    assert len({(len(s["pt_pos"]), len(s["seg_spos"]), len(s["kf_T"])) for s in case["streams"]}) == 9
    lens = {len(l) for s in case["streams"] for l in s["kf_pt"] + s["kf_seg"]}
    assert {0, 1, 63, 64, 65, 130} <= lens
    nov = {(len(ov), len(s["kf_T"])) for s, ov in zip(case["streams"], case["overlap"])}
    assert {0, 1, 10} <= {a for a, _ in nov} and all(any(b > a for a, b in nov if a == want) for want in (1, 10))
    obs = {len(l) for s in case["streams"] for l in s["pt_obs"] + s["seg_obs"]}
    assert set(range(1, 13)) <= obs


def test_inputs_reach_every_path():
    e = Cc.edge_case()
    st, T, ov, nm = e["streams"][0], e["T"][0], list(e["overlap"][0]), e["names"]
    lists = lambda lm: [k for k in range(len(st["kf_T"])) if lm in st["kf_pt"][k]]
    # a repeat visit whose winner is not the keyframe with the lowest table index
    ranks = sorted(ov.index(k) for k in lists(nm["repeat"]) if k in ov)
    assert len(ranks) >= 2 and ov[ranks[0]] > min(ov[r] for r in ranks[1:])
    # a landmark seen only by a keyframe outside the overlap list; it would project inside
    assert lists(nm["outside_only"]) and not set(lists(nm["outside_only"])) & set(ov) and _in_frame(T, st["pt_pos"][nm["outside_only"]])
    assert nm["outside_only"] not in st["pt_cand"]
    # a chosen observation in a keyframe outside the overlap list
    lm = nm["obs_outside"]
    cos = _cosines(st, T, st["pt_pos"][lm], st["pt_obs"][lm])
    best = int(np.argmax(cos))
    assert cos[best] >= 0.5 and st["pt_obs"][lm][best]["kf"] not in ov and set(lists(lm)) & set(ov)
    # a projection that fails on each of the four borders (the float pixel itself is inside the image), one with z < 0 that lands inside
    w, h, b = Cc.CAM_T[4], Cc.CAM_T[5], Cc.BOUNDARY
    for name, test in (("left", lambda x, y: 0 <= x < b and b <= y < h - b), ("right", lambda x, y: w - b <= x < w and b <= y < h - b),
                       ("top", lambda x, y: 0 <= y < b and b <= x < w - b), ("bottom", lambda x, y: h - b <= y < h and b <= x < w - b)):
        px, cell = N.reproject(T, st["pt_pos"][nm[name]], Cc.CAM_T, Cc.CELL, b)
        assert test(int(px[0]), int(px[1])) and cell == -1 and set(lists(nm[name])) & set(ov), name
    assert K.se3_act(T, st["pt_pos"][nm["behind"]])[2] < 0 and _in_frame(T, st["pt_pos"][nm["behind"]]) and set(lists(nm["behind"])) & set(ov)
    # a segment with exactly one end point out of frame
    s, en = st["seg_spos"][nm["seg_half"]], st["seg_epos"][nm["seg_half"]]
    assert _in_frame(T, s, Cc.SEG_CELL) != _in_frame(T, en, Cc.SEG_CELL) and any(nm["seg_half"] in st["kf_seg"][k] for k in ov)
    # has_view = 0 with the best cosine in (0, 0.5), and with every cosine <= 0
    cos = _cosines(st, T, st["pt_pos"][nm["view_side"]], st["pt_obs"][nm["view_side"]])
    assert 0.0 < max(cos) < 0.5 and int(np.argmax(cos)) != 0 and _in_frame(T, st["pt_pos"][nm["view_side"]])
    cos = _cosines(st, T, st["pt_pos"][nm["view_none"]], st["pt_obs"][nm["view_none"]])
    assert len(cos) >= 2 and max(cos) <= 0.0 and _in_frame(T, st["pt_pos"][nm["view_none"]])
    # two observations from keyframes with identical poses: equal cosines, the best of the list, the first of them not at the front
    lm = nm["equal_cos"]
    cos = _cosines(st, T, st["pt_pos"][lm], st["pt_obs"][lm])
    top = [i for i, c in enumerate(cos) if c == max(cos)]
    assert len(top) == 2 and top[0] > 0 and max(cos) >= 0.5
    kfs = [st["pt_obs"][lm][i]["kf"] for i in top]
    assert kfs[0] != kfs[1] and st["kf_T"][kfs[0]] == st["kf_T"][kfs[1]]
    # an empty observation list on a landmark that is filed
    assert st["pt_obs"][nm["no_obs"]] == [] and _in_frame(T, st["pt_pos"][nm["no_obs"]]) and set(lists(nm["no_obs"])) & set(ov)
    # all four types in one cell, out of type order on filing (one list, so list order is filing order)
    cells = {N.reproject(T, st["pt_pos"][lm], Cc.CAM_T, Cc.CELL, b)[1] for lm in nm["cell"]}
    types = [st["pt_type"][lm] for lm in nm["cell"]]
    assert len(cells) == 1 and cells != {-1} and set(types) == {0, 1, 2, 3} and types != sorted(types, reverse=True)
    k = [k for k in ov if nm["cell"][0] in st["kf_pt"][k]][0]
    assert [lm for lm in st["kf_pt"][k] if lm in nm["cell"]] == nm["cell"]
    # a TYPE_DELETED landmark that is filed and counted
    assert st["pt_type"][nm["deleted"]] == N.TYPE_DELETED and _in_frame(T, st["pt_pos"][nm["deleted"]])
    # a map candidate that fails, and one that is also a keyframe's landmark
    assert nm["cand_fail"] in st["pt_cand"] and not _in_frame(T, st["pt_pos"][nm["cand_fail"]])
    assert nm["repeat"] in st["pt_cand"] and _in_frame(T, st["pt_pos"][nm["repeat"]])
    assert nm["seg_in"] in st["seg_cand"] and any(nm["seg_in"] in st["kf_seg"][k] for k in ov)

    # ... and what the restatement makes of them
    r = N.candidates(st, T, ov, Cc.CAM_T, Cc.CELL, Cc.SEG_CELL, Cc.BOUNDARY)
    at = lambda lm: r["pt_lm"].index(lm)
    assert r["visits"]["pt_repeat"] >= 2 and r["pt_lm"].count(nm["repeat"]) == 2 and r["seg_lm"].count(nm["seg_in"]) == 2
    assert nm["outside_only"] not in r["pt_lm"] and nm["seg_half"] not in r["seg_lm"]
    assert all(nm[k] not in r["pt_lm"] for k in ("left", "right", "top", "bottom", "cand_fail")) and nm["behind"] in r["pt_lm"]
    assert r["pt_cand_failed"] == [1, 0, 0] and r["seg_cand_failed"] == [1, 0]
    assert st["pt_obs"][nm["obs_outside"]][r["pt_obs"][at(nm["obs_outside"])]]["kf"] == 6 and r["pt_has_view"][at(nm["obs_outside"])] == 1
    assert (r["pt_obs"][at(nm["view_side"])], r["pt_has_view"][at(nm["view_side"])], r["pt_active"][at(nm["view_side"])]) == (1, 0, 0)
    assert (r["pt_obs"][at(nm["view_none"])], r["pt_has_view"][at(nm["view_none"])]) == (0, 0)
    assert (r["pt_obs"][at(nm["equal_cos"])], r["pt_has_view"][at(nm["equal_cos"])]) == (1, 1)
    assert (r["pt_obs"][at(nm["no_obs"])], r["pt_has_view"][at(nm["no_obs"])], r["pt_active"][at(nm["no_obs"])]) == (-1, 0, 0)
    assert r["pt_lm"][-1] == nm["deleted"] and r["pt_active"][-1] == 0 and r["pt_has_view"][-1] == 1
    assert r["kf_count"][ov.index(4)] == len(nm["cell"])                      # the DELETED one is counted
    assert r["kf_count"][ov.index(0)] == 2                                    # `behind` and the segment inside; `repeat` went to keyframe 2


def test_the_random_streams_reach_repeats_failures_and_every_type():
    """the paths a generated scene does reach, counted on the restatement (the others are constructed: edge_case)"""
    tot = dict(visits=0, repeats=0, filed=0, failed=0)
    types = set()
    for (name, _), st, T, ov in _all_streams():
        if name != "sizes":
            continue
        r = N.candidates(st, T, ov, Cc.CAM_T, Cc.CELL, Cc.SEG_CELL, Cc.BOUNDARY)
        tot["visits"] += r["visits"]["pt"] + r["visits"]["seg"]
        tot["repeats"] += r["visits"]["pt_repeat"] + r["visits"]["seg_repeat"]
        tot["filed"] += r["n_filed_pt"] + r["n_filed_seg"]
        tot["failed"] += sum(r["pt_cand_failed"]) + sum(r["seg_cand_failed"])
        types |= set(r["pt_type"]) | set(r["seg_type"])
    assert types == {0, 1, 2, 3} and tot["visits"] > 1000 and tot["repeats"] > 100 and tot["filed"] > 300 and tot["failed"] > 0, tot


@pytest.mark.parametrize("name", sorted(Cc.ALL))
def test_filed_sets_equal_a_brute_force_set_computation(name):
    case = Cc.ALL[name]()
    for st, T, ov, r in zip(case["streams"], case["T"], case["overlap"], Cc.restate(case)):
        for kind, lists, ok, cand in (
                ("pt", st["kf_pt"], lambda lm: _in_frame(T, st["pt_pos"][lm]), st["pt_cand"]),
                ("seg", st["kf_seg"], lambda lm: _in_frame(T, st["seg_spos"][lm], Cc.SEG_CELL) and _in_frame(T, st["seg_epos"][lm], Cc.SEG_CELL), st["seg_cand"])):
            seen = {lm for k in ov for lm in lists[k] if lm >= 0}
            want = sorted([lm for lm in seen if ok(lm)] + [lm for lm in cand if ok(lm)])
            assert sorted(r[kind + "_lm"]) == want
            assert r[kind + "_cand_failed"] == [0 if ok(lm) else 1 for lm in cand]
        # a keyframe's count: its landmarks that no keyframe before it in the list holds, and that project inside
        before_pt, before_seg = set(), set()
        for rank, k in enumerate(ov):
            mine_pt = {lm for lm in st["kf_pt"][k] if lm >= 0} - before_pt
            mine_seg = {lm for lm in st["kf_seg"][k] if lm >= 0} - before_seg
            n = sum(_in_frame(T, st["pt_pos"][lm]) for lm in mine_pt)
            n += sum(_in_frame(T, st["seg_spos"][lm], Cc.SEG_CELL) and _in_frame(T, st["seg_epos"][lm], Cc.SEG_CELL) for lm in mine_seg)
            assert r["kf_count"][rank] == n
            before_pt |= mine_pt; before_seg |= mine_seg


@pytest.mark.parametrize("name", sorted(Cc.ALL))
def test_output_order_in_every_cell_is_a_stable_sort_of_the_cell(name):
    case = Cc.ALL[name]()
    for st, T, ov, r in zip(case["streams"], case["T"], case["overlap"], Cc.restate(case)):
        for kind, typ, cell_of in (("pt", st["pt_type"], lambda lm: [N.reproject(T, st["pt_pos"][lm], Cc.CAM_T, Cc.CELL, Cc.BOUNDARY)[1]]),
                                   ("seg", st["seg_type"], lambda lm: [N.reproject(T, st["seg_spos"][lm], Cc.CAM_T, Cc.SEG_CELL, Cc.BOUNDARY)[1],
                                                                       N.reproject(T, st["seg_epos"][lm], Cc.CAM_T, Cc.SEG_CELL, Cc.BOUNDARY)[1]])):
            filing, out = r["filing_" + kind], r[kind + "_lm"]
            assert sorted(filing) == sorted(out)
            cells = {c for lm in filing for c in cell_of(lm)}
            for c in cells:
                cell_list = [lm for lm in filing if c in cell_of(lm)]                  # the cell as the reference fills it
                cell_list.sort(key=lambda lm: -typ[lm])                                  # cell.sort(qualityComparator): stable
                assert [lm for lm in out if c in cell_of(lm)] == cell_list
            types = [typ[lm] for lm in out]
            assert types == sorted(types, reverse=True)


def test_ctypes_mirrors_have_the_c_layouts(tmp_path):
    """the new structs of include/plsvo_hip.h against their ctypes mirrors, size and every offset (as tests/test_abi_cpu.py does for the others)"""
    import ctypes as C
    import os
    import subprocess
    A = Cc.abi
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plsvo_hip.h")
    structs = {"plsvo_cand_map": A.CandMap, "plsvo_cand_params": A.CandParams, "plsvo_cand_frame": A.CandFrame, "plsvo_cand_out": A.CandOut,
               "plsvo_cand_match_out": A.CandMatchOut, "plsvo_cand_dev": A.CandDev}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append(f'printf("K %d %d\\n", PLSVO_K_CANDIDATES, PLSVO_K_COUNT);')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in out.strip().splitlines()}
    for cname, ct in structs.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(v) for v in got["K"]] == [A.K_CANDIDATES, A.K_COUNT]
    assert (A.LM_DELETED, A.LM_CANDIDATE, A.LM_UNKNOWN, A.LM_GOOD) == (N.TYPE_DELETED, N.TYPE_CANDIDATE, N.TYPE_UNKNOWN, N.TYPE_GOOD)
