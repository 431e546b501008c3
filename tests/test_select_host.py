"""The cell selection of the map candidates without a device: the cases of tests/select_cases.py hold every path the kernel has (asserted
as conditions on the INPUTS and on what the restatement does with them, so a case cannot silently miss what it is there for), and the
restatement tests/np_select.py is checked against an independent statement of its invariants."""
import copy

import pytest

import np_candidates as N
import select_cases as Sc

D, C_, U, G = Sc.D, Sc.C_, Sc.U, Sc.G


def run(s, params="default", **kw):
    return Sc.restate(s, Sc.PARAMS[params], **kw)


def test_grids_end_in_a_partial_column_and_row():
    assert Sc.CAM_T[4] % Sc.CELL and Sc.CAM_T[5] % Sc.CELL and Sc.CAM_T[4] % Sc.SEG_CELL and Sc.CAM_T[5] % Sc.SEG_CELL
    assert (Sc.N_CELLS, Sc.SEG_N_CELLS) == (11 * 9, 14 * 10) and (Sc.COLS, Sc.SEG_COLS) == (11, 14)


def test_cell_contents_reach_every_path():
    s = Sc.cells_stream()
    r, m, sel, st = run(s)
    nm = s["names"]
    per_cell = {}
    for lm, cell in zip(r["pt_lm"], r["pt_cell"]):
        per_cell.setdefault(cell, []).append(lm)
    assert len(per_cell) < Sc.N_CELLS                                  # empty cells
    assert per_cell[r["pt_cell"][r["pt_lm"].index(nm["single"])]] == [nm["single"]]
    assert s["found_pt"][nm["first_fails"]] == 0 and s["found_pt"][nm["second_wins"]] == 1
    assert nm["second_wins"] in sel["pt_lm"] and nm["first_fails"] in sel["tried_pt"] and nm["third_untried"] not in sel["tried_pt"]
    four = nm["four_types"]
    assert len({r["pt_cell"][r["pt_lm"].index(lm)] for lm in four}) == 1
    filed_types = [s["st"]["pt_type"][lm] for lm in r["filing_pt"] if lm in four]
    assert sorted(set(filed_types)) == [D, C_, U, G] and filed_types != sorted(filed_types, reverse=True)
    # GOOD, GOOD fail; the UNKNOWN one wins; the CANDIDATEs and the DELETED one are never reached
    assert [lm for lm in sel["tried_pt"] if lm in four] == [four[2], four[4], four[3]]
    crowd = nm["crowd"]
    assert len(crowd) > 64 and len({r["pt_cell"][r["pt_lm"].index(lm)] for lm in crowd}) == 1
    assert [lm for lm in sel["tried_pt"] if lm in crowd][-1] == crowd[65] and sum(lm in crowd for lm in sel["tried_pt"]) == 70
    assert sel["n_matches"] == 4 and sel["n_trials"] == 1 + 2 + 3 + 70


def test_stop_rule_cases():
    s = Sc.stop_stream()
    winners = [12, 14, 16, 36, 60, 75]
    r, m, sel, st = run(s, "untried")
    cell_of_lm = dict(zip(r["pt_lm"], r["pt_cell"]))
    assert [cell_of_lm[lm] for lm in sel["pt_lm"]] == winners[:4] and sel["n_matches"] == 4 == Sc.PARAMS["untried"]["max_fts"] + 1
    untried = [lm for lm in r["pt_lm"] if cell_of_lm[lm] in (60, 75)]
    assert any(s["found_pt"][lm] for lm in untried) and not set(untried) & set(sel["tried_pt"])
    assert all(st["pt_nfail"][lm] == 0 and st["pt_nsucc"][lm] == 0 for lm in untried)
    assert sel["n_ls_matches"] == 2 and len(sel["visited_seg_cells"]) == 49
    # the stop on the LAST cell of the visit order: every cell was visited, and the count exceeds max_fts only there
    r, m, sel, st = run(s, "last_cell")
    p = Sc.PARAMS["last_cell"]
    assert len(sel["visited_cells"]) == Sc.N_CELLS and sel["n_matches"] == p["max_fts"] + 1 and cell_of_lm[sel["pt_lm"][-1]] == p["cell_order"][-1] == 36
    assert len(sel["visited_seg_cells"]) == Sc.SEG_N_CELLS and sel["n_ls_matches"] == p["max_fts_segs"] + 1
    # max_fts = 0: the first match ends the visit
    r, m, sel, st = run(s, "zero")
    assert sel["n_matches"] == 1 and sel["visited_cells"] == list(range(13)) and sel["n_ls_matches"] == 1 and sel["n_trials"] == 2 + 1


def test_segment_cases():
    s = Sc.segments_stream()
    nm = s["names"]
    r, m, sel, st = run(s)
    cells = dict(zip(r["seg_lm"], r["seg_cell"]))
    assert cells[nm["one_cell"]][0] == cells[nm["one_cell"]][1] == cells[nm["one_cell_later"]][0]
    assert sel["seg_lm"].count(nm["one_cell"]) == 1 and nm["one_cell_later"] not in sel["tried_seg"]
    assert cells[nm["wins_both"]][0] != cells[nm["wins_both"]][1] and sel["seg_lm"].count(nm["wins_both"]) == 2
    # promotion decides the second cell: Q was filed first, P overtakes it
    assert r["filing_seg"].index(nm["Q"]) < r["filing_seg"].index(nm["P"]) and s["st"]["seg_type"][nm["P"]] == s["st"]["seg_type"][nm["Q"]] == U
    assert cells[nm["P"]][1] == cells[nm["Q"]][0] and cells[nm["P"]][0] < cells[nm["P"]][1]
    assert sel["seg_lm"].count(nm["P"]) == 2 and nm["Q"] not in sel["tried_seg"] and st["seg_type"][nm["P"]] == G and st["seg_nsucc"][nm["P"]] == 12
    assert sel["seg_event"][nm["P"]] == 1
    _, _, flat, st_flat = run(s, promote=False)
    assert flat["seg_lm"].count(nm["P"]) == 1 and nm["Q"] in flat["seg_lm"] and flat["seg_lm"] != sel["seg_lm"]
    # deleted by its first failure, met again: one increment, two trials
    d = nm["deleted_then_met"]
    assert sel["tried_seg"].count(d) == 2 and st["seg_nfail"][d] == 16 and st["seg_type"][d] == D and sel["seg_event"][d] == 2
    assert all(d not in fts for fts in st["kf_seg"]) and any(d in fts for fts in s["st"]["kf_seg"])
    assert sel["tried_seg"].index(nm["after_deleted"]) < len(sel["tried_seg"]) - 1 - sel["tried_seg"][::-1].index(d)     # the deleted one sorts last
    assert r["seg_has_view"][r["seg_lm"].index(nm["seg_no_view"])] == 0 and st["seg_nfail"][nm["seg_no_view"]] == 2
    assert sel["tried_seg"].count(nm["seg_pre_deleted"]) == 2 and st["seg_nfail"][nm["seg_pre_deleted"]] == 0


@pytest.mark.parametrize("kind", ["pt", "seg"])
def test_counter_thresholds(kind):
    s = Sc.thresholds_pt_stream() if kind == "pt" else Sc.thresholds_seg_stream()
    nm = s["names"]
    r, m, sel, st = run(s)
    k = 1 if kind == "pt" else 2                                       # a segment with both ends in one cell fails twice
    typ, nf, ns, ev = st[kind + "_type"], st[kind + "_nfail"], st[kind + "_nsucc"], sel[kind + "_event"]
    assert (typ[nm["succ9"]], ns[nm["succ9"]], ev[nm["succ9"]]) == (U, 10, 0) and (typ[nm["succ10"]], ns[nm["succ10"]], ev[nm["succ10"]]) == (G, 11, 1)
    if kind == "pt":
        assert (typ[nm["fail14"]], nf[nm["fail14"]], ev[nm["fail14"]]) == (U, 15, 0)
    else:
        assert (typ[nm["fail14"]], nf[nm["fail14"]], ev[nm["fail14"]]) == (D, 16, 2)          # 15, then 16
    assert (typ[nm["fail15"]], nf[nm["fail15"]], ev[nm["fail15"]]) == (D, 16, 2)
    assert all(nm["fail15"] not in fts for fts in st["kf_" + kind])
    if kind == "pt":
        assert (typ[nm["cand29"]], nf[nm["cand29"]]) == (C_, 30) and nm["cand29"] in st["pt_cand"]
    else:
        assert (typ[nm["cand29"]], nf[nm["cand29"]]) == (D, 31) and nm["cand29"] not in st["seg_cand"]
    assert (typ[nm["cand30"]], nf[nm["cand30"]], ev[nm["cand30"]]) == (D, 31, 2) and nm["cand30"] not in st[kind + "_cand"]
    assert typ[nm["cand_unlisted30"]] == C_ and nf[nm["cand_unlisted30"]] == 30 + k and ev[nm["cand_unlisted30"]] == 0
    assert typ[nm["good_fail40"]] == G and nf[nm["good_fail40"]] == 40 + k


def test_segment_thresholds_with_a_single_increment():
    """ends in two cells, the second behind the stop: one failure each, so one below a threshold stays alive AT it"""
    s = Sc.thresholds_seg_two_cells_stream()
    nm = s["names"]
    r, m, sel, st = run(s, "untried")
    cells = dict(zip(r["seg_lm"], r["seg_cell"]))
    assert all(cells[nm[n]][0] in sel["visited_seg_cells"] and cells[nm[n]][1] not in sel["visited_seg_cells"] for n in ("two14", "two15", "two29", "two30"))
    assert all(sel["tried_seg"].count(nm[n]) == 1 for n in ("two14", "two15", "two29", "two30")) and sel["n_ls_matches"] == 2
    typ, nf, ev = st["seg_type"], st["seg_nfail"], sel["seg_event"]
    assert (typ[nm["two14"]], nf[nm["two14"]], ev[nm["two14"]]) == (U, 15, 0) and any(nm["two14"] in fts for fts in st["kf_seg"])
    assert (typ[nm["two15"]], nf[nm["two15"]], ev[nm["two15"]]) == (D, 16, 2) and all(nm["two15"] not in fts for fts in st["kf_seg"])
    assert (typ[nm["two29"]], nf[nm["two29"]], ev[nm["two29"]]) == (C_, 30, 0) and nm["two29"] in st["seg_cand"]
    assert (typ[nm["two30"]], nf[nm["two30"]], ev[nm["two30"]]) == (D, 31, 2) and nm["two30"] not in st["seg_cand"]
    # with every cell visited the second end counts too
    _, _, _, st2 = run(s, "default")
    assert (st2["seg_type"][nm["two14"]], st2["seg_nfail"][nm["two14"]]) == (D, 16) and (st2["seg_type"][nm["two29"]], st2["seg_nfail"][nm["two29"]]) == (D, 31)


def test_other_paths():
    s = Sc.other_stream()
    nm = s["names"]
    r, m, sel, st = run(s)
    assert s["st"]["pt_type"][nm["pre_deleted"]] == D and nm["pre_deleted"] in sel["tried_pt"] and st["pt_nfail"][nm["pre_deleted"]] == 0
    i = r["pt_lm"].index(nm["no_view"])
    assert r["pt_has_view"][i] == 0 and m["found"][i] == 1 and st["pt_nfail"][nm["no_view"]] == 1 and nm["no_view"] not in sel["pt_lm"]
    k = sel["pt_lm"].index(nm["edgelet"])
    assert sel["pt_type"][k] == 1 and abs(sel["pt_grad"][k][0] ** 2 + sel["pt_grad"][k][1] ** 2 - 1.0) < 1e-12 and sel["pt_grad"][k] != [1.0, 0.0]
    assert nm["edgelet_lost"] not in sel["pt_lm"] and all(t == 0 and g == [1.0, 0.0] for lm, t, g in zip(sel["pt_lm"], sel["pt_type"], sel["pt_grad"]) if lm != nm["edgelet"])
    for kind, pre in (("pt", "cand_fail"), ("seg", "seg_cand_fail")):
        a, b, c = nm[pre + "27"], nm[pre + "28"], nm[pre + "31"]
        assert r[kind + "_cand_failed"][:6:1].count(1) == 3
        assert (st[kind + "_nfail"][a], st[kind + "_type"][a]) == (30, C_) and a in st[kind + "_cand"]
        assert (st[kind + "_nfail"][b], st[kind + "_type"][b]) == (31, D) and b not in st[kind + "_cand"]
        assert (st[kind + "_nfail"][c], st[kind + "_type"][c]) == (34, D) and c not in st[kind + "_cand"]
        assert sel[kind + "_event"][b] == 2 and sel[kind + "_event"][a] == 0
    assert st["pt_cand"] == [nm["cand_fail27"], nm["cand_ok"]] and nm["cand_ok"] in sel["pt_lm"] and nm["seg_cand_ok"] in sel["seg_lm"]
    e = Sc.empty_stream()
    r, m, sel, st = run(e)
    assert (sel["n_matches"], sel["n_ls_matches"], sel["n_trials"]) == (0, 0, 0) and len(sel["visited_cells"]) == Sc.N_CELLS


def test_segment_level_is_the_end_points():
    s = Sc.stop_stream()
    r, m, sel, st = run(s)
    n_pt, n_seg = r["n_filed_pt"], r["n_filed_seg"]
    differ = 0
    for lm, lv in zip(sel["seg_lm"], sel["seg_level"]):
        i = r["seg_lm"].index(lm)
        assert lv == m["search_level"][n_pt + n_seg + i]
        differ += int(m["search_level"][n_pt + i] != lv)
    assert differ > 0


@pytest.mark.parametrize("params", sorted(Sc.PARAMS))
def test_the_restatement_keeps_its_invariants(params):
    """an independent statement of what the loops must leave behind, on every stream of the batch"""
    p = Sc.PARAMS[params]
    for k, s in enumerate(Sc.batch()):
        before = copy.deepcopy(s["st"])
        r, m, sel, st = run(s, params)
        n_pt, n_seg = r["n_filed_pt"], r["n_filed_seg"]
        pt_cell = dict(zip(r["pt_lm"], r["pt_cell"]))
        assert len(set(r["pt_lm"])) == n_pt and len(set(r["seg_lm"])) == n_seg                     # the preconditions hold
        # at most one point feature per cell, at most one segment feature per visited cell
        assert len({pt_cell[lm] for lm in sel["pt_lm"]}) == len(sel["pt_lm"]) == sel["n_matches"] <= p["max_fts"] + 1
        assert sel["n_ls_matches"] == len(sel["seg_lm"]) <= min(p["max_fts_segs"] + 1, len(sel["visited_seg_cells"]))
        # every feature's landmark was found, seen, and alive
        for lm in sel["pt_lm"]:
            i = r["pt_lm"].index(lm)
            assert m["found"][i] and r["pt_has_view"][i] and before["pt_type"][lm] != D
        for lm in sel["seg_lm"]:
            i = r["seg_lm"].index(lm)
            assert m["found"][n_pt + i] and m["found"][n_pt + n_seg + i] and r["seg_has_view"][i] and before["seg_type"][lm] != D
        # no trial in a cell that was not visited; a point is tried at most once, a segment at most twice
        assert {pt_cell[lm] for lm in sel["tried_pt"]} <= set(sel["visited_cells"]) and len(set(sel["tried_pt"])) == len(sel["tried_pt"])
        seg_cells = dict(zip(r["seg_lm"], r["seg_cell"]))
        assert all(set(seg_cells[lm]) & set(sel["visited_seg_cells"]) for lm in sel["tried_seg"]) and all(sel["tried_seg"].count(lm) <= 2 for lm in sel["tried_seg"])
        assert sel["n_trials"] == len(sel["tried_pt"]) + len(sel["tried_seg"])
        # the counters move by the number of trials (three per failed projection of a listed candidate), up to the deletion
        for kind, tried in (("pt", sel["tried_pt"]), ("seg", sel["tried_seg"])):
            failed = {lm for lm, f in zip(before[kind + "_cand"], r[kind + "_cand_failed"]) if f}
            for lm in range(len(before[kind + "_type"])):
                moved = (st[kind + "_nfail"][lm] - before[kind + "_nfail"][lm]) + (st[kind + "_nsucc"][lm] - before[kind + "_nsucc"][lm])
                t = tried.count(lm)
                if lm in failed:
                    assert moved == 3 and t == 0
                elif before[kind + "_type"][lm] == D:
                    assert moved == 0
                elif st[kind + "_type"][lm] == D:
                    assert 1 <= moved <= t
                else:
                    assert moved == t
                assert (st[kind + "_type"][lm] != before[kind + "_type"][lm]) == (sel[kind + "_event"][lm] != 0)
            # a deleted landmark is in no keyframe list and no candidate list that the reference would have cleaned
            for lm in range(len(before[kind + "_type"])):
                if sel[kind + "_event"][lm] == 2 and before[kind + "_type"][lm] == U:
                    assert all(lm not in fts for fts in st["kf_" + kind])
                if sel[kind + "_event"][lm] == 2 and before[kind + "_type"][lm] == C_:
                    assert lm not in st[kind + "_cand"]
            assert [lm for lm in before[kind + "_cand"] if lm in st[kind + "_cand"]] == st[kind + "_cand"]       # a stable compaction


def test_the_batch_holds_promotions_deletions_and_erasures_in_its_random_streams():
    seen = set()
    for s in (Sc.batch()[1], Sc.batch()[6]):
        r, m, sel, st = run(s)
        for kind in ("pt", "seg"):
            seen |= {(kind, e) for e in sel[kind + "_event"] if e}
            if len(st[kind + "_cand"]) < len(s["st"][kind + "_cand"]):
                seen.add((kind, "erased"))
    assert {("pt", 1), ("pt", 2), ("seg", 1), ("seg", 2), ("pt", "erased")} <= seen, seen
