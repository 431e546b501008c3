"""The matcher's affine warp (pl-svo_amd/csrc/match_device.hpp::warp_affine_lds) on all three of its paths, bit for bit.

The warp builds the 10 x 10 reference patch in five groups of two rows; a group is STAGED (its source box fits the LDS window: aligned
dword loads, v_alignbyte, byte taps from LDS), LARGE (taps read from the image) or BORDER (per-pixel test, zero fill).  The inputs of
tests/test_match_direct.py only ever reach the first, and see the patch only through the alignment's result.  Here:
  * plsvo_match_warp_patches -- the production kernel instantiated to stop after the warp -- hands out A, the search level, the patch
    and the mask of staged groups;
  * tests/match_warp_cases.py makes inputs that reach every path (zoom-outs, rolls, candidates at the image border);
  * CPU: the oracle's A and patch against the NumPy restatement of tests/test_match_direct.py, and the CONDITIONS on the inputs (how
    many groups take which path, at which box sizes and alignments) -- so that the inputs cannot drift back into the all-staged regime;
  * GPU (and the host emulation build, tests/test_emu_parity.py): A, search level, patch == the oracle's, the mask == the documented
    rule restated in NumPy, match_direct == the oracle end to end, edge cases, and one launch of 1280 candidates == the per-case ones."""
import numpy as np
import pytest

import match_warp_cases as mc
import test_match_direct as tm

ALL = list(range(mc.N_CASES))
N3 = len(mc.CASES)        # the cases with n_pyr_levels = 3


# ---- CPU: the oracle's side against the NumPy restatement --------------------------------------------------------------

def test_oracle_warp_matrix_matches_the_numpy_restatement(P, ob):
    """getWarpMatrixAffine: NumPy's products are ordered differently (tests/test_match_direct.py), so not bit for bit: every entry within
    1e-12 of the matrix's largest entry (A is a difference of pixel coordinates of up to a few thousand, 1 ulp = 4.5e-13 there, over 5;
    relative to the matrix, not entry by entry: without a roll the off-diagonal entries cancel to zero or next to it)"""
    npr = tm.npr
    n_checked = 0
    for k in ALL:
        c = mc.case(P, ob, k)
        d, ow = c["d"], c["oracle_warp"]
        T_ref, T_cur = d["frame_T"][0], d["frame_T"][1]
        q = np.array([-T_ref[0], -T_ref[1], -T_ref[2], T_ref[3]])
        T_ref_inv = np.concatenate([q, npr.q_rot(q, -T_ref[4:])])
        T_cur_ref = npr.se3_mul(T_cur, T_ref_inv)
        for i in np.flatnonzero(ow["search_level"] >= 0):
            depth = np.linalg.norm(T_ref_inv[4:] - d["pos"][i])
            A = tm._np_warp_matrix(d["cam"], d["ref_px"][i], d["ref_f"][i], depth, T_cur_ref, int(d["ref_level"][i])).reshape(4)
            err = np.abs(A - ow["A"][i]).max() / np.abs(A).max()
            assert err <= 1e-12, (k, i, err, A, ow["A"][i])
            n_checked += 1
    assert n_checked > 0.95 * 128 * mc.N_CASES


@pytest.mark.parametrize("k", ALL)
def test_oracle_patch_is_the_numpy_warp_of_its_own_matrix(P, ob, k):
    """after A everything is float32 and deterministic: _np_warp_affine fed the ORACLE's A gives the oracle's patch on every byte of
    every warped candidate; a candidate that is not warped reports a zero patch and a zero A / search level -1 when rejected"""
    c = mc.case(P, ob, k)
    d, ow = c["d"], c["oracle_warp"]
    assert ow["warped"].sum() >= 120
    for i in range(128):
        if not ow["warped"][i]:
            assert not ow["patch"][i].any() and ow["search_level"][i] == -1 and not ow["A"][i].any()      # (the cases hold no NaN inverse)
            continue
        lv, sl = int(d["ref_level"][i]), int(ow["search_level"][i])
        pb = tm._np_warp_affine(ow["A"][i].reshape(2, 2), c["frames"][0][lv], d["ref_px"][i], lv, sl)
        assert np.array_equal(pb, ow["patch"][i]), (k, i, np.argwhere(pb != ow["patch"][i]))
    # the oracle's two entry points share the code up to the warp
    assert np.array_equal(ow["search_level"], c["oracle_match"]["search_level"])


def test_zero_fill_restatement_agrees_with_the_oracle_patches(P, ob):
    """np_zero_filled (used by the conditions below) marks exactly pixels the oracle left at 0 (the images are >= 16 - noise everywhere)"""
    n = 0
    for k in ALL:
        c = mc.case(P, ob, k)
        d, ow = c["d"], c["oracle_warp"]
        zf = mc.np_zero_filled(ow["A"], mc.W, mc.H, d["ref_px"], d["ref_level"], ow["search_level"])
        assert not ow["patch"][zf].any()
        assert c["frames"][0][0].min() > 0 and np.array_equal(ow["patch"][ow["warped"] == 1] == 0, zf[ow["warped"] == 1]), k
        n += zf.any(axis=(1, 2)).sum()
    assert n >= 30


def test_inputs_reach_every_path_of_the_warp(P, ob):
    """CONDITIONS on the inputs, from np_staging_rule on the oracle's A alone, over the whole case set.  Not measurements: whoever
    changes the generator or the cases must keep every path, both sides of both box limits, every alignment of the staged loads and the
    window at the level's last row and last columns populated.  (In brackets: what the cases gave when they were written.)"""
    S, L, B = mc.STAGED, mc.LARGE, mc.BORDER
    t = dict(staged=0, large=0, border=0, mixed=0, zero_filled=0, w19=0, w20=0, h5=0, h6=0, last_row=0, last_cols=0)
    res_c, res_o, pairs = np.zeros(4, int), np.zeros(4, int), {}
    for k in ALL:
        c = mc.case(P, ob, k)
        r, d, ow = c["rule"], c["d"], c["oracle_warp"]
        cls = r["cls"]
        st, ins = cls == S, (cls == S) | (cls == L)
        t["staged"] += st.sum()
        t["large"] += (cls == L).sum()
        t["border"] += (cls == B).sum()
        t["mixed"] += sum(len(set(row[row >= 0])) >= 2 for row in cls)
        t["zero_filled"] += mc.np_zero_filled(ow["A"], mc.W, mc.H, d["ref_px"], d["ref_level"], ow["search_level"]).any(axis=(1, 2)).sum()
        wdt, hgt = r["cmax"] - r["cbase"], r["rmax"] - r["rmin"]
        t["w19"] += (ins & (wdt == 19)).sum()
        t["w20"] += (ins & (wdt == 20)).sum()
        t["h5"] += (ins & (hgt == 5)).sum()
        t["h6"] += (ins & (hgt == 6)).sum()
        for q in range(4):
            res_c[q] += (st & ((r["cmin"] & 3) == q)).sum()                                          # where the window starts in its first dword
            res_o[q] += (st & (((r["rmin"] * r["cols"][:, None] + r["cbase"]) & 3) == q)).sum()       # the v_alignbyte shift of its first row
        t["last_row"] += (st & (r["rmax"] == r["rows"][:, None] - 1)).sum()
        t["last_cols"] += (st & (r["cmax"] >= r["cols"][:, None] - 2)).sum()
        for lv, sl in zip(d["ref_level"], ow["search_level"]):
            pairs[(int(lv), int(sl))] = pairs.get((int(lv), int(sl)), 0) + 1
        # a rule that disagrees with the oracle about who is warped would make the counts meaningless
        assert np.array_equal(cls[:, 0] != mc.NONE, ow["warped"] == 1), k
    print(t, res_c, res_o, sorted(pairs.items()))
    assert t["staged"] >= 1000, t       # (5430)
    assert t["large"] >= 500, t         # (2573)
    assert t["border"] >= 100, t        # (257)
    assert t["mixed"] >= 30, t          # (138) candidates whose groups take at least two different paths
    assert t["zero_filled"] >= 30, t    # (120) candidates with at least one zero-filled pixel
    assert t["w19"] >= 20, t            # (186) box width cmax - cbase exactly at the limit ...
    assert t["w20"] >= 20, t            # (91)  ... and one beyond
    assert t["h5"] >= 50, t             # (412) box height rmax - rmin exactly at the limit ...
    assert t["h6"] >= 50, t             # (377) ... and one beyond
    assert res_c.min() >= 100, res_c    # (1222)
    assert res_o.min() >= 100, res_o    # (717)
    assert t["last_row"] >= 5, t        # (9)   staged groups whose last row is the level's last row (the -0.12 / 0.4 case provides them)
    assert t["last_cols"] >= 20, t      # (137) staged groups whose box reaches the level's last two columns
    # every (reference level, search level) pair the cases can produce.  det(A) ~ 4^level * (depth ratio)^2 and a search level is taken
    # per factor 4 above 3, so search level = level + {-1, 0, +1} for the zooms of CASES, capped at 2; with four levels the cap is 3 and
    # the zoom of 0.88 takes level 0 to search level 2 or 3.  Level 3 is one candidate in twenty and those within 6 of its border are
    # rejected (-1).
    expected = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (0, 2), (0, 3), (1, 3), (2, 3), (3, 3), (3, -1)]
    for pr in expected:
        assert pairs.get(pr, 0) >= 10, (pr, sorted(pairs.items()))


# ---- GPU (and the host emulation build): bit for bit -----------------------------------------------------------------------

def _same_warp(rd, ro, what):
    assert np.array_equal(rd["search_level"], ro["search_level"]), what
    assert np.array_equal(rd["warped"], ro["warped"]), what
    assert rd["A"].tobytes() == ro["A"].tobytes(), (what, np.argwhere(rd["A"] != ro["A"])[:5])      # (bytes: signed zeros and NaNs count)
    bad = np.argwhere(rd["patch"] != ro["patch"])
    assert bad.size == 0, (what, len(bad), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL)
def test_hip_warp_patches_are_bit_exact(P, ob, gpu_ctx, k):
    c = mc.case(P, ob, k)
    mc.load_frames(gpu_ctx, c["frames"])
    _same_warp(gpu_ctx.match_warp_patches(c["job"]), c["oracle_warp"], k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL)
def test_hip_staged_groups_follow_the_documented_rule(P, ob, gpu_ctx, k):
    """which groups read the LDS window: exactly the rule's (a kernel that quietly stopped staging would stay bit-exact and lose its speed)"""
    c = mc.case(P, ob, k)
    mc.load_frames(gpu_ctx, c["frames"])
    rd = gpu_ctx.match_warp_patches(c["job"], fields=("staged",))
    bad = np.flatnonzero(rd["staged"] != c["rule"]["mask"])
    assert bad.size == 0, (k, bad[:8], rd["staged"][bad[:8]], c["rule"]["mask"][bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL)
def test_hip_match_direct_is_bit_exact_on_every_warp_path(P, ob, gpu_ctx, k):
    c = mc.case(P, ob, k)
    mc.load_frames(gpu_ctx, c["frames"])
    tm._assert_same(gpu_ctx.match_direct(c["job"]), c["oracle_match"])


@pytest.mark.gpu
def test_hip_warp_patches_edge_cases(P, ob, gpu_ctx):
    c = mc.case(P, ob, 5)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c["d"].items()}
    d["ref_px"][40] = [5.0, 100.0]                                    # rejected by the border check
    d["ref_level"][41] = 3
    d["ref_px"][41] = [40.0, 100.0]                                   # 40 / 8 = 5 < 6: rejected
    d["pos"][42] = P.synth.se3_inv(d["frame_T"][0])[4:]               # the landmark AT the reference camera centre: depth 0, A = 0, NaN inverse
    for frames in (c["frames"], [ob.build_pyramid(np.full((mc.H, mc.W), 77, np.uint8), 4)] * 2):    # the textured pair, then a flat image
        mc.load_frames(gpu_ctx, frames)
        job = P.match_job_from_batch(d)
        ro, rd = ob.match_warp_patches(job, frames), gpu_ctx.match_warp_patches(job)
        _same_warp(rd, ro, "edge")
        rule = mc.np_staging_rule(ro["A"], mc.W, mc.H, d["ref_px"], d["ref_level"], ro["search_level"])
        assert np.array_equal(rd["staged"], rule["mask"])
        for i in (40, 41):
            assert rd["search_level"][i] == -1 and rd["warped"][i] == 0 and rd["staged"][i] == 0 and not rd["patch"][i].any() and not rd["A"][i].any()
        assert ro["warped"][42] == 0 and rd["warped"][42] == 0 and rd["staged"][42] == 0 and not rd["patch"][42].any() and rd["search_level"][42] == 0
        assert rd["warped"].sum() == 125
        tm._assert_same(gpu_ctx.match_direct(job), ob.match_direct(job, frames))
    # NULL out pointers: each field alone equals its column of the full call; no field at all is a valid call
    for f in ("A", "search_level", "warped", "patch", "staged"):
        one = gpu_ctx.match_warp_patches(job, fields=(f,))
        assert list(one) == [f] and one[f].tobytes() == rd[f].tobytes(), f
    assert gpu_ctx.match_warp_patches(job, fields=()) == {}
    # empty batch: nothing is written
    e = dict(d)
    for k in ("cur_frame", "ref_frame", "ref_px", "ref_f", "ref_level", "ref_type", "ref_grad", "pos", "px_cur"):
        e[k] = d[k][:0]
    assert gpu_ctx.match_warp_patches(P.match_job_from_batch(e))["warped"].size == 0
    # bad arguments, as plsvo_match_direct rejects them
    for key, i, val in (("ref_frame", 0, 7), ("cur_frame", 3, -1), ("ref_level", 0, 9), ("ref_type", 1, 5)):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        b[key][i] = val
        with pytest.raises(P.capi.PlsvoError):
            gpu_ctx.match_warp_patches(P.match_job_from_batch(b))
    with pytest.raises(P.capi.PlsvoError):
        gpu_ctx.match_warp_patches(P.match_job_from_batch(d, 5))                  # more levels than the configured pyramid has
    b = dict(d, frame_slot=np.array([0, 9], np.int32))
    with pytest.raises(P.capi.PlsvoError):
        gpu_ctx.match_warp_patches(P.match_job_from_batch(b))
    import ctypes as C
    assert gpu_ctx.L.plsvo_match_warp_patches(gpu_ctx.h, C.byref(job.c), None) != 0 and gpu_ctx.L.plsvo_match_warp_patches(gpu_ctx.h, None, None) != 0


@pytest.mark.gpu
def test_hip_warp_patches_in_one_launch_equal_the_per_case_results(P, ob, gpu_ctx):
    """the ten three-level cases as ONE launch of 1280 candidates (20 workgroups, 20 pyramid slots): what a lane computes must not depend
    on what its neighbours, or the workgroup before it, left in the shared window"""
    cases = [mc.case(P, ob, k) for k in range(N3)]
    job, slots = mc.concat(P, cases)
    assert job.n == 1280
    mc.load_frames(gpu_ctx, slots)
    rd = gpu_ctx.match_warp_patches(job)
    rm = gpu_ctx.match_direct(job)
    for k, c in enumerate(cases):
        s = slice(128 * k, 128 * (k + 1))
        _same_warp({f: v[s] for f, v in rd.items()}, c["oracle_warp"], k)
        assert np.array_equal(rd["staged"][s], c["rule"]["mask"]), k
        tm._assert_same({f: v[s] for f, v in rm.items()}, c["oracle_match"])
