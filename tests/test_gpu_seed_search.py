"""The depth filter's epipolar search on the device (pl-svo_amd/csrc/seeds_kernels.hip: update_seeds_kernel with load_row8 / v_dot4
scoring, the out-of-line epipolar_search, align2d_lds, triangulation, tau and the posterior) against the oracle on the directed inputs of
tests/seed_search_cases.py -- every exit of the search, reference levels 0..3, search levels 0..3, image widths that are no multiple of
4 (the byte phase of a scored patch changes from row to row), ties, walks over the border -- which tests/test_seed_search.py pins to an
independent restatement on the CPU and whose reach it asserts.  Also: one launch of all cases against the per-case launches, and the
same seeds in other lanes (a permutation; the point / line boundary at the start, in the middle and at the end of a wave).
The resident kernel runs the same per-seed bodies; tests/test_gpu_seedlist.py ties it byte for byte to plsvo_update_seeds."""
import numpy as np
import pytest

import seed_search_cases as sc
from test_seed_search import assert_close_with_tight_rows, oracle_of

_gpu = {}


def _per_case(P, ob, ctx, k):
    """the device's answer for case k alone in slots 0, 1 (once per process)"""
    if k not in _gpu:
        c = sc.case(P, ob, k)
        sc.load_frames(ctx, c["frames"])
        _gpu[k] = ctx.update_seeds(c["job"])
    return _gpu[k]


def _same_bytes(got, want, rows_got, rows_want, prefix, what):
    for f in want:
        if f.startswith(prefix):
            a, b = got[f][rows_got], want[f][rows_want]
            assert a.tobytes() == b.tobytes(), (what, f, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(sc.N_CASES))
def test_hip_update_seeds_matches_the_oracle_on_every_search_path(P, ob, gpu_ctx, k):
    c = sc.case(P, ob, k)
    assert_close_with_tight_rows(P, _per_case(P, ob, gpu_ctx, k), c["oracle"])


@pytest.mark.gpu
@pytest.mark.parametrize("v", range(len(sc.VARIANTS)))
def test_hip_update_seeds_matches_the_oracle_with_other_settings(P, ob, gpu_ctx, v):
    """max_epi_search_steps = 5 (every longer walk is skipped) and the edgelet filter off, two cases each; align_max_iter = 3"""
    k, over = sc.VARIANTS[v]
    c = sc.case(P, ob, k)
    sc.load_frames(gpu_ctx, c["frames"])
    assert_close_with_tight_rows(P, gpu_ctx.update_seeds(sc.job_of(P, c, **over)), oracle_of(P, ob, k, over))


@pytest.mark.gpu
@pytest.mark.parametrize("n_pyr", [3, 4])
def test_hip_update_seeds_in_one_launch_equals_the_per_case_launches(P, ob, gpu_ctx, n_pyr):
    """all cases with the same settings as ONE job (their frames in slots 2j, 2j + 1; 16 cases: 1536 point and 256 line seeds, 28
    workgroups): every seed's outputs are the bytes of its per-case launch"""
    ks = [k for k in range(sc.N_CASES) if sc.CASES[k][4] == n_pyr]
    per = [_per_case(P, ob, gpu_ctx, k) for k in ks]
    job, slots = sc.concat(P, [sc.case(P, ob, k) for k in ks])
    sc.load_frames(gpu_ctx, slots)
    rd = gpu_ctx.update_seeds(job)
    for j, k in enumerate(ks):
        _same_bytes(rd, per[j], slice(sc.N_PTS * j, sc.N_PTS * (j + 1)), slice(None), "pt_", k)
        _same_bytes(rd, per[j], slice(sc.N_SEG * j, sc.N_SEG * (j + 1)), slice(None), "seg_", k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, sc.TIE_CASE])
def test_hip_update_seeds_does_not_depend_on_the_lane(P, ob, gpu_ctx, k):
    """a seed's outputs are the same bytes wherever it sits: in a fixed random permutation of the point and of the line seeds, and with
    only the first 1, 63, 64, 65 point seeds in front of the line seeds, so that the point / line boundary -- where the lanes of a wave
    part into update_point_seed and update_line_seed, and call the out-of-line epipolar_search at different times on their own LDS
    patch (s_patch + lane) -- falls at the start of a wave, in its middle and at its end"""
    c = sc.case(P, ob, k)
    base = _per_case(P, ob, gpu_ctx, k)
    sc.load_frames(gpu_ctx, c["frames"])
    rng = np.random.default_rng(77 + k)
    pp, ps = rng.permutation(sc.N_PTS), rng.permutation(sc.N_SEG)
    layouts = [(pp, ps)] + [(np.arange(n), np.arange(sc.N_SEG)) for n in (1, 63, 64, 65)] + [(np.arange(0), ps), (pp, np.arange(0))]
    for rows_pt, rows_seg in layouts:
        pt, seg = sc.select(c, rows_pt, rows_seg)
        job = P.abi.SeedsJob(c["st"].cam, c["frame_T"], np.array([0, 1]), pt if len(rows_pt) else None, seg if len(rows_seg) else None, **sc.options(c))
        rd = gpu_ctx.update_seeds(job)
        _same_bytes(rd, base, slice(None), rows_pt, "pt_", (k, len(rows_pt), len(rows_seg)))
        _same_bytes(rd, base, slice(None), rows_seg, "seg_", (k, len(rows_pt), len(rows_seg)))
