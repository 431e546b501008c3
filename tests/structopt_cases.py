"""Directed inputs for the structure optimiser (tests/test_structopt_paths.py on the CPU, tests/test_gpu_structopt_paths.py on the device).

  SOLVER_SYSTEMS   symmetric 3x3 systems A x = b, one per branch of the pivoted LDLT with Eigen 3.2's zero-pivot rule (oracle flavour 320,
                   the only one the device's 3x3 solve implements): pivot orders, ties, rank deficiency, the cutoff and tolerance
                   branches, NaN/Inf in every position
  geometry_*       landmarks with explicit or seeded observations that drive Point::optimize / LineSeg::optimize through every exit
  layouts          the same landmarks at the batch shapes where the kernel's indexing can go wrong

Which branch each input reaches is not claimed here: tests/test_structopt_paths.py::test_inputs_reach_every_path reads it off the records
of tests/np_structopt.py.  Nothing is read from anywhere at test time; every number is written out or comes from a seeded generator below."""
import math

import numpy as np

NAN, INF = float("nan"), float("inf")


def sym(a00, a10, a11, a20, a21, a22):
    return np.array([[a00, a10, a20], [a10, a11, a21], [a20, a21, a22]], dtype=np.float64)


def _solver_systems():
    S = []
    B = (1.0, 2.0, 3.0)
    # full rank, each of the six pivot orders: the diagonal holds 4, 2, 1 in every arrangement
    for name, dg in (("order012", (4, 2, 1)), ("order021", (4, 1, 2)), ("order102", (2, 4, 1)), ("order120", (1, 4, 2)), ("order201", (2, 1, 4)), ("order210", (1, 2, 4))):
        S.append((name, sym(dg[0], 0.3, dg[1], -0.2, 0.1, dg[2]), B))
    # exact ties (first maximum wins); the rank-2 variants return a ZERO in the component that was pivoted last, so the order shows in x
    S.append(("tie01", sym(2, 0.3, 2, -0.2, 0.1, 1), B))
    S.append(("tie01_negative", sym(2, 0.3, -2, -0.2, 0.1, 1), B))
    S.append(("tie12_step1", sym(4, 0.3, 2, -0.2, 0.1, 2), B))
    S.append(("tie012", sym(3, 0.3, 3, -0.2, 0.1, 3), B))
    S.append(("tie02", sym(2, 0.3, 1, -0.2, 0.1, 2), B))
    S.append(("tie01_rank2", sym(1, 1, 1, 0, 0, 0.5), (1, 1, 1)))
    S.append(("tie12_step1_rank2", sym(4, 0, 1, 0, 1, 1), (4, 1, 1)))
    S.append(("tie012_rank1", sym(1, 1, 1, 1, 1, 1), (1, 1, 1)))
    # rank 2 (v1 v1^T + v2 v2^T, v1 = (1,2,0), v2 = (0,1,1)), rank 1 ((1,2,3)(1,2,3)^T), rank 0
    S.append(("rank2", sym(1, 2, 5, 0, 1, 1), (3, 8, 2)))
    S.append(("rank2_b_outside_range", sym(1, 2, 5, 0, 1, 1), B))
    S.append(("rank1", sym(1, 2, 4, 3, 6, 9), (2, 4, 6)))
    S.append(("zero_matrix", sym(0, 0, 0, 0, 0, 0), B))
    S.append(("zero_matrix_zero_b", sym(0, 0, 0, 0, 0, 0), (0, 0, 0)))
    S.append(("negative_zeros", sym(-0.0, -0.0, -0.0, -0.0, -0.0, -0.0), (-0.0, 1.0, -0.0)))
    S.append(("zero_diagonal", sym(0, 1, 0, 2, 3, 0), B))            # cutoff 0 and |d0| = 0: column 0 stays unscaled
    # indefinite, negative definite
    S.append(("indefinite", sym(1, 2, -3, 0, 1, 0.5), B))
    S.append(("indefinite_big_offdiagonal", sym(0.5, 4, -0.25, -3, 2, 0.125), B))
    S.append(("negative_definite", sym(-4, -0.3, -2, 0.2, -0.1, -1), B))
    S.append(("negative_diagonals_order210", sym(-1, 0.3, -2, -0.2, 0.1, -4), B))
    # a dominant first diagonal, the other two below eps * max: the factorisation stops at step 1 and the substitution runs on the raw,
    # unscaled a21 (which the zeroed D entries then multiply by 0 -- unless it is not finite)
    S.append(("early_stop_step1", sym(1, 0.5, 1e-17, 0.25, 0.125, -5e-18), B))
    S.append(("early_stop_step1_dominant_last", sym(-5e-18, 0.125, 1e-17, 0.25, 0.5, 1), B))
    S.append(("early_stop_step1_inf_a21", sym(1, 0.5, 1e-17, 0.25, INF, -5e-18), B))
    S.append(("early_stop_step1_nan_a21", sym(1, 0.5, 1e-17, 0.25, NAN, -5e-18), B))
    S.append(("early_stop_step1_huge", sym(1e36, 3e17, 1e18, -2e17, 5e8, 2.5e17), (1e18, 2e9, 3e9)))
    # stored a22 below the cutoff while a11 is not: step 2 is skipped, D2 keeps the stored entry
    S.append(("skip_step2", sym(1, 0.5, 0.5, 0.25, 0.125, 1e-17), B))
    S.append(("skip_step2_swapped", sym(1, 0.25, 1e-17, 0.5, 0.125, 0.5), B))
    S.append(("skip_step2_exactly_at_cutoff_runs", sym(1, 0.5, 0.5, 0.25, 0.125, 2.220446049250313e-16), B))
    # |d1| at or below the cutoff after the elimination: column 1 stays unscaled and multiplies a non-zero y1 in the forward substitution
    S.append(("d1_cancels", sym(1, 1, 1, 0.5, 0.25, 0.5), B))
    S.append(("d1_below_cutoff", sym(1, 1, 1 + 2.220446049250313e-16, 0.5, 0.25, 0.5), B))
    # a non-zero D entry zeroed by the relative tolerance max|D| * eps
    S.append(("d2_zeroed_by_relative_tolerance", sym(1, 0.5, 0.25 + 1e-16, 0.25, 0.125, 0.5), B))
    S.append(("d_zeroed_diagonal", sym(1, 0, 1e-16, 0, 0, 3e-16), B))
    # tiny systems: max|D| * eps falls below 1/DBL_MAX and the tolerance is the floor
    S.append(("tolerance_floor", 1e-300 * sym(4, 0.3, 2, -0.2, 0.1, 1), (1e-300, 2e-300, 3e-300)))
    S.append(("tolerance_floor_zeroes_subnormal_d", sym(1e-300, 0, 2e-300, 0, 0, 1e-310), (1e-300, 2e-300, 3e-310)))
    S.append(("tolerance_floor_keeps_small_d", sym(1e-300, 0, 2e-300, 0, 0, 1e-308), (1e-300, 2e-300, 3e-308)))
    # huge systems whose products overflow
    S.append(("overflow_products", 1e300 * sym(1, 1e5, 0.5, 2e4, 3, 0.25), (1e300, 2e300, 3e300)))
    S.append(("overflow_b", 1e300 * sym(4, 0.3, 2, -0.2, 0.1, 1), (1e308, -1e308, 1e308)))
    # one NaN at a time: the six lower-triangle positions, the three right-hand sides
    base = sym(4, 0.3, 2, -0.2, 0.1, 1)
    for name, (i, j) in (("a00", (0, 0)), ("a10", (1, 0)), ("a11", (1, 1)), ("a20", (2, 0)), ("a21", (2, 1)), ("a22", (2, 2))):
        A = base.copy()
        A[i, j] = A[j, i] = NAN
        S.append(("nan_" + name, A, B))
    for k in range(3):
        b = list(B)
        b[k] = NAN
        S.append(("nan_b%d" % k, base, tuple(b)))
    S.append(("nan_b0_last_pivot", sym(1, 0.3, 2, -0.2, 0.1, 4), (NAN, 2.0, 3.0)))
    S.append(("nan_b2_diagonal_matrix_order210", sym(1, 0, 2, 0, 0, 4), (1.0, 2.0, NAN)))     # L = 0 exactly, and 0 * NaN still reaches every x
    S.append(("nan_a21_order210", sym(1, 0.3, 2, -0.2, NAN, 4), B))
    # +-Inf on a diagonal (|Inf| > cutoff = Inf is false: the column stays unscaled)
    S.append(("inf_a00", sym(INF, 0.3, 2, -0.2, 0.1, 1), B))
    S.append(("minus_inf_a11", sym(4, 0.3, -INF, -0.2, 0.1, 1), B))
    S.append(("inf_a22", sym(4, 0.3, 2, -0.2, 0.1, INF), B))
    S.append(("inf_b1", base, (1.0, INF, 3.0)))
    # a NaN a11 beside an a22 below the cutoff: the pivot search of step 1 starts on the NaN, no comparison with it is true, and the
    # factorisation goes on (fmax would drop the NaN); the mirror image -- a22 NaN, a11 small -- finds the small a11 and stops.
    # The overflow variant makes the difference visible in x: step 1 runs, l21 = a21 - l20 * (d0 * l10) overflows, Inf * 0 is NaN.
    S.append(("nan_a11_small_a22", sym(1, 0.5, NAN, 0.25, 0.125, 1e-20), B))
    S.append(("nan_a11_small_a22_overflowing_l21", sym(1, -1e200, NAN, 1e200, 1.0, 1e-20), B))
    S.append(("nan_a22_small_a11", sym(1, 0.5, 1e-20, 0.25, 0.125, NAN), B))
    S.append(("nan_a22_small_a11_overflowing_l21", sym(1, -1e200, 1e-20, 1e200, 1.0, NAN), B))
    S.append(("nan_a11_zero_a22", sym(1, 0.5, NAN, 0.25, 0.125, 0.0), B))
    return [(n, np.asarray(A, np.float64), np.asarray(b, np.float64)) for n, A, b in S]


SOLVER_SYSTEMS = _solver_systems()


def solver_arrays():
    """names, A [n, 3, 3], b [n, 3]"""
    return [s[0] for s in SOLVER_SYSTEMS], np.stack([s[1] for s in SOLVER_SYSTEMS]), np.stack([s[2] for s in SOLVER_SYSTEMS])


# ------------------------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------------------------
def _frames():
    """0: identity.  1, 2: the two 120-degree turns about (1,1,1), whose rotation matrices are exact permutations -- with the identity
    they put the depth direction on world z, y and x.  3..8: six nearby cameras in general position (seeded)."""
    rng = np.random.default_rng(20240607)
    T = [[0, 0, 0, 1, 0, 0, 0], [0.5, 0.5, 0.5, 0.5, 0, 0, 0], [-0.5, -0.5, -0.5, 0.5, 0, 0, 0]]
    for _ in range(6):
        q = np.concatenate([rng.uniform(-0.04, 0.04, 3), [1.0]])
        T.append(list(q / math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])) + list(rng.uniform(-0.4, 0.4, 3)))
    return np.array(T, dtype=np.float64)


FRAMES = _frames()


def _act(T, X):
    """R X + t, written out on scalars: the inputs must be the same bits wherever this file runs, whatever BLAS numpy has"""
    x, y, z, w = (float(v) for v in T[:4])
    R = ((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)),
         (2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)),
         (2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)))
    X = [float(v) for v in X]
    return [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + float(T[4 + i]) for i in range(3)]


def bearing(frame, X, noise=(0.0, 0.0)):
    p = _act(FRAMES[frame], X)
    r = [p[0] / p[2] + float(noise[0]), p[1] / p[2] + float(noise[1]), 1.0]
    n = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    return np.array([r[0] / n, r[1] / n, r[2] / n])


def pt(name, pos, obs):
    """a point: start position and observations [(frame, bearing f)]"""
    return dict(name=name, pos=np.asarray(pos, np.float64), frames=[int(o[0]) for o in obs], f=[np.asarray(o[1], np.float64) for o in obs])


def seg(name, s, e):
    """a segment from two points observed by the same frames in the same order"""
    assert s["frames"] == e["frames"], name
    return dict(name=name, spos=s["pos"], epos=e["pos"], frames=s["frames"], sf=s["f"], ef=e["f"])


POOL_FRAMES = (3, 4, 5)


def pool_point(i):
    """seeded, noisy, well-posed: point i of an endless pool, observed by frames 3, 4, 5.  The perturbation of the start and the pixel
    noise (0.5 px at a focal length of 416 px) are those of synth.make_structure_batch, where chi2 stops falling near the noise floor."""
    rng = np.random.default_rng(77000 + i)
    X = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(3.0, 8.0)])
    obs = [(f, bearing(f, X, rng.normal(0.0, 0.5 / 416.0, 2))) for f in POOL_FRAMES]
    return pt("pool%d" % i, X + rng.normal(0, 0.05, 3), obs)


def rough_point(i):
    """seeded: a close landmark started metres off -- the first Gauss-Newton steps overshoot and chi2 rises early"""
    rng = np.random.default_rng(76000 + i)
    X = np.array([rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(1.0, 3.0)])
    obs = [(f, bearing(f, X, rng.normal(0.0, 0.5 / 416.0, 2))) for f in POOL_FRAMES]
    return pt("rough%d" % i, X + rng.normal(0, 1.5, 3), obs)


def exact_point(i, frames=POOL_FRAMES):
    """noise-free bearings and the true position as the start"""
    rng = np.random.default_rng(78000 + i)
    X = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(3.0, 8.0)])
    return pt("exact%d" % i, X, [(f, bearing(f, X)) for f in frames])


def wild_point(i):
    """seeded: a pool point one of whose bearings has a huge first or second component (e of the order of DBL_MAX: b overflows, dp holds
    Inf and NaN side by side): full-rank systems whose accepted step has dp[0] = +-Inf beside NaN components"""
    rng = np.random.default_rng(79000 + i)
    p = pool_point(1000 + i)
    k = int(rng.integers(0, 3))
    p["f"][k] = np.array([rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(305, 308), rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(305, 308), 1.0])
    p["name"] = "wild%d" % i
    return p


def _named_points():
    P = {}
    add = lambda p: P.__setitem__(p["name"], p)
    add(exact_point(0))
    add(exact_point(1, (3, 4, 5, 6, 7, 8)))
    # one observation: rank-2 normal equations; on the optical axis J = -P R has exact zeros and two equal diagonals
    add(pt("axis_z", (0, 0, 4), [(0, (0.001, -0.002, 1.0))]))
    add(pt("axis_y", (0, 4, 0), [(1, (0.001, -0.002, 1.0))]))
    add(pt("axis_x", (4, 0, 0), [(2, (0.001, -0.002, 1.0))]))
    add(pt("off_axis_z", (0.5, -0.25, 4), [(0, (0.13, -0.06, 1.0))]))
    add(pt("off_axis_y", (0.5, 4, -0.25), [(1, (-0.06, 0.13, 1.0))]))
    add(pt("off_axis_x", (4, -0.25, 0.5), [(2, (-0.07, 0.12, 1.0))]))
    add(pt("off_axis_z_far_bearing", (0.5, -0.25, 4), [(0, (0.5, 0.4, 1.0))]))
    add(pt("axis_z_two_views", (0, 0, 4), [(0, (0.001, -0.002, 1.0)), (0, (-0.001, 0.001, 1.0))]))
    # camera-frame depth 1e-9 of the lateral offset: A22 dwarfs the other diagonals
    add(pt("shallow", (1, 0.5, 1e-9), [(0, (1.0, 0.5, 1.0000001e-9))]))
    add(pt("shallow_two_views", (1, 0.5, 1e-9), [(0, (1.0, 0.5, 1.0000001e-9)), (3, bearing(3, (1, 0.5, 1e-9)))]))
    add(pt("shallow_y", (0.5, 1e-9, 1), [(1, (1.0, 0.5, 1.0000001e-9))]))
    # the same with a bearing whose f[2] == 0 (0/0: e, and with it all of b, is NaN while A stays finite).  The depth column pivots first,
    # the factorisation stops at step 1 and D^+ replaces the two other components -- NaN after the forward substitution -- by 0: dp is NaN
    # on the depth axis only.  Depth on world z or y: dp[0] = 0 passes the reference's isnan(dp[0]), norm_max passes over the NaN, and
    # the landmark "converges" at iteration 0 with a NaN written into it.  Depth on world x: dp[0] is the NaN, and the step is rolled back.
    add(pt("shallow_f2_zero", (1, 0.5, 1e-9), [(0, (0.0, 1.0, 0.0))]))
    add(pt("shallow_y_f2_zero", (0.5, 1e-9, 1), [(1, (0.0, 1.0, 0.0))]))
    add(pt("shallow_x_f2_zero", (1e-9, 1, 0.5), [(2, (0.0, 1.0, 0.0))]))
    add(pt("shallow_nan_bearing", (1, 0.5, 1e-9), [(0, (NAN, 0.5, 1e-9))]))
    # depth exactly 0 in one observing frame: z_inv = Inf
    add(pt("zero_depth", (0.3, 0.2, 0.0), [(0, (0.3, 0.2, 1.0)), (3, bearing(3, (0.3, 0.2, 1.0)))]))
    add(pt("zero_depth_on_axis", (0.0, 0.0, 0.0), [(0, (0.0, 0.0, 1.0))]))
    add(pt("regular_03", (0.31, 0.18, 4.0), [(0, (0.08, 0.05, 1.0)), (3, bearing(3, (0.3, 0.2, 4.1)))]))
    # a bearing in the image plane of its camera: project2d divides by f[2] == 0
    g = pool_point(900)
    g["name"], g["f"][1] = "bearing_f2_zero", np.array([1.0, 0.0, 0.0])
    add(g)
    g = pool_point(901)
    g["name"], g["f"][0] = "bearing_f2_zero_inf_inf", np.array([0.6, -0.8, 0.0])
    add(g)
    # a landmark at 1e150: J ~ 1e-150, A ~ 1e-300, max|D| eps below 1/DBL_MAX
    add(pt("far_1e150", (1e150, 2e150, 3e150), [(0, (0.3, 0.6, 1.0)), (3, (0.31, 0.61, 1.0))]))
    add(pt("far_1e150_one_view", (1e150, 2e150, 3e150), [(0, (0.3, 0.6, 1.0))]))
    # e = 1.7e308 on the optical axis at depth 10: b = 1.7e307, D = 0.01, dp = (Inf, 0, 0) is accepted at iteration 0; the next
    # iteration transforms a position holding Inf and dp[0] is NaN: roll-back to the input at a LATER iteration
    add(pt("step_to_infinity", (0, 0, 10), [(0, (1.7e308, 0.0, 1.0))]))
    add(pt("regular_0", (0.2, -0.1, 9.0), [(0, (0.03, -0.02, 1.0))]))
    add(pt("no_observations", (1.0, 2.0, 3.0), []))
    add(pt("no_observations_nan", (NAN, 2.0, INF), []))
    return P


NAMED = _named_points()


# The seeded pools were classified on the CPU with tests/np_structopt.py; what each index reaches is asserted, not assumed, by
# tests/test_structopt_paths.py::test_inputs_reach_every_path.  pool1, pool6: chi2 rises at the last iteration, pool0, pool3 / pool37: converge at
# iteration 4 / 3, pool2, pool4: run out of iterations; rough3 / rough6 / rough78: chi2 rises at iteration 1 / 2 / 3; wild9, wild22: an
# accepted step with dp[0] = +-Inf beside NaN components, then NaN at iteration 1; wild7: NaN at iteration 1; wild4: NaN at iteration 0
_POOL = dict(pool=(0, 1, 2, 3, 4, 6, 37), rough=(3, 5, 6, 57, 78, 29), wild=(4, 7, 9, 22), exact=(2,))
for _i in _POOL["pool"]:
    NAMED["pool%d" % _i] = pool_point(_i)
for _i in _POOL["rough"]:
    NAMED["rough%d" % _i] = rough_point(_i)
for _i in _POOL["wild"]:
    NAMED["wild%d" % _i] = wild_point(_i)
for _i in _POOL["exact"]:
    NAMED["exact%d" % _i] = exact_point(_i)

# points in launch order: the landmarks without observations sit between landmarks with observations
POINT_ORDER = ("exact0", "no_observations", "axis_z", "axis_y", "axis_x", "exact1", "off_axis_z", "off_axis_y", "off_axis_x", "off_axis_z_far_bearing",
               "axis_z_two_views", "shallow", "no_observations_nan", "shallow_two_views", "shallow_y", "zero_depth", "zero_depth_on_axis", "regular_03",
               "bearing_f2_zero", "bearing_f2_zero_inf_inf", "far_1e150", "far_1e150_one_view", "step_to_infinity", "regular_0", "pool0", "pool1",
               "pool2", "pool37", "no_observations", "shallow_f2_zero", "shallow_y_f2_zero", "shallow_x_f2_zero", "shallow_nan_bearing", "rough3", "rough6", "rough78", "rough29", "wild4", "wild7", "wild9", "wild22", "exact2")
POINTS = [NAMED[n] for n in POINT_ORDER]

# segments: (start point, end point) observed by the same frames.  Every trigger of the joint roll-back and of the joint stop on the
# start point only, the end point only and both.
SEGMENT_PAIRS = (
    ("exact0", "pool0"), ("pool0", "exact0"), ("exact0", "exact2"),                         # at rest at iteration 0: s, e, both
    ("pool37", "pool0"), ("pool0", "pool37"), ("pool37", "pool37"),                         # one end converges while the other still moves
    ("pool0", "pool2"), ("pool2", "pool0"), ("pool0", "pool3"),
    ("no_observations", "no_observations"),
    ("rough3", "pool0"), ("pool0", "rough3"), ("rough3", "rough5"),                         # chi2 rises at iteration 1: s, e, both
    ("rough6", "pool0"), ("pool0", "rough6"), ("rough6", "rough57"),                        # ... at iteration 2
    ("pool1", "pool0"), ("pool0", "pool1"), ("pool1", "pool6"),                            # ... at the last iteration
    ("pool2", "pool4"),                                                                     # out of iterations
    ("zero_depth", "regular_03"), ("regular_03", "zero_depth"), ("zero_depth", "zero_depth"),      # NaN at iteration 0: s, e, both
    ("bearing_f2_zero", "pool2"), ("pool2", "bearing_f2_zero_inf_inf"),
    ("step_to_infinity", "regular_0"), ("regular_0", "step_to_infinity"), ("step_to_infinity", "step_to_infinity"),   # NaN at iteration 1
    ("wild9", "pool2"), ("pool2", "wild22"), ("wild7", "wild9"),
    ("shallow_f2_zero", "off_axis_z"), ("off_axis_z", "shallow_f2_zero"), ("shallow_f2_zero", "shallow_nan_bearing"),   # at rest with a NaN written: s, e, both
    ("shallow_y_f2_zero", "axis_y"),
    ("axis_z", "off_axis_z"), ("shallow", "off_axis_z"), ("far_1e150_one_view", "regular_0"), ("axis_y", "shallow_y"), ("axis_x", "off_axis_x"),
)


SEGMENTS = [seg(a + "+" + b, NAMED[a], NAMED[b]) for a, b in SEGMENT_PAIRS]

ITER_VARIANTS = ((5, 5), (2, 3), (1, 1), (0, 5), (5, 0))       # (n_iter_pts, n_iter_segs)


def batch(points, segments, frames=None):
    """the flat arrays of plsvo_structopt_in (the dict synth.make_structure_batch returns, without its ground truth)"""
    frames = FRAMES if frames is None else frames
    z3 = np.zeros((0, 3))
    st = lambda rows: np.array(rows, dtype=np.float64).reshape(-1, 3) if len(rows) else z3
    pt_off, pt_fr, pt_f = [0], [], []
    for p in points:
        pt_fr += p["frames"]
        pt_f += list(p["f"])
        pt_off.append(len(pt_fr))
    sg_off, sg_fr, sg_sf, sg_ef = [0], [], [], []
    for g in segments:
        sg_fr += g["frames"]
        sg_sf += list(g["sf"])
        sg_ef += list(g["ef"])
        sg_off.append(len(sg_fr))
    return dict(frame_T=np.array(frames, dtype=np.float64), pt_pos=st([p["pos"] for p in points]), pt_obs_off=np.array(pt_off, np.int32),
                pt_obs_frame=np.array(pt_fr, np.int32), pt_obs_f=st(pt_f), seg_spos=st([g["spos"] for g in segments]),
                seg_epos=st([g["epos"] for g in segments]), seg_obs_off=np.array(sg_off, np.int32), seg_obs_frame=np.array(sg_fr, np.int32),
                seg_obs_sf=st(sg_sf), seg_obs_ef=st(sg_ef))


def geometry_batch():
    """every directed point and segment in one launch"""
    return batch(POINTS, SEGMENTS)


LAYOUT_SIZES = [(n_pts, n_seg) for n_pts in (1, 63, 64, 65) for n_seg in (0, 1, 64, 65)]


def layout(n_pts, n_seg):
    """n_pts points and n_seg segments drawn round-robin from the directed cases: points and segments in one wave (1 + 1), the
    point/segment boundary before, on and after a wave edge (63, 64, 65), the last wave partly filled"""
    return batch([POINTS[(3 * k) % len(POINTS)] for k in range(n_pts)], [SEGMENTS[(5 * k) % len(SEGMENTS)] for k in range(n_seg)])


def permuted(points, segments, seed):
    """the same landmarks in another order over a relabelled frame table; every landmark keeps the order of its own observations (the
    sums over observations are not associative).  Returns (batch, point order, segment order): new landmark k is old landmark order[k]."""
    rng = np.random.default_rng(seed)
    po, so, fo = rng.permutation(len(points)), rng.permutation(len(segments)), rng.permutation(len(FRAMES))
    new_index = np.empty(len(FRAMES), int)
    new_index[fo] = np.arange(len(FRAMES))                    # new frame table row k is old frame fo[k]
    rel = lambda x: dict(x, frames=[int(new_index[f]) for f in x["frames"]])
    return batch([rel(points[i]) for i in po], [rel(segments[i]) for i in so], FRAMES[fo]), po, so
