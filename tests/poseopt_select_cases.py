"""Rows of bit patterns for tests/test_gpu_poseopt_select.py (MI355X) and tests/test_emu_poseopt_select.py (the same file run against the
host emulation build): the select of the pose optimiser's row kernels (poseopt_select.hpp) through plsvo_poseopt_row_select.  The
expected value of a row is np.sort(patterns)[k] on the unsigned patterns; `model_path` restates which route the device function takes
for a row (minimum == maximum, rank finish, extra histogram pass, every digit), so that the test can say how often each one ran."""
import numpy as np

CAP = 320                      # PLSVO_ROW_SELECT_CAP
EQUAL, RANK, EXTRA, FALLBACK, DIGITS = 1, 2, 4, 8, 16   # PLSVO_ROW_SELECT_*
SIZES = (1, 2, 3, 15, 16, 17, 31, 33, 255, 256, 257, 280, CAP - 1, CAP, CAP + 1, 700)

_F = {32: (np.float32, np.uint32, 23, 255), 64: (np.float64, np.uint64, 52, 2047)}   # float type, pattern type, mantissa bits, top exponent


def ks(n):
    return sorted({0, n // 2, n - 1})


def bits_of(x, bits):
    ft, ut = _F[bits][:2]
    return np.asarray(x, ft).view(ut)


def _distinct(rng, n, bits):
    """n distinct patterns of non-negative finite floats"""
    ut, mant, top = _F[bits][1:]
    return rng.choice((top << mant) - 1, size=n, replace=False).astype(ut)


def model_errors(rng, n, bits):
    """the errors the medians are taken over: pairs of N(0, 1/400) residuals, one in ten an outlier; the float scale error is their norm,
    the 64-bit select runs over the squared error"""
    e = rng.normal(0.0, 1.0 / 400.0, (n, 2)) * np.where(rng.random(n) < 0.1, 20.0, 1.0)[:, None]
    sq = (e * e).sum(1)
    return bits_of(np.sqrt(sq), 32) if bits == 32 else bits_of(sq, 64)


def families(rng, n, k, bits):
    """[(name, patterns)] of one (n, k, width): every value family, in a shuffled order of the elements"""
    ft, ut, mant, top = _F[bits]
    out = [("all-equal", np.full(n, bits_of(1.5, bits), ut))]
    lo, hi = bits_of(0.37, bits), bits_of(0.52, bits)
    for name, n_lo in (("two-values-split-below-k", k - 1), ("two-values-split-at-k", k), ("two-values-split-above-k", k + 1)):
        n_lo = min(max(n_lo, 0), n)
        out.append((name, np.concatenate([np.full(n_lo, lo, ut), np.full(n - n_lo, hi, ut)])))
    out.append(("random-distinct", _distinct(rng, n, bits)))
    base = int(bits_of(0.7, bits))
    out.append(("lowest-byte-differs", ((base & ~0xff) | rng.integers(0, 256, n)).astype(ut)))
    mid = 8 * (bits // 16)   # byte 2 of 4, byte 4 of 8
    out.append(("one-middle-byte-differs", ((base & ~(0xff << mid)) | (rng.integers(0, 256, n) << mid)).astype(ut)))
    # one value per binade over the whole exponent range; 0, a denormal and +Inf come first
    special = [0, int(rng.integers(1, 1 << mant)), top << mant]
    expo = np.linspace(1, top - 1, max(n - 3, 0)).astype(np.int64)
    binades = (expo << mant) | rng.integers(0, 1 << mant, len(expo))
    out.append(("one-per-binade", np.concatenate([np.array(special[:n], np.int64).astype(ut), binades.astype(ut)])[:n]))
    out.append(("inf-and-one-finite", np.concatenate([np.full(n - 1, top << mant, ut), bits_of([0.25], bits)])))
    for copies in (17, 40):   # more than 16 copies of the value at rank n / 2 among distinct others (all copies, where n is smaller)
        c = min(copies, n)
        others = np.sort(_distinct(rng, n - c + 1, bits))
        med = others[(n - c) // 2]
        out.append((f"{copies}-copies-of-the-median", np.concatenate([others[others != med], np.full(c, med, ut)])))
    out.append(("model-errors", model_errors(rng, n, bits)))
    # a tight cluster (distinct in the low 16 bits only) and one value far below: the first bins are crowded, a later pass thins them out
    out.append(("cluster-and-one-far-value", np.concatenate([np.zeros(1, ut), ((base & ~0xffff) | rng.choice(1 << 16, n - 1, replace=False)).astype(ut)])))
    return [(name, rng.permutation(v)) for name, v in out]


def model_path(v, k, bits):
    """the route row_select_regs takes for one row of at most CAP values (poseopt_select.hpp).  It restates the device's pass schedule
    (first digit at the highest differing bit, eight bits per pass, rank finish at <= 16 candidates), so it is no independent check of
    that schedule -- the selected VALUE is checked against np.sort; a deliberate change of the schedule changes this model and the
    ROUTES counts of tests/test_gpu_poseopt_select.py with it."""
    v = [int(x) for x in v]
    full = (1 << bits) - 1
    mn, mx = min(v), max(v)
    if mn == mx:
        return EQUAL
    hb = (mn ^ mx).bit_length() - 1
    mask = (full << (hb + 1)) & full
    prefix, shift, passes = mn & mask, max(hb - 7, 0), 0
    while True:
        digits = sorted(((x & ~mask) >> shift) & 255 for x in v if (x & mask) == prefix)
        d = digits[k]
        k -= digits.index(d)
        passes += 1
        prefix |= d << shift
        mask |= 255 << shift
        extra = EXTRA if passes > 1 else 0
        if shift == 0:
            return DIGITS | extra
        if digits.count(d) <= 16:
            return RANK | extra
        shift = max(shift - 8, 0)


class Rows:
    """rows for one plsvo_poseopt_row_select call"""

    def __init__(self, bits):
        self.bits, self.ut = bits, _F[bits][1]
        self.vals, self.off, self.n, self.k, self.active, self.names = [], [], [], [], [], []
        self._len = 0

    def add(self, name, v, k, active=True):
        v = np.asarray(v, self.ut)
        self.vals.append(v); self.off.append(self._len); self.n.append(len(v)); self.k.append(k); self.active.append(1 if active else 0)
        self.names.append(name)
        self._len += len(v)

    def pad_to_workgroup(self):
        while len(self.n) % 4:
            self.add("padding", np.zeros(0, self.ut), 0, False)

    def run(self, ctx):
        pats = np.concatenate(self.vals) if self.vals else np.zeros(0, self.ut)
        return ctx.poseopt_row_select(pats, self.off, self.n, self.k, self.active)

    def expected(self):
        return np.array([np.sort(v)[k] if a and len(v) else 0 for v, k, a in zip(self.vals, self.k, self.active)], self.ut)


def family_rows(bits, seed=20260):
    """every (size, k, family) of one width: the rows at or below the cap first, then -- from a workgroup of their own on -- the rows above"""
    rng = np.random.default_rng(seed + bits)
    rows = Rows(bits)
    for big in (False, True):
        for n in SIZES:
            if (n > CAP) != big:
                continue
            for k in ks(n):
                for name, v in families(rng, n, k, bits):
                    rows.add(f"{name} n={n} k={k}", v, k)
        rows.pad_to_workgroup()
    return rows
