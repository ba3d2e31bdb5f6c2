"""bigkrls_dev_syr2k (csrc/gemm.hip: syrk_lower, syrk_mirror with 128- and 64-wide tiles, syrk_mirror_cols,
syrk_mirror_set; their tile map csrc/syrkmap.h) against the region rule of the update, by the method of
test_gpu_gemm_core.py: A and B sit inside NaN-filled parents with odd leading dimensions, C inside a sentinel-filled one.

Region rule. With P = A B' (A, B general m x k, so that B A' or the wrong triangle shows) and the element columns
J = [begin BN, min(end BN, m)) of the call (BN = 128 for the tile-column forms 1 and 2, 64 for form 3, everything for forms
0 and 4; skip_first_column moves the start of J by 64):
    new[i, j] = C0[i, j] + alpha P[i, j]      for i >= j, j in J         (form 4: alpha P[i, j], C0 is not read)
    new[j, i] = new[i, j]                     for i >  j, j in J         (mirror forms 1 - 4)
and every other element of C is C0 bit for bit.

Exact cases: integer entries in [-64, 64], alpha in {-1, 0.5, 2}: every sum is an integer (or half of one) below 2^23, so
the result does not depend on the summation order or on FMA contraction and np.array_equal is the assertion.
Rounding case: standard normal entries, reference in np.longdouble,
    |C - ref| <= (k + 3) 2^-53 (|alpha| |A||B|' + |C0|),
the forward bound of a k-term inner product summed in any order plus the scaling and the add (there is no split-K here).
The bound is derived, not measured.

Shapes come from the branches of the code: m around the 128-row tile and the 64-wide column (193 and 513 end in an odd
64-wide column, whose second tile column lies outside the matrix), 901 = 8 row tiles (an interior tile, the unpredicated
epilogue, several bands: k = 64 / 512 / 1024 give 32 / 4 / 2 rows per band, i.e. 1, 2 and 4 bands); k through one to 64
k-tiles with partial last tiles."""
import numpy as np
import pytest

from bigkrls_amd import _lib

from _placement import SENT, place, take

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
LOWER, MIRROR128, MIRROR64, COLS, SET = range(5)
FORMS = (LOWER, MIRROR128, MIRROR64, COLS, SET)
MS = (1, 63, 64, 65, 127, 128, 129, 192, 193, 257, 300, 513, 901)
KS = (1, 15, 16, 17, 33, 128, 512, 1024)
ALPHAS = (-1.0, 0.5, 2.0)
SKIP = 1                                     # flags bit 0: skip_first_column


def tiles_of(m):
    return (m + 127) // 128


def columns(form, m, begin, end, flags):
    """The element columns [j0, j1) that a call updates (the clamping of csrc/gemm.hip's wrappers)."""
    t = tiles_of(m)
    if form in (LOWER, SET):
        return 0, m
    if form == COLS:
        if end < 0 or end > 2 * t:
            end = 2 * t
        begin = max(begin, 0)
        j0, j1 = 64 * begin, min(64 * end, m)
    else:
        if end < 0 or end > t:
            end = t
        if begin >= end:
            return 0, 0
        j0, j1 = 128 * begin + (64 if flags & SKIP else 0), min(128 * end, m)
    return (j0, j1) if j0 < j1 else (0, 0)


def region_rule(form, alpha, P, C0, j0, j1, dtype=np.float64):
    """new C of one call by the rule of the module docstring; P = A B' and C0 in `dtype`."""
    m = C0.shape[0]
    new = C0.astype(dtype).copy()
    upd = np.tril(np.ones((m, m), dtype=bool))
    upd[:, :j0] = False
    upd[:, j1:] = False
    val = dtype(alpha) * P if form == SET else C0.astype(dtype) + dtype(alpha) * P
    new[upd] = val[upd]
    if form != LOWER:
        strict = upd & ~np.eye(m, dtype=bool)
        new.T[strict] = new[strict]
    return new


class Operands:
    """A and B (m x k) uploaded once, inside NaN-filled parents; call() runs one update on a fresh or a given C."""

    def __init__(self, ctx, A, B):
        self.ctx, self.A, self.B = ctx, A, B
        self.m, self.k = A.shape
        self.dA, self.pA, self.lda, _, _ = place(ctx, A)
        self.dB, self.pB, self.ldb, _, _ = place(ctx, B, ld=A.shape[0] + 7 + (A.shape[0] % 2))   # odd, and not A's
        self.P = A @ B.T

    def upload_c(self, C0):
        return place(self.ctx, C0, fill=SENT)

    def update(self, placed, form, alpha, begin=0, end=-1, flags=0):
        _, pC, ldc, _, _ = placed
        _lib.call("bigkrls_dev_syr2k", self.ctx.handle, form, self.m, self.k, float(alpha), self.pA, self.lda, self.pB,
                  self.ldb, pC, ldc, begin, end, flags)

    def download_c(self, placed, what):
        dC, _, _, r0, c0 = placed
        return take(dC, r0, c0, self.m, self.m, what)

    def call(self, form, alpha, C0, begin=0, end=-1, flags=0):
        placed = self.upload_c(C0)
        self.update(placed, form, alpha, begin, end, flags)
        return self.download_c(placed, ("syr2k", form, self.m, self.k, alpha, begin, end, flags))


def int_operands(ctx, rng, m, k):
    A = rng.integers(-64, 65, size=(m, k)).astype(np.float64)
    B = rng.integers(-64, 65, size=(m, k)).astype(np.float64)
    return Operands(ctx, A, B)


def sym_int(rng, m):
    L = np.tril(rng.integers(-64, 65, size=(m, m))).astype(np.float64)
    return L + np.tril(L, -1).T


def same_bits(a, b):
    """Bitwise equality that also accepts NaN == NaN (a C that must not be touched may hold NaN)."""
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check_exact(ops, rng, form, alpha, begin=0, end=-1, flags=0, C0=None):
    m = ops.m
    if C0 is None:
        C0 = sym_int(rng, m)
    j0, j1 = columns(form, m, begin, end, flags)
    ref = region_rule(form, alpha, ops.P, np.zeros((m, m)) if form == SET else C0, j0, j1)
    # form 4 must not read C: it starts as NaN
    got = ops.call(form, alpha, np.full((m, m), np.nan) if form == SET else C0, begin, end, flags)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"syr2k form={form} m={m} k={ops.k} alpha={alpha} range=({begin}, {end}) flags={flags} "
                             f"columns [{j0}, {j1}): {len(bad)} wrong entries, first at {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]}, expected {ref[tuple(bad[0])]}, C0 {C0[tuple(bad[0])]}")
    return got


# ---- shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_row_counts(ctx, form):
    """Every m of the list, each with another k and alpha: one tile, a partial tile, the odd last 64-wide column, an
    interior tile (m >= 257) and the unpredicated epilogue (m = 901: tile rows 1 .. 6 of column 0 lie inside)."""
    rng = np.random.default_rng(1000 + form)
    for i, m in enumerate(MS):
        ops = int_operands(ctx, rng, m, KS[(i + form) % len(KS)])
        check_exact(ops, rng, form, ALPHAS[i % 3])


@pytest.mark.parametrize("form", FORMS)
def test_k_tiles(ctx, form):
    """k through one k-tile, partial last tiles and up to 64 tiles, at m = 129 (a full and a one-row tile row)."""
    rng = np.random.default_rng(1100 + form)
    for i, k in enumerate(KS):
        ops = int_operands(ctx, rng, 129, k)
        check_exact(ops, rng, form, ALPHAS[(i + 1) % 3])


@pytest.mark.parametrize("k", [64, 512, 1024])
def test_bands(ctx, k):
    """m = 901 (8 row tiles): k = 64 / 512 / 1024 give 32 / 4 / 2 rows per band, i.e. 1, 2 and 4 bands of the tile order,
    for every form and both tile widths."""
    rng = np.random.default_rng(1200 + k)
    ops = int_operands(ctx, rng, 901, k)
    for i, form in enumerate(FORMS):
        check_exact(ops, rng, form, ALPHAS[i % 3])


@pytest.mark.parametrize("form", [LOWER, MIRROR128, MIRROR64, COLS])
def test_reads_the_lower_triangle_only(ctx, form):
    """C0 not symmetric: the rule takes C0[i, j] with i >= j; a kernel that reads the mirror image instead shows. For
    form 0 the strict upper triangle comes back unchanged."""
    rng = np.random.default_rng(1300 + form)
    ops = int_operands(ctx, rng, 300, 33)
    C0 = rng.integers(-64, 65, size=(300, 300)).astype(np.float64)
    got = check_exact(ops, rng, form, 2.0, C0=C0)
    if form == LOWER:
        assert np.array_equal(np.triu(got, 1), np.triu(C0, 1))


# ---- ranges ----------------------------------------------------------------------------------------------------------
COL_RANGES = [(0, -1), (0, 1), (1, 2), (3, 16), (5, 11), (14, -1), (15, 16), (16, 16), (-3, 4), (2, 40)]


@pytest.mark.parametrize("m,k", [(901, 128), (513, 33)])
def test_column_ranges(ctx, m, k):
    """syrk_mirror_cols over ranges of 64-wide columns: the first, an inner one, ranges that start at an odd column, the
    last column pair, empty ranges, begin < 0 and end > 2 tiles (both clamped). m = 901 has 16 columns (15 of them inside
    the matrix, the last 5 elements wide), m = 513 has 10 with only the first element of column 8 inside."""
    rng = np.random.default_rng(1400 + m)
    ops = int_operands(ctx, rng, m, k)
    for i, (begin, end) in enumerate(COL_RANGES):
        check_exact(ops, rng, COLS, ALPHAS[i % 3], begin, end)


@pytest.mark.parametrize("m,k", [(901, 128), (513, 33)])
def test_tile_column_ranges(ctx, m, k):
    """syrk_mirror over ranges of 128-wide tile columns, with both tile widths, and for the 64-wide tiles with and without
    skip_first_column: whole, the first, all but the first, an inner range, begin = tiles (nothing to do)."""
    rng = np.random.default_rng(1500 + m)
    ops = int_operands(ctx, rng, m, k)
    t = tiles_of(m)
    for i, (begin, end) in enumerate([(0, -1), (0, 1), (1, -1), (3, 5), (t, -1)]):
        check_exact(ops, rng, MIRROR128, ALPHAS[i % 3], begin, end)
        for flags in (0, SKIP):
            check_exact(ops, rng, MIRROR64, ALPHAS[(i + 1 + flags) % 3], begin, end, flags)


def test_unknown_form_or_flag_is_rejected(ctx):
    rng = np.random.default_rng(16)
    ops = int_operands(ctx, rng, 64, 16)
    placed = ops.upload_c(sym_int(rng, 64))
    for form, flags in ((5, 0), (-1, 0), (MIRROR128, SKIP), (COLS, SKIP), (MIRROR64, 2)):
        with pytest.raises(_lib.BigKRLSError) as e:
            ops.update(placed, form, 1.0, 0, -1, flags)
        assert e.value.code == _lib.EINVAL and "dev_syr2k" in str(e.value)


# ---- composition -------------------------------------------------------------------------------------------------------
def run_pieces(ops, C0, pieces):
    placed = ops.upload_c(C0)
    for form, begin, end, flags in pieces:
        ops.update(placed, form, -1.0, begin, end, flags)
    return ops.download_c(placed, ("syr2k pieces", pieces))


@pytest.mark.parametrize("k", [128, 512])
def test_pieces_compose_to_the_whole_update(ctx, k):
    """Stage 1 of the eigensolver applies one trailing update in pieces; applied in turn to one C they must give the
    single whole call bit for bit (general real inputs: every tile has to be computed in the same order whichever call
    it belongs to). The compositions of csrc/eigen_2stage.inc:
      * syrk_mirror_cols on the columns [0, 5), [5, 11), [11, end);
      * 64-wide tiles: the next panel's tile column (0, 1), then the rest (1, end);
      * the first 64-wide column by itself (there: by the fused panel products), then (0, end) with skip_first_column."""
    rng = np.random.default_rng(1700 + k)
    m = 901
    ops = Operands(ctx, rng.standard_normal((m, k)), rng.standard_normal((m, k)))
    L = np.tril(rng.standard_normal((m, m)))
    C0 = L + np.tril(L, -1).T
    whole_cols = run_pieces(ops, C0, [(COLS, 0, -1, 0)])
    whole_64 = run_pieces(ops, C0, [(MIRROR64, 0, -1, 0)])
    assert np.isfinite(whole_cols).all() and np.array_equal(whole_cols, whole_64)    # the same kernel and tiles
    assert np.array_equal(run_pieces(ops, C0, [(COLS, 0, 5, 0), (COLS, 5, 11, 0), (COLS, 11, -1, 0)]), whole_cols)
    assert np.array_equal(run_pieces(ops, C0, [(MIRROR64, 0, 1, 0), (MIRROR64, 1, -1, 0)]), whole_64)
    assert np.array_equal(run_pieces(ops, C0, [(COLS, 0, 1, 0), (MIRROR64, 0, -1, SKIP)]), whole_64)


def test_overlapping_pieces_follow_the_region_rule(ctx):
    """(0, 1) and then (0, end) with skip_first_column, both with 64-wide tiles, overlap in the columns [64, 128): those
    are updated twice, everything else once -- the rule applied in turn, exactly."""
    rng = np.random.default_rng(18)
    m = 513
    ops = int_operands(ctx, rng, m, 17)
    C0 = sym_int(rng, m)
    got = run_pieces(ops, C0, [(MIRROR64, 0, 1, 0), (MIRROR64, 0, -1, SKIP)])
    ref = region_rule(MIRROR64, -1.0, ops.P, C0, *columns(MIRROR64, m, 0, 1, 0))
    ref = region_rule(MIRROR64, -1.0, ops.P, ref, *columns(MIRROR64, m, 0, -1, SKIP))
    assert np.array_equal(got, ref)


# ---- rounding reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_rounding_bound(ctx, form):
    rng = np.random.default_rng(1900 + form)
    m, Lf = 300, np.longdouble
    for k, alpha in ((33, 0.7), (512, -1.3)):
        A, B = rng.standard_normal((m, k)), rng.standard_normal((m, k))
        ops = Operands(ctx, A, B)
        Lo = np.tril(rng.standard_normal((m, m)))
        C0 = Lo + np.tril(Lo, -1).T
        ref = region_rule(form, alpha, A.astype(Lf) @ B.astype(Lf).T, np.zeros((m, m)) if form == SET else C0, 0, m, dtype=Lf)
        bound = (k + 3) * EPS * (abs(alpha) * (np.abs(A) @ np.abs(B).T) + (0.0 if form == SET else np.abs(C0)))
        start = np.full((m, m), np.nan) if form == SET else C0
        got = ops.call(form, alpha, start)
        assert np.isfinite(got).all()
        err = np.abs(got.astype(Lf) - ref).astype(np.float64)
        if form == LOWER:                      # the strict upper triangle: untouched, bit for bit
            assert np.array_equal(np.triu(got, 1), np.triu(C0, 1))
            err, bound = np.tril(err), np.where(np.tril(np.ones((m, m), dtype=bool)), bound, 1.0)
        worst = float(np.max(err / bound))
        print(f"syr2k form={form} m={m} k={k}: error / bound = {worst:.3g}")
        assert worst <= 1.0, (form, k, worst, np.unravel_index(np.argmax(err / bound), err.shape))
        if form != LOWER:
            assert np.array_equal(got, got.T), (form, k, "the mirrored update is not exactly symmetric")
        again = ops.call(form, alpha, start)
        assert same_bits(got, again), (form, k, "two calls differ")
