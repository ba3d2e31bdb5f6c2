"""The marginal-effects pass (csrc/deriv.hip) called directly through the C ABI: bigkrls_dev_deriv_rows in full and in
row-block mode, bigkrls_dev_deriv_var, and ops.bDerivatives / bigkrls_derivmat on top of them.

Exact reference (deriv_rows): the "kernel matrix" M, X and c hold integers in [-8, 8] and sigma is a power of two. Every
entry of the one product K [1, c, x_j, x_j o c | b_j, b_j o c] is then an integer below 2^35 whatever the summation
order, tile or split count, the finalise step of a continuous column is exact too, and
    D[:, j] = (-2 / sigma) (x o (M c) - M (x o c)),      S[:, j] = x o (M 1) - M x
must equal numpy bit for bit.

Binary columns: the group sums S1, Sc (same group as the row), O1, Oc (other group) are exact integers as well, but
E = exp(phi), phi = -(z1 - z0)^2 / sigma, is not. D and S are compared with a np.longdouble evaluation of the definition
    D = sd (+-1) ((1 - E) Sc + (1 - 1/E) Oc),      S = +-((1 - E) S1 + (1/E - 1) O1),      sd = 1 / (z1 - z0),
elementwise within (n + 16) 2^-53 times the absolute sums
    D: |sd| (|1 - E| (sum_same |K||c| + sum_all |K||c|) + |1 - 1/E| (sum_other |K||c| + sum_all |K||c|)),   S: |c| -> 1,
the forward bound of an n-term inner product summed in any order plus the subtraction Kc - Kbc. The bound is derived,
not measured. With integer sums the n-term part is slack; what it has to cover are the scalar roundings of the finalise
kernel: phi is computed as -1 / (sd sd sigma) (relative error <= 4u, u = 2^-53), exp is good to one unit in the last
place (2u), so E and 1/E carry (4 |phi| + 2) u, and the products and sums around them a few u more. slack_ok() checks
from these figures that the codings and sigma of a case fit the bound at its n before the kernel is looked at: a
property of the test's inputs, not of the code under test.

Placement: K, X, D and S are sub-blocks of larger parents (tests/_placement.py): odd leading dimension > rows, first
element 8- but not 16-byte aligned, NaN around the inputs, a finite sentinel around the outputs, NaN in the output
blocks themselves. Everything outside the n_rows x p blocks of D and S must come back untouched.

deriv_var: integer Q and S, weights from {+-1, +-2, +-0.5, 0} and power-of-two scales give an exact
var_j = scale_j sum_k wv_k (q_k' s_j)^2; standard normal data are compared with np.longdouble within
    scale [(n + 16) 2^-53 2 sum_k |w_k| |t_k| a_k + (k + 16) 2^-53 sum_k |w_k| t_k^2],   t_k = q_k' s,  a_k = |q_k|' |s|
(the inner products' forward error carried through the square, plus the k-term weighted sum)."""
import ctypes as C

import numpy as np
import pytest

from bigkrls_amd import _lib, ops
from oracle import krls_oracle as orc

from _placement import SENT, place, take

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
L = np.longdouble
CODINGS = {"01": (0.0, 1.0), "neg": (-1.5, 2.25), "zeros": (0.0, 1.0)}     # "zeros": half of the lows are -0.0


# ---- inputs ------------------------------------------------------------------------------------------------------------
def binary_column(rng, n, coding, single_high):
    lo, hi = CODINGS[coding]
    if single_high:
        b = np.zeros(n, dtype=bool)
        b[int(rng.integers(0, n))] = True
    else:
        b = rng.random(n) < 0.4
        b[0], b[n - 1] = True, False                       # both groups occur
    x = np.where(b, hi, lo)
    if coding == "zeros":
        idx = np.flatnonzero(~b)
        x[idx[::2]] = -0.0
        assert np.signbit(x).any() and np.unique(x).size == 2
    return x


def make_inputs(rng, n, p, binaries):
    """X (n x p) and c with integers in [-8, 8]; `binaries` = [(column, coding, single_high), ...]."""
    X = rng.integers(-8, 9, size=(n, p)).astype(np.float64)
    isb = np.zeros(p, dtype=np.int32)
    for j, coding, single in binaries:
        X[:, j] = binary_column(rng, n, coding, single)
        isb[j] = 1
    c = rng.integers(-8, 9, size=n).astype(np.float64)
    return X, isb, c


def default_binaries(n, p, seed):
    """One or two binary columns where the shape allows them, the codings and the single-row high group in turn."""
    kinds = [("01", False), ("neg", False), ("zeros", False), ("neg", True), ("01", True), ("zeros", True)]
    if n < 2:
        return []
    if p < 3:
        return [(p - 1, *kinds[seed % 6])]
    return [(1, *kinds[seed % 6]), (p - 1, *kinds[(seed + 3) % 6])]


def slack_ok(n, d, sigma):
    """Do the scalar roundings of a binary column with z1 - z0 = d fit the (n + 16) 2^-53 bound at this n? (Module
    docstring: relative errors in units of u; each absolute sum appears in the bound once in its own term and once
    in sum_all.)"""
    phi = d * d / sigma
    assert phi <= 30.0
    E, Einv = np.exp(-phi), np.exp(phi)
    e = 4.0 * phi + 2.0                                   # E and 1/E, in u
    room_same = (n + 16) * (2.0 * (1.0 - E) + (Einv - 1.0))
    room_other = (n + 16) * ((1.0 - E) + 2.0 * (Einv - 1.0))
    # D: sd (2u), the factor (e E + (1 - E)) resp. (e / E + (1/E - 1)), two products and one sum (3u)
    ok_d = (e * E + 6.0 * (1.0 - E) <= room_same) and (e * Einv + 6.0 * (Einv - 1.0) <= room_other)
    # S: kt = S1 + O1/E, kc = E S1 + O1 (or the mirror image), then kt - kc
    ok_s = ((1.0 + 2.0 * E) + e * E + (1.0 - E) <= room_same) and ((1.0 + 2.0 * Einv) + e * Einv + (Einv - 1.0) <= room_other)
    return ok_d and ok_s


# ---- reference -----------------------------------------------------------------------------------------------------------
def check_against_numpy(Mop, row0, X, isb, c, sigma, D, S, what):
    """Mop (n_rows x n): the rows of the matrix the pass multiplies with; row r is row row0 + r of the problem."""
    n_rows, n = Mop.shape
    xr = X[row0:row0 + n_rows]
    M1, Mc = Mop.sum(axis=1), Mop @ c
    aM = np.abs(Mop)
    MX, MXc = Mop @ X, Mop @ (X * c[:, None])              # (integers: exact in any order; binary columns do not use them)
    for j in range(X.shape[1]):
        x = X[:, j]
        if not isb[j]:
            d_ref = (-2.0 / sigma) * (xr[:, j] * Mc - MXc[:, j])
            s_ref = xr[:, j] * M1 - MX[:, j]
            for name, got, ref in (("D", D[:, j], d_ref), ("S", S[:, j], s_ref)):
                if not np.array_equal(got, ref):
                    bad = np.flatnonzero(~(got == ref))
                    raise AssertionError(f"{what}: {name}[:, {j}] (continuous) has {bad.size} wrong entries, first at row "
                                         f"{bad[0]}: got {got[bad[0]]!r}, expected {ref[bad[0]]!r}")
            continue
        z0, z1 = x.min(), x.max()
        assert slack_ok(n, z1 - z0, sigma), (what, j, "this coding and sigma do not fit the derived bound at this n")
        g = x == z1                                         # group of every column of the product
        hi = xr[:, j] == z1                                 # group of every row of the block
        d = L(z1) - L(z0)
        sd, phi = 1 / d, -(d * d) / L(sigma)
        E = np.exp(phi)
        Einv = 1 / E
        Kb, Kbc = Mop @ g.astype(np.float64), Mop @ (g * c)             # exact integers
        S1, O1 = np.where(hi, Kb, M1 - Kb).astype(L), np.where(hi, M1 - Kb, Kb).astype(L)
        Sc, Oc = np.where(hi, Kbc, Mc - Kbc).astype(L), np.where(hi, Mc - Kbc, Kbc).astype(L)
        sgn = np.where(hi, 1.0, -1.0).astype(L)
        d_ref = sd * sgn * ((1 - E) * Sc + (1 - Einv) * Oc)
        s_ref = sgn * ((1 - E) * S1 + (Einv - 1) * O1)
        for name, got, ref, w in (("D", D[:, j], d_ref, np.abs(c)), ("S", S[:, j], s_ref, np.ones(n))):
            a_hi, a_all = aM @ (g * w), aM @ w
            a_same, a_other = np.where(hi, a_hi, a_all - a_hi), np.where(hi, a_all - a_hi, a_hi)
            e1, e2 = float(abs(1 - E)), float(abs(1 - Einv))
            bound = (n + 16) * EPS * (e1 * (a_same + a_all) + e2 * (a_other + a_all)) * (float(abs(sd)) if name == "D" else 1.0)
            err = np.abs(got.astype(L) - ref).astype(np.float64)
            assert np.isfinite(got).all(), (what, name, j, "NaN / Inf")
            over = np.flatnonzero(~(err <= bound))
            assert over.size == 0, (f"{what}: {name}[:, {j}] (binary): {over.size} entries over the bound, first at row {over[0]}: "
                                    f"got {got[over[0]]!r}, expected {float(ref[over[0]])!r}, bound {bound[over[0]]:.3g}")


# ---- the call ------------------------------------------------------------------------------------------------------------
def deriv_rows_call(ctx, Kblock, n, n_rows, row0, X, isb, c, sigma, sub=True, ld_out=None, placed_k=None):
    """bigkrls_dev_deriv_rows on placed operands. Kblock: n x n_rows on the host (or `placed_k` = a placement made
    before). Returns the n_rows x p blocks of D and S."""
    p = X.shape[1]
    dK, pK, ldk, _, _ = placed_k if placed_k is not None else place(ctx, Kblock, sub)
    dX, pX, ldx, _, _ = place(ctx, X, sub)
    dc = ctx.from_numpy(c.reshape(n, 1))
    blank = np.full((n_rows, p), np.nan)
    dD, pD, ldd, r0, c0 = place(ctx, blank, sub, fill=SENT, ld=ld_out)
    dS, pS, lds, _, _ = place(ctx, blank, sub, fill=SENT, ld=ld_out)
    isb = np.ascontiguousarray(isb, dtype=np.int32)
    _lib.call("bigkrls_dev_deriv_rows", ctx.handle, pK, n, n_rows, ldk, row0, pX, p, ldx, isb.ctypes.data, dc.ptr,
              float(sigma), pD, ldd, pS, lds)
    return take(dD, r0, c0, n_rows, p, "deriv_rows D"), take(dS, r0, c0, n_rows, p, "deriv_rows S")


def full_mode_case(ctx, n, p, seed, sigma, sub=True, placed_k=None, M=None):
    rng = np.random.default_rng(seed)
    if M is None:
        M = rng.integers(-8, 9, size=(n, n)).astype(np.float64)          # not symmetric: the product is M B
    X, isb, c = make_inputs(rng, n, p, default_binaries(n, p, seed))
    D, S = deriv_rows_call(ctx, M, n, n, 0, X, isb, c, sigma, sub=sub, placed_k=placed_k)
    check_against_numpy(M, 0, X, isb, c, sigma, D, S, f"full mode n={n} p={p}")


# ---- deriv_rows, full mode -------------------------------------------------------------------------------------------
FULL_CASES = [(1, 1), (2, 1), (127, 3), (128, 15), (129, 16), (257, 31), (130, 32), (300, 70), (1100, 5)]


@pytest.mark.parametrize("n,p", FULL_CASES)
def test_deriv_rows_full_mode_exact(ctx, n, p):
    """row0 = 0, n_rows = n: tiny shapes, 2 + 2p = 32 / 34 / 64 / 66 / 142 operand columns (the 32-, 64- and 128-wide
    tiles, exactly full and one past, two N tiles) and n >= 1024 (split-K). sigma = 4 keeps |phi| in [0.25, 3.6], which
    fits the bound from n = 1 on (slack_ok)."""
    full_mode_case(ctx, n, p, 1000 + 37 * n + p, 4.0)


def test_deriv_rows_packed_layout(ctx):
    """The same entry on matrices of their own (ld = rows, 16-byte aligned), other powers of two for sigma."""
    full_mode_case(ctx, 200, 7, 5, 0.5, sub=False)
    full_mode_case(ctx, 129, 16, 6, 2.0, sub=False)


@pytest.fixture(scope="module")
def big_k(ctx):
    """The integer matrices of the n = 4095 / 4096 cases, placed once (134 MB each) and shared, unchanged, by the cases."""
    cache = {}

    def get(n):
        if n not in cache:
            M = np.random.default_rng(n).integers(-8, 9, size=(n, n)).astype(np.float64)
            cache[n] = (M, place(ctx, M, True))
        return cache[n]
    yield get
    cache.clear()


@pytest.mark.parametrize("n,p", [(4096, 16), (4096, 23), (4095, 16), (4096, 15), (4096, 24), (4096, 20)])
def test_deriv_rows_48_wide_tile_and_its_edges(ctx, big_k, n, p):
    """The 128 x 48 tile is taken for n >= 4096 and 32 < 2 + 2p <= 48: (4096, 16) is its clamped B loader (34 columns),
    (4096, 23) the fast one (48), (4096, 20) the shape of the flagship fit; (4095, 16), (4096, 15) and (4096, 24) lie
    just outside and take the generic tiles. K is an odd-offset block with ldk = n + 3 (n + 4 at n = 4095)."""
    M, placed = big_k(n)
    assert placed[2] == (n + 3 if n % 2 == 0 else n + 4)
    full_mode_case(ctx, n, p, 7000 + n + p, 2.0, placed_k=placed, M=M)


# ---- deriv_rows, row blocks ------------------------------------------------------------------------------------------
def test_deriv_rows_row_block_is_the_transposed_product(ctx):
    """The entry computes Krows' B: with a non-symmetric M and Krows = M[:, r0:r0 + n_rows] it gives rows r0 .. of M' B;
    the n_rows == n call gives M B. The column blocks are pointers into one placed copy of M that is followed by n
    columns of NaN: whichever way a block were read, n_rows x n or n x n_rows, the reads stay inside that parent, and
    the wrong way meets other numbers or NaN."""
    rng = np.random.default_rng(77)
    n, p, sigma = 200, 5, 4.0
    M = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
    assert not np.array_equal(M, M.T)
    X, isb, c = make_inputs(rng, n, p, [(2, "neg", False)])
    dM, pM, ldk, _, _ = place(ctx, np.hstack([M, np.full((n, n), np.nan)]))
    for r0, nr in ((37, 90), (0, 64), (199, 1)):
        block = (dM, C.c_void_p(pM.value + 8 * r0 * ldk), ldk, 0, 0)
        D, S = deriv_rows_call(ctx, None, n, nr, r0, X, isb, c, sigma, ld_out=nr + 3, placed_k=block)
        check_against_numpy(np.ascontiguousarray(M.T[r0:r0 + nr]), r0, X, isb, c, sigma, D, S, f"row block ({r0}, {nr}) of M'")
    D, S = deriv_rows_call(ctx, None, n, n, 0, X, isb, c, sigma, placed_k=(dM, pM, ldk, 0, 0))
    check_against_numpy(M, 0, X, isb, c, sigma, D, S, "n_rows == n: M B")


@pytest.mark.parametrize("n,p,blocks", [(300, 6, [(0, 128), (128, 128), (256, 44), (299, 1)]),
                                        (1300, 4, [(0, 1024), (1024, 276)])])
def test_deriv_rows_blocks_assemble_to_the_full_pass(ctx, n, p, blocks):
    """Symmetric integer M = A + A'. The 128-column partition of the distributed plan, a ragged last block and a single
    row at n = 300; two blocks that reach split-K (inner dimension >= 1024) at n = 1300. Every block has its own
    ldd = lds = n_rows + 3. Each block equals numpy, and the same rows of the full-mode call bit for bit."""
    rng = np.random.default_rng(n)
    A = rng.integers(-4, 5, size=(n, n)).astype(np.float64)
    M = A + A.T
    sigma = 2.0
    X, isb, c = make_inputs(rng, n, p, [(1, "zeros", False), (p - 1, "neg", True)])
    Dfull, Sfull = deriv_rows_call(ctx, M, n, n, 0, X, isb, c, sigma)
    check_against_numpy(M, 0, X, isb, c, sigma, Dfull, Sfull, f"full mode n={n}")
    for r0, nr in blocks:
        D, S = deriv_rows_call(ctx, np.asfortranarray(M[:, r0:r0 + nr]), n, nr, r0, X, isb, c, sigma, ld_out=nr + 3)
        check_against_numpy(M[r0:r0 + nr], r0, X, isb, c, sigma, D, S, f"row block ({r0}, {nr}) of n={n}")
        assert np.array_equal(D, Dfull[r0:r0 + nr]) and np.array_equal(S, Sfull[r0:r0 + nr]), (n, r0, nr)


# ---- deriv_var ---------------------------------------------------------------------------------------------------------
def deriv_var_call(ctx, Q, wv, S, scale, sub=True):
    n, k = Q.shape
    p = S.shape[1]
    dQ, pQ, ldq, _, _ = place(ctx, Q, sub)
    dS, pS, lds, _, _ = place(ctx, S, sub)
    dw = ctx.from_numpy(wv.reshape(k, 1))
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    var = np.full(p + 2, SENT)
    _lib.call("bigkrls_dev_deriv_var", ctx.handle, pQ, n, k, ldq, dw.ptr, pS, p, lds, scale.ctypes.data,
              var[1:].ctypes.data)
    assert var[0] == SENT and var[p + 1] == SENT
    return var[1:p + 1].copy()


@pytest.mark.parametrize("n,k,p", [(1, 1, 1), (257, 1, 3), (300, 255, 2), (300, 256, 33), (1000, 257, 5), (1100, 1000, 1)])
def test_deriv_var_exact(ctx, n, k, p):
    """Small shapes; p > 32 (the 64-wide tile) with k at the 256-thread stride of the column reduction and one past
    it; an inner dimension >= 1024 (split-K). |q_k' s| <= 32 n, so every term and the sum stay far below 2^53 in
    halves."""
    rng = np.random.default_rng(10000 + n + k + p)
    Q = rng.integers(-4, 5, size=(n, k)).astype(np.float64)
    S = rng.integers(-8, 9, size=(n, p)).astype(np.float64)
    wv = rng.choice(np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 0.0]), size=k)
    scale = 2.0 ** rng.integers(-6, 4, size=p)
    ref = scale * (wv[:, None] * (Q.T @ S) ** 2).sum(axis=0)
    assert np.abs(wv[:, None] * (Q.T @ S) ** 2).sum(axis=0).max() < 2.0 ** 52
    got = deriv_var_call(ctx, Q, wv, S, scale)
    assert np.array_equal(got, ref), (n, k, p, got, ref)


@pytest.mark.parametrize("n,k,p", [(257, 100, 3), (300, 256, 33), (1100, 1000, 2)])
def test_deriv_var_rounding_bound(ctx, n, k, p):
    """Standard normal Q and S, weights of mixed sign, against np.longdouble within the derived bound (module
    docstring)."""
    rng = np.random.default_rng(20000 + n + k + p)
    Q, S = rng.standard_normal((n, k)), rng.standard_normal((n, p))
    wv = rng.standard_normal(k)
    scale = np.exp(rng.standard_normal(p))
    T = Q.T.astype(L) @ S.astype(L)
    ref = scale.astype(L) * (wv.astype(L)[:, None] * T * T).sum(axis=0)
    Tabs, A = np.abs(T).astype(np.float64), np.abs(Q.T) @ np.abs(S)
    aw = np.abs(wv)[:, None]
    bound = scale * ((n + 16) * EPS * 2.0 * (aw * Tabs * A).sum(axis=0) + (k + 16) * EPS * (aw * Tabs * Tabs).sum(axis=0))
    got = deriv_var_call(ctx, Q, wv, S, scale)
    err = np.abs(got.astype(L) - ref).astype(np.float64)
    assert np.isfinite(got).all() and float(np.max(err / bound)) <= 1.0, (n, k, p, float(np.max(err / bound)))


# ---- argument checks -------------------------------------------------------------------------------------------------
def _rejected(name, *args):
    with pytest.raises(_lib.BigKRLSError) as e:
        _lib.call(name, *args)
    assert e.value.code == _lib.EINVAL, (name, e.value)
    assert name.replace("bigkrls_dev_", "") in str(e.value)


def test_deriv_rows_rejects_bad_arguments(ctx):
    """Every leading dimension that is too small, an empty or out-of-range row block and every null pointer:
    BIGKRLS_EINVAL with a message, before any launch -- sentinel-filled outputs stay as they were -- and the context
    computes the right answer afterwards."""
    rng = np.random.default_rng(3)
    n, p, nr, r0, sigma = 40, 3, 16, 8, 4.0
    A = rng.integers(-4, 5, size=(n, n)).astype(np.float64)
    M = A + A.T
    X, isb, c = make_inputs(rng, n, p, [(1, "01", False)])
    dK, dX, dc = ctx.from_numpy(np.asfortranarray(M[:, r0:r0 + nr])), ctx.from_numpy(X), ctx.from_numpy(c.reshape(n, 1))
    dD, dS = ctx.from_numpy(np.full((nr, p), SENT)), ctx.from_numpy(np.full((nr, p), SENT))
    ip = isb.ctypes.data
    h = ctx.handle
    good = dict(K=dK.ptr, n=n, nr=nr, ldk=n, r0=r0, X=dX.ptr, p=p, ldx=n, isb=ip, c=dc.ptr, D=dD.ptr, ldd=nr, S=dS.ptr, lds=nr)
    bad = [dict(ldk=n - 1), dict(ldx=n - 1), dict(ldd=nr - 1), dict(lds=nr - 1), dict(ldk=0), dict(ldd=0),
           dict(nr=0), dict(r0=n - nr + 1), dict(r0=-1), dict(n=0), dict(p=0),
           dict(K=None), dict(X=None), dict(isb=None), dict(c=None), dict(D=None), dict(S=None)]
    for change in bad:
        a = dict(good, **change)
        _rejected("bigkrls_dev_deriv_rows", h, a["K"], a["n"], a["nr"], a["ldk"], a["r0"], a["X"], a["p"], a["ldx"], a["isb"],
                  a["c"], sigma, a["D"], a["ldd"], a["S"], a["lds"])
        assert (dD.to_numpy() == SENT).all() and (dS.to_numpy() == SENT).all(), change
    D, S = deriv_rows_call(ctx, np.asfortranarray(M[:, r0:r0 + nr]), n, nr, r0, X, isb, c, sigma)
    check_against_numpy(M[r0:r0 + nr], r0, X, isb, c, sigma, D, S, "after the rejected calls")


def test_deriv_var_rejects_bad_arguments(ctx):
    rng = np.random.default_rng(4)
    n, k, p = 50, 7, 3
    Q = rng.integers(-4, 5, size=(n, k)).astype(np.float64)
    S = rng.integers(-8, 9, size=(n, p)).astype(np.float64)
    wv, scale = np.ones(k), np.ones(p)
    dQ, dS, dw = ctx.from_numpy(Q), ctx.from_numpy(S), ctx.from_numpy(wv.reshape(k, 1))
    var = np.full(p, SENT)
    good = dict(Q=dQ.ptr, n=n, k=k, ldq=n, w=dw.ptr, S=dS.ptr, p=p, lds=n, sc=scale.ctypes.data, var=var.ctypes.data)
    bad = [dict(ldq=n - 1), dict(lds=n - 1), dict(ldq=0), dict(n=0), dict(k=0), dict(p=0),
           dict(Q=None), dict(w=None), dict(S=None), dict(sc=None), dict(var=None)]
    for change in bad:
        a = dict(good, **change)
        _rejected("bigkrls_dev_deriv_var", ctx.handle, a["Q"], a["n"], a["k"], a["ldq"], a["w"], a["S"], a["p"], a["lds"],
                  a["sc"], a["var"])
        assert (var == SENT).all(), change
    assert np.array_equal(deriv_var_call(ctx, Q, wv, S, scale), ((Q.T @ S) ** 2).sum(axis=0))


# ---- ops.bDerivatives and bigkrls_derivmat -------------------------------------------------------------------------------
def _relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("n,p,binaries", [(150, 3, []), (257, 6, [(0, "neg", False), (4, "zeros", False)])])
def test_bderivatives_and_derivmat_agree_with_the_literal(ctx, lib, n, p, binaries):
    """ops.bDerivatives (V as factors: deriv_rows + deriv_var) and bigkrls_derivmat (V explicit) against the literal
    N^3 restatement of src/bigderiv_v3.cpp, at the tolerances of test_derivmat_matches_literal (1e-10 on D, 1e-8 on the
    variances). Both entries run the same kernels for D, so their D agree bit for bit; each derives the binary flags
    itself (ops.binary_columns / the loop in bigkrls_derivmat), and a {-0.0, 0.0, 1.0} column is binary for both and
    for the oracle."""
    rng = np.random.default_rng(500 + n)
    sigma = float(p)
    X = rng.standard_normal((n, p))
    for j, coding, single in binaries:
        X[:, j] = binary_column(rng, n, coding, single)
    K = orc.gauss_kernel_literal(X, sigma)
    vals, vecs = np.linalg.eigh(K)
    k = n // 2
    Q = np.ascontiguousarray(vecs[:, ::-1][:, :k])
    wv = rng.random(k) + 0.1
    V = (Q * wv) @ Q.T
    c = rng.standard_normal(n) / n
    D_ref, var_ref = orc.derivmat_literal(X, K, V, c, sigma)
    flags = ops.binary_columns(X)
    assert flags.tolist() == [orc.is_binary_column(X[:, j]) for j in range(p)] == [j in [b[0] for b in binaries] for j in range(p)]

    eig = ops.Eigenobject(values=vals[::-1].copy(), lastkeeper=k, vectors=ctx.from_numpy(Q),
                          values_dev=ctx.from_numpy(vals[::-1].copy()))
    out = ops.bDerivatives(ctx.from_numpy(X), sigma, ctx.from_numpy(K), ctx.from_numpy(c.reshape(n, 1)), eig, wv, X)
    D_ops, var_ops = out["derivatives"].to_numpy(), out["varavgderiv"]
    assert _relerr(D_ops, D_ref) < 1e-10
    assert np.max(np.abs(var_ops - var_ref) / np.abs(var_ref)) < 1e-8

    P = lambda a: C.c_void_p(a.ctypes.data)
    Xf, Kf, Vf, cf = np.asfortranarray(X), np.asfortranarray(K), np.asfortranarray(V), np.ascontiguousarray(c)
    D_l1, var_l1 = np.asfortranarray(np.full((n, p), np.nan)), np.full(p, np.nan)
    st = lib.bigkrls_derivmat(P(Xf), n, p, P(Kf), P(Vf), P(D_l1), P(var_l1), P(cf), sigma)
    assert st == 0, lib.bigkrls_last_error()
    assert np.array_equal(D_l1, D_ops)                     # (a differing binary flag would change a whole column)
    assert np.max(np.abs(var_l1 - var_ref) / np.abs(var_ref)) < 1e-8
