"""The four device eigensolver entries of include/bigkrls.h -- bigkrls_dev_eigen, bigkrls_dev_eigen_part,
bigkrls_dev_eigen_implicit, bigkrls_dev_eigen_auto -- on sub-blocks, by the method of test_gpu_gemm_core.py
(tests/_placement.py): A (or X) sits inside a NaN-filled parent, vecs inside a sentinel-filled one, with an odd leading
dimension and a first element that is 8- but not 16-byte aligned; one variant per group uses the even ld = n + 4, whose
block starts 16-byte aligned while its columns still do not follow each other packed. A kernel that indexes with n
instead of ldz, runs past its block or assumes aligned loads reads a NaN or overwrites the sentinel.

Reference, independent of the library: numpy.linalg.eigvalsh of the host matrix; orthogonality and residual on the host.
    dense paths (the bars of test_eigen_full / test_eigen_partial):
        |vals - lambda| <= 1e-12 max|lambda|,  max|Q'Q - I| < 1e-11,  max|A Q - Q diag(vals)| / max|lambda| < 1e-11
    block Lanczos, stored and implicit (the bars of test_eigen_block_lanczos_matches_dense_and_arpack):
        |vals - lambda| <= 1e-9 lambda_1,  max|Q'Q - I| < 1e-11
Only the kept columns 0 .. *h_n_vecs of the block are compared (the header specifies no others); they must be finite.

Packed against placed. Every case runs the same call packed under the same switches, prints max|difference| of values
and vectors and asserts BITWISE equality, on every path. The code reason, path by path:
  - dense: A is copied into the packed workspace W (copy_matrix) before anything else reads it; the reduction, the divide
    & conquer and gather_cols' source work on packed workspace. vecs enters with gather_cols (element-wise), the
    stage-2 back-transform kernels (bt2_block / bt2_wy / bt2_persistent / bt2_chain: scalar loads and stores at
    Z + r + c * ldz, nothing chosen by ldz or alignment) and the GEMMs of back_transform / back_transform_stage1 /
    back_transform_stage1_grouped, whose tile, split-K plan and load form depend on (m, n, k) only (csrc/gemm.hip,
    csrc/splitplan.h take no leading dimension and test no pointer).
  - block Lanczos on a stored matrix: A is read by gemm(A, lda) alone (k_times); vecs is written by copy_matrix, or by
    one gemm with ldc = ldv under BIGKRLS_KRY_REFINE=1.
  - implicit: X is read by col_means and shift_rows_sqnorms (one thread per column / row, the same order of additions
    for every ldx), which write the packed centred copy everything else works on.
No kernel was found that picks a form by ldz or alignment, so no comparison is relaxed to rounding.

The block Lanczos cases use P = 3 columns of data: at n = 1100 the iteration's subspace limit is n / 2 = 512 columns
(four steps), within which 64 pairs of a P = 6 kernel (lambda_64 / lambda_1 = 8e-3, 202 eigenvalues above 1e-3) reach a
residual of 2e-6 lambda_1 in exact arithmetic against the 1e-10 the iteration asks for: BIGKRLS_EIGK=krylov and the
implicit form end in BIGKRLS_ENOCONV there and never reach deliver(). With P = 3 (lambda_64 / lambda_1 = 1e-3) four
steps reach 1e-13. The shape, the 64 pairs and the routes are the same."""
import ctypes as C
import functools

import numpy as np
import pytest

from bigkrls_amd import _lib
from oracle import krls_oracle as orc

from _placement import SENT, place, take

pytestmark = pytest.mark.gpu

SWITCHES = ("BIGKRLS_EIG", "BIGKRLS_EIGK", "BIGKRLS_BT1", "BIGKRLS_BT2", "BIGKRLS_BT2_SEG", "BIGKRLS_S1", "BIGKRLS_DC",
            "BIGKRLS_KRY_REFINE")
ODD, EVEN = "odd_ld", "even_ld"
P_KRY = 3                                    # see the module docstring


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def _problem(n, p, seed, standardised=False):
    """(X, K, descending eigvalsh(K)) of orc.synth data; computed once, shared, read-only."""
    X, _ = orc.synth(n, p, seed)
    if standardised:                                          # as _block_lanczos_cases._data
        X = (X - X.mean(0)) / X.std(0, ddof=1)
    K = orc.gauss_kernel_literal(X, float(p))
    lam = np.linalg.eigvalsh(K)[::-1].copy()
    for a in (X, K, lam):
        a.setflags(write=False)
    return X, K, lam


def _ld(n, placement):
    return n + 4 if placement == EVEN else None               # None: place()'s odd default


class Result:
    pass


def _run(ctx, entry, M, n, n_vals, ncols, thresh, sub, placement=ODD, part=None, p=0, stored=True):
    """One call of `entry`. M: the host matrix A (n x n), or the data X (n x p) for the operator forms. Returns the
    values, the n x ncols block of vecs (after the sentinel check around it) and the counts."""
    ld = _ld(n, placement) if sub else None
    dM, pM, ldm, _, _ = place(ctx, np.asarray(M), sub=sub, fill=np.nan, ld=ld)
    dV, pV, ldv, r0, c0 = place(ctx, np.full((n, ncols), np.nan), sub=sub, fill=SENT, ld=ld)
    if sub and placement == EVEN:
        assert ldv == n + 4 and (dV.t.data_ptr() + 8 * (ldv + 2)) % 16 == 0
    before = np.array(dM.to_numpy())
    vals = ctx.zeros(n_vals, 1)
    nv, nvals = C.c_int64(-1), C.c_int64(-1)
    h = ctx.handle
    error = None
    try:
        if entry == "eigen":
            _lib.call("bigkrls_dev_eigen", h, pM, n, ldm, n_vals, vals.ptr, ncols, float(thresh), pV, ldv, C.byref(nv))
        elif entry == "part":
            _lib.call("bigkrls_dev_eigen_part", h, pM, n, ldm, n_vals, vals.ptr, ncols, float(thresh), pV, ldv,
                      C.byref(nv), int(part[0]), int(part[1]))
        elif entry == "implicit":
            _lib.call("bigkrls_dev_eigen_implicit", h, pM, n, ldm, p, float(p), n_vals, vals.ptr, ncols, float(thresh),
                      pV, ldv, C.byref(nv))
        elif entry == "auto" and stored:
            _lib.call("bigkrls_dev_eigen_auto", h, pM, n, ldm, None, n, 0, 1.0, float(thresh), n_vals, vals.ptr, pV, ldv,
                      C.byref(nvals), C.byref(nv))
        elif entry == "auto":
            _lib.call("bigkrls_dev_eigen_auto", h, None, n, n, pM, ldm, p, float(p), float(thresh), n_vals, vals.ptr, pV,
                      ldv, C.byref(nvals), C.byref(nv))
        else:
            raise ValueError(entry)
    except _lib.BigKRLSError as e:
        error = e
    out = Result()
    what = (entry, n, n_vals, ncols, thresh, placement, part)
    # (also after an error: whatever the call returns, it writes nothing around the block and leaves its input alone)
    out.vecs = take(dV, r0, c0, n, ncols, what) if sub else np.array(dV.to_numpy())
    assert np.array_equal(np.array(dM.to_numpy()), before, equal_nan=True), (what, "the input was changed")
    if error is not None:
        raise error
    out.nv = int(nv.value)
    out.nvals = int(nvals.value) if entry == "auto" else n_vals
    out.vals = vals.to_numpy().ravel()[:out.nvals].copy()
    assert 0 <= out.nv <= ncols and 0 < out.nvals <= n_vals, what
    return out


def _watched(ctx, name, fn):
    """fn() with the context's recovery counters watched, as the digest helpers do: a watchdog replay runs other
    kernels than the case is about, so the case is run once more; counters that move twice in a row are a failure."""
    for _attempt in range(2):
        before = ctx.counters()
        res = fn()
        if ctx.counters() == before:
            return res
    raise AssertionError(f"{name}: the context's recovery counters moved in two runs in a row: {before} -> {ctx.counters()}")


def _pair(ctx, name, entry, M, n, n_vals, ncols, thresh, placement, **kw):
    """(packed, placed) results of one call; prints their differences and asserts that there are none (module docstring)."""
    packed, placed = _watched(ctx, name, lambda: (_run(ctx, entry, M, n, n_vals, ncols, thresh, False, **kw),
                                                  _run(ctx, entry, M, n, n_vals, ncols, thresh, True, placement, **kw)))
    assert placed.nv == packed.nv and placed.nvals == packed.nvals, (name, placed.nv, packed.nv, placed.nvals, packed.nvals)
    k = placed.nv
    dvals = float(np.max(np.abs(placed.vals - packed.vals)))
    dvecs = float(np.max(np.abs(placed.vecs[:, :k] - packed.vecs[:, :k]))) if k else 0.0
    print(f"{name} [{placement}]: packed vs placed max|d vals| = {dvals:.3e}, max|d vecs| = {dvecs:.3e} ({k} columns)")
    assert np.array_equal(placed.vals, packed.vals), (name, dvals)
    assert np.array_equal(placed.vecs[:, :k], packed.vecs[:, :k]), (name, dvecs)
    return packed, placed


def _lastkeeper(vals, thresh, cap):
    """bEigen's rule on the returned values: max(which(values >= eigtrunc * values[1])), capped."""
    if thresh < 0:
        return cap
    keep = np.nonzero(vals >= thresh * vals[0])[0]
    return min(int(keep[-1]) + 1 if keep.size else 0, cap)


def _check_dense(name, K, lam, out, thresh, ncols):
    scale = np.abs(lam).max()
    nvals = len(out.vals)
    print(f"{name}: max|vals - eigvalsh| / max|lambda| = {np.max(np.abs(out.vals - lam[:nvals])) / scale:.3e}")
    assert np.max(np.abs(out.vals - lam[:nvals])) <= 1e-12 * scale, name
    assert np.all(np.diff(out.vals) <= 0), name
    assert out.nv == _lastkeeper(out.vals, thresh, ncols), (name, out.nv)
    Q = out.vecs[:, :out.nv]
    assert np.isfinite(Q).all(), (name, "padding was read")
    orth = np.max(np.abs(Q.T @ Q - np.eye(out.nv)))
    resid = np.max(np.abs(K @ Q - Q * out.vals[:out.nv])) / scale
    print(f"{name}: max|Q'Q - I| = {orth:.3e}, max|A Q - Q diag(vals)| / max|lambda| = {resid:.3e}")
    assert orth < 1e-11 and resid < 1e-11, (name, orth, resid)


def _check_lanczos(name, lam, out, thresh, ncols):
    nvals = len(out.vals)
    print(f"{name}: max|vals - eigvalsh| / lambda_1 = {np.max(np.abs(out.vals - lam[:nvals])) / lam[0]:.3e}")
    assert np.max(np.abs(out.vals - lam[:nvals])) <= 1e-9 * lam[0], name
    assert out.nv == _lastkeeper(out.vals, thresh, ncols), (name, out.nv)
    Q = out.vecs[:, :out.nv]
    assert np.isfinite(Q).all(), (name, "padding was read")
    orth = np.max(np.abs(Q.T @ Q - np.eye(out.nv)))
    print(f"{name}: max|Q'Q - I| = {orth:.3e}")
    assert orth < 1e-11, (name, orth)


# ---- one-stage path: gather_cols, back_transform ------------------------------------------------------------------------
@pytest.mark.parametrize("n,env,placement", [(65, {}, ODD), (200, {}, ODD), (200, {}, EVEN),
                                             (300, {"BIGKRLS_EIG": "1stage"}, ODD)])
def test_one_stage_all_vectors(ctx, monkeypatch, n, env, placement):
    """n <= 256 by default and n = 300 under BIGKRLS_EIG=1stage: gather_cols and the panel GEMMs of back_transform write
    vecs with ldv."""
    _setenv(monkeypatch, env)
    _, K, lam = _problem(n, 3, 9)
    name = f"one-stage n={n} {env}"
    _, placed = _pair(ctx, name, "eigen", K, n, n, n, -1.0, placement)
    _check_dense(name, K, lam, placed, -1.0, n)


# ---- two-stage path: every form of the stage-2 back-transform, both of stage 1 ------------------------------------------
BT_FORMS = {
    "default": {},
    "wavefront": {"BIGKRLS_BT2": "wavefront"},
    "chain": {"BIGKRLS_BT2": "chain"},
    "chain3": {"BIGKRLS_BT2": "chain", "BIGKRLS_BT2_SEG": "3"},
    "seq": {"BIGKRLS_BT2": "seq", "BIGKRLS_BT1": "panel", "BIGKRLS_S1": "gemm"},
}


@pytest.mark.parametrize("form,placement", [(f, ODD) for f in BT_FORMS] + [("default", EVEN)])
def test_two_stage_all_vectors(ctx, monkeypatch, form, placement):
    """n = 700, the forms of test_eigen_back_transform_variants: bt2_persistent (default), bt2_wy per anti-diagonal,
    bt2_chain with its LDS window (whole chains and segments of three), bt2_block with the panel-by-panel stage-1
    back-transform; the default stage-1 form is back_transform_stage1_grouped."""
    _setenv(monkeypatch, BT_FORMS[form])
    n = 700
    _, K, lam = _problem(n, 4, 23)
    name = f"two-stage n={n} {form}"
    _, placed = _pair(ctx, name, "eigen", K, n, n, n, -1.0, placement)
    _check_dense(name, K, lam, placed, -1.0, n)


# ---- few vectors: the factored / explicit top of the divide & conquer, lastkeeper counted by the threshold ---------------
@pytest.mark.parametrize("env,thresh,placement", [({"BIGKRLS_DC": "factored"}, -1.0, ODD),
                                                  ({"BIGKRLS_DC": "factored"}, -1.0, EVEN),
                                                  ({"BIGKRLS_DC": "explicit"}, -1.0, ODD),
                                                  ({}, 0.001, ODD)])
def test_few_vectors(ctx, monkeypatch, env, thresh, placement):
    """n = 1100, all values, at most 100 vectors: the back-transforms run on a 100-column slab of vecs (two 64-column
    slabs, the second partial). keep_thresh = 0.001: lastkeeper (65 by the host spectrum) is counted by the threshold."""
    _setenv(monkeypatch, env)
    n, cap = 1100, 100
    _, K, lam = _problem(n, 3, 31, True)
    name = f"few vectors n={n} {env} keep_thresh={thresh}"
    _, placed = _pair(ctx, name, "eigen", K, n, n, cap, thresh, placement)
    if thresh >= 0:
        assert 0 < placed.nv < cap, (name, placed.nv)            # (the count is the threshold's, not the cap's)
    _check_dense(name, K, lam, placed, thresh, cap)


# ---- the column partition ---------------------------------------------------------------------------------------------
def _partition(ctx, name, K, lam, n, n_vals, cap, parts, placement, check):
    """Every part of `parts`, placed: the other parts' columns exactly 0 inside the block, the surroundings intact (take),
    the sum of the blocks equal to the part_count = 1 result, as test_eigen_column_partition_sums_to_full checks it."""
    _, full = _pair(ctx, name + " part 0/1", "part", K, n, n_vals, cap, -1.0, placement, part=(0, 1))
    check(name + " part 0/1", full)
    nv = full.nv
    acc = np.zeros((n, nv))
    for r in range(parts):
        _, part = _pair(ctx, f"{name} part {r}/{parts}", "part", K, n, n_vals, cap, -1.0, placement, part=(r, parts))
        assert part.nv == nv and np.array_equal(part.vals, full.vals), (name, r)
        c0, c1 = nv * r // parts, nv * (r + 1) // parts
        Qp = part.vecs[:, :nv]
        assert not Qp[:, :c0].any() and not Qp[:, c1:].any(), (name, r, "the other parts' columns are not zero")
        assert np.isfinite(Qp).all(), (name, r)
        acc += Qp
    assert np.array_equal(acc, full.vecs[:, :nv]), name


@pytest.mark.parametrize("placement", [ODD, EVEN])
def test_partition_dense(ctx, placement):
    """bigkrls_dev_eigen_part, n = 700, at most 100 vectors, three parts (DenseEig::back_transform_slice)."""
    n, cap = 700, 100
    _, K, lam = _problem(n, 4, 11, True)
    name = f"partition dense n={n}"
    _partition(ctx, name, K, lam, n, n, cap, 3, placement, lambda nm, out: _check_dense(nm, K, lam, out, -1.0, cap))


def test_partition_part_that_owns_no_column(ctx):
    """Two vectors over three parts: part 0 owns [0, 0). Both columns are zeros, nothing around them is touched, and the
    values are all there."""
    n = 700
    _, K, lam = _problem(n, 4, 11, True)
    name = "partition dense n=700, 2 vectors, part 0/3"
    _, placed = _pair(ctx, name, "part", K, n, n, 2, -1.0, ODD, part=(0, 3))
    assert placed.nv == 2 and not placed.vecs.any(), name
    assert np.max(np.abs(placed.vals - lam)) <= 1e-12 * np.abs(lam).max(), name


def test_partition_block_lanczos(ctx, monkeypatch):
    """The same on the block Lanczos path (BlockLanczos::deliver), two parts."""
    monkeypatch.setenv("BIGKRLS_EIGK", "krylov")
    n, k = 1100, 64
    _, K, lam = _problem(n, P_KRY, 31, True)
    name = f"partition block Lanczos n={n}"
    _partition(ctx, name, K, lam, n, k, k, 2, ODD, lambda nm, out: _check_lanczos(nm, lam, out, -1.0, k))


# ---- block Lanczos on a stored matrix ----------------------------------------------------------------------------------
@pytest.mark.parametrize("env,placement", [({}, ODD), ({}, EVEN), ({"BIGKRLS_KRY_REFINE": "1"}, ODD)])
def test_block_lanczos_stored(ctx, monkeypatch, env, placement):
    """BIGKRLS_EIGK=krylov, n = 1100, 64 pairs: A is read with lda by the products K B_j; deliver() writes vecs with
    copy_matrix, under BIGKRLS_KRY_REFINE=1 with the GEMM of the Rayleigh-Ritz step (ldc = ldv)."""
    monkeypatch.setenv("BIGKRLS_EIGK", "krylov")
    _setenv(monkeypatch, env)
    n, k = 1100, 64
    _, K, lam = _problem(n, P_KRY, 31, True)
    name = f"block Lanczos stored n={n} {env}"
    _, placed = _pair(ctx, name, "eigen", K, n, k, k, -1.0, placement)
    assert placed.nv == k
    _check_lanczos(name, lam, placed, -1.0, k)


@pytest.mark.parametrize("entry", ["eigen", "implicit"])
def test_block_lanczos_p6_shape_whichever_way_it_ends(ctx, monkeypatch, entry):
    """n = 1100, P = 6, 64 pairs (module docstring): the iteration is not expected to converge within its 512 columns.
    If it ends in BIGKRLS_ENOCONV, the placed call has still written nothing around the block of vecs and left its
    input alone (checked by _run before the error is raised); should it converge one day, the checks of the P = 3
    cases apply."""
    monkeypatch.setenv("BIGKRLS_EIGK", "krylov")
    n, k, p = 1100, 64, 6
    X, K, lam = _problem(n, p, 31, True)
    name = f"block Lanczos P=6 n={n} {entry}"
    try:
        placed = _watched(ctx, name, lambda: _run(ctx, entry, K if entry == "eigen" else X, n, k, k, -1.0, True, ODD, p=p))
    except _lib.BigKRLSError as err:
        print(f"{name}: {err}")
        assert err.code == _lib.ENOCONV, (name, str(err))
        return
    _check_lanczos(name, lam, placed, -1.0, k)


# ---- the operator form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", [ODD, EVEN])
def test_implicit(ctx, placement):
    """bigkrls_dev_eigen_implicit, n = 1100, 64 pairs: X inside a NaN-filled parent (ldx > n), vecs placed; the host
    matrix is the literal Gaussian kernel of the same X."""
    n, k = 1100, 64
    X, _, lam = _problem(n, P_KRY, 31, True)
    name = f"implicit n={n}"
    _, placed = _pair(ctx, name, "implicit", X, n, k, k, -1.0, placement, p=P_KRY)
    assert placed.nv == k
    _check_lanczos(name, lam, placed, -1.0, k)


# ---- auto rank ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stored,placement", [(True, ODD), (True, EVEN), (False, ODD)])
def test_auto(ctx, stored, placement):
    """bigkrls_dev_eigen_auto with keep_thresh = 0.001 and a cap of 128, on the stored matrix placed and on X placed: the
    same *h_n_vals and *h_n_vecs as the packed call (asserted by _pair), *h_n_vals = *h_n_vecs + 1, the rank that of the
    host spectrum."""
    n, cap, tau = 1100, 128, 0.001
    X, K, lam = _problem(n, P_KRY, 31, True)
    name = f"auto n={n} {'stored' if stored else 'operator'}"
    _, placed = _pair(ctx, name, "auto", K if stored else X, n, cap, cap, tau, placement, p=P_KRY, stored=stored)
    assert placed.nvals == placed.nv + 1, (name, placed.nvals, placed.nv)
    ratios = lam[:cap] / lam[0]
    if np.min(np.abs(ratios - tau)) > 1e-6:                       # (no eigenvalue sits on the threshold)
        assert placed.nv == int((ratios >= tau).sum()), (name, placed.nv)
    _check_lanczos(name, lam, placed, tau, cap)


# ---- refusals: nothing is launched, nothing is written --------------------------------------------------------------------
def _refused(ctx, names_what, call):
    """`call(pV, ldv_true)` must end in BIGKRLS_EINVAL with a message that names the leading dimension, and leave the
    (sentinel-filled, packed) eigenvector buffer as it was."""
    n = names_what[1]
    dV = ctx.from_numpy(np.full((n, 4), SENT, order="F"))
    with pytest.raises(_lib.BigKRLSError) as err:
        call(dV)
    assert err.value.code == _lib.EINVAL, (names_what, str(err.value))
    assert "leading dimension" in str(err.value) and names_what[2] in str(err.value), (names_what, str(err.value))
    assert (np.array(dV.to_numpy()) == SENT).all(), (names_what, "vecs was touched by a refused call")


@pytest.mark.parametrize("short", ["lda", "ldv"])
@pytest.mark.parametrize("entry", ["eigen", "part", "implicit", "auto_stored", "auto_operator"])
def test_short_leading_dimension_is_refused_by_name(ctx, entry, short):
    """lda (ldx for the operator forms) = n - 1 and ldv = n - 1: BIGKRLS_EINVAL, the message names the leading dimension
    and the operand, vecs is untouched. (The other arguments are valid; nothing is launched.)"""
    operator = entry in ("implicit", "auto_operator")
    n, p, k = (1100, 3, 4) if operator else (65, 3, 4)
    rng = np.random.default_rng(5)
    if operator:
        dM = ctx.from_numpy(np.asfortranarray(rng.standard_normal((n, p))))
    else:
        S = rng.standard_normal((n, n))
        dM = ctx.from_numpy(np.asfortranarray(S + S.T))
    ldm = n - 1 if short == "lda" else n
    vals = ctx.zeros(n, 1)
    nv, nvals = C.c_int64(-1), C.c_int64(-1)
    h = ctx.handle

    def call(dV):
        ldv = n - 1 if short == "ldv" else n
        if entry == "eigen":
            _lib.call("bigkrls_dev_eigen", h, dM.ptr, n, ldm, n, vals.ptr, k, -1.0, dV.ptr, ldv, C.byref(nv))
        elif entry == "part":
            _lib.call("bigkrls_dev_eigen_part", h, dM.ptr, n, ldm, n, vals.ptr, k, -1.0, dV.ptr, ldv, C.byref(nv), 1, 3)
        elif entry == "implicit":
            _lib.call("bigkrls_dev_eigen_implicit", h, dM.ptr, n, ldm, p, float(p), k, vals.ptr, k, -1.0, dV.ptr, ldv,
                      C.byref(nv))
        elif entry == "auto_stored":
            _lib.call("bigkrls_dev_eigen_auto", h, dM.ptr, n, ldm, None, n, 0, 1.0, 0.001, k, vals.ptr, dV.ptr, ldv,
                      C.byref(nvals), C.byref(nv))
        else:
            _lib.call("bigkrls_dev_eigen_auto", h, None, n, n, dM.ptr, ldm, p, float(p), 0.001, k, vals.ptr, dV.ptr, ldv,
                      C.byref(nvals), C.byref(nv))

    operand = "vecs" if short == "ldv" else (" of X" if operator else " of A")
    _refused(ctx, (entry, n, operand, short), call)
    assert not vals.to_numpy().any(), (entry, short, "vals was touched by a refused call")
