"""The fused kernel-tile entries of csrc/gemm.hip on sub-blocks: bigkrls_dev_kernel_block (all four arms of kb_plan),
bigkrls_dev_kernel_contract (narrow and wide, both trans), _contract_grouped, _loo_colsums, _loo_binsums, _loo_moments.

Every case makes a PACKED call (every operand a matrix of its own, ld = rows) and PLACED calls (tests/_placement.py: every
device operand inside a NaN-filled parent, the output inside a sentinel-filled one whose surroundings must still hold
the sentinel afterwards), and asserts

1. placed == packed BIT FOR BIT. Nothing in the arithmetic may depend on a leading dimension: A and B are copied into
   packed, centred copies by col_means and shift_rows_sqnorms (one thread per column or row, the same order of additions
   for every lda), the plans are functions of the shapes and of the device only, and W and out are only addressed with
   their leading dimensions. Placements (of every operand of the call, the output included):
       odd              odd ld, first element 8- but not 16-byte aligned      (scalar stores)
       even-aligned     even ld > rows, first element 16-byte aligned         (vector stores with ldo != rows)
       even-misaligned  even ld, first element 8- but not 16-byte aligned     (scalar stores although ldo is even)
   kernel_block, whose store code looks at the alignment, is held to all three; the other entries to the first two.
   ACHIEVED on the MI355X: bitwise for every entry, arm and placement below; no case had to be moved to the bound.
2. packed within the project's bound of a direct sum in np.longdouble:
       kernel_block     _bound of tests/test_gpu_kernel_build.py
       kernel_contract  bK @ |W| + (L + 8) 2^-53 (K @ |W|), L the loop length (test_kernel_contract_uncentred)
   and beside the GPU's error / bound the test prints that of a float64 numpy restatement of the same formula (column
   means of A subtracted, norms expanded, clamped at 0). The grouped and leave-out entries have extended-precision tests
   of their own (test_gpu_group_effects.py, test_gpu_partial_dependence.py, test_gpu_accumulated_effects.py,
   test_gpu_conditional_effects.py): here bitwise equality with the packed call.
   Worst error / bound on the MI355X, the float64 restatement's worst in brackets:
       kernel_block             0.145   (0.108)    KB_SYM_WAVE n = 70, p = 5; the tiled arm 0.068 (0.057)
       kernel_contract narrow   0.0328  (0.0328)   trans = 0, p = 3, q = 40;  trans = 1: 8.5e-4 (1.3e-3)
       kernel_contract wide     0.0364  (0.0335)   trans = 0, p = 3, q = 130; trans = 1: 1.2e-3 (1.3e-3)
3. a leading dimension one short of the row count is BIGKRLS_EINVAL for every entry and every ld, and the context stays
   usable.

Shapes: the smallest at which each arm of kb_plan (csrc/ktplan.h) still has interior and edge tiles; the contractions on
the operands of tests/_fused_tile_cases.py (U = 1100 loop rows: trans = 1 cuts the loop into partial sums added by
contract_reduce_kernel, trans = 0 does not)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from bigkrls_amd import _lib

import _fused_tile_cases as cases
from _placement import SENT, place, placements, take

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
L = np.longdouble


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


kb = _load("_kernel_build_for_tile_placement", "test_gpu_kernel_build.py")     # _literal_ld, _bound

ALL3 = ("odd", "even-aligned", "even-misaligned")
TWO = ("odd", "even-aligned")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def put(ctx, block, how, fill=np.nan):
    """how = None: packed; else a name of _placement.placements. (parent, pointer, ld, r0, c0)"""
    if how is None:
        return place(ctx, block, sub=False)
    return place(ctx, block, fill=fill, **placements(block.shape[0])[how])


def out_block(ctx, r, c, how):
    return put(ctx, np.full((r, c), SENT), how, fill=SENT)


def result(o, r, c, how, what):
    blk = np.array(o[0].to_numpy()) if how is None else take(o[0], o[3], o[4], r, c, (what, how))
    assert np.all(blk != SENT), (what, how, "an entry was never written")
    return blk


def ratio(got, ref, bound):
    return float(np.max((np.abs(got.astype(L) - ref) / bound).astype(np.float64)))


def restated_kernel(A, B, sigma):
    """float64 numpy, the library's formula: both operands moved by the column means of A, |a|^2 + |b|^2 - 2 a.b clamped
    at 0"""
    mu = A.mean(axis=0)
    a, b = A - mu, B - mu
    d2 = np.maximum(np.sum(a * a, axis=1)[:, None] + np.sum(b * b, axis=1)[None, :] - 2.0 * (a @ b.T), 0.0)
    return np.exp(-d2 / sigma)


# ---- kernel_block -------------------------------------------------------------------------------------------------------
def run_kernel_block(ctx, A, B, sigma, how, form, c0=0):
    """form "sym": B is the placed A itself (diag_shift 0); "cols": B = rows [c0, c0 + v) of the placed A, same parent and
    ld (diag_shift c0); "rect": B an operand of its own (diag_shift -1)."""
    u, p = A.shape
    v = B.shape[0]
    a = put(ctx, A, how)
    if form == "rect":
        b = put(ctx, B, how)
        bptr, ldb, shift = b[1], b[2], -1
    else:
        bptr, ldb, shift = C.c_void_p(a[1].value + 8 * c0), a[2], c0
    o = out_block(ctx, u, v, how)
    _lib.call("bigkrls_dev_kernel_block", ctx.handle, a[1], u, a[2], bptr, v, ldb, p, float(sigma), o[1], o[2], shift)
    return result(o, u, v, how, f"kernel_block {form} u={u} v={v} p={p}")


KB_CASES = {
    "sym_wave": dict(form="sym", u=70, v=70, p=5),
    "wave": dict(form="rect", u=70, v=45, p=5),
    "wave_cols": dict(form="cols", u=70, v=40, p=5, c0=13),
    "generic": dict(form="rect", u=140, v=70, p=130),
    "generic_sym": dict(form="sym", u=140, v=140, p=130),
    "tiled_sym": dict(form="sym", u=1030, v=1030, p=33),
    "tiled": dict(form="rect", u=1030, v=1100, p=33),
}


@pytest.mark.parametrize("name", sorted(KB_CASES))
def test_kernel_block_placed(ctx, name):
    c = KB_CASES[name]
    form, u, v, p, c0 = c["form"], c["u"], c["v"], c["p"], c.get("c0", 0)
    rng = np.random.default_rng(sum(map(ord, name)) + p)
    A = rng.standard_normal((u, p))
    B = rng.standard_normal((v, p)) if form == "rect" else A[c0:c0 + v]
    sigma = float(p)
    packed = run_kernel_block(ctx, A, B, sigma, None, form, c0)
    ref = kb._literal_ld(A, B, sigma)
    bound = kb._bound(A, B, sigma, ref)
    r_gpu, r_np = ratio(packed, ref, bound), ratio(restated_kernel(A, B, sigma), ref, bound)
    print(f"kernel_block {name}: error / bound GPU {r_gpu:.3g}, float64 numpy restatement {r_np:.3g}")
    assert np.isfinite(packed).all() and r_gpu <= 1.0, (name, r_gpu)
    j = np.arange(v)
    for how in ALL3:
        got = run_kernel_block(ctx, A, B, sigma, how, form, c0)
        assert same_bits(got, packed), (name, how, "placed != packed", int(np.sum(got != packed)))
        if form != "rect":
            assert np.all(got[c0 + j, j] == 1.0), (name, how, "the diagonal is not exactly 1")
        if form == "sym":
            assert np.array_equal(got, got.T), (name, how)


# ---- kernel_contract ------------------------------------------------------------------------------------------------------
_host = {}


def host_operands(ctx, p, q):
    """the operands of tests/_fused_tile_cases.py on the host: A (U x p), B (V x p), WA (U x q), WB (V x q)"""
    if (p, q) not in _host:
        _host[(p, q)] = tuple(np.array(d.to_numpy()) for d in cases.operands(ctx, p, q))
    return _host[(p, q)]


_kref = {}


def kernel_reference(ctx, p):
    """K(A, B) in longdouble with its elementwise bound and the float64 restatement, once per p"""
    if p not in _kref:
        A, B, _, _ = host_operands(ctx, p, 0)
        K = kb._literal_ld(A, B, float(p))
        _kref[p] = (K, kb._bound(A, B, float(p), K), restated_kernel(A, B, float(p)))
    return _kref[p]


def run_contract(ctx, A, B, W, sigma, trans, how):
    u, p = A.shape
    v, q = B.shape[0], W.shape[1]
    ns = v if trans else u
    a, b, w = put(ctx, A, how), put(ctx, B, how), put(ctx, W, how)
    o = out_block(ctx, ns, q, how)
    _lib.call("bigkrls_dev_kernel_contract", ctx.handle, a[1], u, a[2], b[1], v, b[2], p, float(sigma), w[1], q, w[2],
              int(trans), o[1], o[2])
    return result(o, ns, q, how, f"kernel_contract p={p} q={q} trans={trans}")


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("q", cases.QS_NARROW + cases.QS_WIDE)
@pytest.mark.parametrize("p", cases.PS)
def test_kernel_contract_placed(ctx, p, q, trans):
    A, B, WA, WB = host_operands(ctx, p, q)
    W = WA if trans else WB
    packed = run_contract(ctx, A, B, W, float(p), trans, None)
    K, bK, K64 = kernel_reference(ctx, p)
    if trans:
        K, bK, K64 = K.T, bK.T, K64.T
    Wl = np.abs(W).astype(L)
    ref = K @ W.astype(L)
    bound = bK @ Wl + (K.shape[1] + 8) * L(2.0) ** -53 * (K @ Wl)
    r_gpu, r_np = ratio(packed, ref, bound), ratio(K64 @ W, ref, bound)
    print(f"kernel_contract {'wide' if q > 64 else 'narrow'} p={p} q={q} trans={trans}: error / bound GPU {r_gpu:.3g}, "
          f"float64 numpy restatement {r_np:.3g}")
    assert np.isfinite(packed).all() and r_gpu <= 1.0, (p, q, trans, r_gpu)
    for how in TWO:
        got = run_contract(ctx, A, B, W, float(p), trans, how)
        assert same_bits(got, packed), (p, q, trans, how, "placed != packed", int(np.sum(got != packed)))


# ---- kernel_contract_grouped ---------------------------------------------------------------------------------------------
def run_grouped(ctx, A, B, W, sigma, lab, G, how):
    u, p = A.shape
    v, q = B.shape[0], W.shape[1]
    a, b, w = put(ctx, A, how), put(ctx, B, how), put(ctx, W, how)
    o = out_block(ctx, v, G * q, how)
    lab = np.ascontiguousarray(lab, dtype=np.int64)
    _lib.call("bigkrls_dev_kernel_contract_grouped", ctx.handle, a[1], u, a[2], b[1], v, b[2], p, float(sigma), w[1], q,
              w[2], lab.ctypes.data, G, o[1], o[2])
    return result(o, v, G * q, how, f"kernel_contract_grouped p={p} q={q}")


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("q", cases.QS_NARROW)
@pytest.mark.parametrize("p", cases.PS)
def test_kernel_contract_grouped_placed(ctx, p, q, shuffled):
    """Sorted labels: the tile kernel reads W with ldw; shuffled labels: contract_gather_kernel reads it (and A's copy)
    into group order. The empty group's columns are zeros, written, not left."""
    A, B, WA, _ = host_operands(ctx, p, q)
    lab = cases.labels(shuffled)
    packed = run_grouped(ctx, A, B, WA, float(p), lab, cases.GROUPS, None)
    assert np.isfinite(packed).all()
    assert np.all(packed[:, q:2 * q] == 0.0)                                  # group 1 is empty
    for how in TWO:
        got = run_grouped(ctx, A, B, WA, float(p), lab, cases.GROUPS, how)
        assert same_bits(got, packed), (p, q, shuffled, how, "placed != packed", int(np.sum(got != packed)))


# ---- the leave-out entries ------------------------------------------------------------------------------------------------
def run_loo(ctx, entry, A, B, sigma, how, ncols_out, *host_args):
    u, p = A.shape
    v = B.shape[0]
    a, b = put(ctx, A, how), put(ctx, B, how)
    o = out_block(ctx, v, ncols_out, how)
    _lib.call(entry, ctx.handle, a[1], u, a[2], b[1], v, b[2], p, float(sigma), *host_args, o[1], o[2])
    return result(o, v, ncols_out, how, f"{entry} p={p}")


@pytest.mark.parametrize("p", cases.PS)
def test_kernel_loo_colsums_placed(ctx, p):
    A, B, _, _ = host_operands(ctx, p, 0)
    cols = np.ascontiguousarray(cases.loo_cols(p), dtype=np.int64)
    args = (cols.ctypes.data, int(cols.size))
    packed = run_loo(ctx, "bigkrls_dev_kernel_loo_colsums", A, B, float(p), None, cols.size, *args)
    assert np.isfinite(packed).all()
    for how in TWO:
        got = run_loo(ctx, "bigkrls_dev_kernel_loo_colsums", A, B, float(p), how, cols.size, *args)
        assert same_bits(got, packed), (p, how, "placed != packed", int(np.sum(got != packed)))


@pytest.mark.parametrize("in_order", [True, False], ids=["in_order", "scattered"])
@pytest.mark.parametrize("p", cases.PS)
def test_kernel_loo_moments_placed(ctx, p, in_order):
    """In order: the launches write their columns into out; scattered: through the staging buffer and
    loo_moments_scatter_kernel."""
    A, B, _, _ = host_operands(ctx, p, 0)
    ent = np.ascontiguousarray(np.asarray(cases.loo_entries(p, in_order), dtype=np.int64).reshape(-1, 3))
    args = (ent.ctypes.data, int(ent.shape[0]))
    packed = run_loo(ctx, "bigkrls_dev_kernel_loo_moments", A, B, float(p), None, ent.shape[0], *args)
    assert np.isfinite(packed).all()
    for how in TWO:
        got = run_loo(ctx, "bigkrls_dev_kernel_loo_moments", A, B, float(p), how, ent.shape[0], *args)
        assert same_bits(got, packed), (p, in_order, how, "placed != packed", int(np.sum(got != packed)))


def binsums_labels():
    """Two selected columns: 3 bins of 1090, 0 and 10 rows (long enough to be cut into segments; empty; fewer than 16), and
    5 bins of 600, 250, 200, 43 and 7 rows; both from a seeded shuffle."""
    rng = np.random.default_rng(11)
    three = np.repeat([0, 2], [cases.U - 10, 10])[rng.permutation(cases.U)]
    five = np.repeat(np.arange(5), [600, 250, 200, 43, 7])[rng.permutation(cases.U)]
    assert five.size == cases.U
    return np.stack([three, five], axis=1).astype(np.int64), np.array([3, 5], dtype=np.int64)


@pytest.mark.parametrize("p", [3, 20, 37])
def test_kernel_loo_binsums_placed(ctx, p):
    """No digest pins this entry: two packed calls must give the same bits as well. The bins of a column add up to
    kernel_loo_colsums' sum of that column: U positive terms in another order, (U + 8) 2^-53 relative for each of the two
    sums, plus twice a term's own error by _bound of tests/test_gpu_kernel_build.py, ((p + 12) D + 4) 2^-53 with
    D = (|a| + |b|)^2 / sigma <= 8 (entries within +-1.2, centred: |a|^2 <= 1.44 p up to the means, sigma = p)."""
    A, B, _, _ = host_operands(ctx, p, 0)
    lab, nbins = binsums_labels()
    cols = np.array([0, p - 1], dtype=np.int64)
    labcm = np.ascontiguousarray(lab.T)                                       # column-major u x n_cols
    args = (cols.ctypes.data, 2, labcm.ctypes.data, nbins.ctypes.data)
    packed = run_loo(ctx, "bigkrls_dev_kernel_loo_binsums", A, B, float(p), None, 8, *args)
    again = run_loo(ctx, "bigkrls_dev_kernel_loo_binsums", A, B, float(p), None, 8, *args)
    assert same_bits(packed, again), "two packed calls differ"
    assert np.isfinite(packed).all() and np.all(packed[:, 1] == 0.0)          # the empty bin: zeros
    colsums = run_loo(ctx, "bigkrls_dev_kernel_loo_colsums", A, B, float(p), None, 2, cols.ctypes.data, 2)
    for jj, sl in enumerate((slice(0, 3), slice(3, 8))):
        total = packed[:, sl].sum(axis=1)
        assert np.max(np.abs(total - colsums[:, jj]) / colsums[:, jj]) <= 2 * (cases.U + 8 + 8 * (p + 12) + 4) * 2.0 ** -53
    for how in TWO:
        got = run_loo(ctx, "bigkrls_dev_kernel_loo_binsums", A, B, float(p), how, 8, *args)
        assert same_bits(got, packed), (p, how, "placed != packed", int(np.sum(got != packed)))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_short_leading_dimensions_are_refused(ctx):
    """lda, ldb, ldw, ldo one short of the row count, each in turn, for every entry: BIGKRLS_EINVAL before anything is
    written (out keeps the sentinel), and the context stays usable."""
    p, q = 3, 20
    A, B, WA, WB = host_operands(ctx, p, q)
    u, v = A.shape[0], B.shape[0]
    dA, dB, dWA, dWB = (ctx.from_numpy(x) for x in (A, B, WA, WB))
    out = ctx.from_numpy(np.full((u, max(v, 3 * q, 16)), SENT))               # large enough for every entry below
    cols = np.ascontiguousarray(cases.loo_cols(p), dtype=np.int64)
    ent = np.ascontiguousarray(np.asarray(cases.loo_entries(p, True), dtype=np.int64).reshape(-1, 3))
    lab = np.ascontiguousarray(cases.labels(False), dtype=np.int64)
    blab, nbins = binsums_labels()
    blab = np.ascontiguousarray(blab.T)
    h, s = ctx.handle, float(p)

    def entries(lda, ldb, ldw0, ldw1, ldo_u, ldo_v):
        """every entry with the given leading dimensions (ldw0 / ldo_u: W and out of trans = 0)"""
        return {
            "kernel_block": ("bigkrls_dev_kernel_block", h, dA.ptr, u, lda, dB.ptr, v, ldb, p, s, out.ptr, ldo_u, -1),
            "kernel_contract trans=0": ("bigkrls_dev_kernel_contract", h, dA.ptr, u, lda, dB.ptr, v, ldb, p, s, dWB.ptr, q,
                                        ldw0, 0, out.ptr, ldo_u),
            "kernel_contract trans=1": ("bigkrls_dev_kernel_contract", h, dA.ptr, u, lda, dB.ptr, v, ldb, p, s, dWA.ptr, q,
                                        ldw1, 1, out.ptr, ldo_v),
            "kernel_contract_grouped": ("bigkrls_dev_kernel_contract_grouped", h, dA.ptr, u, lda, dB.ptr, v, ldb, p, s,
                                        dWA.ptr, q, ldw1, lab.ctypes.data, cases.GROUPS, out.ptr, ldo_v),
            "kernel_loo_colsums": ("bigkrls_dev_kernel_loo_colsums", h, dA.ptr, u, lda, dB.ptr, v, ldb, p, s, cols.ctypes.data,
                                   int(cols.size), out.ptr, ldo_v),
            "kernel_loo_binsums": ("bigkrls_dev_kernel_loo_binsums", h, dA.ptr, u, lda, dB.ptr, v, ldb, p, s,
                                   np.array([0, p - 1], dtype=np.int64).ctypes.data, 2, blab.ctypes.data, nbins.ctypes.data,
                                   out.ptr, ldo_v),
            "kernel_loo_moments": ("bigkrls_dev_kernel_loo_moments", h, dA.ptr, u, lda, dB.ptr, v, ldb, p, s, ent.ctypes.data,
                                   int(ent.shape[0]), out.ptr, ldo_v),
        }

    good = dict(lda=u, ldb=v, ldw0=v, ldw1=u, ldo_u=u, ldo_v=v)
    takes_w = ("kernel_contract trans=0", "kernel_contract trans=1", "kernel_contract_grouped")
    for short in ("lda", "ldb", "ldw", "ldo"):
        lds = dict(good)
        for key in ([short] if short in good else [short + "0", short + "1"] if short == "ldw" else ["ldo_u", "ldo_v"]):
            lds[key] = good[key] - 1
        for name, call in entries(**lds).items():
            if short == "ldw" and name not in takes_w:
                continue
            with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*leading dimension"):
                _lib.call(*call)
    assert np.all(out.to_numpy() == SENT), "a refused call wrote into out"
    for name, call in entries(**good).items():                                # the context is still usable
        _lib.call(*call)
    ctx.sync()
    assert np.isfinite(out.to_numpy()[:v, :1]).all()
