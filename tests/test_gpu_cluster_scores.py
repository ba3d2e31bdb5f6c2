"""bigkrls_dev_cluster_scores (csrc/robust.hip: cluster_scores, cluster_scores_kernel, cluster_combine_kernel):
S[j, g] = sum over the rows i of cluster g of e[i] A[i, j], called through the C ABI so that leading dimensions exceed
the row counts.

Exact reference: A holds integers with |value| <= 8 and e integers with |value| <= 3; every product and every partial
sum is an integer below 24 n < 2^53, so the result does not depend on the order of the sums and must equal a numpy
scatter-add bit for bit -- every indexing, segment, piece and permutation error shows.

n lies below, at and above the 64-row chunk of one wave and covers several chunks; k lies below, at and above the 64
columns of one workgroup (16 per wave); G runs from one cluster to one per row, with the labels contiguous (the
identity permutation: no indirection) and shuffled (the sort permutation is used), one empty cluster, and one cluster
of n - 1 rows that spans every chunk. Operand padding holds NaN and the result's parent a sentinel."""
import numpy as np
import pytest

from bigkrls_amd import _lib

pytestmark = pytest.mark.gpu

SENT = -98765.4321


def place(ctx, block, fill=np.nan):
    r, c = block.shape
    ld = r + 3 if (r + 3) % 2 else r + 4
    host = np.full((ld, c + 2), fill, order="F")
    host[2:2 + r, 1:1 + c] = block
    d = ctx.from_numpy(host)
    return d, d.col_ptr(1, 2), ld, 2, 1


def vec(ctx, v):
    host = np.full((v.size + 9, 1), np.nan, order="F")
    host[1:1 + v.size, 0] = v
    d = ctx.from_numpy(host)
    return d, d.col_ptr(0, 1)


def scores(ctx, A, e, labels, G):
    n, k = A.shape
    dA, pA, lda, _, _ = place(ctx, A)
    de, pe = vec(ctx, e)
    dS, pS, lds, r0, c0 = place(ctx, np.full((k, G), np.nan), fill=SENT)      # S is overwritten, never read
    lab = np.ascontiguousarray(labels, dtype=np.int64)
    _lib.call("bigkrls_dev_cluster_scores", ctx.handle, n, k, pA, lda, pe, lab.ctypes.data, G, pS, lds)
    out = np.array(dS.to_numpy())
    blk = out[r0:r0 + k, c0:c0 + G].copy()
    out[r0:r0 + k, c0:c0 + G] = SENT
    assert (out == SENT).all(), ("wrote outside the k x G block", n, k, G)
    return blk


def reference(A, e, labels, G):
    S = np.zeros((A.shape[1], G))
    np.add.at(S.T, np.asarray(labels), e[:, None] * A)
    return S


def balanced_labels(n, G):
    """G contiguous clusters of (almost) equal size"""
    return (np.arange(n) * G) // n


def check_exact(ctx, rng, n, k, labels, G, what):
    A = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
    e = rng.integers(-3, 4, size=n).astype(np.float64)
    got = scores(ctx, A, e, labels, G)
    ref = reference(A, e, labels, G)
    assert np.isfinite(got).all(), (n, k, G, what, "NaN / Inf in the result")
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"cluster_scores n={n} k={k} G={G} ({what}): {len(bad)} wrong entries, first at "
                             f"{tuple(bad[0])}: got {got[tuple(bad[0])]}, expected {ref[tuple(bad[0])]}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_exact_integer_scores(ctx, n):
    rng = np.random.default_rng(3000 + n)
    for k in (1, 64, 65, 250):
        for G in sorted({1, 2, 7, max(n // 2, 1), n}):
            if G > n:
                continue
            lab = balanced_labels(n, G)
            check_exact(ctx, rng, n, k, lab, G, "contiguous")
            check_exact(ctx, rng, n, k, rng.permutation(lab), G, "shuffled")


def test_empty_cluster_and_one_large_cluster(ctx):
    rng = np.random.default_rng(5)
    n, k = 1000, 70
    lab = balanced_labels(n, 6)
    lab[lab >= 3] += 1                                       # cluster 3 of G = 7 is empty
    got_rng = np.random.default_rng(6)
    check_exact(ctx, got_rng, n, k, lab, 7, "empty cluster, contiguous")
    check_exact(ctx, got_rng, n, k, rng.permutation(lab), 7, "empty cluster, shuffled")
    A = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
    e = rng.integers(-3, 4, size=n).astype(np.float64)
    assert (scores(ctx, A, e, lab, 7)[:, 3] == 0.0).all()
    big = np.zeros(n, dtype=np.int64)                        # one cluster of n - 1 rows, one row of its own
    for pos in (0, 500, n - 1):
        lab2 = big.copy()
        lab2[pos] = 1
        check_exact(ctx, got_rng, n, k, lab2, 2, f"n - 1 rows in one cluster, the other row at {pos}")


@pytest.mark.parametrize("n,k,G", [(257, 65, 7), (5000, 250, 2), (5000, 33, 2500), (5000, 64, 5000)])
def test_repeatable_on_real_data(ctx, n, k, G):
    rng = np.random.default_rng(n + 7 * k + G)
    A, e = rng.standard_normal((n, k)), rng.standard_normal(n)
    lab = rng.permutation(balanced_labels(n, G))
    a = scores(ctx, A, e, lab, G)
    assert np.array_equal(a, scores(ctx, A, e, lab, G))
    ref = reference(A, e, lab, G)
    big = np.zeros((k, G))
    np.add.at(big.T, lab, np.abs(e)[:, None] * np.abs(A))
    m = int(np.max(np.bincount(lab, minlength=G)))           # the longest sum; one rounding for the product
    assert (np.abs(a - ref) <= 2 * (m + 1) * 2.0 ** -53 * big + 1e-300).all()


def test_refusals(ctx):
    A = np.ones((10, 3))
    dA, de, dS = ctx.from_numpy(A), ctx.from_numpy(np.ones(10)), ctx.from_numpy(np.full((3, 4), SENT))
    lab = np.arange(10, dtype=np.int64) % 4

    def call(n, k, lda, labels, G, lds):
        _lib.call("bigkrls_dev_cluster_scores", ctx.handle, n, k, dA.ptr, lda, de.ptr, labels.ctypes.data, G, dS.ptr, lds)
    bad = lab.copy()
    bad[7] = 4
    with pytest.raises(_lib.BigKRLSError, match=r"label of row 8 is outside \[0, G\)"):
        call(10, 3, 10, bad, 4, 3)
    bad[7] = -1
    with pytest.raises(_lib.BigKRLSError, match="outside"):
        call(10, 3, 10, bad, 4, 3)
    with pytest.raises(_lib.BigKRLSError, match="G must be at least 1"):
        call(10, 3, 10, lab, 0, 3)
    with pytest.raises(_lib.BigKRLSError, match="leading dimension"):
        call(10, 3, 9, lab, 4, 3)
    with pytest.raises(_lib.BigKRLSError, match="leading dimension"):
        call(10, 3, 10, lab, 4, 2)
    assert (dS.to_numpy() == SENT).all()                     # nothing was written by a refused call
    call(10, 0, 10, lab, 4, 3)                               # k == 0: nothing
    assert (dS.to_numpy() == SENT).all()
    call(0, 3, 10, lab, 4, 3)                                # n == 0: every cluster is empty
    assert (dS.to_numpy() == 0.0).all()


def test_ops_wrapper_and_profile_name(ctx):
    from bigkrls_amd import ops
    rng = np.random.default_rng(12)
    n, k, G = 300, 20, 9
    A = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
    e = rng.integers(-3, 4, size=n).astype(np.float64)
    lab = rng.integers(0, G, size=n)
    ctx.set_profile(True)
    try:
        got = ops.bClusterScores(ctx.from_numpy(A), e, lab, G).to_numpy()
        ms, work, launches = ctx.get_profile("cluster_scores")
    finally:
        ctx.set_profile(False)
    assert np.array_equal(got, reference(A, e, lab, G))
    assert launches == 1 and work == 8 * n * k
    with pytest.raises(ValueError, match="labels must have"):
        ops.bClusterScores(ctx.from_numpy(A), e, lab[:-1], G)
    with pytest.raises(ValueError, match="G must be"):
        ops.bClusterScores(ctx.from_numpy(A), e, lab, 0)
