"""bigkrls_dev_gemm_batched (csrc/gemm.hip: gemm_batched_nn, gemm_batched_nn_kernel), the merge products of the divide &
conquer eigensolver: one launch over a list of independent problems C_i = A_i[:, kidx_i] B_i of different sizes, by the
method of test_gpu_gemm_core.py. Every A and B sits inside a NaN-filled parent with an odd leading dimension, every C
starts as NaN inside a sentinel-filled parent of its own. Integer entries in [-64, 64]: the reference A[:, kidx] @ B in
numpy fp64 is exact and np.array_equal is the assertion."""
import ctypes as C

import numpy as np
import pytest

from bigkrls_amd import _lib

from _placement import SENT, place, take

pytestmark = pytest.mark.gpu


def device_ints(ctx, values):
    """int32 values on the device (kept alive by the returned tensor)."""
    with ctx.on_stream():
        t = ctx.torch.tensor(np.asarray(values, dtype=np.int32), dtype=ctx.torch.int32, device=ctx.device)
    ctx.sync()
    return t


def addr(p):
    return int(p.value) if isinstance(p, C.c_void_p) else int(p)


def batched_call(ctx, fields, max_m, max_n):
    """fields: per problem (m, n, k, A address, lda, B address, ldb, C address, ldc, kidx address or 0)."""
    cols = [np.ascontiguousarray([f[j] for f in fields], dtype=np.int64) for j in range(10)]
    P = lambda a: a.ctypes.data_as(_lib.pi64)
    m, n, k, pA, lda, pB, ldb, pC, ldc, kidx = cols
    _lib.call("bigkrls_dev_gemm_batched", ctx.handle, len(fields), P(m), P(n), P(k), P(pA), P(lda), P(pB), P(ldb), P(pC),
              P(ldc), P(kidx), max_m, max_n)


def test_mixed_batch(ctx):
    """Five problems of different shapes in one launch, the grid sized for 300 x 260: most workgroups of every problem
    find their tile outside it and return. One element; partial tiles in both directions with a partial k-tile; a whole
    tile whose gather permutes and repeats columns of a wider A; three row tiles by three columns with a gather; two
    column tiles without one (kidx = 0: the strided loader of a plain product)."""
    rng = np.random.default_rng(31)
    shapes = [(1, 1, 1, None), (130, 129, 17, None), (128, 128, 16, 23), (257, 3, 40, 57), (64, 200, 33, None)]
    keep, fields, outs = [], [], []
    for m, n, k, wide in shapes:
        A = rng.integers(-64, 65, size=(m, wide or k)).astype(np.float64)
        B = rng.integers(-64, 65, size=(k, n)).astype(np.float64)
        if wide:
            idx = rng.integers(0, wide, size=k)          # a permutation of some columns, others repeated
            idx[:3] = idx[3]
            d_idx = device_ints(ctx, idx)
            keep.append(d_idx)
            ref, kaddr = A[:, idx] @ B, int(d_idx.data_ptr())
        else:
            ref, kaddr = A @ B, 0
        dA, pA, lda, _, _ = place(ctx, A)
        dB, pB, ldb, _, _ = place(ctx, B)
        dC, pC, ldc, r0, c0 = place(ctx, np.full((m, n), np.nan), fill=SENT)
        keep += [dA, dB]
        fields.append((m, n, k, addr(pA), lda, addr(pB), ldb, addr(pC), ldc, kaddr))
        outs.append((dC, r0, c0, m, n, ref))
    batched_call(ctx, fields, 300, 260)
    for i, (dC, r0, c0, m, n, ref) in enumerate(outs):
        got = take(dC, r0, c0, m, n, ("gemm_batched problem", i))
        assert np.array_equal(got, ref), (i, shapes[i], np.argwhere(~(got == ref))[:4])


def test_more_problems_than_one_launch_takes(ctx):
    """65 537 problems of 1 x 1 x 2, problem i writing element i of one vector: a launch takes 65 535 problems (the limit
    of the grid's second dimension), so the last two prove the second launch and its descriptor offset."""
    rng = np.random.default_rng(32)
    nb = 65537
    A = rng.integers(-64, 65, size=(nb, 2)).astype(np.float64)      # problem i: row i (1 x 2, lda = the parent's)
    B = rng.integers(-64, 65, size=(2, nb)).astype(np.float64)      # ... times column i (2 x 1)
    dA, pA, lda, _, _ = place(ctx, A)
    dB, pB, ldb, _, _ = place(ctx, B)
    dC, pC, ldc, r0, c0 = place(ctx, np.full((nb, 1), np.nan), fill=SENT)
    i = np.arange(nb, dtype=np.int64)
    one, zero = np.ones(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
    P = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(_lib.pi64)
    cols = [one, one, 2 * one, addr(pA) + 8 * i, lda * one, addr(pB) + 8 * ldb * i, ldb * one, addr(pC) + 8 * i, ldc * one, zero]
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in cols]
    _lib.call("bigkrls_dev_gemm_batched", ctx.handle, nb, *[P(c) for c in cols], 1, 1)
    got = take(dC, r0, c0, nb, 1, "gemm_batched, 65 537 problems")[:, 0]
    ref = np.sum(A * B.T, axis=1)
    assert np.array_equal(got, ref), np.argwhere(~(got == ref))[:4]


def test_bad_descriptors_are_rejected(ctx):
    rng = np.random.default_rng(33)
    dA, pA, lda, _, _ = place(ctx, rng.standard_normal((8, 8)))
    good = (8, 8, 8, addr(pA), lda, addr(pA), lda, addr(pA), lda, 0)
    for j, bad in ((0, -1), (0, 9), (3, 0), (4, 7), (6, 7), (8, 7)):      # m < 0, m > max_m, null A, lda / ldb / ldc < rows
        f = list(good)
        f[j] = bad
        with pytest.raises(_lib.BigKRLSError) as e:
            batched_call(ctx, [good, tuple(f)], 8, 8)
        assert e.value.code == _lib.EINVAL and "dev_gemm_batched" in str(e.value)
