"""Seeded inputs and output digests of the plain GEMM family of csrc/gemm.hip (gemm, gemm_modulated, gemm_modulated2,
gram_weighted, quadform_diag, gemm_nn_skinny48, the symmetric rank-2k forms, gemm_batched_nn), shared by
tests/test_gpu_gemm_family_digests.py and tools/gemm_family_digests.py (which records
tests/golden/gemm_family_digests.json).

Every entry is called through the C ABI on operands placed inside larger parents (tests/_placement.py): inputs inside
NaN, the output inside a sentinel-filled parent, and a digest covers the whole parent of the output, so a write outside
the block changes it. Inputs are standard normal from fixed seeds: a change of the split count or of the summation order
changes the bits.

Shapes, the smallest that reach each branch: m = 130 (two row tiles, the second of two rows), n in {20, 50, 130} (the
32-, 64- and 128-wide tiles; 130 is two column tiles), k = 37 (two k-tiles and a partial one), k = 2100 (split-K:
k >= 1024 on a few tiles), k = 0 (the empty sum). gram_weighted: 20, 50, 130 and 300 columns are the three one-tile
widths, then T = 2 and T = 3 tile rows; 2100 rows split. quadform_diag: n = 1100 is its split case. The rank-2k forms:
m = 63, 130, 300 are one partial tile, two and three tile rows."""
import hashlib
import itertools

import numpy as np

from _placement import SENT, place

M = 130
NS = (20, 50, 130)
K_SHORT, K_SPLIT = 37, 2100
TRANS = list(itertools.product((0, 1), (0, 1)))


def digest(parent):
    return hashlib.sha256(np.ascontiguousarray(parent.to_numpy()).tobytes()).hexdigest()


def _rng(*key):
    return np.random.default_rng([20251, *key])


def _vec(ctx, v):
    """A vector inside a NaN-filled parent: (keep-alive, pointer)."""
    d, p, _, _, _ = place(ctx, np.asarray(v, dtype=np.float64).reshape(-1, 1))
    return d, p


def _gemm(ctx, ta, tb, m, n, k, beta, seed):
    from bigkrls_amd import _lib
    rng = _rng(1, seed, ta, tb, m, n, k)
    A = rng.standard_normal((k, m) if ta else (m, k))
    B = rng.standard_normal((n, k) if tb else (k, n))
    C0 = rng.standard_normal((m, n)) if beta != 0.0 else np.full((m, n), np.nan)
    if k == 0:
        pA = pB = None
        lda = ldb = max(m, n)
    else:
        dA, pA, lda, _, _ = place(ctx, A)
        dB, pB, ldb, _, _ = place(ctx, B)
    dC, pC, ldc, _, _ = place(ctx, C0, fill=SENT)
    _lib.call("bigkrls_dev_gemm", ctx.handle, ta, tb, m, n, k, 0.7, pA, lda, pB, ldb, float(beta), pC, ldc)
    return digest(dC)


def _modulated(ctx, two, m, n, k):
    from bigkrls_amd import _lib
    rng = _rng(2, int(two), m, n, k)
    kk = max(k, 1)
    dA, pA, lda, _, _ = place(ctx, rng.standard_normal((m, kk)))
    dB, pB, ldb, _, _ = place(ctx, rng.standard_normal((kk, n)))
    vecs = [_vec(ctx, rng.standard_normal(ln)) for ln in ((m, m, kk, m, m, kk) if two else (m, m, kk))]
    ptrs = [p for _, p in vecs]
    dC, pC, ldc, _, _ = place(ctx, np.full((m, n), np.nan), fill=SENT)
    if two:
        _lib.call("bigkrls_dev_gemm_modulated2", ctx.handle, m, n, k, pA, lda, *ptrs, -0.3, pB, ldb, pC, ldc)
    else:
        _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, m, n, k, pA, lda, *ptrs, pB, ldb, pC, ldc)
    return digest(dC)


def _gram(ctx, n, k):
    from bigkrls_amd import _lib
    rng = _rng(3, n, k)
    dA, pA, lda, _, _ = place(ctx, rng.standard_normal((n, k)))
    dw, pw = _vec(ctx, rng.standard_normal(n))
    dM, pM, ldm, _, _ = place(ctx, np.full((k, k), np.nan), fill=SENT)
    _lib.call("bigkrls_dev_gram_weighted", ctx.handle, n, k, pA, lda, pw, pM, ldm)
    return digest(dM)


def _quadform(ctx, m, n):
    from bigkrls_amd import _lib
    rng = _rng(4, m, n)
    dA, pA, lda, _, _ = place(ctx, rng.standard_normal((m, n)))
    dV, pV, ldv, _, _ = place(ctx, rng.standard_normal((n, n)))
    do, po, _, _, _ = place(ctx, np.full((m, 1), np.nan), fill=SENT)
    _lib.call("bigkrls_dev_quadform_diag", ctx.handle, m, n, pA, lda, pV, ldv, po)
    return digest(do)


def _skinny(ctx, m, n, k):
    from bigkrls_amd import _lib
    rng = _rng(5, m, n, k)
    dA, pA, lda, _, _ = place(ctx, rng.standard_normal((m, k)))
    dB, pB, ldb, _, _ = place(ctx, rng.standard_normal((k, n)))
    dC, pC, ldc, _, _ = place(ctx, np.full((m, n), np.nan), fill=SENT)
    _lib.call("bigkrls_dev_gemm_skinny48", ctx.handle, m, n, k, pA, lda, pB, ldb, pC, ldc)
    return digest(dC)


def _syr2k(ctx, form, m, k):
    from bigkrls_amd import _lib
    rng = _rng(6, m, k)                       # (the same operands for the five forms)
    dA, pA, lda, _, _ = place(ctx, rng.standard_normal((m, k)))
    dB, pB, ldb, _, _ = place(ctx, rng.standard_normal((m, k)), ld=m + 7 + (m % 2))
    L = np.tril(rng.standard_normal((m, m)))
    C0 = np.full((m, m), np.nan) if form == 4 else L + np.tril(L, -1).T
    dC, pC, ldc, _, _ = place(ctx, C0, fill=SENT)
    _lib.call("bigkrls_dev_syr2k", ctx.handle, form, m, k, -0.7, pA, lda, pB, ldb, pC, ldc, 0, -1, 0)
    return digest(dC)


def _batched(ctx):
    """Two descriptors in one launch: (130, 140, 37) with a gather of A's columns, (5, 3, 16) without."""
    import ctypes as C
    from bigkrls_amd import _lib
    rng = _rng(7)
    addr = lambda p: int(p.value) if isinstance(p, C.c_void_p) else int(p)
    keep, fields, outs = [], [], []
    for m, n, k, wide in ((130, 140, 37, 51), (5, 3, 16, None)):
        dA, pA, lda, _, _ = place(ctx, rng.standard_normal((m, wide or k)))
        dB, pB, ldb, _, _ = place(ctx, rng.standard_normal((k, n)))
        kaddr = 0
        if wide:
            idx = rng.integers(0, wide, size=k)
            with ctx.on_stream():
                d_idx = ctx.torch.tensor(np.asarray(idx, dtype=np.int32), dtype=ctx.torch.int32, device=ctx.device)
            ctx.sync()
            keep.append(d_idx)
            kaddr = int(d_idx.data_ptr())
        dC, pC, ldc, _, _ = place(ctx, np.full((m, n), np.nan), fill=SENT)
        keep += [dA, dB]
        outs.append(dC)
        fields.append((m, n, k, addr(pA), lda, addr(pB), ldb, addr(pC), ldc, kaddr))
    cols = [np.ascontiguousarray([f[j] for f in fields], dtype=np.int64) for j in range(10)]
    _lib.call("bigkrls_dev_gemm_batched", ctx.handle, len(fields), *[c.ctypes.data_as(_lib.pi64) for c in cols], 130, 140)
    return {"gathered_130x140x37": digest(outs[0]), "plain_5x3x16": digest(outs[1])}


GRAM_ROWS, GRAM_COLS = (37, 2100), (20, 50, 130, 300)
QF_NS = (20, 50, 130, 1100)
SK_NS, SK_KS = (1, 42, 48), (37, 2100)
SYR_MS, SYR_KS = (63, 130, 300), (15, 128)


def case_names():
    return (["gemm_short", "gemm_split", "gemm_empty", "modulated", "modulated2", "gram_weighted", "quadform_diag",
             "skinny48", "batched"] + [f"syr2k_form{f}" for f in range(5)])


def run_case(ctx, name):
    """{sub-case: sha256 of the bytes of the output's whole parent array} of one case."""
    out = {}
    if name == "gemm_short":
        for n, (ta, tb), beta in itertools.product(NS, TRANS, (0.0, 0.5)):
            out[f"n{n}_ta{ta}_tb{tb}_beta{beta}"] = _gemm(ctx, ta, tb, M, n, K_SHORT, beta, 0)
    elif name == "gemm_split":
        for (ta, tb), beta in itertools.product(((0, 0), (1, 0)), (0.0, 0.5)):
            out[f"ta{ta}_tb{tb}_beta{beta}"] = _gemm(ctx, ta, tb, M, 50, K_SPLIT, beta, 1)
    elif name == "gemm_empty":
        for beta in (0.0, 1.0, 0.5):
            out[f"beta{beta}"] = _gemm(ctx, 0, 0, M, 50, 0, beta, 2)
    elif name in ("modulated", "modulated2"):
        for n, k in [(n, K_SHORT) for n in NS] + [(50, K_SPLIT), (50, 0)]:
            out[f"n{n}_k{k}"] = _modulated(ctx, name == "modulated2", M, n, k)
    elif name == "gram_weighted":
        for n, k in itertools.product(GRAM_ROWS, GRAM_COLS):
            out[f"rows{n}_k{k}"] = _gram(ctx, n, k)
    elif name == "quadform_diag":
        for n in QF_NS:
            out[f"n{n}"] = _quadform(ctx, M, n)
    elif name == "skinny48":
        for n, k in itertools.product(SK_NS, SK_KS):
            out[f"n{n}_k{k}"] = _skinny(ctx, M, n, k)
    elif name == "batched":
        out = _batched(ctx)
    elif name.startswith("syr2k_form"):
        form = int(name[len("syr2k_form"):])
        for m, k in itertools.product(SYR_MS, SYR_KS):
            out[f"m{m}_k{k}"] = _syr2k(ctx, form, m, k)
    else:
        raise KeyError(name)
    return out
