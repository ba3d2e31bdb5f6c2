"""Cases of tests/test_gpu_gemm_deep_pipeline.py and tools/gemm_deep_pipeline_digests.py: the k loop of gemm_tile's
two-tiles-in-flight path (csrc/gemm.hip, every tile up to GEMM_DEEP_BN wide), swept over the NUMBER OF K-TILES.

The prologue, the interior loop, its hand-over to the general loop, the early break after an even tile and the partial
last tile are where a wait or a register set goes wrong, so k runs over one to six k-tiles (BK = 16), each with and
without a partial tail, and over seven and eight; the interior loop runs from four full tiles on (k >= 64: once, then
the general loop finishes two to four tiles; k >= 96: twice) and the split case (k = 2100) runs it for many iterations
in every slab. m and n are the smallest that reach one and two row tiles, full and ragged, and the 32- and 64-wide
column tiles, full (n = 32, 64) and ragged.

Which groups run the interior loop: it needs both operands on the strided loader, i.e. a not-contiguous operand
(a transposed A, a not-transposed B) must fill its tile. So with tb = 0 only n = 32 and n = 64 enter it, with ta = 1
only m = 128 and the first row tile of m = 130; gemm_modulated (B not transposed) enters it at n = 32 and n = 64 and
not at n = 50. gemm_modulated2 is kept off it in the kernel, and gram_weighted's 32- and 64-wide tiles can never
enter it (its transposed A operand has at most 64 of the 128 rows of a tile): their groups hold the general loop,
which the interior loop's code surrounds, to the parent's bits.

Every operand sits inside a larger parent (tests/_placement.py): inputs inside NaN, the output inside a sentinel-filled
parent. A group is one (entry, transposes, k): its sub-cases run in a fixed order and its digest is the SHA-256 of the
bytes of all their outputs' whole parents, so a write outside a block, another summation order or another split count
changes it. Inputs are standard normal from seeds fixed per group.

Each sub-case also carries a numpy float64 reference and the componentwise bound
    |C - C_ref| <= (k + 4) 2^-53 (|alpha| |op(A)| |op(B)| + |beta| |C0|):
the gamma_k bound of a length-k inner product, plus four roundings for the scale by alpha, the scale by beta and the add
(three; one to spare). The other entries have alpha = 1 and beta = 0, so those four roundings are free for the
operand's own preparation, with op(A) as the kernel forms it:
  * gemm_modulated: op(A) = A o F, F = fma(t, s, r): two roundings (the fma, the product), both relative to |A o F|
    (the reference forms t s + r in extended precision, so that its own F is the rounded exact value too, up to 2^-64
    of |t s| + |r|, and no cancellation in t s + r enters the comparison);
  * gemm_modulated2: F = fma(f1, f2, d) with f1 = fma(t1, s1, r1), f2 = fma(t2, s2, r2): f1 and f2 carry one rounding
    each, the outer fma one more, relative to |f1 f2| + |d| (the sum can cancel), and the product with A a fourth: the
    bound takes |op(A)| = |A| (|f1 f2| + |d|);
  * gram_weighted: op(A)(i, l) = A(l, i) w(l): one rounding."""
import hashlib
import itertools

import numpy as np

from _placement import SENT, place, take

KS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 80, 81,
      96, 113)      # two interior iterations, handing over two tiles, and three with a partial fourth
MS = (1, 127, 128, 130)
NS = (1, 20, 32, 33, 50, 64)
TRANS = tuple(itertools.product((0, 1), (0, 1)))
BETAS = (0.0, 0.5)
ALPHA = 0.7
SPLIT_M, SPLIT_N, SPLIT_K = 130, 50, 2100
MOD_M, MOD_NS = 130, (50, 64, 32)      # 50: the issue's shape (general loop); 64, 32: full tiles (interior loop)
GRAM_COLS = 50
U = 2.0 ** -53


def group_names():
    return ([f"gemm_ta{ta}_tb{tb}_k{k}" for (ta, tb) in TRANS for k in KS]
            + [f"gemm_split_ta{ta}_tb{tb}" for (ta, tb) in TRANS]
            + [f"{e}_k{k}" for e in ("modulated", "modulated2", "gram_weighted") for k in KS]
            + ["modulated_split"])


def _rng(*key):
    return np.random.default_rng([20261, *key])


def _vec(ctx, v):
    d, p, _, _, _ = place(ctx, np.asarray(v, dtype=np.float64).reshape(-1, 1))
    return d, p


def _gemm_group(ctx, ta, tb, k, ms, ns, seed):
    """Yields (sub-case, output parent, output block, reference, bound) for every (m, n, beta)."""
    from bigkrls_amd import _lib
    rng = _rng(1, seed, ta, tb, k)
    opA = rng.standard_normal((max(ms), k))
    opB = rng.standard_normal((k, max(ns)))
    C0 = rng.standard_normal((max(ms), max(ns)))
    placedA = {m: place(ctx, np.ascontiguousarray(opA[:m].T) if ta else opA[:m]) for m in ms}
    placedB = {n: place(ctx, np.ascontiguousarray(opB[:, :n].T) if tb else opB[:, :n]) for n in ns}
    for m, n in itertools.product(ms, ns):
        _, pA, lda, _, _ = placedA[m]
        _, pB, ldb, _, _ = placedB[n]
        prod = opA[:m] @ opB[:, :n]
        mag = np.abs(opA[:m]) @ np.abs(opB[:, :n])
        for beta in BETAS:
            c0 = C0[:m, :n] if beta != 0.0 else np.full((m, n), np.nan)     # (beta = 0 must not read C)
            dC, pC, ldc, r0, c0_, = place(ctx, c0, fill=SENT)
            _lib.call("bigkrls_dev_gemm", ctx.handle, ta, tb, m, n, k, ALPHA, pA, lda, pB, ldb, float(beta), pC, ldc)
            sub = f"m{m}_n{n}_beta{beta}"
            ref = ALPHA * prod + (beta * C0[:m, :n] if beta != 0.0 else 0.0)
            bound = (k + 4) * U * (abs(ALPHA) * mag + (abs(beta) * np.abs(C0[:m, :n]) if beta != 0.0 else 0.0))
            yield sub, dC, take(dC, r0, c0_, m, n, sub), ref, bound


def _modulated_group(ctx, two, k, ns=MOD_NS):
    from bigkrls_amd import _lib
    m = MOD_M
    rng = _rng(2, int(two), k)
    A = rng.standard_normal((m, k))
    Bfull = rng.standard_normal((k, max(ns)))
    v = [rng.standard_normal(ln) for ln in ((m, m, k, m, m, k) if two else (m, m, k))]
    d = -0.3
    dA, pA, lda, _, _ = place(ctx, A)
    vecs = [_vec(ctx, x) for x in v]
    ptrs = [p for _, p in vecs]
    ld = np.longdouble
    f1 = (v[1].astype(ld)[:, None] * v[2].astype(ld)[None, :] + v[0].astype(ld)[:, None]).astype(np.float64)
    if two:
        f2 = (v[4].astype(ld)[:, None] * v[5].astype(ld)[None, :] + v[3].astype(ld)[:, None]).astype(np.float64)
        F, Fmag = f1 * f2 + d, np.abs(f1 * f2) + abs(d)
    else:
        F, Fmag = f1, np.abs(f1)
    for n in ns:
        B = Bfull[:, :n]
        dB, pB, ldb, _, _ = place(ctx, B)
        dC, pC, ldc, r0, c0 = place(ctx, np.full((m, n), np.nan), fill=SENT)
        if two:
            _lib.call("bigkrls_dev_gemm_modulated2", ctx.handle, m, n, k, pA, lda, *ptrs, d, pB, ldb, pC, ldc)
        else:
            _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, m, n, k, pA, lda, *ptrs, pB, ldb, pC, ldc)
        ref = (A * F) @ B
        bound = (k + 4) * U * ((np.abs(A) * Fmag) @ np.abs(B))
        sub = f"m{m}_n{n}"
        yield sub, dC, take(dC, r0, c0, m, n, sub), ref, bound


def _gram_group(ctx, rows):
    from bigkrls_amd import _lib
    k = GRAM_COLS
    rng = _rng(3, rows)
    A = rng.standard_normal((rows, k))
    w = rng.standard_normal(rows)
    dA, pA, lda, _, _ = place(ctx, A)
    dw, pw = _vec(ctx, w)
    dM, pM, ldm, r0, c0 = place(ctx, np.full((k, k), np.nan), fill=SENT)
    _lib.call("bigkrls_dev_gram_weighted", ctx.handle, rows, k, pA, lda, pw, pM, ldm)
    ref = (A * w[:, None]).T @ A
    bound = (rows + 4) * U * ((np.abs(A) * np.abs(w)[:, None]).T @ np.abs(A))
    sub = f"rows{rows}_cols{k}"
    yield sub, dM, take(dM, r0, c0, k, k, sub), ref, bound


def run_group(ctx, name):
    """(digest of the group, [(sub-case, max over the block of |C - C_ref| / bound, all entries finite)])."""
    parts = name.split("_")
    if name.startswith("gemm_split_"):
        gen = _gemm_group(ctx, int(parts[2][2:]), int(parts[3][2:]), SPLIT_K, (SPLIT_M,), (SPLIT_N,), 1)
    elif name.startswith("gemm_"):
        gen = _gemm_group(ctx, int(parts[1][2:]), int(parts[2][2:]), int(parts[3][1:]), MS, NS, 0)
    elif name == "modulated_split":
        gen = _modulated_group(ctx, False, SPLIT_K, (64,))
    elif name.startswith("modulated2_"):
        gen = _modulated_group(ctx, True, int(parts[1][1:]))
    elif name.startswith("modulated_"):
        gen = _modulated_group(ctx, False, int(parts[1][1:]))
    elif name.startswith("gram_weighted_"):
        gen = _gram_group(ctx, int(parts[2][1:]))
    else:
        raise KeyError(name)
    h = hashlib.sha256()
    figures = []
    for sub, parent, blk, ref, bound in gen:
        h.update(np.ascontiguousarray(parent.to_numpy()).tobytes())
        finite = bool(np.isfinite(blk).all())
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bound > 0.0, np.abs(blk - ref) / bound, np.where(blk == ref, 0.0, np.inf))
        figures.append((sub, float(np.max(ratio)) if finite else float("inf"), finite))
    return h.hexdigest(), figures
