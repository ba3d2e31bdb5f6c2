"""Seeded inputs and output digests of the five fused kernel-tile entry points (csrc/gemm.hip), shared by
tests/test_gpu_fused_tile_digests.py and tools/fused_tile_digests.py (which records tests/golden/fused_tile_digests.json).

Shapes: loop rows U = 1100 (69 loop tiles: up to 4 loop splits allowed; not a multiple of 16) and stationary rows V = 70
(two tile groups of 64, the second partial, so few tasks that the split search cuts the loop). Swapping the roles (trans = 0
of bKernelContract) leaves 5 loop tiles, fewer than the 32 a cut needs: nsplit == 1. P in {3, 20, 32, 37}: KS = 1, 5, 8 and
the re-reading path (KS = 0), none but 20 and 32 a multiple of 4."""
import hashlib

import numpy as np

U, V = 1100, 70
PS = (3, 20, 32, 37)
QS_NARROW = (1, 20, 40)      # CT = 1, 2, 4
QS_WIDE = (128, 130)         # the wide kernel's full body; a full chunk and a partial one
GROUPS = 3                   # group 0: 1090 rows (long enough to be cut), group 1: empty, group 2: 10 rows (< 16)


def _uniform(rng, shape):
    # (Generator.random: the plain double stream, the same on every NumPy)
    return (rng.random(shape) - 0.5) * 2.4


def operands(ctx, p, q=0):
    rng = np.random.default_rng(1000 + p)
    A, B = _uniform(rng, (U, p)), _uniform(rng, (V, p))
    WA, WB = _uniform(rng, (U, max(q, 1))), _uniform(rng, (V, max(q, 1)))
    return ctx.from_numpy(A), ctx.from_numpy(B), ctx.from_numpy(WA), ctx.from_numpy(WB)


def labels(shuffled):
    lab = np.zeros(U, dtype=np.int64)
    lab[U - 10:] = 2
    if shuffled:
        lab = lab[np.random.default_rng(7).permutation(U)]
    return lab


def loo_cols(p):
    """Selected columns with a repeat; 5 or 7 of them: chunks of (2, 3) or (3, 4), i.e. a chunk below KL_CW = 4."""
    cols = [0, p - 1, 1, 0, p - 1] if p < 8 else [0, p - 1, 7, 3, 3, 5, 1]
    return np.asarray(cols, dtype=np.int64)


def loo_entries(p, in_order):
    """(kind, c, j): all three kinds; five entries of c = 0 (more than KM_CW = 3: two chunks of one c, of 2 and 3 entries
    -- with KS = 8 three chunks), three of c = p - 1, one of c = 1. in_order: sorted by c, so that the launch writes its
    columns in place; otherwise they pass through the staging buffer and are scattered."""
    c1, j1, j2 = p - 1, 1, p - 2
    ent = [(0, 0, 0), (1, 0, j1), (2, 0, j2), (1, 0, j2), (2, 0, j1), (0, 1, 0), (0, c1, 0), (1, c1, 0), (2, c1, j1)]
    if not in_order:
        ent = [ent[i] for i in (6, 0, 5, 2, 7, 1, 8, 3, 4)]
    return np.asarray(ent, dtype=np.int64)


def digest(dm):
    return hashlib.sha256(np.ascontiguousarray(dm.to_numpy()).tobytes()).hexdigest()


def case_names():
    return ([f"contract_p{p}" for p in PS] + [f"wide_p{p}" for p in PS] + [f"grouped_p{p}" for p in PS]
            + [f"loo_colsums_p{p}" for p in PS] + [f"loo_moments_p{p}" for p in PS])


def run_case(ctx, name):
    """{sub-case: sha256 of the output bytes} of one case."""
    from bigkrls_amd import ops
    kind, p = name.rsplit("_p", 1)
    p = int(p)
    sigma = float(p)
    out = {}
    if kind in ("contract", "wide"):
        for q in (QS_NARROW if kind == "contract" else QS_WIDE):
            dA, dB, dWA, dWB = operands(ctx, p, q)
            out[f"q{q}_trans0"] = digest(ops.bKernelContract(dA, dB, dWB, sigma, trans=0))
            out[f"q{q}_trans1"] = digest(ops.bKernelContract(dA, dB, dWA, sigma, trans=1))
    elif kind == "grouped":
        for q in QS_NARROW:
            dA, dB, dWA, _ = operands(ctx, p, q)
            for shuffled in (False, True):
                got = ops.bKernelContractGrouped(dA, dB, dWA, sigma, labels(shuffled), GROUPS)
                out[f"q{q}_{'shuffled' if shuffled else 'sorted'}"] = digest(got)
    elif kind == "loo_colsums":
        dA, dB, _, _ = operands(ctx, p)
        out["cols"] = digest(ops.bKernelLooColsums(dA, dB, sigma, loo_cols(p)))
    elif kind == "loo_moments":
        dA, dB, _, _ = operands(ctx, p)
        for in_order in (True, False):
            got = ops.bKernelLooMoments(dA, dB, sigma, loo_entries(p, in_order))
            out["in_order" if in_order else "scattered"] = digest(got)
    else:
        raise KeyError(name)
    return out
