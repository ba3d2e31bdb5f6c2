"""Seeded inputs and output digests for the host plans of the kernel builds and the fused kernel-tile entry points
(csrc/ktplan.h, csrc/gemm.hip), shared by tests/test_gpu_kt_plan_digests.py and tools/kt_plan_digests.py (which records
tests/golden/kt_plan_digests.json). Beside tests/_fused_tile_cases.py, which they leave alone, these reach

  * every arm of the kernel build: the workgroup-tiled kernel (symmetric with odd n: scalar stores; rectangular), the
    symmetric wave kernel at ks = 2, 5 and 8, the rectangular wave kernel, a column block with a diagonal shift, and the
    LDS-generic kernel (p > 128);
  * the grouped pass whose table is too long to travel as a kernel argument (more than 160 segments, or more than 32
    groups that are empty or cut): the pinned upload behind an event, with and without a permutation;
  * leave-out moments in three launches (130 entries, 64 per launch), in no order."""
import hashlib

import numpy as np

GRP_U, GRP_V, GRP_P, GRP_Q = 400, 20, 3, 2


def _uniform(rng, shape):
    # (Generator.random: the plain double stream, the same on every NumPy)
    return np.asfortranarray((rng.random(shape) - 0.5) * 2.4)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# name: (what, rows of the first operand, rows of the second (None: the same matrix), p, column block or None)
KERNEL_CASES = {
    "kb_tiled_sym_n1153_p50": ("sym", 1153, None, 50, None),
    "kb_tiled_rect_1024x1300_p33": ("rect", 1024, 1300, 33, None),
    "kb_sym_wave_n100_p5": ("sym", 100, None, 5, None),
    "kb_sym_wave_n100_p37": ("sym", 100, None, 37, None),
    "kb_sym_wave_n100_p128": ("sym", 100, None, 128, None),
    "kb_wave_rect_70x100_p3": ("rect", 70, 100, 3, None),
    "kb_cols_n200_p20_30_170": ("sym", 200, None, 20, (30, 170)),
    "kb_generic_70x100_p129": ("rect", 70, 100, 129, None),
}


def grouped_labels(name):
    """(labels, G) of a grouped case."""
    if name in ("grouped_200_sorted", "grouped_200_shuffled"):
        lab = np.repeat(np.arange(200, dtype=np.int64), 2)           # 200 segments: the table leaves the inline limit
        if name.endswith("shuffled"):
            lab = lab[np.random.default_rng(11).permutation(GRP_U)]   # ... and travels with the permutation
        return lab, 200
    if name == "grouped_33_empty":
        sizes = np.zeros(40, dtype=np.int64)                          # 7 segments, but 33 entries for the empty groups
        sizes[::6] = (100, 37, 80, 3, 120, 16, 44)
        return np.repeat(np.arange(40, dtype=np.int64), sizes), 40
    raise KeyError(name)


GROUPED_CASES = ("grouped_200_sorted", "grouped_200_shuffled", "grouped_33_empty")
assert all(len(grouped_labels(n)[0]) == GRP_U for n in GROUPED_CASES)


def grouped_inputs():
    """A (u x p: the labelled rows), B (v x p), W (u x q), sigma."""
    rng = np.random.default_rng(4100)
    return _uniform(rng, (GRP_U, GRP_P)), _uniform(rng, (GRP_V, GRP_P)), _uniform(rng, (GRP_U, GRP_Q)), float(GRP_P)


def grouped_outputs(ctx, name):
    """Two calls in a row (the second waits on the event behind the first one's upload), as arrays."""
    from bigkrls_amd import ops
    A, B, W, sigma = grouped_inputs()
    lab, G = grouped_labels(name)
    dA, dB, dW = ctx.from_numpy(A), ctx.from_numpy(B), ctx.from_numpy(W)
    first = ops.bKernelContractGrouped(dA, dB, dW, sigma, lab, G)
    second = ops.bKernelContractGrouped(dA, dB, dW, sigma, lab, G)
    return first.to_numpy(), second.to_numpy()


def many_entries():
    """130 entries (kind, c, j) over p = 5 columns, all kinds, in no order: tests/ktplan_check.cpp's list."""
    ent = [(i % 3, (i * 7) % 5, ((i * 7) % 5 + 1 + i % 4) % 5) for i in range(130)]
    return np.asarray(ent, dtype=np.int64)


def case_names():
    return list(KERNEL_CASES) + list(GROUPED_CASES) + ["loo_moments_130_p5"]


def run_case(ctx, name):
    """{sub-case: sha256 of the output bytes} of one case."""
    from bigkrls_amd import ops
    if name in KERNEL_CASES:
        what, u, v, p, cols = KERNEL_CASES[name]
        rng = np.random.default_rng(4000 + u + p)
        X = ctx.from_numpy(_uniform(rng, (u, p)))
        if what == "sym":
            return {"K": digest(ops.bGaussKernel(X, float(p), cols=cols).to_numpy())}
        Y = ctx.from_numpy(_uniform(rng, (v, p)))
        return {"K": digest(ops.bTempKernel(X, Y, float(p)).to_numpy())}
    if name in GROUPED_CASES:
        first, second = grouped_outputs(ctx, name)
        return {"first": digest(first), "second": digest(second)}
    if name == "loo_moments_130_p5":
        rng = np.random.default_rng(4200)
        dA, dB = ctx.from_numpy(_uniform(rng, (1100, 5))), ctx.from_numpy(_uniform(rng, (70, 5)))
        return {"scattered": digest(ops.bKernelLooMoments(dA, dB, 5.0, many_entries()).to_numpy())}
    raise KeyError(name)
