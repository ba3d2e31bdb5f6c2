"""The fused kernel contraction for more than 64 operand columns (kernel_contract_wide_kernel, csrc/gemm.hip): the
kernel behind the products of a fit that never stores K. Same construction and tolerance as
test_kernel_contract_matches_unfused_chain (tests/test_gpu_marginal_effects.py): bigkrls_dev_kernel_contract against
kernel_block followed by bigkrls_dev_gemm."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _wide_cases():
    """Every u and v of {17, 513, 4099} (one tile that is not full, several blocks with a ragged edge, enough rows for
    the loop to be split), with P and q cycling through P in {1, 20, 33, 67} (resident fragments with KS = 1 and 5, and
    the re-reading path) and q in {65, 127, 128, 129, 200} (a partial chunk, a full one, a full one plus a partial)."""
    ps, qs = [1, 20, 33, 67], [65, 127, 128, 129, 200]
    out, i = [], 0
    for u in (17, 513, 4099):
        for v in (17, 513, 4099):
            out.append((u, v, ps[i % 4], qs[i % 5]))
            i += 1
    # the pairs of (P, q) the cycle above leaves out, at the middle size
    seen = {(p, q) for _, _, p, q in out}
    out += [(513, 513, p, q) for p in ps for q in qs if (p, q) not in seen]
    return out


def _contract_vs_chain(ctx, A, B, W, sigma, trans):
    from bigkrls_amd import ops, _lib
    dA, dB, dW = ctx.from_numpy(A), ctx.from_numpy(B), ctx.from_numpy(W)
    u, v, q = A.shape[0], B.shape[0], W.shape[1]
    K = ops.bTempKernel(dA, dB, sigma)                                    # kernel_block, diag_shift = -1
    got = ops.bKernelContract(dA, dB, dW, sigma, trans=trans).to_numpy()
    m = u if trans == 0 else v
    ref = ctx.empty(m, q)
    _lib.call("bigkrls_dev_gemm", ctx.handle, trans, 0, m, q, v if trans == 0 else u, 1.0, K.ptr, K.ld,
              dW.ptr, dW.ld, 0.0, ref.ptr, ref.ld)
    assert got.shape == (m, q)
    return got, ref.to_numpy()


@pytest.mark.parametrize("u,v,p,q", _wide_cases())
def test_wide_contract_matches_unfused_chain(ctx, u, v, p, q):
    rng = np.random.default_rng(u * 7919 + v * 31 + p * 3 + q)
    A = rng.standard_normal((u, p)) * 0.7
    B = rng.standard_normal((v, p)) * 0.7
    for trans in (0, 1):
        W = rng.standard_normal((v if trans == 0 else u, q))
        got, ref = _contract_vs_chain(ctx, A, B, W, float(p), trans)
        err = rel(got, ref)
        print(f"u={u} v={v} p={p} q={q} trans={trans}: relative error {err:.3e}")
        assert err < 1e-13, (trans, u, v, p, q)


def test_wide_contract_on_data_that_are_not_centred(ctx):
    """Rows near 1e5: |a|^2 + |b|^2 - 2 a.b would cancel; the contraction centres its operands like kernel_block."""
    rng = np.random.default_rng(99)
    u, v, p, q = 513, 4099, 20, 128
    A = rng.standard_normal((u, p)) * 0.7 + 1e5
    B = rng.standard_normal((v, p)) * 0.7 + 1e5
    for trans in (0, 1):
        W = rng.standard_normal((v if trans == 0 else u, q))
        got, ref = _contract_vs_chain(ctx, A, B, W, float(p), trans)
        err = rel(got, ref)
        print(f"not centred, trans={trans}: relative error {err:.3e}")
        assert err < 1e-13, trans


@pytest.mark.parametrize("u,v,p,q", [(4099, 4099, 20, 128), (513, 4099, 67, 200)])
def test_wide_contract_is_bitwise_reproducible(ctx, u, v, p, q):
    """The loop splits are reduced in a fixed order (no atomics): two calls give the same bits."""
    from bigkrls_amd import ops
    rng = np.random.default_rng(5)
    dA, dB = ctx.from_numpy(rng.standard_normal((u, p))), ctx.from_numpy(rng.standard_normal((v, p)))
    dW = ctx.from_numpy(rng.standard_normal((v, q)))
    one = ops.bKernelContract(dA, dB, dW, float(p), trans=0).to_numpy()
    two = ops.bKernelContract(dA, dB, dW, float(p), trans=0).to_numpy()
    assert np.array_equal(one, two)


def test_profile_names_the_kernel_that_ran(ctx):
    """q = 128 runs under the profile name kernel_contract_wide, q = 21 under kernel_contract."""
    from bigkrls_amd import ops
    rng = np.random.default_rng(6)
    dA, dB = ctx.from_numpy(rng.standard_normal((513, 20))), ctx.from_numpy(rng.standard_normal((600, 20)))
    try:
        ctx.set_profile(True)
        ops.bKernelContract(dA, dB, ctx.from_numpy(rng.standard_normal((600, 128))), 20.0)
        assert ctx.get_profile("kernel_contract_wide")[2] > 0
        assert ctx.get_profile("kernel_contract")[2] == 0
        ctx.set_profile(True)                                             # (enabling clears the samples)
        ops.bKernelContract(dA, dB, ctx.from_numpy(rng.standard_normal((600, 21))), 20.0)
        assert ctx.get_profile("kernel_contract_wide")[2] == 0
        assert ctx.get_profile("kernel_contract")[2] > 0
    finally:
        ctx.set_profile(False)
