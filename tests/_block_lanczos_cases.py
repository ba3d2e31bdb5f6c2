"""Seeded runs of the block Lanczos eigensolver (eigen_krylov of csrc/eigen.hip) and SHA-256 digests of what they return,
shared by tests/test_gpu_block_lanczos_digests.py and tools/block_lanczos_digests.py (which records
tests/golden/block_lanczos_digests.json).

One case per path through the iteration: the plain loop with the sample check against K, the eigtrunc count, one part
of three of the eigenvector columns, the Rayleigh-Ritz refinement, a fit (whose own check replaces the sample check),
the implicit operator, the auto rank and its cap error, a numerically low-rank kernel (re-orthogonalised and replaced
blocks; a breakdown short of Neig columns), the hand-over of a non-converged iteration to the dense path (test build of
the library, in a process of its own: the library path is per process; BIGKRLS_FAULT_LIB names another test build than
the tree's), the row-sharded form with one rank, and the compressed estimate check (twice: it forecasts, it reports
convergence). Data are oracle.synth, standardised as the fit does; N < 16384 takes the iteration with
BIGKRLS_EIGK=krylov.

A digest covers the bytes of the eigenvalues, of the kept eigenvectors (N x lastkeeper, column-major as returned),
lastkeeper and the number of values; of coeffs, lambda and lastkeeper for a fit; of the status and the whole error text
for an error. MARKERS names the BIGKRLS_VERBOSE lines that show which path a run took; REQUIRED lists, per case, the
ones the recording must show ("!name": must not show)."""
import contextlib
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MARKERS = {
    "lanczos": "[bigkrls] block Lanczos: n=",
    "check": "[bigkrls] block Lanczos check:",
    "sample_check": "block Lanczos: true residual of the last",
    "auto_rank": "[bigkrls] block Lanczos (auto rank):",
    "reorthogonalised": ") re-orthogonalised",
    "random_block": "continued with a random block",
    "estimate": "[bigkrls] block Lanczos estimate:",
    "dense_handover": "[bigkrls] block Lanczos did not converge: dense path",
}

# (a fit, and BIGKRLS_KRY_REFINE=1, leave the sample check out: its line must be absent)
REQUIRED = {
    "stored_fixed": ["lanczos", "check", "sample_check"],
    "stored_trunc": ["lanczos", "sample_check"],
    "stored_part": ["lanczos", "sample_check"],
    "stored_refine": ["lanczos", "!sample_check"],
    "fit_caller_verifies": ["lanczos", "!sample_check"],
    "implicit": ["lanczos", "sample_check"],
    "auto_rank": ["lanczos", "auto_rank"],
    "auto_rank_cap": ["!lanczos"],
    "low_rank_replace": ["lanczos", "reorthogonalised", "random_block"],
    "low_rank_breakdown": ["lanczos"],
    "noconv_fallback": ["lanczos", "dense_handover"],
    "dist_world1": ["lanczos"],
    "estimate": ["lanczos", "estimate"],
    "estimate_then_full": ["lanczos", "estimate"],
}
# what the error text of the two error cases must hold (the digest covers all of it)
ERROR_TEXT = {"auto_rank_cap": "more than kcap = 100 eigenvalues reach the threshold",
              "low_rank_breakdown": "breakdown with a subspace smaller than the number of requested pairs"}

N, P, NEIG = 4608, 6, 128
# The smallest N (from 2048, in steps of 1024) at which the two low-rank kernels show their lines on the commit the golden
# file was recorded from (P = 2, Neig = 512 breaks down short of Neig columns at 2048 and 3072).
N_LOW_RANK_REPLACE = 4096
N_LOW_RANK_BREAKDOWN = 2048
# (N, P) at which the first check, moved to step 8 (BIGKRLS_KRY_FIRST_CHECK), still sits on the plateau of the worst
# residual and forecasts four more steps, so that the check at step 12 is the compressed estimate (640 instead of 1536
# columns). P = 10 and 20 at N = 4608 and 8192 have left the plateau by step 8 (forecasts of two and three steps: no
# estimate); P = 50 has not. At (8192, 30) the estimate itself reports convergence and the full check follows at once.
ESTIMATE_SHAPE = (4608, 50)
ESTIMATE_THEN_FULL_SHAPE = (8192, 30)

_SWITCHES = ("BIGKRLS_EIGK", "BIGKRLS_FAULT", "BIGKRLS_KRY_FIRST_CHECK", "BIGKRLS_KRY_CGS", "BIGKRLS_KRY_PIVOTS",
             "BIGKRLS_KRY_NOEST", "BIGKRLS_KRY_CHECK_EVERY", "BIGKRLS_KRY_REFINE", "BIGKRLS_KRY_SAMPLE")


def case_names():
    return list(REQUIRED)


@contextlib.contextmanager
def _env(**kv):
    """Exactly these switches of the iteration for the duration of a case (the library reads them at every call)."""
    saved = {k: os.environ.get(k) for k in _SWITCHES}
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _sha(*parts):
    h = hashlib.sha256()
    for part in parts:
        if isinstance(part, str):
            h.update(part.encode())
        elif isinstance(part, (int, np.integer)):
            h.update(np.int64(part).tobytes())
        else:
            h.update(np.asfortranarray(np.asarray(part, dtype=np.float64)).tobytes(order="F"))
    return h.hexdigest()


def _data(n, p, seed):
    from oracle import krls_oracle as orc
    X, y = orc.synth(n, p, seed)
    return X, y, (X - X.mean(0)) / X.std(0, ddof=1)


def _kernel(ctx, n, p, seed):
    from bigkrls_amd import ops
    return ops.bGaussKernel(ctx.from_numpy(_data(n, p, seed)[2]), float(p))


def _eig(call):
    """Digests of an Eigenobject, or of the error the call ends in."""
    from bigkrls_amd import _lib
    try:
        e = call()
    except _lib.BigKRLSError as err:
        return {"digests": {"error": _sha(int(err.code), str(err))}, "info": {"status": int(err.code), "error": str(err)}}
    values = np.asarray(e.values, dtype=np.float64)
    return {"digests": {"values": _sha(values), "vectors": _sha(e.vectors.to_numpy()),
                        "counts": _sha(int(e.lastkeeper), int(len(values)))},
            "info": {"lastkeeper": int(e.lastkeeper), "rank": int(len(values))}}


def _fit(out):
    return {"digests": {"coeffs": _sha(out["coeffs"]), "lambda": _sha(np.float64(out["lambda"])),
                        "lastkeeper": _sha(int(out["lastkeeper"]))},
            "info": {"lastkeeper": int(out["lastkeeper"]), "lambda": float(out["lambda"])}}


def _noconv_fallback_here():
    """(in the process of its own) auto rank on the stored kernel: the one route on which the default choice takes the
    iteration at N = 4608; BIGKRLS_FAULT=noconv lets it report non-convergence, the same call decomposes densely."""
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    ctx = bk.Context(0)
    with _env(BIGKRLS_FAULT="noconv"):
        Xs = ctx.from_numpy(_data(N, P, 31)[2])
        return _eig(lambda: ops.bEigenAuto(Xs, float(P), 1e-3, K=ops.bGaussKernel(Xs, float(P))))


def run_case(ctx, name):
    """{"digests": {part: sha256}, "info": {...}} of one case (info: plain figures, for the reader of the golden file)."""
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    if name == "stored_fixed":
        with _env(BIGKRLS_EIGK="krylov"):
            return _eig(lambda: ops.bEigen(_kernel(ctx, N, P, 31), NEIG, 0.0))
    if name == "stored_trunc":
        with _env(BIGKRLS_EIGK="krylov"):
            return _eig(lambda: ops.bEigen(_kernel(ctx, 5000, 10, 31), 300, 1e-3))
    if name == "stored_part":          # part 1 of 3 of the kept columns: the other parts' columns come back as zeros
        with _env(BIGKRLS_EIGK="krylov"):
            return _eig(lambda: ops.bEigen(_kernel(ctx, N, P, 31), NEIG, 0.0, part=(1, 3)))
    if name == "stored_refine":
        with _env(BIGKRLS_EIGK="krylov", BIGKRLS_KRY_REFINE="1"):
            return _eig(lambda: ops.bEigen(_kernel(ctx, N, P, 31), NEIG, 0.0))
    if name == "fit_caller_verifies":
        X, y, _ = _data(N, P, 31)
        with _env(BIGKRLS_EIGK="krylov"):
            return _fit(bk.bigKRLS(y, X, Neig=NEIG, ctx=ctx, noisy=False, derivative=False))
    if name == "implicit":
        with _env():
            return _eig(lambda: ops.bEigenImplicit(ctx.from_numpy(_data(N, P, 31)[2]), float(P), NEIG, 0.0))
    if name in ("auto_rank", "auto_rank_cap"):
        with _env():
            return _eig(lambda: ops.bEigenAuto(ctx.from_numpy(_data(N, P, 31)[2]), float(P), 1e-3,
                                               max_pairs=100 if name == "auto_rank_cap" else None))
    if name == "low_rank_replace":
        with _env(BIGKRLS_EIGK="krylov"):
            return _eig(lambda: ops.bEigen(_kernel(ctx, N_LOW_RANK_REPLACE, 2, 41), 512, 1e-3))
    if name == "low_rank_breakdown":
        with _env(BIGKRLS_EIGK="krylov"):
            return _eig(lambda: ops.bEigen(_kernel(ctx, N_LOW_RANK_BREAKDOWN, 1, 41), 256, 1e-3))
    if name == "noconv_fallback":
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name], stdout=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, f"the process of {name} ended with {r.returncode}"
        return json.loads(r.stdout.strip().splitlines()[-1])
    if name == "dist_world1":
        from bigkrls_amd import dist as bkdist
        X, y, _ = _data(4500, 6, 52)
        with _env():
            return _fit(bkdist.bigKRLS_dist(y, X, Neig=96, ctx=ctx, eigen_mode="krylov"))
    if name in ("estimate", "estimate_then_full"):
        n, p = ESTIMATE_SHAPE if name == "estimate" else ESTIMATE_THEN_FULL_SHAPE
        with _env(BIGKRLS_EIGK="krylov", BIGKRLS_KRY_FIRST_CHECK="8"):
            return _eig(lambda: ops.bEigen(_kernel(ctx, n, p, 31), NEIG, 0.0))
    raise KeyError(name)


if __name__ == "__main__":
    assert sys.argv[1:] == ["noconv_fallback"], sys.argv
    sys.path.insert(0, os.path.dirname(HERE))
    import bigkrls_amd._lib as L
    L.LIB_PATH = os.environ.get("BIGKRLS_FAULT_LIB", os.path.join(HERE, "capi", "libbigkrls_hip_fault.so"))
    print(json.dumps(_noconv_fallback_here()))
