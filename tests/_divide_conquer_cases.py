"""Seeded runs of the dense eigensolver that pin the divide & conquer on the tridiagonal matrix (DivideConquer of
csrc/eigen.hip, its host arithmetic in csrc/dcplan.h) and SHA-256 digests of what they return, shared by
tests/test_gpu_divide_conquer_digests.py and tools/divide_conquer_digests.py (which records
tests/golden/divide_conquer_digests.json).

A case is one ops.bEigen under BIGKRLS_EIGK=dense and BIGKRLS_VERBOSE=1 with the process's stderr collected. It digests
all returned values, the kept vectors and lastkeeper, and keeps as plain data the figures of every "d&c depth" line the
library prints -- [depth, factored?, merges, largest, non-deflated, rotations], in the order printed -- and whether the
"redoing the top levels explicitly" and "factored levels applied to" lines appeared: that pins the path taken (which
levels stay factored, what deflates, what rotates), not only the result. A case during which the context's recovery
counters moved is run once more; if they move again it fails.

The inputs are reproducible to the bit without BLAS or LAPACK (no np.linalg, no @): the identity and Wilkinson's matrix are
exact; a prescribed spectrum D is carried by ONE Householder similarity H = I - 2 u u', written elementwise,
    u = v / ||v||,  s = sum_k u_k^2 D_k,  A_ij = D_i delta_ij - 2 u_i u_j (D_i + D_j) + 4 s u_i u_j,
with both sums by math.fsum and A symmetrised at the end; the kernel cases are bGaussKernel of seeded standardised data,
as in tests/_stage1_cases.py. input_digest() is the digest of what a case uploads; the golden file stores it, and the
test compares it first, so that another numpy is not mistaken for a changed solver.

redo_natural was found on the commit the golden file was recorded from: of P in {10, 20} x eigtrunc in {1e-6, 1e-9} at
n = 4100, the first setting whose root keeps more than n / 8 columns (see REDO_NATURAL_SEARCH)."""
import contextlib
import hashlib
import math
import os
import re
import sys
import tempfile

import numpy as np

_SWITCHES = ("BIGKRLS_DC", "BIGKRLS_DCLEAF", "BIGKRLS_EIGK", "BIGKRLS_EIG", "BIGKRLS_FAULT")

_FACTORED_SHAPES = (("clusters", 1100, 100), ("wilkinson", 1501, 150), ("identity", 640, 64), ("rank3", 900, 20),
                    ("graded", 1024, 128))

# what the search for redo_natural tried, in order, and the setting it kept (index into this list)
REDO_NATURAL_SEARCH = ((10, 1e-6), (10, 1e-9), (20, 1e-6), (20, 1e-9))
REDO_NATURAL_KEPT = 0


def _cases():
    c = {
        "n48_wilkinson": dict(kind="wilkinson", n=48),                     # n <= 64: 1 x 1 leaves, explicit
        "n65_graded": dict(kind="graded", n=65),                           # the first n with QL leaves
        "n300_dcleaf1": dict(kind="graded", n=300, env={"BIGKRLS_DCLEAF": "1"}),
    }
    for kind in ("graded", "clusters", "identity", "rank3", "wilkinson", "negdef"):
        c[f"n777_{kind}"] = dict(kind=kind, n=777)                         # all vectors, explicit
    for mode in ("factored", "explicit"):
        for kind, n, neig in _FACTORED_SHAPES:
            c[f"{mode}_{kind}_{n}_{neig}"] = dict(kind=kind, n=n, neig=neig, env={"BIGKRLS_DC": mode})
    c["kernel_4300_neig200"] = dict(kind="kernel", n=4300, p=6, seed=41, neig=200)           # lazy: n_vecs_max * 8 <= N
    c["kernel_4300_trunc"] = dict(kind="kernel", n=4300, p=6, seed=41, trunc=0.001)          # lazy: keep_thresh > 0
    c["redo_forced_900"] = dict(kind="graded", n=900, env={"BIGKRLS_DC": "factored"})        # all vectors: redone
    p, trunc = REDO_NATURAL_SEARCH[REDO_NATURAL_KEPT]
    c["redo_natural"] = dict(kind="kernel", n=4100, p=p, seed=41, trunc=trunc)
    for case in c.values():
        case.setdefault("neig", None)       # None: all n
        case.setdefault("trunc", -1.0)      # (what bigkrls_eigen passes: no truncation)
        case.setdefault("env", {})
    return c


CASES = _cases()
REDO_CASES = ("redo_forced_900", "redo_natural")

LEVEL_LINE = re.compile(r"d&c depth\s+(\d+)( \(factored\))?:\s+(\d+) merges, largest\s+(\d+) "
                        r"\(non-deflated\s+(\d+), (\d+) rotations\)")
REDO_LINE = "redoing the top levels explicitly"
APPLIED_LINE = "factored levels applied to"


def case_names():
    return list(CASES)


def _spectrum(kind, n, rng):
    if kind == "graded":
        return np.logspace(0, -16, n)
    if kind == "clusters":
        return np.r_[1 + 1e-13 * rng.standard_normal(n // 2), 2 + 1e-13 * rng.standard_normal(n - n // 2)]
    if kind == "rank3":
        return np.r_[[5.0, 3.0, 1.0], 1e-14 * rng.random(n - 3)]
    if kind == "negdef":
        return -np.logspace(0, -10, n)
    raise ValueError(kind)


def _with_spectrum(D, v):
    """H diag(D) H for the Householder reflector H = I - 2 u u', u = v / ||v||, elementwise."""
    u = v / math.sqrt(math.fsum((v * v).tolist()))
    s = math.fsum(((u * u) * D).tolist())
    uu = u[:, None] * u[None, :]
    A = (-2.0 * uu) * (D[:, None] + D[None, :]) + (4.0 * s) * uu
    idx = np.arange(len(D))
    A[idx, idx] = A[idx, idx] + D
    return (A + A.T) / 2


def make_input(name):
    """What the case uploads: the n x n matrix, or the standardised n x p data of a kernel case."""
    case = CASES[name]
    kind, n = case["kind"], case["n"]
    if kind == "kernel":
        from bigkrls_amd.synth import synth
        X, _y = synth(n, case["p"], case["seed"])
        return (X - X.mean(0)) / X.std(0, ddof=1)
    if kind == "identity":
        return np.eye(n)
    if kind == "wilkinson":
        A = np.zeros((n, n))
        idx = np.arange(n)
        A[idx, idx] = np.abs(idx - n // 2).astype(float)
        A[idx[:-1], idx[:-1] + 1] = 1.0
        A[idx[:-1] + 1, idx[:-1]] = 1.0
        return A
    rng = np.random.default_rng(n)
    D = _spectrum(kind, n, rng)
    return _with_spectrum(D, rng.standard_normal(n))


def _sha(*parts):
    h = hashlib.sha256()
    for part in parts:
        if isinstance(part, (int, np.integer)):
            h.update(np.int64(part).tobytes())
        else:
            h.update(np.asfortranarray(np.asarray(part, dtype=np.float64)).tobytes(order="F"))
    return h.hexdigest()


def input_digest(name):
    return _sha(make_input(name))


@contextlib.contextmanager
def _env(**kv):
    """Exactly these switches of the divide & conquer for the duration of a case (the library reads them at every call)."""
    saved = {k: os.environ.get(k) for k in _SWITCHES + ("BIGKRLS_VERBOSE",)}
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(kv)
    os.environ["BIGKRLS_EIGK"] = "dense"
    os.environ["BIGKRLS_VERBOSE"] = "1"
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@contextlib.contextmanager
def _stderr_to(path):
    """File descriptor 2 of this process appended to `path` for the duration."""
    sys.stderr.flush()
    saved = os.dup(2)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_APPEND, 0o644)
    os.dup2(fd, 2)
    os.close(fd)
    try:
        yield
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        os.close(saved)


def parse_path(text):
    """The figures of the "d&c depth" lines, in the order printed, and which of the two other lines appeared."""
    levels = [[int(m[0]), bool(m[1]), int(m[2]), int(m[3]), int(m[4]), int(m[5])] for m in LEVEL_LINE.findall(text)]
    return {"levels": levels, "redo": REDO_LINE in text, "applied": APPLIED_LINE in text}


def _once(ctx, name, A):
    from bigkrls_amd import ops
    case = CASES[name]
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "stderr.log")
        with _env(**case["env"]), _stderr_to(log):
            M = ctx.from_numpy(A)
            if case["kind"] == "kernel":
                M = ops.bGaussKernel(M, float(case["p"]))
            e = ops.bEigen(M, case["neig"], case["trunc"])
            values = np.asarray(e.values, dtype=np.float64)
            vectors = e.vectors.to_numpy()
        with open(log) as f:
            text = f.read()
    assert len(values) == (case["neig"] or case["n"])
    return {"digests": {"values": _sha(values), "vectors": _sha(vectors), "lastkeeper": _sha(int(e.lastkeeper))},
            "info": {"lastkeeper": int(e.lastkeeper)}, "path": parse_path(text)}


def run_case(ctx, name, A=None):
    """{"input": sha256, "digests": {part: sha256}, "info": {...}, "path": {"levels": [...], "redo", "applied"}}."""
    if A is None:
        A = make_input(name)
    for _attempt in range(2):
        before = ctx.counters()
        res = _once(ctx, name, A)
        if ctx.counters() == before:
            res["input"] = _sha(A)
            return res
    raise AssertionError(f"{name}: the context's recovery counters moved in two runs in a row: {before} -> {ctx.counters()}")


if __name__ == "__main__":
    # the input digests alone (no GPU): one line per case
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for _name in case_names():
        print(_name, input_digest(_name))
