"""Seeded runs of the dense eigensolver that pin stage 1 (full matrix to band: Stage1 of csrc/eigen_2stage.inc, dist_s1_*
of csrc/eigen.hip) and SHA-256 digests of what they return, shared by tests/test_gpu_stage1_digests.py and
tools/stage1_digests.py (which records tests/golden/stage1_digests.json).

One case per arm of the schedule (csrc/s1sched.h) and per switch that changes what stage 1 launches: bEigen(K, None,
0.001) of the Gaussian kernel of seeded standardised data. Every bit of the band and of every reflector feeds the n
eigenvalues and the kept eigenvectors, so the digests pin every launch, operand and summation order of stage 1. n is
never a multiple of 64: the ragged last panel is always there. The last two cases are a fit through bigKRLS_dist with one
rank (the row-block distributed stage 1, group path included) and BIGKRLS_S1_SWAP_M=0, which is read once per process
and so runs in a process of its own.

A case runs under BIGKRLS_VERBOSE=1 with the process's stderr collected: "counts" are the figures of the library's
"stage 1 schedule" line (None where the build prints none: the commit the golden file was recorded from, and the
distributed stage 1, whose loop is driven rank by rank from csrc/dist.hip). COUNTS is what csrc/s1sched.h gives for each
case; tests/test_s1sched_cpu.py holds the header to this table, the GPU test holds the loop to it. A case during which the
context's recovery counters moved is run once more; if they move again it fails."""
import contextlib
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

_SWITCHES = ("BIGKRLS_PQ", "BIGKRLS_S1", "BIGKRLS_S1_TPQ", "BIGKRLS_S1AGG", "BIGKRLS_S1AGG_MIN", "BIGKRLS_S1AGG4_MIN",
             "BIGKRLS_S1_GRAPH", "BIGKRLS_EIGK", "BIGKRLS_DIST_EIGEN")

# name: (n, p, seed, switches)
CASES = {
    "n1100": (1100, 7, 91, {}),
    "n1100_pq_steps": (1100, 7, 91, {"BIGKRLS_PQ": "steps"}),
    "n1100_pq_householder": (1100, 7, 91, {"BIGKRLS_PQ": "householder"}),
    "n1100_pq_fused": (1100, 7, 91, {"BIGKRLS_PQ": "fused"}),
    "n1100_s1_gemm": (1100, 7, 91, {"BIGKRLS_S1": "gemm"}),
    "n1100_s1_nopanel": (1100, 7, 91, {"BIGKRLS_S1": "nopanel"}),
    "n1100_tpq0": (1100, 7, 91, {"BIGKRLS_S1_TPQ": "0"}),
    "n2100_p2": (2100, 2, 5, {}),
    "n2100_p2_tpq0": (2100, 2, 5, {"BIGKRLS_S1_TPQ": "0"}),
    "n7000": (7000, 7, 91, {}),
    "n13150": (13150, 7, 91, {}),
    "n11300": (11300, 7, 91, {}),
    "n11300_agg0": (11300, 7, 91, {"BIGKRLS_S1AGG": "0"}),
    "n11300_agg2": (11300, 7, 91, {"BIGKRLS_S1AGG": "2"}),
    "n11300_low_thresholds": (11300, 7, 91, {"BIGKRLS_S1AGG_MIN": "9000", "BIGKRLS_S1AGG4_MIN": "9600"}),
    "dist_n13150": (13150, 7, 91, {}),
    "n1100_swap0": (1100, 7, 91, {}),
}

# (groups of four, pair groups, two-stream panels, one-stream panels) by csrc/s1sched.h -- tests/s1sched_check.cpp prints
# them, tests/test_s1sched_cpu.py compares. None: no line (see above).
COUNTS = {
    "n1100": (0, 0, 0, 16),
    "n1100_pq_steps": (0, 0, 16, 0),
    "n1100_pq_householder": (0, 0, 0, 16),
    "n1100_pq_fused": (0, 0, 0, 16),
    "n1100_s1_gemm": (0, 0, 16, 0),
    "n1100_s1_nopanel": (0, 0, 16, 0),
    "n1100_tpq0": (0, 0, 0, 16),
    "n2100_p2": (0, 0, 0, 31),
    "n2100_p2_tpq0": (0, 0, 0, 31),
    "n7000": (0, 0, 12, 96),
    "n13150": (1, 16, 72, 96),
    "n11300": (0, 4, 71, 96),
    "n11300_agg0": (0, 0, 79, 96),
    "n11300_agg2": (0, 4, 71, 96),
    "n11300_low_thresholds": (6, 5, 45, 96),
    "dist_n13150": None,
    "n1100_swap0": (0, 0, 16, 0),
}

SCHEDULE_LINE = re.compile(r"\[bigkrls\] stage 1 schedule: n=(\d+): (\d+) groups of four, (\d+) pair groups, "
                           r"(\d+) two-stream panels, (\d+) one-stream panels")
FALLBACK_LINE = re.compile(r"panels left to the Householder kernel by pq_chol: (\d+)")


def case_names():
    return list(CASES)


@contextlib.contextmanager
def _env(**kv):
    """Exactly these switches of stage 1 for the duration of a case (the library reads them at every call)."""
    saved = {k: os.environ.get(k) for k in _SWITCHES + ("BIGKRLS_VERBOSE",)}
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(kv)
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


def _sha(*parts):
    h = hashlib.sha256()
    for part in parts:
        if isinstance(part, (int, np.integer)):
            h.update(np.int64(part).tobytes())
        else:
            h.update(np.asfortranarray(np.asarray(part, dtype=np.float64)).tobytes(order="F"))
    return h.hexdigest()


def _data(n, p, seed):
    from bigkrls_amd.synth import synth
    X, y = synth(n, p, seed)
    return X, y, (X - X.mean(0)) / X.std(0, ddof=1)


def _once(ctx, name):
    from bigkrls_amd import ops
    n, p, seed, switches = CASES[name]
    X, y, Xs = _data(n, p, seed)
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "stderr.log")
        with _env(**switches), _stderr_to(log):
            if name.startswith("dist_"):
                from bigkrls_amd import dist as bkdist
                out = bkdist.bigKRLS_dist(y, X, ctx=ctx, eigen_mode="dense", derivative=False)
                res = {"digests": {"coeffs": _sha(out["coeffs"]), "lambda": _sha(np.float64(out["lambda"])),
                                   "lastkeeper": _sha(int(out["lastkeeper"]))},
                       "info": {"lastkeeper": int(out["lastkeeper"]), "lambda": float(out["lambda"])}}
            else:
                e = ops.bEigen(ops.bGaussKernel(ctx.from_numpy(Xs), float(p)), None, 0.001)
                values = np.asarray(e.values, dtype=np.float64)
                assert len(values) == n
                res = {"digests": {"values": _sha(values), "vectors": _sha(e.vectors.to_numpy()),
                                   "lastkeeper": _sha(int(e.lastkeeper))},
                       "info": {"lastkeeper": int(e.lastkeeper)}}
        with open(log) as f:
            text = f.read()
    lines = SCHEDULE_LINE.findall(text)
    res["counts"] = [int(v) for v in lines[-1][1:]] if lines else None
    if lines:
        assert all(int(l[0]) == n for l in lines), lines
    fb = FALLBACK_LINE.findall(text)
    if fb:
        res["info"]["fallback_panels"] = int(fb[-1])
    return res


def _run_here(ctx, name):
    for attempt in range(2):
        before = ctx.counters()
        res = _once(ctx, name)
        if ctx.counters() == before:
            return res
    raise AssertionError(f"{name}: the context's recovery counters moved in two runs in a row: {before} -> {ctx.counters()}")


def run_case(ctx, name, lib_path=None):
    """{"digests": {part: sha256}, "info": {...}, "counts": [4 figures] or None} of one case. `lib_path`: the library the
    process of its own loads (default: the tree's)."""
    if name == "n1100_swap0":
        env = dict(os.environ, BIGKRLS_S1_SWAP_M="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name] + ([lib_path] if lib_path else []),
                           stdout=subprocess.PIPE, text=True, timeout=300, env=env)
        assert r.returncode == 0, f"the process of {name} ended with {r.returncode}"
        return json.loads(r.stdout.strip().splitlines()[-1])
    return _run_here(ctx, name)


if __name__ == "__main__":
    assert sys.argv[1] == "n1100_swap0" and os.environ.get("BIGKRLS_S1_SWAP_M") == "0", sys.argv
    sys.path.insert(0, os.path.dirname(HERE))
    import bigkrls_amd._lib as L
    if len(sys.argv) > 2:
        L.LIB_PATH = os.path.abspath(sys.argv[2])
    import bigkrls_amd as bk
    print(json.dumps(_run_here(bk.Context(0), sys.argv[1])))
