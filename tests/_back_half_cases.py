"""Seeded runs of the dense eigensolver that pin its back half -- band to tridiagonal (stage2_to_tridiag), the stage-2
back-transform (bt2_build_t, back_transform_stage2) and the stage-1 back-transform (bt1_precompute,
back_transform_stage1_grouped / back_transform_stage1) of csrc/eigen_2stage.inc, their host arithmetic in csrc/s2plan.h
-- and SHA-256 digests of what they return, shared by tests/test_gpu_back_half_digests.py and tools/back_half_digests.py
(which records tests/golden/back_half_digests.json).

A case is one ops.bEigen of the Gaussian kernel of seeded standardised data under BIGKRLS_EIGK=dense, as in
tests/_stage1_cases.py. It digests all n values, the kept vectors and lastkeeper. Every bit of every reflector of stage 2
and of both back-transforms feeds them, so the digests pin every launch, operand and summation order of the back half.

    n = 259    the smallest two-stage size: three panels, one merged group of three
    n = 1100   17 panels, merged groups of 8, 8 and 1 (the one-panel group skips its Gram product), 35 reflector groups
               of 32, no multiple of 64; once with eigtrunc = 0.001 (one 64-column slab), once with all n vectors
               (18 slabs, the last 12 columns wide); the all-vectors shape on every arm of BIGKRLS_BC / BIGKRLS_BC_T,
               BIGKRLS_BT2 / BIGKRLS_BT2_SEG and BIGKRLS_BT1, and as part 0 and part 1 of a two-part column split
               (bigkrls_dev_eigen_part: pnv, the slab count and the zeroed columns)
    n = 8100   defaults, eigtrunc = 0.001: the size rule n > BT2_CHAIN_MIN_N, reached without a switch
BIGKRLS_BT1_GRP is read once per process, so its two cases run in a process of their own.

input_digest() is the digest of what a case uploads; the golden file stores it, and the test compares it first, so that
another numpy is not mistaken for a changed solver. A case during which the context's recovery counters moved is run
once more; if they move again it fails."""
import contextlib
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

_SWITCHES = ("BIGKRLS_BC", "BIGKRLS_BC_T", "BIGKRLS_BT2", "BIGKRLS_BT2_SEG", "BIGKRLS_BT1", "BIGKRLS_EIG", "BIGKRLS_EIGK",
             "BIGKRLS_S1", "BIGKRLS_PQ", "BIGKRLS_DC", "BIGKRLS_DCLEAF", "BIGKRLS_FAULT")
_PER_PROCESS = "BIGKRLS_BT1_GRP"

ALL = -1.0          # eigtrunc that keeps all n vectors (what bigkrls_eigen passes: no truncation)
P, SEED = 7, 91     # (data columns, seed) of every case that does not name its own


def _cases():
    c = {
        "n259": dict(n=259, trunc=ALL),
        "n1100_trunc": dict(n=1100, trunc=0.001, p=2, seed=5),      # 31 of its eigenvalues are above the threshold
        "n1100": dict(n=1100, trunc=ALL),
        "n1100_bc_lds": dict(n=1100, trunc=ALL, env={"BIGKRLS_BC": "lds"}),
        "n1100_bc_lds_t256": dict(n=1100, trunc=ALL, env={"BIGKRLS_BC": "lds", "BIGKRLS_BC_T": "256"}),
        "n1100_bc_persistent": dict(n=1100, trunc=ALL, env={"BIGKRLS_BC": "persistent"}),
        "n1100_bc_wavefront": dict(n=1100, trunc=ALL, env={"BIGKRLS_BC": "wavefront"}),
        "n1100_bt2_chain": dict(n=1100, trunc=ALL, env={"BIGKRLS_BT2": "chain"}),
        "n1100_bt2_chain_seg3": dict(n=1100, trunc=ALL, env={"BIGKRLS_BT2": "chain", "BIGKRLS_BT2_SEG": "3"}),
        "n1100_bt2_wavefront": dict(n=1100, trunc=ALL, env={"BIGKRLS_BT2": "wavefront"}),
        "n1100_bt2_seq": dict(n=1100, trunc=ALL, env={"BIGKRLS_BT2": "seq"}),
        "n1100_bt1_panel": dict(n=1100, trunc=ALL, env={"BIGKRLS_BT1": "panel"}),
        "n1100_bt1_grp2": dict(n=1100, trunc=ALL, own_process={_PER_PROCESS: "2"}),
        "n1100_bt1_grp4": dict(n=1100, trunc=ALL, own_process={_PER_PROCESS: "4"}),
        "n8100_trunc": dict(n=8100, trunc=0.001),
        "n1100_part0of2": dict(n=1100, trunc=ALL, part=(0, 2)),
        "n1100_part1of2": dict(n=1100, trunc=ALL, part=(1, 2)),
    }
    for case in c.values():
        case.setdefault("p", P)
        case.setdefault("seed", SEED)
        case.setdefault("env", {})
        case.setdefault("own_process", None)
        case.setdefault("part", None)
    return c


CASES = _cases()


def case_names():
    return list(CASES)


def make_input(name):
    """What the case uploads: the standardised n x p data."""
    from bigkrls_amd.synth import synth
    X, _y = synth(CASES[name]["n"], CASES[name]["p"], CASES[name]["seed"])
    return (X - X.mean(0)) / X.std(0, ddof=1)


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
    """Exactly these switches of the dense eigensolver for the duration of a case (the library reads them at every call)."""
    saved = {k: os.environ.get(k) for k in _SWITCHES}
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(kv)
    os.environ["BIGKRLS_EIGK"] = "dense"
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _once(ctx, name, Xs):
    from bigkrls_amd import ops
    case = CASES[name]
    n = case["n"]
    with _env(**case["env"]):
        e = ops.bEigen(ops.bGaussKernel(ctx.from_numpy(Xs), float(case["p"])), None, case["trunc"], part=case["part"])
        values = np.asarray(e.values, dtype=np.float64)
        vectors = e.vectors.to_numpy()
    assert len(values) == n
    return {"digests": {"values": _sha(values), "vectors": _sha(vectors), "lastkeeper": _sha(int(e.lastkeeper))},
            "info": {"lastkeeper": int(e.lastkeeper)}}


def _run_here(ctx, name, Xs):
    for _attempt in range(2):
        before = ctx.counters()
        res = _once(ctx, name, Xs)
        if ctx.counters() == before:
            res["input"] = _sha(Xs)
            return res
    raise AssertionError(f"{name}: the context's recovery counters moved in two runs in a row: {before} -> {ctx.counters()}")


def run_case(ctx, name, Xs=None, lib_path=None):
    """{"input": sha256, "digests": {part: sha256}, "info": {...}} of one case. `lib_path`: the library a process of its
    own loads (default: the tree's)."""
    own = CASES[name]["own_process"]
    if own:
        env = dict(os.environ, **own)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name] + ([lib_path] if lib_path else []),
                           stdout=subprocess.PIPE, text=True, timeout=300, env=env)
        assert r.returncode == 0, f"the process of {name} ended with {r.returncode}"
        return json.loads(r.stdout.strip().splitlines()[-1])
    assert _PER_PROCESS not in os.environ, f"{_PER_PROCESS} is set for the whole process: {name} would not run its own arm"
    return _run_here(ctx, name, make_input(name) if Xs is None else Xs)


if __name__ == "__main__":
    _name = sys.argv[1]
    assert CASES[_name]["own_process"] and all(os.environ.get(k) == v for k, v in CASES[_name]["own_process"].items()), sys.argv
    sys.path.insert(0, os.path.dirname(HERE))
    import bigkrls_amd._lib as L
    if len(sys.argv) > 2:
        L.LIB_PATH = os.path.abspath(sys.argv[2])
    import bigkrls_amd as bk
    print(json.dumps(_run_here(bk.Context(0), _name, make_input(_name))))
