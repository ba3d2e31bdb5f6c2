"""The host references of tests/_lambda_search_ref.py and the inputs of tests/test_gpu_lambda_search.py, checked without
the code under test: the control replay against the oracle's search, the loss bound against numpy's own double-precision
evaluation, and for every GPU case the probe count (np.float64 and np.longdouble loss: equal, and the count the case was
chosen for), the launch shape it was chosen for and the room of every comparison of the search (at least 100 loss
bounds). The chain cases reach 47, 48, 49 and 50 probes; the largest count these inputs reach with that room is 51,
which stands in for a case of about 60 (at 60 probes |S1 - S2| is below the loss bound itself). A third chain (more than
96 probes) is out of reach for any input: the interval falls below the spacing of doubles near lambda at about 70."""
import numpy as np
import pytest

from oracle import krls_oracle as orc

import _lambda_search_ref as ref


def test_replay_reproduces_the_oracle_search():
    """The oracle's search (its own bounds loops, its own float64 loss) and the replay of its recorded losses: the same
    lambdas probed, the same count, the same result. The oracle's solver recomputes Q'y on every probe, so this also ties
    Loss.f64 (a hoisted) to it at rounding level."""
    rng = np.random.default_rng(21)
    n, k = 60, 25
    Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    vals = np.sort(rng.uniform(0.01, 50.0, k + 6))[::-1].copy()
    y = rng.standard_normal(n)
    for kw in (dict(), dict(L=0.5, U=20.0, tol=1e-7), dict(L=0.5), dict(U=30.0, tol=1e-3)):
        tr = orc.LambdaTrace(0.0, 0.0)
        lam = orc.lambda_search(orc.EigenObject(values=vals, lastkeeper=k, vectors=Q), y, trace=tr, **kw)
        probes = np.array(tr.probes)
        ref.check_trace(tr.L0, tr.U0, kw.get("tol", 1e-3 * n), probes, len(tr.probes), lam)
        loss = ref.Loss(Q, vals[:k], Q.T @ y)
        assert ref.check_losses(loss, probes) <= 1.0
        assert abs(loss.f64(probes[0, 0]) - probes[0, 1]) <= 2 * loss.ld(probes[0, 0])[1]


def test_replay_notices_a_wrong_trace():
    """What reference A is for: a loss taken from the wrong probe, a lost probe, a duplicated one, a lambda one unit in the
    last place off, a wrong count or result each fail it."""
    cs = ref.case("300x120")
    L, U, tol = cs.bounds()
    lam, asked, _ = ref.search(L, U, tol, lambda x, t: cs.loss.f64(x))
    tr = np.array([(x, cs.loss.f64(x)) for x in asked])
    n = len(asked)
    ref.check_trace(L, U, tol, tr, n, lam)
    swapped = tr.copy()
    swapped[[4, 5], 1] = swapped[[5, 4], 1]
    nudged = tr.copy()
    nudged[7, 0] = np.nextafter(nudged[7, 0], np.inf)
    for bad, nb, lb in ((swapped, n, lam), (np.delete(tr, 6, axis=0), n - 1, lam), (np.insert(tr, 6, tr[6], axis=0), n + 1, lam),
                        (nudged, n, lam), (tr[:-1], n - 1, lam), (tr, n, np.nextafter(lam, 0.0))):
        with pytest.raises((AssertionError, ref.OutOfLosses)):
            ref.check_trace(L, U, tol, bad, nb, lb)


def test_launch_shape_formulae():
    """The numbers the table rows were chosen for, spelt out where they matter."""
    s = ref.launch_shape
    assert s(257, 257)["splits"] == 2 and s(257, 257)["last"] == 1
    assert s(16416, 600) == dict(rows=32, rb=513, splits=2, kps=512, nle=65, last=88)         # two LDS chunks in split 0
    assert s(10000, 600)["kps"] == 256 and s(10000, 600)["splits"] == 3                        # (fewer row blocks: three splits of one chunk)
    assert s(32800, 300)["nle"] == 1025 and s(32800, 300)["kps"] == 512                        # chunks of 256 + 44
    assert s(524288, 3)["rows"] == 32 and s(524289, 3)["rows"] == 256 and s(524289, 3)["nle"] == 2049


@pytest.mark.parametrize("name", list(ref.TABLE))
def test_case_inputs(name):
    """Probe count in both precisions, launch shape and decision room of one GPU case (ref.check_case asserts them)."""
    probes, room = ref.check_case(name)
    cs = ref.case(name)
    assert probes == cs.probes and room >= ref.ROOM
    print(f"{name}: {probes} probes, smallest room {room:.3g} loss bounds")


def test_chain_cases_straddle_the_chain_boundary():
    counts = sorted(ref.CHAIN_TOLS)
    assert counts[:4] == [ref.CHAIN - 1, ref.CHAIN, ref.CHAIN + 1, ref.CHAIN + 2] and counts[-1] > ref.CHAIN + 2
    assert all(ref.case(f"chain{p}").probes == p for p in counts)
