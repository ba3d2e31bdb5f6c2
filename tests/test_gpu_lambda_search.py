"""bigkrls_dev_lambda_search (csrc/solveforc.hip) called directly: the golden-section search whose control flow runs on
the device, a chain of 48 probe launches and a closing launch, resumed by the host until the search is done.

Every search is run once with a trace and held to the two host references of tests/_lambda_search_ref.py (derivations
in its docstring):
  A. R's loop replayed on the recorded losses probes the recorded lambdas bit for bit, stops after *h_nprobes losses and
     returns *h_lambda;
  B. every recorded loss lies within the derived forward bound of the np.longdouble loss at its lambda.
No tolerance here is a measured number: each is that bound or bit equality. The cases, the launch shape each was chosen
for and their probe counts are tests/_lambda_search_ref.TABLE; tests/test_lambda_search_ref_cpu.py checks on the host
that every comparison of every case is decided with at least 100 bounds of room, so A cannot hinge on a rounding of the
device. Q is a sub-block of a NaN-filled parent (tests/_placement.py: odd ldq > n, first element 8- but not 16-byte
aligned); d and a are plain vectors; the eigenvalues for the bounds loops are a host array, longer than k in the cases
with extra eigenvalues (quirk Q5).

The chain cases reach 47, 48, 49, 50 and 51 probes: the last probe before the closing launch, the one it consumes, the
first of the second chain (whose launches find state and losses in the other buffer of each pair: a chain is 49
launches) and beyond. 51 is the largest count these inputs reach with the required room; a third chain is out of reach
of any input (the interval falls below the spacing of doubles at about 70 probes). The row-block search with a
communicator is not reachable through this entry (tests/test_gpu_fit.py runs it at world size 1)."""
import ctypes as C

import numpy as np
import pytest

from bigkrls_amd import _lib, ops

import _lambda_search_ref as ref
from _placement import SENT, place

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -53
ROOM = 96                   # trace entries offered to the entry (no search takes more than about 70 probes)


def vec(ctx, v):
    return ctx.from_numpy(np.asarray(v, dtype=np.float64).reshape(-1, 1))


def hptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Device:
    """One case's operands on the device."""

    def __init__(self, ctx, cs, a=None):
        self.ctx, self.cs = ctx, cs
        self.parent, self.pQ, self.ldq, _, _ = place(ctx, cs.Q)
        assert self.ldq % 2 == 1 and self.ldq > cs.n
        self.d, self.a = vec(ctx, cs.d), vec(ctx, cs.a if a is None else a)

    def search(self, L, U, tol, vals="all", max_trace=ROOM, trace=True, count=True, status=False, **over):
        """One call of the entry; `over` replaces single arguments (the rejection tests). Returns a dict."""
        cs = self.cs
        vals = cs.vals_all if isinstance(vals, str) else vals
        buf = np.full(2 * ROOM + 8, SENT)
        lam, npr = C.c_double(SENT), C.c_int64(-7)
        args = dict(Q=self.pQ, n=cs.n, k=cs.k, ldq=self.ldq, d=self.d.ptr, a=self.a.ptr, vals=hptr(vals),
                    n_vals=0 if vals is None else vals.size, L=L, U=U, tol=tol, lam=C.byref(lam),
                    npr=C.byref(npr) if count else None, trace=hptr(buf) if trace else None, max_trace=max_trace)
        args.update(over)
        rc = _lib.load().bigkrls_dev_lambda_search(self.ctx.handle, *[args[x] for x in (
            "Q", "n", "k", "ldq", "d", "a", "vals", "n_vals", "L", "U", "tol", "lam", "npr", "trace", "max_trace")])
        if not status:
            _lib.check(rc)
        msg = _lib.load().bigkrls_last_error()
        return dict(rc=rc, msg=msg.decode() if msg else "", lam=lam.value, n=npr.value, buf=buf)


def full_trace(out):
    """The n recorded probes of a search run with room for all of them; the rest of the buffer still holds the sentinel."""
    n = out["n"]
    assert 2 <= n <= ROOM
    assert (out["buf"][2 * n:] == SENT).all(), "trace entries written past the probe count"
    return out["buf"][:2 * n].reshape(-1, 2).copy()


def same_bits(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64).view(np.uint64), np.asarray(y, dtype=np.float64).view(np.uint64))


# ---- the table of shapes and the chain cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.TABLE))
def test_search_case(ctx, name):
    cs = ref.case(name)
    assert ref.launch_shape(cs.n, cs.k) == cs.shape, "the case no longer reaches the launch shape it was chosen for"
    dev = Device(ctx, cs)
    L, U, tol = cs.bounds()
    out = dev.search(cs.L, cs.U, cs.tol)
    tr = full_trace(out)
    print(f"{name}: {out['n']} probes, lambda {out['lam']!r}")
    ref.check_trace(L, U, tol, tr, out["n"], out["lam"])                       # A
    worst = ref.check_losses(cs.loss, tr, name)                                 # B
    print(f"{name}: largest error / bound over the probes {worst:.3g}")
    assert out["n"] == cs.probes, (name, out["n"], cs.probes)


# ---- the output contract (257 x 257: two splits, the finish kernel) ------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    cs = ref.case("257x257")
    dev = Device(ctx, cs)
    L, U, tol = cs.bounds()
    out = dev.search(L, U, tol)
    tr = full_trace(out)
    ref.check_trace(L, U, tol, tr, out["n"], out["lam"])
    assert out["n"] == cs.probes
    return dev, (L, U, tol), out, tr


def test_derived_bounds(ctx, small):
    """h_L = h_U = -1: the search starts from exactly the bounds of bigkrls_lambda_bounds; likewise with one of them given."""
    dev, (L, U, tol), _, _ = small
    cs = dev.cs
    L0, U0 = ops.lambda_bounds(cs.vals_all, cs.n)
    assert (L0, U0) == (L, U)
    for hl, hu, l, u in ((-1.0, -1.0, L0, U0), (-1.0, 150.0, L0, 150.0), (0.7, -1.0, 0.7, U0)):
        out = dev.search(hl, hu, tol)
        ref.check_trace(l, u, tol, full_trace(out), out["n"], out["lam"])
        assert out["n"] > 2
    # Q5: the bounds come from ALL eigenvalues, not from the k the search uses
    longer = np.concatenate([cs.vals_all, [0.004, 0.002, 0.001]])
    L1, U1 = ops.lambda_bounds(longer, cs.n)
    out = dev.search(-1.0, -1.0, tol, vals=longer)
    ref.check_trace(L1, U1, tol, full_trace(out), out["n"], out["lam"])


def test_given_bounds_need_no_eigenvalues(ctx, small):
    dev, (L, U, tol), full, tr = small
    out = dev.search(L, U, tol, vals=None)
    assert out["n"] == full["n"] and same_bits(out["lam"], full["lam"]) and same_bits(full_trace(out), tr)


def test_default_tolerance(ctx, small):
    """h_tol = -1 and h_tol = 0 are 1e-3 n (R/bigKRLS_Rcpp_functions.R:11-12)."""
    dev, (L, U, _), _, _ = small
    outs = [dev.search(L, U, t) for t in (-1.0, 0.0, 1e-3 * dev.cs.n)]
    for out in outs:
        ref.check_trace(L, U, 1e-3 * dev.cs.n, full_trace(out), out["n"], out["lam"])
        assert out["n"] == outs[0]["n"] and same_bits(out["buf"], outs[0]["buf"])


def test_short_trace(ctx, small):
    """max_trace below the probe count: exactly 2 max_trace doubles, the head of the full trace; the count stays whole."""
    dev, (L, U, tol), full, tr = small
    for m in (1, 5, full["n"] - 1, full["n"]):
        out = dev.search(L, U, tol, max_trace=m)
        assert out["n"] == full["n"] and same_bits(out["lam"], full["lam"])
        assert same_bits(out["buf"][:2 * m], tr.ravel()[:2 * m]), m
        assert (out["buf"][2 * m:] == SENT).all(), m


def test_optional_outputs(ctx, small):
    dev, (L, U, tol), full, _ = small
    for kw in (dict(trace=False), dict(max_trace=0), dict(count=False), dict(trace=False, max_trace=0, count=False)):
        out = dev.search(L, U, tol, **kw)
        assert same_bits(out["lam"], full["lam"]), kw
        if not kw.get("count", True):
            assert out["n"] == -7
        if kw.get("max_trace") == 0:
            assert (out["buf"] == SENT).all()


def test_repeatable_and_shares_its_workspace(ctx, small):
    """Two identical calls agree bit for bit; a single probe between them uses the same workspace slot and changes nothing."""
    dev, (L, U, tol), full, _ = small
    again = dev.search(L, U, tol)
    assert again["n"] == full["n"] and same_bits(again["lam"], full["lam"]) and same_bits(again["buf"], full["buf"])
    le = C.c_double(np.nan)
    _lib.call("bigkrls_dev_solveforc", ctx.handle, dev.pQ, dev.cs.n, dev.cs.k, dev.ldq, dev.d.ptr, dev.a.ptr, 0.3, None,
              C.byref(le))
    assert np.isfinite(le.value)
    third = dev.search(L, U, tol)
    assert third["n"] == full["n"] and same_bits(third["lam"], full["lam"]) and same_bits(third["buf"], full["buf"])


def test_nan_loss_ends_the_search_after_two_probes(ctx, small):
    """One NaN in a makes every loss NaN. R's loop then ends at once: abs(NaN) > tol is FALSE, and S1 < S2 is FALSE, so
    lambda = X2 after the two opening probes, with BIGKRLS_OK (arithmetic on NaN values, no device fault)."""
    dev, (L, U, tol), full, _ = small
    a = dev.cs.a.copy()
    a[3] = np.nan
    bad = Device(ctx, dev.cs, a=a)
    out = bad.search(L, U, tol)
    tr = full_trace(out)
    assert out["n"] == 2 and np.isnan(tr[:, 1]).all()
    X1 = L + ref.GOLDEN * (U - L)
    X2 = U - ref.GOLDEN * (U - L)
    assert same_bits(tr[:, 0], [X1, X2]) and same_bits(out["lam"], X2)
    ref.check_trace(L, U, tol, tr, 2, out["lam"])
    good = dev.search(L, U, tol)
    assert same_bits(good["buf"], full["buf"]) and same_bits(good["lam"], full["lam"])


NANVALS = ref.case("257x257").vals_all.copy()
NANVALS[100] = np.nan
REJECTED = {
    "ldq = n - 1": dict(ldq=256), "ldq = 0": dict(ldq=0), "k = 0": dict(k=0), "n = 0": dict(n=0),
    "Q NULL": dict(Q=None), "d NULL": dict(d=None), "a NULL": dict(a=None), "h_lambda NULL": dict(lam=None),
    "no eigenvalues, L derived": dict(vals=None, n_vals=0, L=-1.0), "no eigenvalues, U derived": dict(vals=None, n_vals=0, U=-1.0),
    "no eigenvalues, both derived": dict(vals=None, n_vals=0, L=-1.0, U=-1.0), "n_vals = 0": dict(n_vals=0, L=-1.0),
    "NaN eigenvalue": dict(vals=NANVALS, L=-1.0, U=-1.0),
}


@pytest.mark.parametrize("what", list(REJECTED))
def test_rejected_arguments(ctx, small, what):
    """BIGKRLS_EINVAL naming lambda_search, before anything is launched or written: trace, lambda and count untouched, and
    the context computes a correct search afterwards."""
    dev, (L, U, tol), full, _ = small
    kw = dict(REJECTED[what])
    out = dev.search(kw.pop("L", L), kw.pop("U", U), tol, status=True, **kw)
    assert out["rc"] == _lib.EINVAL, (what, out["rc"], out["msg"])
    assert "lambda_search" in out["msg"], (what, out["msg"])
    assert (out["buf"] == SENT).all() and out["lam"] == SENT and out["n"] == -7, what
    good = dev.search(L, U, tol)
    assert good["n"] == full["n"] and same_bits(good["buf"], full["buf"]) and same_bits(good["lam"], full["lam"])


def test_solveforc_and_qty_reject_a_small_leading_dimension(ctx, small):
    dev, _, _, _ = small
    n, k = dev.cs.n, dev.cs.k
    lib = _lib.load()
    for ldq in (n - 1, 0):
        c, le = vec(ctx, np.full(n, SENT)), C.c_double(SENT)
        rc = lib.bigkrls_dev_solveforc(ctx.handle, dev.pQ, n, k, ldq, dev.d.ptr, dev.a.ptr, 0.3, c.ptr, C.byref(le))
        assert rc == _lib.EINVAL and "solveforc" in lib.bigkrls_last_error().decode(), (ldq, rc)
        assert le.value == SENT and (c.to_numpy() == SENT).all()
        a, y = vec(ctx, np.full(k, SENT)), vec(ctx, np.ones(n))
        rc = lib.bigkrls_dev_qty(ctx.handle, dev.pQ, n, k, ldq, y.ptr, a.ptr)
        assert rc == _lib.EINVAL and "lda < m" in lib.bigkrls_last_error().decode(), (ldq, rc)
        assert (a.to_numpy() == SENT).all()
    le = C.c_double(SENT)
    _lib.call("bigkrls_dev_solveforc", ctx.handle, dev.pQ, n, k, dev.ldq, dev.d.ptr, dev.a.ptr, 0.3, None, C.byref(le))
    ref_le, bound = dev.cs.loss.ld(0.3)
    assert abs(LD(le.value) - ref_le) <= bound


# ---- the single probe: bigkrls_dev_solveforc held to the same bound ------------------------------------------------------------
def probe_inputs(n, k):
    """Q = standard normal / sqrt(n) (drawn in single precision at the large shape: any doubles will do), d, a."""
    rng = np.random.default_rng(1000 * n + k)
    Q = np.empty((n, k), order="F")
    for j in range(k):
        Q[:, j] = rng.standard_normal(n, dtype=np.float32)
    Q /= np.sqrt(n)
    d = np.sort(rng.uniform(0.01, 50.0, k))[::-1].copy()
    return Q, d, rng.standard_normal(k)


@pytest.mark.parametrize("n,k", [(257, 257), (300, 300), (262400, 257)])
def test_solveforc_probe_within_bound(ctx, n, k):
    """One probe with and without c: Le within bound B, every coefficient within (k + 16) u C_i, nothing written around
    c. 262 400 x 257 is the smallest shape at which sf_partial_kernel stages two chunks (256 + 1 eigenpairs) in one
    workgroup: 1025 row blocks leave one split."""
    rb = -(-n // 256)
    splits = max(min(-(-1024 // rb), -(-k // 256)), 1)
    kps = -(-(-(-k // splits)) // 256) * 256
    assert (kps, -(-k // kps)) == ((512, 1) if n == 262400 else (256, 2))
    Q, d, a = probe_inputs(n, k)
    lam = 0.3
    loss = ref.Loss(Q, d, a)
    cr, g, Cabs = loss.rows(lam)
    le_ref, le_bound = loss.from_rows(cr, g, Cabs)
    parent, pQ, ldq, _, _ = place(ctx, Q)
    dd, da = vec(ctx, d), vec(ctx, a)
    for with_c in (True, False):
        c = vec(ctx, np.full(n + 4, SENT))
        le = C.c_double(np.nan)
        _lib.call("bigkrls_dev_solveforc", ctx.handle, pQ, n, k, ldq, dd.ptr, da.ptr, lam,
                  c.col_ptr(0, 2) if with_c else None, C.byref(le))
        err = float(abs(LD(le.value) - le_ref))
        print(f"solveforc {n} x {k}, c {with_c}: Le error / bound {err / le_bound:.3g}")
        assert err <= le_bound, (with_c, le.value, float(le_ref), err, le_bound)
        got = c.to_numpy().ravel()
        if with_c:
            assert (got[:2] == SENT).all() and (got[-2:] == SENT).all()
            cerr = np.abs(got[2:-2].astype(LD) - cr).astype(np.float64)
            cb = (k + 16) * EPS * Cabs
            print(f"solveforc {n} x {k}: largest coefficient error / bound {float(np.max(cerr / cb)):.3g}")
            assert np.all(cerr <= cb)
        else:
            assert (got == SENT).all()

