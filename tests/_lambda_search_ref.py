"""Host references and seeded inputs for the direct tests of the golden-section lambda search
(bigkrls_dev_lambda_search, csrc/solveforc.hip): tests/test_lambda_search_ref_cpu.py checks them without the code under
test, tests/test_gpu_lambda_search.py applies them to the device's trace.

A. Control replay
-----------------
search(L, U, tol, loss) is R's loop (R/bigKRLS_Rcpp_functions.R:38-77) statement for statement in Python floats: IEEE
doubles, one rounding per operation, no contraction. replay() runs it on a recorded list of losses in place of a loss
function. Given (L, U, tol) and the device's trace (lambda_t, Le_t) the replay must ask for lambda_0, lambda_1, ... bit
for bit, stop after exactly *h_nprobes losses and return exactly *h_lambda. That pins the control flow (which buffer a
loss is consumed from, the state slot a launch reads, the probe around a chain boundary, a fused multiply-add in the
step, the index of a trace entry) and does not depend on the last bits of the device's losses.

B. Loss bound
-------------
    Le(lambda) = sum_i r_i^2,   r_i = c_i / g_i,   c_i = sum_k Q_ik a_k w_k,   g_i = sum_k Q_ik^2 w_k,   w_k = 1 / (d_k + lambda)
is evaluated in np.longdouble (64-bit significand: its own error is below 2^-10 of the bound and is not counted).
With d >= 0 and lambda > 0 every term of g is positive. Write u = 2^-53, C_i = sum_k |Q_ik a_k| w_k.

  * w_k is computed as 1 / (d_k + lambda): two roundings. a_k w_k one more, Q_ik (a_k w_k) one more (none if the
    product is fused into the sum): each term of c_i carries at most 4 roundings; Q_ik Q_ik w_k likewise 4.
  * A sum of k terms in ANY order (two accumulators, column groups, LDS chunks, k-splits: every partial sum is a node of
    one summation tree) puts at most k - 1 further roundings on each term. So
        |c^_i - c_i| <= (k + 3) u C_i,    |g^_i - g_i| <= (k + 3) u g_i     (first order).
  * r^_i = fl(c^_i / g^_i):   |r^_i - r_i| <= (k + 3) u (C_i / g_i + |r_i|) + u |r_i| <= (k + 4) u (C_i / g_i + |r_i|).
  * t^_i = fl(r^_i^2):   |t^_i - r_i^2| <= 2 |r_i| |r^_i - r_i| + u r_i^2 <= 2 |r_i| (k + 5) u (C_i / g_i + |r_i|)
    (C_i >= |c_i|, so u r_i^2 is at most a quarter of one more count).
  * The n row terms (rows past the end contribute exact zeros) summed in any order: at most (n - 1) u sum_i t^_i more.

The derivation gives k + 5 and n - 1; the tests use k + 16 and n + 16, the constants the project's other derived bounds
carry (tests/test_gpu_deriv_pass.py), and the factor 1.01 for the second-order terms:

    |Le^ - Le| <= 1.01 [ sum_i 2 |r_i| (k + 16) u (C_i / g_i + |r_i|) + (n + 16) u sum_i r_i^2 ],
    |c^_i - c_i| <= (k + 16) u C_i                          (the coefficients of bigkrls_dev_solveforc).

The bound is derived, not measured; nothing here is fitted to what the kernels return.

Inputs
------
Every case is built from a seed by case(name). Q is orthonormal (QR) at the small shapes and standard normal / sqrt(n)
at the large ones: neither reference needs orthogonality. d is uniform in [0.01, 50], sorted downwards, a = Q'y.
check_case() computes, without the code under test, the probe count of the search with the np.float64 loss and with the
np.longdouble loss (they must agree and be the count the case was chosen for) and the room of every comparison:
| |S1 - S2| - tol | at every step and |S1 - S2| at every step that branches must be at least 100 x the case's loss bound
(its largest value over the probes), so that no decision of the device can hinge on a rounding.

Probe counts much above 70 cannot be reached: the interval falls below the spacing of doubles near lambda. A chain is
48 probes, so a third chain (more than 96) is out of reach and is not tested.
"""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

GOLDEN = 0.381966
EPS = 2.0 ** -53
LD = np.longdouble
SF_KC = 256            # eigenpairs per LDS chunk (csrc/solveforc.hip)
CHAIN = 48             # probe launches per chain
ROOM = 100.0           # decisions are taken with at least this many loss bounds of room


# ---- A: the control loop -------------------------------------------------------------------------------------------------
class OutOfLosses(Exception):
    pass


def search(L, U, tol, loss):
    """R's loop on loss(lambda, t), t the probe's index. Returns (lambda, asked, steps): `asked` the lambdas in the order
    they were probed, `steps` one (S1, S2, branched) per evaluation of the while condition."""
    L, U, tol = float(L), float(U), float(tol)
    asked, steps = [], []

    def probe(x):
        asked.append(x)
        return float(loss(x, len(asked) - 1))

    X1 = L + GOLDEN * (U - L)
    X2 = U - GOLDEN * (U - L)
    S1 = probe(X1)
    S2 = probe(X2)
    while True:
        go = abs(S1 - S2) > tol
        steps.append((S1, S2, bool(go)))
        if not go:
            break
        if S1 < S2:
            U = X2
            X2 = X1
            X1 = L + GOLDEN * (U - L)
            S2 = S1
            S1 = probe(X1)
        else:
            L = X1
            X1 = X2
            X2 = U - GOLDEN * (U - L)
            S1 = S2
            S2 = probe(X2)
        if len(asked) > 10000:
            raise RuntimeError("search: no end")
    return (X1 if S1 < S2 else X2), asked, steps


def replay(L, U, tol, losses):
    """The loop fed with recorded losses. Returns (lambda, asked); raises OutOfLosses if it wants more than it is given."""
    losses = [float(x) for x in losses]

    def loss(x, t):
        if t >= len(losses):
            raise OutOfLosses(f"the replay asks for probe {t}, {len(losses)} were recorded")
        return losses[t]

    lam, asked, _ = search(L, U, tol, loss)
    return lam, asked


def check_trace(L, U, tol, trace, nprobes, lam):
    """Reference A on a device trace ((lambda_t, Le_t) rows, all `nprobes` of them)."""
    trace = np.asarray(trace, dtype=np.float64).reshape(-1, 2)
    assert trace.shape[0] == nprobes, (trace.shape, nprobes)
    lam_r, asked = replay(L, U, tol, trace[:, 1])
    assert len(asked) == nprobes, f"the replay stops after {len(asked)} losses, the device reports {nprobes}"
    got, want = trace[:, 0], np.array(asked)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        t = int(np.flatnonzero(~same)[0])
        raise AssertionError(f"probe {t}: the device probed {got[t]!r}, R's loop asks for {want[t]!r}")
    assert np.float64(lam).view(np.uint64) == np.float64(lam_r).view(np.uint64) or (np.isnan(lam) and np.isnan(lam_r)), (lam, lam_r)


# ---- B: the loss and its bound -----------------------------------------------------------------------------------------------
class Loss:
    """Le(lambda) of one (Q, d, a) in np.float64 and np.longdouble. The extended-precision results are kept per lambda
    (the CPU check of a case and the GPU test ask for the same ones); Q is taken to extended precision a column at a time,
    so a large Q costs no extra memory."""

    def __init__(self, Q, d, a):
        self.Q, self.d, self.a = Q, np.asarray(d, dtype=np.float64), np.asarray(a, dtype=np.float64)
        self.n, self.k = Q.shape
        self._done = {}

    def f64(self, lam):
        w = 1.0 / (self.d + lam)
        c = self.Q @ (w * self.a)
        g = (self.Q * self.Q) @ w
        return float(np.sum((c / g) ** 2))

    def rows(self, lam):
        """(c, g, C) per row: c and g in np.longdouble, C (which only enters the bounds) in np.float64."""
        w = 1 / (self.d.astype(LD) + LD(lam))
        wa = w * self.a.astype(LD)
        awa = np.abs(wa).astype(np.float64)
        c, g, C = np.zeros(self.n, dtype=LD), np.zeros(self.n, dtype=LD), np.zeros(self.n)
        for j in range(self.k):                              # (one contiguous column at a time)
            q = self.Q[:, j].astype(LD)
            c += q * wa[j]
            g += q * q * w[j]
            C += np.abs(self.Q[:, j]) * awa[j]
        return c, g, C

    def ld(self, lam):
        """(Le, bound): the extended-precision loss and the derived bound on a double-precision evaluation of it."""
        key = float(lam).hex()
        if key not in self._done:
            self._done[key] = self.from_rows(*self.rows(lam))
        return self._done[key]

    def from_rows(self, c, g, C):
        r = c / g
        ar = np.abs(r)
        s2 = np.sum(r * r)
        bound = 1.01 * (np.sum(2 * ar * (self.k + 16) * EPS * (C / g + ar)) + (self.n + 16) * EPS * s2)
        return s2, float(bound)


def check_losses(loss, trace, what=""):
    """Reference B on every probe of a trace. Returns the largest error / bound (reported, never a threshold)."""
    worst = 0.0
    for t, (lam, le) in enumerate(np.asarray(trace, dtype=np.float64).reshape(-1, 2)):
        ref, bound = loss.ld(lam)
        err = float(abs(LD(le) - ref))
        assert err <= bound, f"{what} probe {t} at lambda {lam!r}: Le {le!r}, reference {float(ref)!r}, error {err:.3e} > bound {bound:.3e}"
        worst = max(worst, err / bound)
    return worst


# ---- the launch shape (the formulae of lambda_search) -----------------------------------------------------------------------
def launch_shape(n, k):
    rows = 32 if n <= 32 * 16384 else 256
    rb = max(-(-n // rows), 1)
    rbf = max(-(-n // 256), 1)
    splits = max(min(-(-1024 // rb), -(-k // SF_KC)), 1)
    kps = -(-(-(-k // splits)) // SF_KC) * SF_KC
    splits = -(-k // kps)
    return dict(rows=rows, rb=rb, splits=splits, kps=kps, nle=rbf if splits > 1 else rb,
                last=k - (splits - 1) * kps)


# ---- the cases --------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    n: int
    k: int
    Q: np.ndarray
    d: np.ndarray
    a: np.ndarray
    vals_all: np.ndarray
    L: float            # as passed to the entry (-1: derived)
    U: float
    tol: float          # as passed (-1: 1e-3 n)
    probes: int         # the count the case is meant to reach
    shape: dict         # the launch shape it was chosen for
    loss: Optional[Loss] = None

    def bounds(self):
        """(L, U, tol) the search runs from."""
        from oracle import krls_oracle as orc
        L, U = self.L, self.U
        if L < 0 or U < 0:
            L0, U0 = orc.lambda_bounds(self.vals_all, self.n)
            L, U = (L0 if L < 0 else L), (U0 if U < 0 else U)
        return L, U, (self.tol if self.tol > 0 else 1e-3 * self.n)


def inputs(n, k, seed, qr, extra_vals=0, lead=None):
    """lead = None: y standard normal. lead = e: y = q_0 + e z, the leading eigenvector plus a little noise: the loss then
    rises steeply from L = 2 (relative slope about 0.09 per unit of lambda against 0.01 for a normal y), which is what
    gives the decisions of a 50-probe search their room."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, k))
    if qr:
        Q, _ = np.linalg.qr(Q)
    else:
        Q /= np.sqrt(n)
    Q = np.asfortranarray(Q)
    d = np.sort(rng.uniform(0.01, 50.0, k + extra_vals))[::-1].copy()
    y = rng.standard_normal(n)
    if lead is not None:
        y = Q[:, 0] + lead * y
    return Q, d[:k].copy(), Q.T @ y, d


# name: (n, k, seed, qr, extra eigenvalues, lead, L, U, tol, probes, launch shape); L, U = -1: derived, tol = -1: 1e-3 n
TABLE = {
    "1x1": (1, 1, 1, False, 0, None, 0.5, 20.0, -1.0, 2, dict(rows=32, rb=1, splits=1, kps=256, nle=1, last=1)),
    "31x7": (31, 7, 2, True, 3, None, 0.5, 20.0, 1e-6, 32, dict(rows=32, rb=1, splits=1, kps=256, nle=1, last=7)),
    "33x9": (33, 9, 3, True, 0, None, 0.5, 20.0, 1e-6, 35, dict(rows=32, rb=2, splits=1, kps=256, nle=2, last=9)),
    "300x120": (300, 120, 11, True, 0, None, 2.0, 40.0, -1.0, 11, dict(rows=32, rb=10, splits=1, kps=256, nle=10, last=120)),
    "257x257": (257, 257, 4, True, 0, None, -1.0, -1.0, 1e-4, 14, dict(rows=32, rb=9, splits=2, kps=256, nle=2, last=1)),
    "300x300": (300, 300, 5, True, 0, None, -1.0, -1.0, 1e-4, 21, dict(rows=32, rb=10, splits=2, kps=256, nle=2, last=44)),
    "1100x1000": (1100, 1000, 6, True, 37, None, -1.0, -1.0, 1e-4, 9, dict(rows=32, rb=35, splits=4, kps=256, nle=5, last=232)),
    # the large shapes: a tolerance at which the search takes 10 probes (the extended-precision reference stays at seconds)
    "16416x600": (16416, 600, 7, False, 0, None, 2.0, 40.0, 175.0, 10, dict(rows=32, rb=513, splits=2, kps=512, nle=65, last=88)),
    "32800x300": (32800, 300, 8, False, 0, None, 2.0, 40.0, 950.0, 10, dict(rows=32, rb=1025, splits=1, kps=512, nle=1025, last=300)),
    "524289x3": (524289, 3, 9, False, 0, None, 2.0, 40.0, 6e7, 10, dict(rows=256, rb=2049, splits=1, kps=256, nle=2049, last=3)),
    # one column: r_i = a / Q_i1 whatever lambda is, so the loss is constant (5e19 here, 1 / Q^2 is heavy-tailed) and the
    # search ends after its first two probes; the tolerance stands clear of the bound (3e9) on either loss
    "524289x1": (524289, 1, 10, False, 0, None, 2.0, 40.0, 1e15, 2, dict(rows=256, rb=2049, splits=1, kps=256, nle=2049, last=1)),
}
# The chain cases: 300 x 120, L = 2, U = 40, y = q_0 + 1e-4 z. Probe 47 is the last before the closing launch, 48 the one
# the closing launch consumes, 49 and 50 the first two of the second chain. Each tolerance is the midpoint of the two
# successive |S1 - S2| of the extended-precision search it has to separate. 51 is the largest count these inputs reach
# with 100 bounds of room (52 would have 64); about 60 probes cannot be had with that room. All of them take the
# S1 < S2 branch; inputs that end at U (the other branch) reach 47 probes at most with that room, whatever L and U.
CHAIN_TOLS = {47: 8.48e-10, 48: 5.24e-10, 49: 3.24e-10, 50: 2.00e-10, 51: 1.2377e-10}
for _p, _t in CHAIN_TOLS.items():
    TABLE[f"chain{_p}"] = (300, 120, 11, True, 0, 1e-4, 2.0, 40.0, _t, _p, dict(rows=32, rb=10, splits=1, kps=256, nle=10, last=120))


@functools.lru_cache(maxsize=None)
def _inputs_cached(n, k, seed, qr, extra, lead):
    Q, d, a, vals = inputs(n, k, seed, qr, extra, lead)
    for x in (Q, d, a, vals):
        x.setflags(write=False)                  # shared between the tests: never modified
    return Q, d, a, vals, Loss(Q, d, a)


def case(name):
    n, k, seed, qr, extra, lead, L, U, tol, probes, shape = TABLE[name]
    Q, d, a, vals, loss = _inputs_cached(n, k, seed, qr, extra, lead)
    return Case(name, n, k, Q, d, a, vals, L, U, tol, probes, shape, loss)


@functools.lru_cache(maxsize=None)
def check_case(name):
    """The conditions on a case's inputs (module docstring). Returns (probes, smallest room in loss bounds)."""
    cs = case(name)
    assert launch_shape(cs.n, cs.k) == cs.shape, (name, launch_shape(cs.n, cs.k))
    L, U, tol = cs.bounds()
    lam64, asked64, _ = search(L, U, tol, lambda x, t: cs.loss.f64(x))
    bounds = []

    def ld(x, t):
        le, b = cs.loss.ld(x)
        bounds.append(b)
        return float(le)

    lam_ld, asked_ld, steps = search(L, U, tol, ld)
    assert len(asked64) == len(asked_ld) == cs.probes, (name, len(asked64), len(asked_ld), cs.probes)
    assert asked64 == asked_ld, (name, "the two precisions probe different lambdas")
    assert min(asked_ld) > 0.0
    bound = max(bounds)
    room = min(min(abs(abs(s1 - s2) - tol) for s1, s2, _ in steps),
               min([abs(s1 - s2) for s1, s2, go in steps if go], default=np.inf)) / bound
    assert room >= ROOM, (name, f"a comparison is decided with {room:.3g} loss bounds of room, {ROOM:g} are required")
    return len(asked_ld), room
