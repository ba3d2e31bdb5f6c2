"""influence(), bigkrls_dev_deletion_residuals and robust_vcov(type="CR3") on the GPU (csrc/influence.hip).

1. The primitive against numpy on the same Q, w, e: per unit np.linalg.solve(I - H_SS, e_S), held to
   ||et - ref||_inf <= 64 (m + k) eps cond_2(I - H_SS) ||ref||_inf -- Cholesky and the eigensolver are backward stable,
   the sums are k and m long, 64 is the project's margin (tests/test_gpu_robust_vcov.py). Q has orthonormal columns and w
   lies in (0, 0.9), so every cond is at most 10 (asserted). Every ratio error / bound is printed. The unit sizes stand on
   both sides of every size class of the fused kernel (16, 64, MB = 128 rows with I - H_SS in LDS, 2 MB = 256 with it in
   the workspace) and of the general route behind it.
2. Route 0 against route 1 within the same bound, two calls bit for bit, h_unit = NULL against G = n distinct labels
   BIT FOR BIT (the units of one row take the NULL call's formula on the same leverages), the refusals, the profile.
3. The public call against brute force: numpy TRUE deletion of every cluster (G = 2, 7, 40) and of single rows -- the
   kernel ridge refit on the remaining rows with the kernel Q diag(d) Q' of the kept pairs, which is the fixed-basis
   penalised least-squares refit (well conditioned: cond <= (d_1 + lambda) / lambda). Tolerances: the error floor of the
   numpy closed form against that numpy brute force on the same inputs, times 10 (one decimal for the different
   summation order). Floors measured on the CPU, on numpy's own eigenpairs of the two fits' kernels at the fits' lambda
   (relative to the largest entry compared, worst over the cases below; every run prints them again on its own inputs):
       fitted.deleted  4e-15 (clusters)   4e-15 (single rows)
       dfame           9e-14 (clusters)   8e-13 (single rows)
       cooks           5e-14 (clusters)   3e-13 (single rows)
       R2.loo          3e-16 absolute
   FLOOR below holds these and the assertions use 10 x FLOOR: 4e-14, 9e-13 / 8e-12, 5e-13 / 3e-12 and 3e-15.
4. CR3 against the dense numpy sandwich on deletion residuals under 64 (n + k) eps ||V||_2 times the largest
   cond(I - H_SS) (printed); its var.avgderivatives against influence()'s jackknife variance within 1e-8 of the largest;
   influence() on a kernel="implicit" fit and on newdata."""
import importlib.util
import os

import numpy as np
import pytest

from bigkrls_amd import _lib

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53
MB = 128
FLOOR = {("fitted", "cluster"): 4e-15, ("fitted", "single"): 4e-15, ("dfame", "cluster"): 9e-14,
         ("dfame", "single"): 8e-13, ("cooks", "cluster"): 5e-14, ("cooks", "single"): 3e-13, "r2": 3e-16}


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


me_numpy = _load("_me_cpu_for_influence", "test_marginal_effects_cpu.py").me_numpy
influence_numpy = _load("_inf_cpu_for_influence", "test_influence_cpu.py").influence_numpy


def host(m):
    return m.to_numpy() if hasattr(m, "to_numpy") else np.asarray(m)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the primitive ---------------------------------------------------------------------------------------------------
def labels_of(n, sizes, empty_at=None):
    """units of the given sizes in a cycle until n rows are used (the last one cut short); empty_at: a label nobody has"""
    lab, g, i = [], 0, 0
    while len(lab) < n:
        if g == empty_at:
            g += 1
            continue
        lab += [g] * min(sizes[i % len(sizes)], n - len(lab))
        g += 1
        i += 1
    return np.asarray(lab, dtype=np.int64), g


PATTERNS = {
    "all 1": dict(sizes=[1]),
    "all 2": dict(sizes=[2]),
    "15 16 17": dict(sizes=[15, 16, 17]),
    "63 64 65": dict(sizes=[63, 64, 65]),
    "MB-1 MB MB+1": dict(sizes=[MB - 1, MB, MB + 1]),                      # LDS instance | the instance with I - H_SS in the workspace
    "2MB-1 2MB 2MB+1": dict(sizes=[2 * MB - 1, 2 * MB, 2 * MB + 1]),      # ... | the general route
    "300 and 3s": dict(sizes=[300] + [3] * 10000),
    "2s with an empty unit": dict(sizes=[2], empty_at=5),
}
SHAPES = [(700, 1), (700, 3), (700, 4), (700, 5), (700, 33), (2100, 250)]
_problems = {}


def problem(ctx, n, k):
    """Q with orthonormal columns, w in (0, 0.9), e -- once per shape, with Q on the device"""
    if (n, k) not in _problems:
        rng = np.random.default_rng(1000 * n + k)
        Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
        w = rng.uniform(0.0, 0.9, size=k)
        e = rng.standard_normal(n)
        _problems[(n, k)] = (Q, w, e, (Q * w) @ Q.T, ctx.from_numpy(np.asfortranarray(Q)))
    return _problems[(n, k)]


def primitive(ctx, n, k, labels, G, route=0, **kw):
    from bigkrls_amd import ops
    Q, w, e, H, Qd = problem(ctx, n, k)
    return ops.bDeletionResiduals(Qd, w, e, labels, G, route=route, **kw)


def assert_units_within_bound(et, H, e, labels, G, k, what):
    order = np.argsort(labels, kind="stable")
    cuts = np.searchsorted(labels[order], np.arange(G + 1))
    worst = 0.0
    assert np.isfinite(et).all(), what
    for g in range(G):
        idx = order[cuts[g]:cuts[g + 1]]
        m = idx.size
        if m == 0:
            continue
        A = np.eye(m) - H[np.ix_(idx, idx)]
        ref = np.linalg.solve(A, e[idx])
        cond = np.linalg.cond(A, 2)
        assert cond <= 10.0, (what, g, m, cond)
        bound = 64 * (m + k) * EPS * cond * np.max(np.abs(ref))
        err = float(np.max(np.abs(et[idx] - ref)))
        worst = max(worst, err / bound)
        assert err <= bound, f"{what}: unit {g} (m = {m}): error {err:.3e} over the bound {bound:.3e}"
    print(f"deletion_residuals {what}: worst error / bound {worst:.3e}")
    return worst


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n,k", SHAPES)
def test_primitive_against_numpy(ctx, n, k, pattern):
    Q, w, e, H, Qd = problem(ctx, n, k)
    labels, G = labels_of(n, **PATTERNS[pattern])
    perm = np.random.default_rng(7).permutation(n)
    for order, lab in (("grouped", labels), ("permuted", labels[perm])):
        et = primitive(ctx, n, k, lab, G)
        assert_units_within_bound(et, H, e, lab, G, k, f"n={n} k={k} {pattern} {order}")


# ---- 2. route, determinism, refusals, profile -----------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["15 16 17", "63 64 65", "MB-1 MB MB+1", "2MB-1 2MB 2MB+1", "300 and 3s"])
def test_route_0_equals_route_1_within_the_bound(ctx, pattern):
    n, k = 700, 33
    Q, w, e, H, Qd = problem(ctx, n, k)
    labels, G = labels_of(n, **PATTERNS[pattern])
    if pattern == "300 and 3s":                                            # (a few of the small units: one eigensolver call each)
        labels = np.minimum(labels, 40)
        G = 41
    lab = labels[np.random.default_rng(8).permutation(n)]
    r0 = primitive(ctx, n, k, lab, G, route=0)
    r1 = primitive(ctx, n, k, lab, G, route=1)
    assert_units_within_bound(r0, H, e, lab, G, k, f"route 0 {pattern}")
    assert_units_within_bound(r1, H, e, lab, G, k, f"route 1 {pattern}")
    for g in range(G):                                                     # the routes against each other: part 1's bound
        idx = np.flatnonzero(lab == g)
        if idx.size:
            A = np.eye(idx.size) - H[np.ix_(idx, idx)]
            ref = np.linalg.solve(A, e[idx])
            bound = 64 * (idx.size + k) * EPS * np.linalg.cond(A, 2) * np.max(np.abs(ref))
            assert np.max(np.abs(r0[idx] - r1[idx])) <= bound, (pattern, g, idx.size)


def test_two_calls_give_the_same_bits_and_extras_agree(ctx):
    n, k = 2100, 250
    Q, w, e, H, Qd = problem(ctx, n, k)
    rng = np.random.default_rng(9)
    sizes = list(rng.integers(1, 251, size=40))
    labels, G = labels_of(n, sizes)
    lab = labels[rng.permutation(n)]
    a, hat_a, S_a = primitive(ctx, n, k, lab, G, hat=True, scores=True)
    b, hat_b, S_b = primitive(ctx, n, k, lab, G, hat=True, scores=True)
    assert same_bits(a, b) and same_bits(hat_a, hat_b) and same_bits(host(S_a), host(S_b))
    assert same_bits(a, primitive(ctx, n, k, lab, G))                      # the extras do not change et
    assert np.max(np.abs(hat_a - np.diag(H))) <= 64 * k * EPS
    S_ref = np.zeros((k, G))
    np.add.at(S_ref.T, lab, a[:, None] * Q)
    assert np.max(np.abs(host(S_a) - S_ref)) <= 64 * 250 * EPS * np.max(np.abs(S_ref))


@pytest.mark.parametrize("n,k", [(700, 5), (2100, 250)])
def test_null_labels_equal_distinct_labels_bit_for_bit(ctx, n, k):
    """ACHIEVED: bitwise. A unit of one row takes e / (1 - h) on rowsumsq_weighted's leverage in both calls."""
    Q, w, e, H, Qd = problem(ctx, n, k)
    none = primitive(ctx, n, k, None, 0)
    ident = primitive(ctx, n, k, np.arange(n), n)
    shuffled = primitive(ctx, n, k, np.random.default_rng(3).permutation(n), n)
    assert same_bits(none, ident) and same_bits(none, shuffled)
    ref = e / (1.0 - np.diag(H))
    assert np.max(np.abs(none - ref) / np.abs(ref)) <= 64 * k * EPS * 10.0


def test_refusals_name_the_unit(ctx):
    from bigkrls_amd import ops
    n, k = 40, 6
    Q = np.zeros((n, k), order="F")
    Q[n - k + np.arange(k), np.arange(k)] = 1.0                            # unit vectors: with w = 1 the rows 34 .. 39 have leverage 1
    Qd = ctx.from_numpy(Q)
    e = np.ones(n)
    pairs = np.arange(n) // 2
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*unit 17 \(2 rows\): the pivot of column 1 of I - H_SS is not positive"):
        ops.bDeletionResiduals(Qd, np.ones(k), e, pairs, n // 2)
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*unit 34 \(1 row\): the leverage is >= 1"):
        ops.bDeletionResiduals(Qd, np.ones(k), e)
    # a unit of 21 rows (the four-wave instance): rows 19 .. 39, the first pivot that fails is row 34's, column 16 -- the
    # last of the first column block; unit 0 holds no leverage
    lab = np.where(np.arange(n) < 19, 0, 1)
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*unit 1 \(21 rows\): the pivot of column 16 of"):
        ops.bDeletionResiduals(Qd, np.ones(k), e, lab, 2)
    # the general route: leverage 2, an eigenvalue of -1 (w = 1 would leave a zero that rounds either way)
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*unit 1 \(21 rows\): the smallest eigenvalue of I - H_SS"):
        ops.bDeletionResiduals(Qd, np.full(k, 2.0), e, lab, 2, route=1)
    # one failing unit on each route (260 rows: the general route; 40 rows: the fused kernel; leverage 2 in both): the
    # unit named is the lowest failing label, whichever route it took
    n3 = 300
    Q3 = np.zeros((n3, 2), order="F")
    Q3[0, 0] = Q3[n3 - 1, 1] = 1.0
    Q3d = ctx.from_numpy(Q3)
    big_first = np.where(np.arange(n3) < 260, 0, 1)
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*unit 0 \(260 rows\): the smallest eigenvalue of I - H_SS"):
        ops.bDeletionResiduals(Q3d, np.full(2, 2.0), np.ones(n3), big_first, 2)
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*unit 0 \(40 rows\): the pivot of column 40 of"):
        ops.bDeletionResiduals(Q3d, np.full(2, 2.0), np.ones(n3), 1 - big_first, 2)
    bad = pairs.copy()
    bad[7] = n // 2
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*label of row 8 is outside \[0, G\)"):
        ops.bDeletionResiduals(Qd, np.full(k, 0.5), e, bad, n // 2)
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*route must be"):
        ops.bDeletionResiduals(Qd, np.full(k, 0.5), e, pairs, n // 2, route=2)
    # m over the general route's cap (8 m^2 <= 2^30: m <= 11585): refused by the plan, before any allocation -- Q is
    # 11 600 x 1 (93 KB) and the workspace held by the context does not grow
    n2 = 11600
    Q2 = ctx.from_numpy(np.full((n2, 1), 1.0 / np.sqrt(n2), order="F"))
    lab2 = np.zeros(n2, dtype=np.int64)
    lab2[11586:] = 1
    before = ctx.workspace_bytes()
    with pytest.raises(_lib.BigKRLSError, match=r"EINVAL.*unit 0 \(11586 rows\).*at most 2\^30 \(m <= 11585\)"):
        ops.bDeletionResiduals(Q2, np.array([0.5]), np.ones(n2), lab2, 2)
    assert ctx.workspace_bytes() == before
    # ... and the calls above left the context usable
    ok = ops.bDeletionResiduals(Qd, np.full(k, 0.5), e, pairs, n // 2)
    assert np.isfinite(ok).all()


def test_profile_name_and_work(ctx):
    n, k = 700, 33
    labels, G = labels_of(n, [15, 16, 17])
    sizes = np.bincount(labels, minlength=G).astype(float)
    ctx.sync()
    ctx.set_profile(True)
    try:
        before = ctx.get_profile("deletion_residuals")
        primitive(ctx, n, k, labels, G)
        primitive(ctx, n, k, None, 0)
        after = ctx.get_profile("deletion_residuals")
    finally:
        ctx.set_profile(False)
    d_ms, d_work, d_launches = (after[i] - before[i] for i in range(3))
    assert d_launches == 2 and d_ms > 0.0
    assert d_work == 2.0 * k * float(np.sum(sizes ** 2)) + 2.0 * k * n


# ---- 3. the public call against brute force -----------------------------------------------------------------------------
def _data(n, p, seed, binary):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    if binary:
        X[:, p - 1] = (rng.random(n) < 0.4).astype(np.float64)
    y = np.sin(X @ np.linspace(0.3, 0.9, p)) + (0.1 + 0.4 * np.abs(X[:, 0])) * rng.standard_normal(n)   # heteroskedastic
    return X, y


def _labels(n, G, seed=1):
    return np.random.default_rng(seed).permutation((np.arange(n) * G) // n)


@pytest.fixture(scope="module")
def fits(ctx):
    import bigkrls_amd as bk
    Xs, ys = _data(300, 3, 41, True)
    Xl, yl = _data(1100, 4, 42, False)
    return {"dense300": bk.bigKRLS(ys, Xs, eigtrunc=0, vcov_form="both", ctx=ctx, noisy=False),
            "trunc1100": bk.bigKRLS(yl, Xl, eigtrunc=0.01, vcov_form="both", ctx=ctx, noisy=False)}


def parts(obj):
    Q = host(obj["vcov.est.Q"])
    k = Q.shape[1]
    d = np.asarray(obj["K.eigenvalues"], dtype=np.float64).ravel()[:k]
    y = np.asarray(obj["y"], dtype=np.float64).ravel()
    ysd = float(np.std(y, ddof=1))
    ys = (y - y.mean()) / ysd
    return Q, d, float(obj["lambda"]), y, ysd, ys


def brute_force(obj, units, ame_units=None):
    """TRUE deletion of every unit (a list of row index arrays): the kernel ridge refit on the remaining rows with the
    kernel Q diag(d) Q' of the kept pairs at the same lambda -- the fixed-basis penalised least-squares refit. Per unit:
    the rows' predictions by that fit (original units), AME(full) - AME(deleted) -- the AME is linear in the coefficients,
    so me_numpy on c - c(-S) with c(-S) = Q D^-1 beta(-S); for the units at the positions ame_units only, default all --,
    Cook's numerator, the deletion residuals."""
    Q, d, lam, y, ysd, ys = parts(obj)
    X = np.asarray(obj["X"], dtype=np.float64)
    n = X.shape[0]
    Kt = (Q * d) @ Q.T
    w = d / (d + lam)
    yhat = Q @ (w * (Q.T @ ys))
    c = Q @ ((Q.T @ ys) / (d + lam))
    out = []
    for pos, idx in enumerate(units):
        keep = np.setdiff1d(np.arange(n), idx)
        alpha = np.linalg.solve(Kt[np.ix_(keep, keep)] + lam * np.eye(keep.size), ys[keep])
        t = Q[keep].T @ alpha                                               # beta(-S) = D t, c(-S) = Q t
        out.append({"fitted": y.mean() + ysd * (Q[idx] @ (d * t)),
                    "dfame": me_numpy(X, y, c - Q @ t, obj["sigma"], X)[1] if ame_units is None or pos in ame_units else None,
                    "num": float(np.sum((yhat - Q @ (d * t)) ** 2)), "et": ys[idx] - Q[idx] @ (d * t)})
    e = ys - yhat
    return out, w.sum() * (e @ e) / (n - w.sum()), ys


def closed_form_numpy(obj, labels, unit_ids):
    """the closed form in numpy on the same inputs, in the public call's units (dfame for unit_ids only): what the floor
    is measured with"""
    Q, d, lam, y, ysd, ys = parts(obj)
    X = np.asarray(obj["X"], dtype=np.float64)
    r = influence_numpy(Q, d, lam, ys, labels, np.zeros((X.shape[0], 1)))
    dfame = np.stack([me_numpy(X, y, r["dc"][:, u], obj["sigma"], X)[1] for u in unit_ids])
    return {"fitted": y - ysd * r["et"], "dfame": dfame, "cooks": r["cooks"], "r2": r["r2_loo"]}


def compare(name, kind, got, closed, units, unit_ids, ame_units, brute, den, ys, r2_all):
    """got: influence()'s result; brute: brute_force, with dfame for the units at the positions ame_units; closed:
    closed_form_numpy, whose dfame (the printed floor's only) covers the first len(closed["dfame"]) of them"""
    ref_fitted = np.concatenate([b["fitted"] for b in brute])
    rows = np.concatenate(units)
    ref_df = np.stack([brute[i]["dfame"] for i in ame_units])
    ref_ck = np.array([b["num"] for b in brute]) / den
    for key, g, c, ref in (("fitted", got["fitted.deleted"][rows], closed["fitted"][rows], ref_fitted),
                           ("dfame", got["dfame"][unit_ids[ame_units]], closed["dfame"], ref_df),
                           ("cooks", got["cooks"][unit_ids], closed["cooks"][unit_ids], ref_ck)):
        scale = np.max(np.abs(ref))
        floor = float(np.max(np.abs(c - ref[:len(c)])) / scale)
        err = float(np.max(np.abs(g - ref)) / scale)
        tol = 10.0 * FLOOR[(key, kind)]
        print(f"influence {name} {kind} {key}: numpy floor {floor:.3e}, GPU error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, (name, kind, key, err, tol)
    if r2_all:
        et = np.concatenate([b["et"] for b in brute])
        r2_ref = 1.0 - (et @ et) / (ys @ ys)
        print(f"influence {name} {kind} R2.loo: numpy floor {abs(closed['r2'] - r2_ref):.3e}, GPU error "
              f"{abs(got['R2.loo'] - r2_ref):.3e}, tolerance {10 * FLOOR['r2']:.3e}")
        assert abs(got["R2.loo"] - r2_ref) <= 10 * FLOOR["r2"]


@pytest.mark.parametrize("G", [2, 7, 40])
@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_cluster_deletion_against_brute_force(fits, ctx, name, G):
    import bigkrls_amd as bk
    obj = fits[name]
    n = np.asarray(obj["X"]).shape[0]
    lab = _labels(n, G)
    got = bk.influence(obj, cluster=lab, ctx=ctx)
    # the labels are numbered in order of appearance: map the units back to the caller's labels
    names = got["unit.labels"]
    units = [np.flatnonzero(lab == v) for v in names]
    assert got["units"] == G and list(got["unit.sizes"]) == [u.size for u in units]
    mapped = np.array([names.index(v) for v in lab.tolist()])
    ame_units = np.arange(G)                                               # every unit: refitted, and its AMEs recomputed
    brute, den, ys = brute_force(obj, units)
    closed = closed_form_numpy(obj, mapped, ame_units[:8])                 # (the printed floor of dfame: the first 8 units)
    compare(name, "cluster", got, closed, units, np.arange(G), ame_units, brute, den, ys, True)
    Q, d, lam, _, _, _ = parts(obj)
    assert np.max(np.abs(got["hat"] - (Q ** 2) @ (d / (d + lam)))) <= 64 * Q.shape[1] * EPS
    ame = me_numpy(np.asarray(obj["X"]), np.asarray(obj["y"]).ravel(), np.asarray(obj["coeffs"]).ravel(), obj["sigma"],
                   np.asarray(obj["X"]))[1]
    assert np.max(np.abs(got["ame"].ravel() - ame)) <= 1e-8 * np.max(np.abs(ame))
    f2 = np.where([np.unique(np.asarray(obj["X"])[:, j]).size == 2 for j in range(np.asarray(obj["X"]).shape[1])], 2.0, 1.0)
    assert np.allclose(got["var.avgderivatives.jack"].ravel(), f2 * (G - 1.0) / G * np.sum(got["dfame"] ** 2, axis=0),
                       rtol=1e-13)                                         # (the reference's factor 2 on a binary column)
    assert np.allclose(got["resid.deleted"], np.asarray(obj["y"]).ravel() - got["fitted.deleted"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_single_row_deletion_against_brute_force(fits, ctx, name):
    import bigkrls_amd as bk
    obj = fits[name]
    n = np.asarray(obj["X"]).shape[0]
    got = bk.influence(obj, ctx=ctx)
    assert got["units"] == n and got["unit.labels"] is None and got["dfame"].shape[0] == n
    # n = 300: every row is refitted (R2.loo against the true one), the AME of 25 of them; n = 1100: 25 rows
    rows = np.arange(n) if n <= 300 else np.sort(np.random.default_rng(2).choice(n, size=25, replace=False))
    ame_units = np.sort(np.random.default_rng(2).choice(rows.size, size=25, replace=False))
    units = [np.array([i]) for i in rows]
    brute, den, ys = brute_force(obj, units, set(ame_units.tolist()))
    closed = closed_form_numpy(obj, np.arange(n), rows[ame_units])
    compare(name, "single", got, closed, units, rows, ame_units, brute, den, ys, n <= 300)
    if n > 300:                                                            # every row would be 1100 refits: the closed form
        assert abs(got["R2.loo"] - closed["r2"]) <= 10 * FLOOR["r2"]
    assert got["R2.loo"] < float(obj["R2"])


# ---- 4. CR3 and consistency ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [7, 40])
@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_cr3_against_the_dense_sandwich_and_the_jackknife(fits, ctx, name, G):
    import bigkrls_amd as bk
    obj = fits[name]
    Q, d, lam, y, ysd, ys = parts(obj)
    n, k = Q.shape
    lab = _labels(n, G)
    r = bk.robust_vcov(obj, type="CR3", cluster=lab, ctx=ctx)
    g, w = 1.0 / (d + lam), d / (d + lam)
    H = (Q * w) @ Q.T
    e = ys - H @ ys
    et, cond = np.zeros(n), 0.0
    for v in range(G):
        idx = np.flatnonzero(lab == v)
        A = np.eye(idx.size) - H[np.ix_(idx, idx)]
        et[idx] = np.linalg.solve(A, e[idx])
        cond = max(cond, np.linalg.cond(A, 2))
    Gm = (Q * g) @ Q.T
    V_ref = ysd ** 2 * (G - 1.0) / G * (Gm @ (np.outer(et, et) * (lab[:, None] == lab[None, :])) @ Gm)
    Qr, wr = host(r["vcov.est.Q"]), np.asarray(r["vcov.est.w"])
    V = (Qr * wr) @ Qr.T
    bound = 64 * (n + k) * EPS * np.linalg.norm(V_ref, 2) * cond
    err = float(np.max(np.abs(V - V_ref)))
    print(f"robust_vcov CR3 {name} G={G}: max cond(I - H_SS) {cond:.3e}, max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3e}")
    assert err <= bound
    assert r["vcov.type"] == "CR3" and r["vcov.clusters"] == G and np.all(wr >= 0) and np.all(np.diff(wr) <= 0)
    inf = bk.influence(obj, cluster=lab, ctx=ctx)
    va, vj = np.asarray(r["var.avgderivatives"]).ravel(), inf["var.avgderivatives.jack"].ravel()
    print(f"CR3 var.avgderivatives vs the jackknife: {np.max(np.abs(va - vj)) / np.max(vj):.3e}")
    assert np.max(np.abs(va - vj)) <= 1e-8 * np.max(vj)
    # a robust object carries the fit's own eigenvectors: influence() on it is influence() on the fit
    again = bk.influence(r, cluster=lab, ctx=ctx)
    assert same_bits(again["resid.deleted"], inf["resid.deleted"]) and same_bits(again["dfame"], inf["dfame"])


def test_implicit_fit_and_newdata(ctx):
    import bigkrls_amd as bk
    X, y = _data(1100, 3, 43, False)                                       # (the shape of test_gpu_robust_vcov.py's implicit fit)
    obj = bk.bigKRLS(y, X, sigma=4.0, kernel="implicit", Neig=64, vcov_form="factors", ctx=ctx, noisy=False)
    lab = _labels(1100, 10)
    Z = np.random.default_rng(5).standard_normal((7, 3))
    inf = bk.influence(obj, cluster=lab, which_derivatives=[3, 1], newdata=Z, ctx=ctx)
    Q, d, lam, _, ysd, ys = parts(obj)
    mapped = np.array([inf["unit.labels"].index(v) for v in lab.tolist()])
    ref = influence_numpy(Q, d, lam, ys, mapped, np.zeros((1100, 1)))
    assert np.max(np.abs(inf["resid.deleted"] - ysd * ref["et"])) <= 1e-10 * np.max(np.abs(ysd * ref["et"]))
    assert np.max(np.abs(inf["cooks"] - ref["cooks"])) <= 1e-10 * np.max(ref["cooks"])
    # on newdata the AME is marginal_effects' own, and dfame its change under the deleted coefficients
    me = bk.marginal_effects(obj, Z, which_derivatives=[3, 1], ctx=ctx)
    assert np.max(np.abs(inf["ame"] - me["avgderivatives"])) <= 1e-8 * np.max(np.abs(me["avgderivatives"]))
    coeffs = np.asarray(obj["coeffs"]).ravel()
    g = 1.0 / (d + lam)
    for u in (0, 9):
        idx = np.flatnonzero(mapped == u)
        dc = Q @ (g * (Q[idx].T @ ref["et"][idx]))
        want = me_numpy(X, y, coeffs, obj["sigma"], Z, which=[3, 1])[1] - me_numpy(X, y, coeffs - dc, obj["sigma"], Z, which=[3, 1])[1]
        assert np.max(np.abs(inf["dfame"][u] - want)) <= 1e-8 * np.max(np.abs(inf["dfame"]))
    assert inf["which.derivatives"] == [3, 1] and inf["dfame"].shape == (10, 2)
