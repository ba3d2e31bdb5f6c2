"""CPU checks of vcov.est.c kept as its factors Q diag(w) Q': the C ABI declares the new entries and fields and the
ctypes table matches them, the Python validation of vcov_form / max_factors / vcov= raises before any native call, and
the definitions -- the standard error of a prediction and the variance of an average marginal effect from the
factors -- are restated in numpy on an oracle fit and compared with the quadratic forms in the dense matrix."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = ["bigkrls_dev_rowsumsq_weighted", "bigkrls_predict_factored", "bigkrls_marginal_effects_factored"]


def block_rows_factored(n, k):
    """Rows per block of bigkrls_predict_factored without device outputs (include/bigkrls.h): the largest multiple of
    128 whose b x (n + k) doubles -- the test-kernel block and its product with Q -- fit 1 GiB, at least 128."""
    return max(128, (2 ** 30 // (8 * (n + k))) // 128 * 128)


def oracle_factors(ref):
    """(Q, w, d) of an oracle fit: vcov.est.c = Q diag(w) Q', vcov.est.fitted = Q diag(w d^2) Q'."""
    eig = ref["_eig"]
    k = int(eig.lastkeeper)
    Q, d = np.asarray(eig.vectors)[:, :k], np.asarray(eig.values)[:k]
    ysd = float(np.std(ref["y"], ddof=1))
    w = ysd ** 2 * float(ref["sigmasq"]) * (d + float(ref["lambda"])) ** -2.0
    return Q, w, d


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
def _header():
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_arity(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NEW_ENTRIES)
def test_header_declares_and_ctypes_table_matches(name):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name)


def test_factored_entries_replace_the_matrix_by_four_arguments():
    """(d_Q, ldq, k, h_w) in place of d_vcov_c: three more arguments than the dense entries."""
    assert _header_arity("bigkrls_predict_factored") == _header_arity("bigkrls_predict") + 3
    assert _header_arity("bigkrls_marginal_effects_factored") == _header_arity("bigkrls_marginal_effects") + 3


def test_outputs_struct_gains_the_factor_fields_at_its_end(tmp_path):
    """The four fields follow phase_s, so no existing offset moves; a C compiler and ctypes agree on them."""
    import subprocess
    from bigkrls_amd import _lib
    names = [f[0] for f in _lib.FitOutputs._fields_]
    assert names[-5:] == ["phase_s", "d_vcov_q", "vcov_q_cols_max", "vcov_w", "vcov_q_cols"]
    body = re.search(r"typedef struct bigkrls_fit_outputs \{(.*?)\} bigkrls_fit_outputs;", _header(), flags=re.S).group(1)
    decl = re.findall(r"\b(\w+)\s*(?:\[\d+\])?\s*;", body)
    assert decl[-5:] == ["phase_s", "d_vcov_q", "vcov_q_cols_max", "vcov_w", "vcov_q_cols"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bigkrls.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(bigkrls_fit_outputs), '
                   'offsetof(bigkrls_fit_outputs, d_vcov_q), offsetof(bigkrls_fit_outputs, vcov_q_cols_max), '
                   'offsetof(bigkrls_fit_outputs, vcov_w), offsetof(bigkrls_fit_outputs, vcov_q_cols));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    F = _lib.FitOutputs
    assert got == [C.sizeof(F), F.d_vcov_q.offset, F.vcov_q_cols_max.offset, F.vcov_w.offset, F.vcov_q_cols.offset]
    assert F.d_vcov_q.offset == F.phase_s.offset + 8 * 8


def test_public_api_exposes_the_keywords_and_the_wrapper():
    import bigkrls_amd as bk
    from bigkrls_amd import dist
    sig = inspect.signature(bk.bigKRLS).parameters
    assert sig["vcov_form"].default == "dense" and sig["max_factors"].default is None
    assert inspect.signature(dist.bigKRLS_dist).parameters["vcov_form"].default == "dense"
    assert "max_factors" in inspect.signature(dist.bigKRLS_dist).parameters
    assert inspect.signature(bk.predict).parameters["vcov"].default is None
    assert inspect.signature(bk.marginal_effects).parameters["vcov"].default is None
    assert callable(bk.ops.bRowSumSqWeighted)


def test_block_rows_rule():
    assert block_rows_factored(20000, 250) == 6528
    assert block_rows_factored(20000, 0) == 6656            # the pointwise entry's own rule
    assert block_rows_factored(10 ** 7, 2048) == 128
    b = block_rows_factored(1000, 1000)
    assert b % 128 == 0 and 8 * b * 2000 <= 2 ** 30


# --------------------------------------------------------------------------
# validation happens in Python, before any native call (no GPU here)
# --------------------------------------------------------------------------
class _NoContext:
    """Stands in for a Context: any use of it is a native call."""
    def __getattr__(self, name):
        raise AssertionError("native call reached")


@pytest.fixture
def no_native(monkeypatch):
    from bigkrls_amd import api

    def boom(*a, **k):
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", boom)
    monkeypatch.setattr(api, "default_context", boom)


def _data(n=40, p=3):
    rng = np.random.default_rng(3)
    return rng.standard_normal(n), rng.standard_normal((n, p))


def _object(n=40, p=3, dense=True, factors=False, k=5, multi_gpu=False):
    from bigkrls_amd.api import BigKRLS
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, p))
    obj = BigKRLS({"X": X, "y": rng.standard_normal(n), "coeffs": rng.standard_normal(n), "sigma": float(p),
                   "which.derivatives": None, "has.big.matrices": False, "Neffective": n - 1.0,
                   "xlabs": [f"x{i + 1}" for i in range(p)]})
    if not multi_gpu:
        obj["vcov.est.c"] = np.eye(n) if dense else None
    else:
        obj["rows"] = (0, n // 2)
        obj["vcov.est.c.cols"] = None
    if factors:
        obj["vcov.est.Q"] = np.linalg.qr(rng.standard_normal((n, k)))[0]
        obj["vcov.est.w"] = rng.random(k)
    return obj


@pytest.mark.parametrize("bad", ["Dense", "factor", "", None, 1])
def test_bad_vcov_form_raises(no_native, bad):
    import bigkrls_amd as bk
    y, X = _data()
    with pytest.raises(ValueError, match="vcov_form"):
        bk.bigKRLS(y, X, vcov_form=bad, ctx=_NoContext())


@pytest.mark.parametrize("bad", [0, -3, 2.5, "7", True])
def test_bad_max_factors_raises(no_native, bad):
    import bigkrls_amd as bk
    y, X = _data()
    with pytest.raises(ValueError, match="max_factors"):
        bk.bigKRLS(y, X, vcov_form="factors", max_factors=bad, ctx=_NoContext())


@pytest.mark.parametrize("form", ["factors", "both"])
def test_factors_require_vcov_est(no_native, form):
    import bigkrls_amd as bk
    y, X = _data()
    with pytest.raises(ValueError, match="vcov_est"):
        bk.bigKRLS(y, X, derivative=False, vcov_est=False, vcov_form=form, ctx=_NoContext())


def test_valid_forms_reach_the_allocation(no_native):
    """Nothing about a valid vcov_form / max_factors raises in Python: the first use of the context is reached."""
    import bigkrls_amd as bk
    y, X = _data()
    for kw in ({"vcov_form": "dense"}, {"vcov_form": "factors"}, {"vcov_form": "both", "max_factors": 7},
               {"vcov_form": "factors", "max_factors": np.int64(3)}):
        with pytest.raises(AssertionError, match="native call reached"):
            bk.bigKRLS(y, X, ctx=_NoContext(), **kw)


def test_capacity_rule(monkeypatch):
    """Neig columns when Neig is given or nothing is truncated; otherwise max_factors, default min(n, 2048)."""
    from bigkrls_amd import api

    class Stop(Exception):
        pass

    class Ctx:
        handle = None

        def __init__(self):
            self.shapes = []

        def empty(self, nrow, ncol=1):
            self.shapes.append((nrow, ncol))
            return type("M", (), {"ptr": None})()

    def stop(*a, **k):
        raise Stop()
    monkeypatch.setattr(api, "_call_native", stop)
    y, X = _data(60, 2)

    def capacity(**kw):
        cx = Ctx()
        with pytest.raises(Stop):
            api.bigKRLS(y, X, ctx=cx, vcov_form="factors", **kw)
        assert cx.shapes[0] == (60, 60) and len(cx.shapes) == 2       # K and Q: no other matrix
        assert cx.shapes[1][0] == 60
        return cx.shapes[1][1]
    assert capacity() == 60                                  # n <= 3000: eigtrunc 0, nothing truncated
    assert capacity(Neig=17) == 17
    assert capacity(Neig=17, eigtrunc=0.01, max_factors=5) == 17
    assert capacity(eigtrunc=0.01) == 60                     # min(n, 2048)
    assert capacity(eigtrunc=0.01, max_factors=9) == 9
    assert capacity(eigtrunc=0.01, max_factors=900) == 60
    assert capacity(eigtrunc=0.0, max_factors=9) == 60


@pytest.mark.parametrize("fn", ["predict", "marginal_effects"])
def test_bad_vcov_argument_raises(no_native, fn):
    import bigkrls_amd as bk
    obj = _object(factors=True)
    for bad in ("both", "Factors", 0):
        with pytest.raises(ValueError, match="vcov must be"):
            getattr(bk, fn)(obj, obj["X"][:3], vcov=bad)


@pytest.mark.parametrize("fn", ["predict", "marginal_effects"])
def test_forced_form_that_is_absent_raises(no_native, fn):
    import bigkrls_amd as bk
    f = getattr(bk, fn)
    dense_only, factors_only = _object(), _object(dense=False, factors=True)
    with pytest.raises(ValueError, match="vcov.est.Q"):
        f(dense_only, dense_only["X"][:3], vcov="factors")
    with pytest.raises(ValueError, match="no vcov.est.c"):
        f(factors_only, factors_only["X"][:3], vcov="dense")


def test_predict_without_any_form_keeps_todays_error(no_native):
    import bigkrls_amd as bk
    obj = _object(dense=False)
    with pytest.raises(ValueError, match="recompute bigKRLS object with bigKRLS\\(,vcov.est=TRUE\\)"):
        bk.predict(obj, obj["X"][:3], se_pred=True, ctx=_NoContext())
    mg = _object(multi_gpu=True)                              # a multi-GPU object without factors: the same error
    with pytest.raises(ValueError, match="recompute bigKRLS object"):
        bk.predict(mg, mg["X"][:3], se_pred=True, ctx=_NoContext())


def test_multi_gpu_object_needs_factors_for_marginal_effects(no_native):
    import bigkrls_amd as bk
    mg = _object(multi_gpu=True)
    with pytest.raises(NotImplementedError):
        bk.marginal_effects(mg, mg["X"][:3])
    with pytest.raises(ValueError, match="vcov.est.Q"):
        bk.marginal_effects(mg, mg["X"][:3], vcov="factors")
    mgf = _object(multi_gpu=True, factors=True)               # with factors it is accepted: up to the native call
    with pytest.raises(AssertionError, match="native call reached"):
        bk.marginal_effects(mgf, mgf["X"][:3])


class _FakeCtx:
    handle = None

    def from_numpy(self, a):
        a = np.asarray(a)
        return type("M", (), {"ptr": None, "ld": a.shape[0], "nrow": a.shape[0], "ncol": a.shape[1]})()

    def empty(self, nrow, ncol=1):
        return type("M", (), {"ptr": None, "ld": nrow, "nrow": nrow, "ncol": ncol})()


@pytest.mark.parametrize("obj_kw,vcov,matrices,entry", [
    ({"factors": True}, None, True, "bigkrls_predict"),                         # None prefers the dense matrix
    ({"factors": True}, None, False, "bigkrls_predict_pointwise"),
    ({"factors": True}, "factors", True, "bigkrls_predict_factored"),
    ({"factors": True}, "factors", False, "bigkrls_predict_factored"),
    ({"factors": True, "dense": False}, None, False, "bigkrls_predict_factored"),
    ({"factors": True, "multi_gpu": True}, None, False, "bigkrls_predict_factored"),
])
def test_predict_reaches_the_entry_of_the_chosen_form(monkeypatch, obj_kw, vcov, matrices, entry):
    from bigkrls_amd import _lib, api
    seen = []

    def record(name, *args):
        seen.append((name, args))
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", record)
    obj = _object(**obj_kw)
    with pytest.raises(AssertionError, match="native call reached"):
        api.predict(obj, obj["X"][:3], se_pred=True, ctx=_FakeCtx(), matrices=matrices, vcov=vcov)
    assert [s[0] for s in seen] == [entry]
    assert len(seen[0][1]) == len(_lib.SIGNATURES[entry])


@pytest.mark.parametrize("obj_kw,vcov,entry", [
    ({"factors": True}, None, "bigkrls_marginal_effects"),
    ({"factors": True}, "factors", "bigkrls_marginal_effects_factored"),
    ({"factors": True, "dense": False}, None, "bigkrls_marginal_effects_factored"),
    ({"factors": True, "multi_gpu": True}, None, "bigkrls_marginal_effects_factored"),
])
def test_marginal_effects_reaches_the_entry_of_the_chosen_form(monkeypatch, obj_kw, vcov, entry):
    from bigkrls_amd import _lib, api
    seen = []

    def record(name, *args):
        seen.append((name, args))
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", record)
    obj = _object(**obj_kw)
    with pytest.raises(AssertionError, match="native call reached"):
        api.marginal_effects(obj, obj["X"][:3], ctx=_FakeCtx(), vcov=vcov)
    assert [s[0] for s in seen] == [entry]
    assert len(seen[0][1]) == len(_lib.SIGNATURES[entry])


# --------------------------------------------------------------------------
# the definitions: quadratic forms in Q diag(w) Q' are weighted sums of squares of Q'k
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_fit():
    from oracle import krls_oracle as orc
    X, y = orc.synth(160, 4, 29, binary_last=True)
    return orc.fit(y[:120], X[:120], eigtrunc=0.001, literal=False), X[120:] + 0.05


def test_factors_rebuild_both_variance_matrices(oracle_fit):
    ref, _ = oracle_fit
    Q, w, d = oracle_factors(ref)
    assert Q.shape[1] < Q.shape[0]                            # truncated: fewer columns than rows
    V = np.asarray(ref["vcov.est.c"])
    assert np.max(np.abs((Q * w) @ Q.T - V)) <= 1e-12 * np.max(np.abs(V))
    Vf = np.asarray(ref["vcov.est.fitted"])
    assert np.max(np.abs((Q * (w * d * d)) @ Q.T - Vf)) <= 1e-12 * np.max(np.abs(Vf))


@pytest.mark.parametrize("correct_se", [True, False])
def test_se_from_factors_equals_the_quadratic_form_and_oracle_predict(oracle_fit, correct_se):
    """k'(Q diag(w) Q')k == sum_j w_j (Q'k)_j^2 for every row k of the test kernel, and its square root is the
    reference's se.pred."""
    from oracle import krls_oracle as orc
    ref, Z = oracle_fit
    Q, w, _ = oracle_factors(ref)
    X = np.asarray(ref["X"])
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    Kn = orc.temp_kernel_literal((Z - m) / s, (X - m) / s, float(ref["sigma"]))
    V = np.asarray(ref["vcov.est.c"])
    dense = np.einsum("ij,ij->i", Kn @ V, Kn)
    T = Kn @ Q
    fact = (T ** 2) @ w
    assert np.all(fact >= 0.0)
    assert np.max(np.abs(fact - dense)) <= 1e-12 * np.max(dense)
    if correct_se:
        fact = fact * np.sqrt(X.shape[0] / float(ref["Neffective"]))
    pr = orc.predict(ref, Z, se_pred=True, correct_se=correct_se)
    assert np.max(np.abs(np.sqrt(fact) - pr["se.pred"])) <= 1e-11 * np.max(pr["se.pred"])


def test_marginal_effect_variance_from_factors(oracle_fit):
    """s'(Q diag(w) Q')s == sum_j w_j (Q's)_j^2 for the vectors s of the marginal-effects variance; in sample the
    result is the fit's own var.avgderivatives."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_me_cpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_marginal_effects_cpu.py"))
    me_cpu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(me_cpu)
    ref, _ = oracle_fit
    Q, w, _ = oracle_factors(ref)
    X, y = np.asarray(ref["X"]), np.asarray(ref["y"])
    n, p = X.shape
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    Xs, ysd, sigma = (X - m) / s, float(np.std(y, ddof=1)), float(ref["sigma"])
    Kn = me_cpu._kernel(Xs, Xs, sigma)
    V = np.asarray(ref["vcov.est.c"]) / ysd ** 2
    var_dense, var_fact = np.empty(p), np.empty(p)
    for j in range(p):
        if np.unique(X[:, j]).size == 2:
            z0, z1 = Xs[:, j].min(), Xs[:, j].max()
            Z1, Z0 = Xs.copy(), Xs.copy()
            Z1[:, j], Z0[:, j] = z1, z0
            sv = (me_cpu._kernel(Z1, Xs, sigma) - me_cpu._kernel(Z0, Xs, sigma)).sum(axis=0)
            scale = 2.0 / ((z1 - z0) ** 2 * n ** 2)
        else:
            sv = ((Xs[:, j][:, None] - Xs[:, j][None, :]) * Kn).sum(axis=0)
            scale = 4.0 / (sigma ** 2 * n ** 2)
        g2 = (ysd / s[j]) ** 2
        var_dense[j] = g2 * scale * (sv @ V @ sv)
        var_fact[j] = g2 * scale * float(((Q.T @ sv) ** 2) @ (w / ysd ** 2))
    np.testing.assert_allclose(var_fact, var_dense, rtol=1e-10)
    _, _, var_me = me_cpu.me_numpy(X, y, ref["coeffs"], sigma, X, vcov_c=ref["vcov.est.c"])
    np.testing.assert_allclose(var_fact, var_me, rtol=1e-10)
    np.testing.assert_allclose(var_fact, np.asarray(ref["var.avgderivatives"]).ravel(), rtol=1e-8)
