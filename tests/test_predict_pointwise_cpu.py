"""CPU checks of predict(..., matrices=False): the C ABI declares both new entry points and the ctypes table matches
their arity, predict() raises the same errors in both modes before any native call, and the pointwise definition of
the standard errors -- se^2 = rowsum((Kn V) o Kn) sqrt(n / Neffective), restated here in numpy -- equals the
reference's sqrt(diag(vcov.est.pred)) (orc.predict, R/bigKRLS.R:599-613)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block_rows(n):
    """Rows per block of bigkrls_predict_pointwise (include/bigkrls.h): the largest multiple of 128 whose b x n
    block of doubles fits 1 GiB, at least 128."""
    return max(128, (2 ** 30 // (8 * n)) // 128 * 128)


def se_pointwise_numpy(X, y, sigma, V, newdata, neff=None):
    """se.pred without vcov.est.pred: sqrt(rowsum((Kn V) o Kn) [* sqrt(n / neff)])."""
    X = np.asarray(X, dtype=np.float64)
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    Xs, Zs = (X - m) / s, (np.asarray(newdata, dtype=np.float64) - m) / s
    d2 = ((Zs[:, None, :] - Xs[None, :, :]) ** 2).sum(axis=2)
    Kn = np.exp(-d2 / sigma)
    q = np.einsum("ij,ij->i", Kn @ np.asarray(V), Kn)
    if neff is not None:
        q = q * np.sqrt(X.shape[0] / neff)
    return np.sqrt(q)


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ["bigkrls_dev_quadform_diag", "bigkrls_predict_pointwise"])
def test_header_declares_and_ctypes_table_matches(name):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name)


def test_pointwise_has_predicts_arguments_minus_the_matrices():
    assert _header_arity("bigkrls_predict_pointwise") == _header_arity("bigkrls_predict") - 2


def test_public_api_exposes_the_keyword_and_the_wrapper():
    import inspect
    import bigkrls_amd as bk
    assert inspect.signature(bk.predict).parameters["matrices"].default is True
    assert callable(bk.ops.bQuadformDiag)


def test_block_rows_rule():
    assert block_rows(20000) == 6656
    assert block_rows(10 ** 7) == 128
    assert block_rows(1000) % 128 == 0 and 8 * block_rows(1000) * 1000 <= 2 ** 30


# --------------------------------------------------------------------------
# validation happens in Python, before any native call (no GPU here)
# --------------------------------------------------------------------------
def _object(n=40, p=3, vcov=True):
    from bigkrls_amd.api import BigKRLS
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, p))
    return BigKRLS({"X": X, "y": rng.standard_normal(n), "coeffs": rng.standard_normal(n), "sigma": float(p),
                    "vcov.est.c": np.eye(n) if vcov else None, "has.big.matrices": False, "Neffective": n - 1.0})


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


def _raised(fn):
    try:
        fn()
    except AssertionError:
        raise
    except Exception as e:   # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error raised")


@pytest.mark.parametrize("matrices", [True, False])
def test_not_a_bigkrls_object_raises(no_native, matrices):
    import bigkrls_amd as bk
    with pytest.raises(TypeError, match="Object not of class 'bigKRLS'"):
        bk.predict({"X": np.zeros((3, 2))}, np.zeros((1, 2)), matrices=matrices)


def test_errors_are_the_same_in_both_modes(no_native):
    import bigkrls_amd as bk
    obj, novc = _object(), _object(vcov=False)
    cases = [
        lambda m: bk.predict({"X": np.zeros((3, 2))}, np.zeros((1, 2)), matrices=m),
        lambda m: bk.predict(obj, np.zeros((5, 4)), ctx=_NoContext(), matrices=m),
        lambda m: bk.predict(novc, obj["X"][:3], se_pred=True, ctx=_NoContext(), matrices=m),
    ]
    for case in cases:
        assert _raised(lambda: case(False)) == _raised(lambda: case(True))
    assert _raised(lambda: cases[1](False)) == (ValueError, "ncol(newdata) differs from ncol(X) from fitted bigKRLS "
                                                            "object")
    assert _raised(lambda: cases[2](False)) == (ValueError, "recompute bigKRLS object with bigKRLS(,vcov.est=TRUE) "
                                                            "to compute standard errors")


def test_valid_call_reaches_the_pointwise_entry(monkeypatch):
    """matrices=False goes to bigkrls_predict_pointwise, with predict's arguments minus the two matrices."""
    from bigkrls_amd import api
    seen = []

    def record(name, *args):
        seen.append((name, args))
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", record)
    obj = _object(vcov=False)
    with pytest.raises(AssertionError, match="native call reached"):
        api.predict(obj, obj["X"][:3], ctx=type("C", (), {"handle": None})(), matrices=False)
    assert [s[0] for s in seen] == ["bigkrls_predict_pointwise"]
    from bigkrls_amd import _lib
    assert len(seen[0][1]) == len(_lib.SIGNATURES["bigkrls_predict_pointwise"])


# --------------------------------------------------------------------------
# the definition: the pointwise SEs are the reference's sqrt(diag(vcov.est.pred))
# --------------------------------------------------------------------------
@pytest.mark.parametrize("correct_se", [True, False])
def test_numpy_restatement_equals_oracle_predict(correct_se):
    from oracle import krls_oracle as orc
    X, y = orc.synth(160, 4, 29, binary_last=True)
    ref = orc.fit(y[:120], X[:120], literal=False)
    Z = X[120:] + 0.05
    pr = orc.predict(ref, Z, se_pred=True, correct_se=correct_se)
    neff = float(ref["Neffective"]) if correct_se else None
    se = se_pointwise_numpy(ref["X"], ref["y"], float(ref["sigma"]), ref["vcov.est.c"], Z, neff)
    assert np.max(np.abs(se - pr["se.pred"])) <= 1e-12 * np.max(pr["se.pred"])
