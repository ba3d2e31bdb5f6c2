"""Seeded inputs, cases and output digests of the post-estimation entries (marginal_effects and its standard errors,
interaction_effects and its standard errors, group_effects, partial_dependence, conditional_effects), shared by
tests/test_gpu_effects_digests.py and tools/effects_digests.py (which records tests/golden/effects_digests.json).

The model object is built by hand: no fit feeds the digests. n = 130 training rows, p = 4 columns, column 4 binary,
sigma = p; u = 45 new rows, or 300 with _block_rows = 128 for the pointwise standard errors (two full row blocks and a
ragged third). vcov.est.c is exact in floating point whatever the summation order: Q (n x 9) has entries in
{-1, -0.5, 0, 0.5, 1}, w entries in {0.25, 0.5, 1, 2} and V = Q diag(w) Q' (every product and partial sum is a small
multiple of 1/16), so the dense and the factored form describe one matrix and the inputs do not depend on the BLAS of
the recording machine. Every case records each returned array and the context's workspace_bytes() after the call; the
error cases go through the C ABI directly and record the message."""
import hashlib

import numpy as np

N, P, U, U_SE, K, BLOCK = 130, 4, 45, 300, 9, 128
WHICH = [3, 1, 4]
IE_PAIRS = [(1, 3), (3, 3), (1, 4), (2, 4)]
PD_WHICH = [2, 4, 1]
PD_SIZES = [1, 5, 8]
CE_PAIRS = [(1, 2), (2, 2), (4, 1), (1, 4), (4, 2)]      # continuous j != k, j == k, binary j, binary along, binary j
CE_SIZES = [3, 1, 5, 2, 4]
FORMS = (None, "dense", "factors")


def _uniform(rng, shape):
    # (Generator.random: the plain double stream, the same on every NumPy)
    return (rng.random(shape) - 0.5) * 2.4


def data(u=U, seed=11):
    rng = np.random.default_rng(seed)
    X, Z = np.asfortranarray(_uniform(rng, (N, P))), np.asfortranarray(_uniform(rng, (u, P)))
    X[:, P - 1] = np.where(rng.random(N) < 0.45, 1.0, 0.0)
    Z[:, P - 1] = np.where(rng.random(u) < 0.45, 1.0, 0.0)
    y, c = np.ascontiguousarray(_uniform(rng, N)), np.ascontiguousarray(_uniform(rng, N))
    Q = np.asfortranarray((np.floor(rng.random((N, K)) * 5.0) - 2.0) / 2.0)
    w = np.ascontiguousarray(2.0 ** (np.floor(rng.random(K) * 4.0) - 2.0))
    V = np.asfortranarray((Q * w) @ Q.T)
    return {"X": X, "Z": Z, "y": y, "c": c, "Q": Q, "w": w, "V": V, "u": u}


def model(d, form):
    from bigkrls_amd.api import BigKRLS
    obj = BigKRLS({"X": d["X"], "y": d["y"], "coeffs": d["c"], "sigma": float(P), "which.derivatives": None,
                   "has.big.matrices": False, "Neffective": 57.25, "xlabs": [f"x{i + 1}" for i in range(P)]})
    if form == "dense":
        obj["vcov.est.c"] = d["V"]
    if form == "factors":
        obj["vcov.est.Q"], obj["vcov.est.w"] = d["Q"], d["w"]
    return obj


def labels(u, G, scrambled):
    lab = np.arange(u, dtype=np.int64) * G // u
    return lab[np.random.default_rng(5).permutation(u)] if scrambled else lab


def grids(d, cols, sizes):
    """One grid per entry of cols (1-based) with the given lengths: evenly spaced inside the training range, or the
    two training values in turn for the binary column."""
    out = []
    for j, g in zip(cols, sizes):
        x = d["X"][:, j - 1]
        out.append(np.array([x.min(), x.max()] * g)[:g] if j == P else np.linspace(x.min(), x.max(), g + 2)[1:-1])
    return out


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def digests(out):
    """{key: digest} of every array (or list of arrays) of a result; None is recorded as such."""
    res = {}
    for key, v in out.items():
        if v is None:
            res[key] = "None"
        elif isinstance(v, np.ndarray):
            res[key] = digest(v)
        elif isinstance(v, dict):
            res.update({f"{key}.{k2}": d2 for k2, d2 in digests(v).items()})
        elif isinstance(v, list) and v and all(isinstance(e, np.ndarray) for e in v):
            res.update({f"{key}[{i}]": digest(e) for i, e in enumerate(v)})
    return res


# ---- the C ABI, called directly --------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data


class Raw:
    """The entries through _lib.call on the arrays of data(): vcov.est.c uploaded once in both forms. Every method takes
    overrides of the arrays (the error cases) and returns the outputs it allocated."""

    def __init__(self, ctx, d):
        self.ctx, self.d = ctx, d
        self.Vd, self.Qd = ctx.from_numpy(d["V"]), ctx.from_numpy(d["Q"])

    def vcov(self, form, k=None):
        """(d_vcov_c, d_Q, ldq, k, h_w); form: None, "dense", "factors" or "both"."""
        fac = form in ("factors", "both")
        return (self.Vd.ptr if form in ("dense", "both") else None, self.Qd.ptr if fac else None,
                self.Qd.ld if fac else 0, (K if k is None else k) if fac else 0, _ptr(self.d["w"]) if fac else None)

    def head(self, X=None, y=None):
        d = self.d
        X, y = d["X"] if X is None else X, d["y"] if y is None else y
        self.keep = (X, y)
        return (self.ctx.handle, _ptr(X), N, P, _ptr(y), _ptr(d["c"]), float(P))

    def sel(self, items, count=None):
        """(pointer, count) of a list of columns or pairs; None: the default selection."""
        if items is None:
            return None, 0
        self.items = np.ascontiguousarray(items if len(items) else [0], dtype=np.int64)
        return _ptr(self.items), (len(items) if count is None else count)

    def call(self, name, *args):
        from bigkrls_amd import _lib
        _lib.call(name, *args)

    def me(self, form, which=WHICH, Z=None, k=None, **kw):
        Z = self.d["Z"] if Z is None else Z
        u, nj = Z.shape[0], len(which) if which else P
        D, avg, var = np.empty((u, nj), order="F"), np.empty(nj), np.empty(nj) if form else None
        v = self.vcov(form, k)
        if form == "factors":
            self.call("bigkrls_marginal_effects_factored", *self.head(**kw), *self.sel(which), _ptr(Z), u, *v[1:],
                      _ptr(D), _ptr(avg), _ptr(var))
        else:
            self.call("bigkrls_marginal_effects", *self.head(**kw), *self.sel(which), _ptr(Z), u, v[0], _ptr(D),
                      _ptr(avg), _ptr(var))
        return {"D": D, "avg": avg, "var": var}

    def me_se(self, form, which=WHICH, block_rows=0, k=None):
        Z = self.d["Z"]
        se = np.empty((Z.shape[0], len(which)), order="F")
        self.call("bigkrls_marginal_effects_se", *self.head(), *self.sel(which), _ptr(Z), Z.shape[0],
                  *self.vcov(form, k), block_rows, _ptr(se))
        return {"se": se}

    def ie(self, form, pairs=IE_PAIRS, Z=None, k=None):
        Z = self.d["Z"] if Z is None else Z
        u, m = Z.shape[0], len(pairs)
        vals, avg, var = np.empty((u, m), order="F"), np.empty(m), np.empty(m) if form else None
        self.call("bigkrls_interaction_effects", *self.head(), *self.sel(pairs), _ptr(Z), u, *self.vcov(form, k),
                  _ptr(vals), _ptr(avg), _ptr(var))
        return {"vals": vals, "avg": avg, "var": var}

    def ie_se(self, form, pairs=IE_PAIRS, block_rows=0):
        Z = self.d["Z"]
        se = np.empty((Z.shape[0], len(pairs)), order="F")
        self.call("bigkrls_interaction_effects_se", *self.head(), *self.sel(pairs), _ptr(Z), Z.shape[0],
                  *self.vcov(form), block_rows, _ptr(se))
        return {"se": se}

    def ge(self, form, lab, G, which=WHICH, Z=None, k=None, null_newdata=False):
        Z = self.d["Z"] if Z is None else Z
        u, nj = Z.shape[0], len(which)
        D, ame = np.empty((u, nj), order="F"), np.empty((G, nj), order="F")
        cov = np.empty((G * nj, G * nj), order="F") if form else None
        lab = np.ascontiguousarray(lab, dtype=np.int64)
        self.call("bigkrls_group_effects", *self.head(), *self.sel(which), None if null_newdata else _ptr(Z), u,
                  _ptr(lab), G, *self.vcov(form, k), _ptr(D), _ptr(ame), _ptr(cov))
        return {"D": D, "ame": ame, "cov": cov}

    def curves(self, name, form, items, sizes, newdata=True, se=True, cov=True, neffective=None, off=None, grid=None,
               Z=None, k=None, null_grid=False, **kw):
        """bigkrls_partial_dependence (items: columns) or bigkrls_conditional_effects (items: pairs, the grid on the second)."""
        d = self.d
        Z = (d["Z"] if Z is None else Z) if newdata else None
        gcols = [it if name == "partial_dependence" else it[1] for it in items]
        flat = np.ascontiguousarray(np.concatenate(grids(d, gcols, sizes))) if grid is None else grid
        sizes = np.asarray(sizes, dtype=np.int64)
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]) if off is None else off, dtype=np.int64)
        T = int(np.sum(sizes))
        val, sev = np.empty(T), np.empty(T) if se else None
        cv = np.empty(int(np.sum(sizes * sizes))) if cov else None
        extra = () if neffective is None else (float(neffective),)
        self.call("bigkrls_" + name, *self.head(**kw), *self.sel(items), _ptr(Z), Z.shape[0] if newdata else N,
                  None if null_grid else _ptr(flat), _ptr(off), *self.vcov(form, k), *extra, _ptr(val), _ptr(sev), _ptr(cv))
        return {"val": val, "se": sev, "cov": cv}

    def pd(self, form, which=PD_WHICH, sizes=PD_SIZES, neffective=-1.0, **kw):
        return self.curves("partial_dependence", form, which, sizes, neffective=neffective, **kw)

    def ce(self, form, pairs=CE_PAIRS, sizes=CE_SIZES, **kw):
        return self.curves("conditional_effects", form, pairs, sizes, **kw)


# ---- the cases ---------------------------------------------------------------------------------------------------------
class _Package:
    """bigkrls_amd, imported at the first use (listing the cases needs no library)."""
    def __getattr__(self, name):
        import bigkrls_amd
        return getattr(bigkrls_amd, name)


bk = _Package()


def _api_cases():
    cases = {}

    def add(name, fn, u=U):
        cases[name] = (u, fn)

    for form in FORMS:
        f = form or "none"
        add(f"me_{f}", lambda c, d, form=form: bk.marginal_effects(model(d, form), d["Z"], WHICH, ctx=c))
        add(f"me_{f}_default", lambda c, d, form=form: bk.marginal_effects(model(d, form), d["Z"], ctx=c))
        add(f"ie_{f}", lambda c, d, form=form: bk.interaction_effects(model(d, form), d["Z"], pairs=IE_PAIRS, ctx=c))
        add(f"ie_{f}_default", lambda c, d, form=form: bk.interaction_effects(model(d, form), d["Z"], ctx=c))
        add(f"ge_{f}_G1", lambda c, d, form=form: bk.group_effects(model(d, form), np.zeros(U), d["Z"], WHICH, ctx=c))
        add(f"ge_{f}_G4_scrambled", lambda c, d, form=form: bk.group_effects(model(d, form), labels(U, 4, True) * 3 + 1,
                                                                             d["Z"], ctx=c))
        add(f"pd_{f}_training", lambda c, d, form=form: bk.partial_dependence(
            model(d, form), PD_WHICH, grids(d, PD_WHICH, PD_SIZES), se=form is not None, ctx=c))
        add(f"pd_{f}_newdata", lambda c, d, form=form: bk.partial_dependence(
            model(d, form), PD_WHICH, 6, d["Z"], se=form is not None, correct_SE=False, ctx=c))
        add(f"ce_{f}_training", lambda c, d, form=form: bk.conditional_effects(
            model(d, form), [1, 2, 4], 2, 5, se=form is not None, ctx=c))
        add(f"ce_{f}_newdata_binary_along", lambda c, d, form=form: bk.conditional_effects(
            model(d, form), [1, 2], [4, 1], 4, d["Z"], se=form is not None, ctx=c))
    for form in FORMS[1:]:
        add(f"me_{form}_se_blocks", lambda c, d, form=form: bk.marginal_effects(
            model(d, form), d["Z"], WHICH, ctx=c, se=True, _block_rows=BLOCK), U_SE)
        add(f"ie_{form}_se_blocks", lambda c, d, form=form: bk.interaction_effects(
            model(d, form), d["Z"], pairs=IE_PAIRS, ctx=c, se=True, _block_rows=BLOCK), U_SE)
    return cases


def _raw_cases():
    cases = {}
    for form in FORMS:
        f = form or "none"
        # G = 3 with group 1 empty: NaN means, zero rows and columns of the covariance
        cases[f"ge_{f}_G3_empty_group"] = lambda r, form=form: r.ge(form, labels(U, 2, False) * 2, 3)
        for newdata in (False, True):
            nd = "newdata" if newdata else "training"
            cases[f"pd_{f}_raw_{nd}"] = lambda r, form=form, newdata=newdata: r.pd(
                form, newdata=newdata, se=form is not None, cov=form is not None)
            cases[f"ce_{f}_raw_{nd}"] = lambda r, form=form, newdata=newdata: r.ce(
                form, newdata=newdata, se=form is not None, cov=form is not None)
    for form in FORMS[1:]:
        cases[f"pd_{form}_raw_se_only"] = lambda r, form=form: r.pd(form, cov=False)
        cases[f"pd_{form}_raw_cov_only_neffective"] = lambda r, form=form: r.pd(form, se=False, neffective=57.25)
        cases[f"pd_{form}_raw_values_only"] = lambda r, form=form: r.pd(form, se=False, cov=False)
        cases[f"ce_{form}_raw_se_only"] = lambda r, form=form: r.ce(form, cov=False)
        cases[f"ce_{form}_raw_cov_only"] = lambda r, form=form: r.ce(form, se=False)
        cases[f"ce_{form}_raw_values_only"] = lambda r, form=form: r.ce(form, se=False, cov=False)
    return cases


def _error_cases():
    """Every one raises BIGKRLS_EINVAL before any device work. *_two_faults: the input has two faults; the recorded
    message says which one is reported."""
    def bad_Z(r, rows=U):
        Z = r.d["Z"][:rows].copy(order="F")
        Z[1, 1] = np.inf
        return Z

    def const_col(r):
        X = r.d["X"].copy(order="F")
        X[:, 1] = 3.0
        return X

    gcap = (1 << 30) // (8 * N)
    over = np.array([0, gcap + 1], dtype=np.int64)
    return {
        "err_both_forms_me_se": lambda r: r.me_se("both"),
        "err_both_forms_ie": lambda r: r.ie("both"),
        "err_both_forms_ie_se": lambda r: r.ie_se("both"),
        "err_both_forms_ge": lambda r: r.ge("both", labels(U, 2, False), 2),
        "err_both_forms_pd": lambda r: r.pd("both"),
        "err_both_forms_ce": lambda r: r.ce("both"),
        "err_neither_form_me_se": lambda r: r.me_se(None),
        "err_neither_form_ie_se": lambda r: r.ie_se(None),
        "err_k_over_n_me": lambda r: r.me("factors", k=N + 1),
        "err_k_over_n_me_se": lambda r: r.me_se("factors", k=N + 1),
        "err_k_over_n_ie": lambda r: r.ie("factors", k=N + 1),
        "err_k_over_n_ge": lambda r: r.ge("factors", labels(U, 2, False), 2, k=N + 1),
        "err_k_over_n_pd": lambda r: r.pd("factors", k=N + 1),
        "err_k_over_n_ce": lambda r: r.ce("factors", k=N + 1),
        "err_which_zero_me": lambda r: r.me("dense", which=[3, 0, 4]),
        "err_which_zero_ge": lambda r: r.ge(None, labels(U, 2, False), 2, which=[3, 0, 4]),
        "err_which_zero_pd": lambda r: r.pd(None, which=[2, 0, 1], se=False, cov=False),
        "err_which_empty_me": lambda r: r.me(None, which=[]),
        "err_which_empty_pd": lambda r: r.pd(None, which=[], sizes=[1], grid=np.zeros(1), se=False, cov=False),
        "err_offsets_not_from_zero_pd": lambda r: r.pd("dense", off=[1, 2, 7, 15]),
        "err_offsets_not_from_zero_ce": lambda r: r.ce("dense", off=[1, 4, 5, 10, 12, 16]),
        "err_empty_grid_pd": lambda r: r.pd("dense", off=[0, 1, 1, 9]),
        "err_empty_grid_ce": lambda r: r.ce("dense", off=[0, 3, 3, 8, 10, 14]),
        "err_grid_over_gcap_pd": lambda r: r.pd(None, which=[2], sizes=[1], off=over, se=False, cov=False),
        "err_grid_over_gcap_ce": lambda r: r.ce(None, pairs=[(1, 2)], sizes=[1], off=over, se=False, cov=False),
        "err_nonfinite_newdata_me": lambda r: r.me("dense", Z=bad_Z(r)),
        "err_nonfinite_newdata_ie": lambda r: r.ie("factors", Z=bad_Z(r)),
        "err_nonfinite_newdata_ge": lambda r: r.ge("factors", labels(U, 2, False), 2, Z=bad_Z(r)),
        "err_nonfinite_newdata_pd": lambda r: r.pd("dense", Z=bad_Z(r)),
        "err_nonfinite_newdata_ce": lambda r: r.ce("dense", Z=bad_Z(r)),
        "err_constant_column_me": lambda r: r.me("dense", X=const_col(r)),
        "err_constant_column_pd": lambda r: r.pd("dense", X=const_col(r)),
        "err_constant_column_ce": lambda r: r.ce("dense", X=const_col(r)),
        "err_constant_y_me": lambda r: r.me("dense", y=np.full(N, 2.0)),
        "err_constant_y_pd": lambda r: r.pd("dense", y=np.full(N, 2.0)),
        "err_constant_y_ce": lambda r: r.ce("dense", y=np.full(N, 2.0)),
        "err_binary_diagonal_ie": lambda r: r.ie("dense", pairs=[(1, 2), (4, 4)]),
        "err_binary_diagonal_ce": lambda r: r.ce("dense", pairs=[(1, 2), (4, 4)], sizes=[2, 2]),
        "err_duplicated_pair_ie": lambda r: r.ie("dense", pairs=[(1, 3), (2, 2), (3, 1)]),
        "err_duplicated_pair_ce": lambda r: r.ce("dense", pairs=[(1, 3), (2, 2), (1, 3)], sizes=[2, 2, 2]),
        "err_block_rows_100_me_se": lambda r: r.me_se("factors", block_rows=100),
        "err_block_rows_100_ie_se": lambda r: r.ie_se("dense", block_rows=100),
        "err_label_equal_G_ge": lambda r: r.ge("dense", labels(U, 3, False), 2),
        "err_null_newdata_ge": lambda r: r.ge("dense", labels(U, 2, False), 2, null_newdata=True),
        "err_null_grid_pd": lambda r: r.pd("dense", null_grid=True),
        # two faults each
        "err_two_faults_me_se_both_forms_and_block_rows": lambda r: r.me_se("both", block_rows=100),
        "err_two_faults_me_which_zero_and_nonfinite_newdata": lambda r: r.me("dense", which=[3, 0], Z=bad_Z(r)),
        "err_two_faults_ie_k_over_n_and_duplicated_pair": lambda r: r.ie("factors", pairs=[(1, 3), (3, 1)], k=N + 1),
        "err_two_faults_ge_label_and_k_over_n": lambda r: r.ge("factors", labels(U, 3, False), 2, k=N + 1),
        "err_two_faults_pd_offsets_and_constant_y": lambda r: r.pd("dense", off=[1, 2, 7, 15], y=np.full(N, 2.0)),
        "err_two_faults_ce_duplicated_pair_and_empty_grid": lambda r: r.ce(
            "dense", pairs=[(1, 3), (1, 3)], sizes=[2, 0], off=[0, 2, 2]),
        "err_two_faults_ce_constant_column_and_binary_diagonal": lambda r: r.ce(
            "dense", pairs=[(1, 2), (4, 4)], sizes=[2, 2], X=const_col(r)),
    }


_API, _RAW, _ERR = _api_cases(), _raw_cases(), _error_cases()


def case_names():
    return list(_API) + list(_RAW) + list(_ERR)


def run_case(ctx, name):
    """{output: digest} of one case, with the workspace after the call; an error case: {"message": the text}."""
    from bigkrls_amd import _lib
    ctx.release_workspace()
    if name in _ERR:
        try:
            _ERR[name](Raw(ctx, data()))
        except _lib.BigKRLSError as e:
            return {"message": str(e)}
        return {"message": None}
    if name in _RAW:
        out = _RAW[name](Raw(ctx, data()))
    else:
        u, fn = _API[name]
        out = fn(ctx, data(u))
    ctx.sync()
    res = digests(out)
    res["workspace_bytes"] = int(ctx.workspace_bytes())
    return res
