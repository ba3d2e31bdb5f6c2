"""Every route of stage 1's panel factorisation (csrc/eigen_2stage.inc: Stage1::panel_qr, build_T), called directly through
bigkrls_dev_panel_factor -- which runs whatever stage 1 would run for a panel of m rows under the current BIGKRLS_PQ and
BIGKRLS_S1_TPQ -- packed and in place inside a larger parent, against float64 numpy on the downloaded factors.

Routes: split (default: pq_chol<true> -> pq_resident's slot -> pq_tail), fused (pq_chol<false>), householder (pq_resident
for every panel), steps (pq_first, pq_step, pq_fix_diag, s1_extract_v) and split with BIGKRLS_S1_TPQ=0 (T through the V'V
chain). Whatever the switch, a panel of fewer than 128 rows is pq_resident's and one of more than 80 workgroups goes
column by column.

Checks (tests/_panel_cases.py): max |H'H - I| through E = T'(V'V)T - T - T' in row blocks (and explicitly for m <= 1000),
max |P_in - V T'(V'P_in) - [R; 0]| / max |P_in|, |Vw Tfold - V T| / |V T|, and the structure, exactly. Bars: the project's
(CholeskyQR2 1e-13, 1e-13, W Tfold 1e-14; a Householder kernel 1e-12, 1e-12) or 10 x the error of LAPACK's Householder QR
(numpy.linalg.qr(mode="raw"), T by the forward dlarft recurrence) measured by the same functions on the same panel,
whichever is larger. No bar comes from the device's output.

What the panel holds below the diagonal depends on who did it: CholeskyQR2 leaves V itself, the Householder kernels the
columns as the reflections left them, with 1 / (alpha - beta) in stage 1's `scales` (which the back-transform multiplies
back in and the entry does not return): there column c of the panel times ONE double must be column c of V bit for bit
(_panel_cases.check_structure). No kernel chooses a form by ld or by alignment: every comparison between a placed and the
packed call is bitwise.

m < 64: min(64, m) reflectors (`ncolq`). Columns >= m of V, tau[m - 1:] and rows and columns >= m - 1 of T are exactly
zero (reflector m - 1 has nothing below its head: tau = 0; pq_resident and panel_qr zero the taus behind it), and the whole
m x 64 panel is R, upper trapezoidal.

LAPACK's own errors on these panels (orthogonality, factorisation): normal panels 1e-16 ... 1.4e-15, 2e-16 ... 1.7e-15 at
m = 2 ... 63; 3.2e-15, 6.2e-15 at m = 300; 4.0e-15, 1.2e-14 at m = 4097; 4.0e-15, 2.8e-14 at m = 20 480. Kahan panels:
<= 4.5e-15, <= 4.9e-15 at m = 300; <= 2.7e-15, <= 9.5e-15 at m = 4097.

Measured on an MI355X (worst of each group; LAPACK's worst on the same panels in brackets):
  group (panels)                 done by       orthogonality       factorisation       W Tfold
  in place, packed call (9)      CholeskyQR2   4.4e-15 (4.4e-15)   8.5e-15 (8.5e-15)   5.6e-16
  in place, packed call (12)     Householder   4.4e-15 (4.4e-15)   6.2e-15 (8.5e-15)   Vw == V
  ragged tail, m < 128 (14)      Householder   3.8e-15 (2.2e-15)   2.4e-15 (1.9e-15)   Vw == V
  27 ... 81 workgroups (4)       CholeskyQR2   4.4e-15 (4.4e-15)   3.4e-14 (2.9e-14)   2.2e-16
  27 ... 81 workgroups (6)       Householder   4.0e-15 (4.4e-15)   2.3e-14 (2.9e-14)   Vw == V
  special panels (7)             CholeskyQR2   3.6e-15 (3.2e-15)   5.3e-15 (6.2e-15)   2.4e-16
  special panels (19)            Householder   3.6e-15 (3.6e-15)   7.6e-15 (5.1e-15)   Vw == V
  gate sweep, kept (106)         CholeskyQR2   4.9e-15 (4.5e-15)   1.1e-14 (1.1e-14)   2.4e-16
  gate sweep, left (146)         Householder   4.9e-15 (4.4e-15)   9.1e-15 (1.2e-14)   Vw == V
In place: all five routes at m = 129, 257, 1000 and householder and steps at m = 2, 65, 127 are bit for bit the packed
call in all three placements, in a NaN and in a sentinel parent. Routes against each other: fused against split 0 in T and
V; BIGKRLS_S1_TPQ=0 against the default <= 5.9e-16 in T, 0 in V.

The gate (fallback of the 12 panels of a line: m = 300, 4097 x scales 1, 1e-20, 1e+20 x split, fused):
  Kahan c (cond)     0.20 ... 0.25 (1e6 ... 3.3e7): 0 everywhere      0.26 (6.5e7): 0 for 8, 1 for 4
                     0.27 (1.3e8): 1 for 10, 0 for 2                  0.28 ... 0.40 (2.6e8 ... 1.5e12): 1 everywhere
  mixed e (cond)     5, 6: 0 everywhere                               6.5, 7, 8, 10: 1 everywhere
This sweep found the gate wanting. With the pivot test, the ratio of the first factor's diagonal and the window [0.5, 2] on
the second factor's alone, CholeskyQR2 kept Kahan panels whose first Gram matrix is numerically singular but happened to
factorise: of the 24 panels at c = 0.35 and 0.40, 18 reported 0, with |H'H - I| = 3.8e-14 ... 9.9e-10 and a factorisation
error up to 6.3e-13 max |P| (c = 0.40, m = 300, x 1e+20: 9.9e-10; m = 4097, x 1e-20: 9.4e-10). pq_chol now also leaves a
panel whose second Gram matrix has max |Q1'Q1 - I| >= 2^-7 (PQC_E2MAX: below it cond(Q1) < sqrt(3)); what it keeps is
bit for bit what it kept before.

Teeth, on scratch builds with one arithmetic-only change each (never committed): `ld` replaced by `m` in the load of
pq_resident's top block: the six householder cases of test_in_place red, nothing else; grp[3] left out of pq_resident's
group sum: test_many_workgroups red at 6913, 9217, 20 225 and 20 480 rows under householder (green at 6912: flat);
a wrong sign in pq_fix_diag: every steps case of test_in_place and test_last_panels, test_many_workgroups at 20 736 and
four special panels under steps red (18); PQC_RATIO = 0 with the window on the second factor opened to [0, 1e300]: all green
-- with the bound on the second Gram matrix in place, that bound and the pivot test carry the gate on these panels alone,
the ratio and the window decide nothing here; without the bound (the code as it was) the four Kahan cases of the gate test
are red."""
import ctypes as C

import numpy as np
import pytest

import _panel_cases as pc
from _placement import SENT, place, placements, take

pytestmark = pytest.mark.gpu
B = pc.B
ROUTES = {
    "split": {},
    "fused": {"BIGKRLS_PQ": "fused"},
    "householder": {"BIGKRLS_PQ": "householder"},
    "steps": {"BIGKRLS_PQ": "steps"},
    "split-tpq0": {"BIGKRLS_S1_TPQ": "0"},
}
CHOL_ROUTES = ("split", "fused", "split-tpq0")
OUTPUTS = ("P", "Vw", "V", "T", "Tfold", "tau")


def F(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def set_route(monkeypatch, route):
    """(Stage1::init reads both switches at every call)"""
    monkeypatch.delenv("BIGKRLS_PQ", raising=False)
    monkeypatch.delenv("BIGKRLS_S1_TPQ", raising=False)
    for key, value in ROUTES[route].items():
        monkeypatch.setenv(key, value)


def cholqr2_takes(route, m):
    return route in CHOL_ROUTES and 2 * B <= m <= 80 * 256


def factor(ctx, P0, placement=None, fill=np.nan):
    """One call. placement: keyword arguments of _placement.place -- the panel then lies inside a parent filled with
    `fill`, and everything around it must come back untouched. The outputs start as NaN: whatever is not written shows."""
    from bigkrls_amd import _lib
    m = P0.shape[0]
    if placement is None:
        parent, ptr, ld, r0, c0 = place(ctx, F(P0), sub=False)
    else:
        parent, ptr, ld, r0, c0 = place(ctx, F(P0), fill=fill, **placement)
    nan = lambda r, c: ctx.from_numpy(np.full((r, c), np.nan, order="F"))
    Vw, V, T, Tf, tau = nan(m, B), nan(m, B), nan(B, B), nan(B, B), nan(B, 1)
    fb = C.c_int32(-1)
    _lib.call("bigkrls_dev_panel_factor", ctx.handle, ptr, ld, m, Vw.ptr, V.ptr, T.ptr, Tf.ptr, tau.ptr, C.byref(fb))
    if placement is None:
        P = parent.to_numpy()
    elif isinstance(fill, float) and np.isnan(fill):
        whole = np.array(parent.to_numpy())
        P = whole[r0:r0 + m, c0:c0 + B].copy()
        whole[r0:r0 + m, c0:c0 + B] = np.nan
        assert np.isnan(whole).all(), "the NaN around the panel did not survive"
    else:
        P = take(parent, r0, c0, m, B, "panel_factor")
    return dict(P=np.array(P), Vw=Vw.to_numpy(), V=V.to_numpy(), T=T.to_numpy(), Tfold=Tf.to_numpy(),
                tau=tau.to_numpy().ravel(), fallback=fb.value)


def check(P0, out, route, ref, label, fallback=0):
    """The identities against their bars and the structure, exactly. fallback: the value the call must report (None: either;
    the bars follow what it did report). Returns the three errors."""
    m = P0.shape[0]
    if fallback is not None:
        assert out["fallback"] == fallback, (label, out["fallback"])
    assert out["fallback"] in (0, 1) and (out["fallback"] == 0 or cholqr2_takes(route, m))
    chol = cholqr2_takes(route, m) and out["fallback"] == 0
    for key in OUTPUTS:
        assert np.isfinite(out[key]).all(), (label, key)
    orth, fact, fold = pc.errors(P0, out)
    bar_o, bar_f = pc.bars("cholqr2" if chol else "householder", ref)
    print(f"{label} m={m} {route}: {'CholeskyQR2' if chol else 'Householder'} fallback {out['fallback']} |H'H - I| {orth:.2e} "
          f"(LAPACK {ref[0]:.1e}) |H'P - R| / max|P| {fact:.2e} (LAPACK {ref[1]:.1e}) |W Tfold - V T| / |V T| {fold:.2e}")
    pc.check_structure(out, m, scaled_in_place=chol)
    assert orth <= bar_o, (label, orth, bar_o)
    assert fact <= bar_f, (label, fact, bar_f)
    if chol and route in ("split", "split-tpq0"):
        assert fold <= pc.FOLD_BAR, (label, fold)
    else:       # W-space is V-space, bit for bit
        assert np.array_equal(out["Vw"], out["V"]) and np.array_equal(out["Tfold"], out["T"]), label
    return orth, fact, fold


def same_bits(a, b, what):
    for key in OUTPUTS:
        assert np.array_equal(a[key], b[key]), (what, key)
    assert a["fallback"] == b["fallback"], what


# ---- a. in place ----------------------------------------------------------------------------------------------------------
IN_PLACE = [(m, r) for m in (129, 257, 1000) for r in ROUTES] + [(m, r) for m in (2, 65, 127) for r in ("householder", "steps")]


@pytest.mark.parametrize("m,route", IN_PLACE)
def test_in_place_is_bitwise_the_packed_call(ctx, monkeypatch, m, route):
    """The panel inside a parent (ld > m, three alignments), once surrounded by NaN -- a read outside the block poisons
    the factors -- and once by a sentinel that must survive: every output is bit for bit that of the packed call, which
    passes the checks."""
    set_route(monkeypatch, route)
    P0 = pc.normal_panel(m)
    packed = factor(ctx, P0)
    check(P0, packed, route, pc.reference_errors(pc.normal_panel, m), "packed")
    for name, kw in placements(m).items():
        same_bits(factor(ctx, P0, kw, np.nan), packed, (name, "NaN parent"))
        same_bits(factor(ctx, P0, kw, SENT), packed, (name, "sentinel parent"))


# ---- b. the ragged tail -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["split", "steps"])
@pytest.mark.parametrize("m", [2, 3, 12, 63, 64, 65, 127])
def test_last_panels_of_a_decomposition(ctx, monkeypatch, m, route):
    """m = n - k - 64 < 128: pq_resident by default (one workgroup, ncolq = min(64, m), a partial top block), the
    per-column kernels under BIGKRLS_PQ=steps; CholeskyQR2 is never asked, so fallback stays 0."""
    set_route(monkeypatch, route)
    P0 = pc.normal_panel(m)
    check(P0, factor(ctx, P0), route, pc.reference_errors(pc.normal_panel, m), "tail")


# ---- c. workgroup counts ----------------------------------------------------------------------------------------------------
# 27 workgroups (flat exchange), 28 (the first grouped launch; its last group holds one workgroup), 37, 80 with a ragged
# and with a full last workgroup; 81: resident_qr is false, the per-column kernels run whatever the switch
WORKGROUPS = [(m, "householder") for m in (6912, 6913, 9217, 20225, 20480)] + \
             [(m, r) for m in (20225, 20480) for r in ("split", "fused")] + [(20736, "split")]


@pytest.mark.parametrize("m,route", WORKGROUPS)
def test_many_workgroups(ctx, monkeypatch, m, route):
    set_route(monkeypatch, route)
    P0 = pc.normal_panel(m)
    a = factor(ctx, P0)
    check(P0, a, route, pc.reference_errors(pc.normal_panel, m), "workgroups")
    same_bits(factor(ctx, P0), a, "second call")


# ---- d. the gate --------------------------------------------------------------------------------------------------------------
def gate_cases():
    for c in pc.KAHAN_C:
        yield "kahan", c, pc.kahan_panel, (0 if c <= 0.24 else 1 if c >= 0.35 else None)
    for e in pc.MIXED_E:
        yield "mixed", e, pc.mixed_panel, (0 if e <= 6 else 1 if e >= 8 else None)


_gate_refs = {}


def gate_reference(family, maker, par, m, scale):
    key = (family, par, m, scale)
    if key not in _gate_refs:
        P0 = maker(m, par) * scale
        ref = pc.lapack_factor(P0)
        _gate_refs[key] = (pc.orth_error(ref["V"], ref["T"]), pc.fact_error(P0, ref), pc.cond(maker(300, par)))
    return _gate_refs[key]


@pytest.mark.parametrize("route", ["split", "fused"])
@pytest.mark.parametrize("m", [300, 4097])
@pytest.mark.parametrize("family", ["kahan", "mixed"])
def test_gate_between_choleskyqr2_and_householder(ctx, monkeypatch, family, m, route):
    """P = Q0 R with cond(R) from 1e5 to 1.5e12, at scales 1, 1e-20 (a deflated trailing matrix) and 1e+20. Every panel is
    either left to the Householder kernel (fallback 1) and meets that kernel's bars, or done by CholeskyQR2 (0) and meets
    CholeskyQR2's: a panel that passes the gate with Q short of orthonormal fails here. Kahan c <= 0.24 and mixed e <= 6
    must report 0, Kahan c >= 0.35 and mixed e >= 8 must report 1; between them either. The whole table is printed before
    anything is asserted."""
    set_route(monkeypatch, route)
    failures = []
    for fam, par, maker, must in gate_cases():
        if fam != family:
            continue
        for scale in (1.0, 1e-20, 1e20):
            P0 = maker(m, par) * scale
            ref = gate_reference(fam, maker, par, m, scale)
            out = factor(ctx, P0)
            chol = out["fallback"] == 0
            orth, fact, fold = pc.errors(P0, out)
            bar_o, bar_f = pc.bars("cholqr2" if chol else "householder", ref[:2])
            bad = []
            if must is not None and out["fallback"] != must:
                bad.append(f"fallback must be {must}")
            if not orth <= bar_o:
                bad.append(f"orthogonality > {bar_o:.1e}")
            if not fact <= bar_f:
                bad.append(f"factorisation > {bar_f:.1e}")
            if chol and route == "split" and not fold <= pc.FOLD_BAR:
                bad.append("W Tfold")
            try:
                pc.check_structure(out, m, scaled_in_place=chol)
                if not (chol and route == "split"):
                    assert np.array_equal(out["Vw"], out["V"]) and np.array_equal(out["Tfold"], out["T"])
            except AssertionError as e:
                bad.append(f"structure: {e}")
            print(f"gate {fam} {par:<5} x{scale:<6g} m={m} {route}: cond {ref[2]:.1e} fallback {out['fallback']} "
                  f"orth {orth:.2e} fact {fact:.2e} fold {fold:.2e} (LAPACK {ref[0]:.1e} {ref[1]:.1e}){'  <-- ' + '; '.join(bad) if bad else ''}")
            if bad:
                failures.append((fam, par, scale, bad))
    assert not failures, failures


# ---- e. special panels ----------------------------------------------------------------------------------------------------
def special_panels():
    m = 300
    rng = np.random.default_rng(77)
    X = rng.standard_normal((m, B))
    zero_col = X.copy()
    zero_col[:, 17] = 0.0
    twins = X.copy()
    twins[:, 40] = twins[:, 9]
    eye = np.zeros((m, B))
    eye[:B] = np.eye(B)
    low = X.copy()
    low[:B] = 0.0
    # (name, panel, what CholeskyQR2's gate must report: the rank-deficient ones have no Cholesky factor)
    return {"zeros": (np.zeros((m, B)), 1), "zero-column": (zero_col, 1), "equal-columns": (twins, 1),
            "identity-on-zeros": (eye, 0), "zero-top-block": (low, 0)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(special_panels()))
def test_special_panels(ctx, monkeypatch, name, route):
    """All zeros, a zero column, two equal columns (left to the Householder kernel by every CholeskyQR2 route), [I; 0] and
    [0; X]. [I; 0] is triangular already: V = [I; 0] exactly on every route; the Householder kernels find nothing below
    any head (tau = 0, R = I), CholeskyQR2's reconstruction takes tau = 1 + |q_ii| = 2, R = -I (to a few units in the last place of 2)."""
    set_route(monkeypatch, route)
    P0, gate = special_panels()[name]
    ref_out = pc.lapack_factor(P0)
    ref = (pc.orth_error(ref_out["V"], ref_out["T"]), pc.fact_error(P0, ref_out))
    out = factor(ctx, P0)
    check(P0, out, route, ref, name, fallback=gate if cholqr2_takes(route, 300) else 0)
    if name == "identity-on-zeros":
        assert np.array_equal(out["V"], P0)
        if cholqr2_takes(route, 300):
            assert np.allclose(out["tau"], 2.0, rtol=0, atol=4e-15) and np.allclose(out["P"][:B], -np.eye(B), rtol=0, atol=4e-15)
        else:
            assert not out["tau"].any() and np.array_equal(out["P"], P0)
    if name == "zeros":
        assert not out["tau"].any() and not out["T"].any() and not out["P"].any()


# ---- f. routes against each other -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [257, 4097])
@pytest.mark.parametrize("maker", [pc.normal_panel, pc.graded_panel], ids=["normal", "graded"])
def test_routes_agree(ctx, monkeypatch, maker, m):
    """T from the V'V chain (BIGKRLS_S1_TPQ=0) against T written by the reconstruction, and the one-kernel form against
    the split one: the same tau signs, T and V to 1e-13."""
    P0 = maker(m)
    outs = {}
    for route in ("split", "split-tpq0", "fused"):
        set_route(monkeypatch, route)
        outs[route] = factor(ctx, P0)
        assert outs[route]["fallback"] == 0
    for route in ("split-tpq0", "fused"):
        a, b = outs[route], outs["split"]
        dT, dV = float(np.abs(a["T"] - b["T"]).max()), float(np.abs(a["V"] - b["V"]).max())
        print(f"{maker.__name__} m={m}: {route} against split: max |dT| {dT:.2e}, max |dV| {dV:.2e}")
        assert np.array_equal(np.sign(a["tau"]), np.sign(b["tau"]))
        assert dT <= 1e-13 and dV <= 1e-13


# ---- g. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, monkeypatch):
    from bigkrls_amd import _lib
    set_route(monkeypatch, "split")
    m = 300
    P0 = pc.normal_panel(m)
    P = ctx.from_numpy(F(P0))
    Vw, V, T, Tf, tau = ctx.empty(m, B), ctx.empty(m, B), ctx.empty(B, B), ctx.empty(B, B), ctx.empty(B, 1)
    fb = C.c_int32(-1)
    good = [P.ptr, m, m, Vw.ptr, V.ptr, T.ptr, Tf.ptr, tau.ptr, C.byref(fb)]

    def refused(args, words):
        with pytest.raises(_lib.BigKRLSError) as e:
            _lib.call("bigkrls_dev_panel_factor", ctx.handle, *args)
        assert e.value.code == _lib.EINVAL and "panel_factor" in str(e.value) and words in str(e.value), str(e.value)

    for bad_m in (0, 1):
        refused(good[:1] + [max(bad_m, 1), bad_m] + good[3:], "m out of range")
    refused(good[:1] + [m - 1, m] + good[3:], "ld too small")
    for i in (0, 3, 4, 5, 6, 7, 8):
        refused(good[:i] + [None] + good[i + 1:], "null pointer")
    # CholeskyQR2's kernels reach row r of column c at the 32-bit byte offset 8 r + c (8 ld): 63 ld + m <= 2^29
    ld_max = (2 ** 29 - m) // 63
    refused(good[:1] + [ld_max + 1, m] + good[3:], "ld too large")
    assert fb.value == -1
    _lib.call("bigkrls_dev_panel_factor", ctx.handle, *good)
    assert fb.value == 0
    out = dict(P=P.to_numpy(), Vw=Vw.to_numpy(), V=V.to_numpy(), T=T.to_numpy(), Tfold=Tf.to_numpy(),
               tau=tau.to_numpy().ravel(), fallback=fb.value)
    check(P0, out, "split", pc.reference_errors(pc.normal_panel, m), "after the refusals")
