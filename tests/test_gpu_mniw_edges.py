"""The MNIW solve kernels (csrc/pgas_marginal.hip.h) held to their componentwise backward error in exact arithmetic, at every size edge.

Three factorisation families -- k_mniw_solve_mfma<NT> (option 6 = 0, the default), k_mniw_solve<MT> (= 1), k_mniw_solve_wide (= 2, M > 62
or nv > 1) -- and the stored-factor solves k_mniw_trisolve / k_mniw_trisolve_wide.  The judges and the input families are those of
tests/mniw_cases.py (tests/test_mniw_cases.py shows on the CPU that each of them can fail): the device's own packed factor must satisfy
    | B_ij - sum_k L_ik L_jk | <= 4.0 (j + 2) u sum_k |L_ik L_jk|
whatever the condition number, the returned scalars must be the sums over that factor's own rows to 2.0 (M + 2) u sum |terms|, and the
failure flag behind ops.check() must see every matrix that is not positive definite, and nothing else.

Every launch is tiny (n = 13: particle p carries family p % 6, so the last workgroup is partly filled for blocks of 4, 3 and 2 waves);
the time goes into the host judge, which looks at no more than 8 particles per case (2 above M = 62).  The worst ratio per kernel family is
printed when the module is done (pytest -s shows it)."""
import math

import numpy as np
import pytest
import torch

import mniw_cases as mc
from common import pgas_amd  # noqa: F401

pytestmark = pytest.mark.gpu

KERNEL = {0: "k_mniw_solve_mfma", 1: "k_mniw_solve", 2: "k_mniw_solve_wide"}
F = len(mc.FAMILIES)
N_LAUNCH = 2 * F + 1
JUDGED = (0, 1, 2, 3, 4, 5, 7, 12)        # every family once, one from the second round, the lone particle of the last workgroup
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from pgas_amd._lib import MarginalOps

    o = MarginalOps(64)
    o.check()
    yield o
    o.eng.set_option(6, 0)
    for key in sorted(WORST):
        print("mniw edges: worst %-22s %-17s %.3f" % (key + (WORST[key],)))


def _note(kernel, what, ratio):
    WORST[(kernel, what)] = max(WORST.get((kernel, what), 0.0), float(ratio))


def _dev(a, ops):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=ops.device)


def _solve(ops, knob, mats, want=("m", "c", "q", "logdet"), keep_factor=True):
    """The exact-input form: P1 = 0, P0 = 0, scale = 1.0, T1[p] = eta1_p, T0[p] = eta0_p, so that what the kernel factorises is the input
    itself, whether or not the compiler contracts P1 + scale T1 into an FMA.  mats: list of (eta1, phi, eta0) -> dict of NumPy arrays."""
    T1 = np.stack([m[0] for m in mats])
    phi = np.stack([m[1] for m in mats])
    T0 = np.stack([m[2] for m in mats])
    M = T1.shape[1]
    P1, P0 = np.zeros((M, M)), np.zeros(T0.shape[1:])
    ops.eng.set_option(6, knob)
    try:
        out = ops.mniw_solve(_dev(P0, ops), _dev(P1, ops), _dev(T0, ops), _dev(T1, ops), scale=1.0, phi=_dev(phi, ops), want=want, keep_factor=keep_factor)
    finally:
        ops.eng.set_option(6, 0)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _launch_mats(M, nv=1, n=N_LAUNCH):
    return [mc.family(mc.FAMILIES[p % F], M, p // F, nv) for p in range(n)]


def _judge(kernel, mats, out, M, judged, nv=1, forward=False):
    for p in judged:
        eta1, phi, eta0 = mats[p]
        r = mc.backward_ratio(mc.augmented(eta1, phi, eta0), out["L"][p], M, nv)
        s = mc.scalar_ratios(out["L"][p], out["c"][p], out["m"][p], out["q"][p], out["logdet"][p], M, nv)
        _note(kernel, "backward" if M >= 13 else "backward, M < 13", r)      # small M: one or two panels, the families do the same operations
        _note(kernel, "scalars", max(s.values()))
        assert r <= mc.BACKWARD_LIMIT, (kernel, M, p, mc.FAMILIES[p % F], r)
        assert max(s.values()) <= mc.SCALAR_LIMIT, (kernel, M, p, mc.FAMILIES[p % F], s)
        if forward:
            fe, kappa = mc.forward_errors(eta1, phi, eta0, out["c"][p], out["m"][p], out["q"][p], out["logdet"][p])
            if kappa <= mc.FORWARD_MAX_KAPPA:
                _note(kernel, "forward", max(fe.values()))
                assert max(fe.values()) <= mc.FORWARD_LIMIT, (kernel, M, p, mc.FAMILIES[p % F], fe, kappa)
    for k in ("m", "c", "q", "logdet"):
        assert np.all(np.isfinite(out[k])), k


PANEL = (1, 2, 3, 4, 5)                                                      # positions inside a panel of four columns
TILES = (13, 14, 15, 16, 17, 29, 30, 31, 32, 45, 46, 47, 48, 61, 62)         # MFMA tile counts; rows M, M + 1 in different tiles at 15, 31, 47
MT_EDGES = (22, 23, 42, 43)                                                  # the remaining instance boundaries of k_mniw_solve<MT>
# the forward check is calibrated at these sizes only: below them kappa_s is ~ 1 and its unit, (M + 2) u kappa_s, is smaller than the
# two or three roundings that forming c = v.v from a correctly rounded v costs
FORWARD_SIZES = (15, 41, 62)


@pytest.mark.parametrize("knob", [0, 1])
@pytest.mark.parametrize("M", PANEL + TILES + MT_EDGES)
def test_backward_error_narrow(ops, M, knob):
    mats = _launch_mats(M)
    out = _solve(ops, knob, mats)
    ops.check()
    _judge(KERNEL[knob], mats, out, M, JUDGED, forward=M in FORWARD_SIZES)


def _general_case(ops, knob, M, nv=1, n=N_LAUNCH):
    """scale = 0.999, a gathering anc, R0 / R1: B is formed exactly on the host; the bound gains 2 u (|P| + |scale T| + |R|)."""
    rng = np.random.default_rng([M, nv, 99])
    mats = _launch_mats(M, nv, n)
    T1, T0 = np.stack([m[0] for m in mats]), np.stack([m[2] for m in mats])
    phi = np.stack([m[1] for m in mats])
    anc = (5 * np.arange(n) + 3) % n
    anc[1] = anc[0]                                           # two children of one parent
    P1 = 1e-3 * np.diag(rng.uniform(0.5, 1.5, M))
    G = rng.standard_normal((M, M))
    R1 = 1e-3 / M * mc.sym(G @ G.T)
    P0, R0 = rng.standard_normal(T0.shape[1:]), rng.standard_normal(T0.shape[1:])
    ops.eng.set_option(6, knob)
    try:
        out = ops.mniw_solve(_dev(P0, ops), _dev(P1, ops), _dev(T0, ops), _dev(T1, ops), scale=0.999, anc=torch.as_tensor(anc, device=ops.device),
                             R0=_dev(R0, ops), R1=_dev(R1, ops), phi=_dev(phi, ops), keep_factor=True)
    finally:
        ops.eng.set_option(6, 0)
    ops.check()
    out = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    return out, [(P1, P0, 0.999, T1[anc[p]], T0[anc[p]], phi[p], R1, R0) for p in range(n)]


@pytest.mark.parametrize("knob", [0, 1, 2])
@pytest.mark.parametrize("M", [15, 41, 62])
def test_backward_error_general_form(ops, M, knob):
    out, parts = _general_case(ops, knob, M)
    for p in JUDGED:
        B, slack = mc.augmented_affine(*parts[p])
        r = mc.backward_ratio(B, out["L"][p], M, slack=slack)
        s = mc.scalar_ratios(out["L"][p], out["c"][p], out["m"][p], out["q"][p], out["logdet"][p], M)
        _note(KERNEL[knob], "general", r)
        _note(KERNEL[knob], "scalars", max(s.values()))
        assert r <= mc.BACKWARD_LIMIT and max(s.values()) <= mc.SCALAR_LIMIT, (knob, M, p, r, s)


@pytest.mark.parametrize("M,knob", [(15, 2), (47, 2), (62, 2), (63, 0), (64, 0), (65, 0), (126, 0)])
def test_backward_error_wide(ops, M, knob):
    """k_mniw_solve_wide through the test knob at M <= 62 and natively above (two rows per lane from M + 2 > 64 on)."""
    mats = _launch_mats(M)
    out = _solve(ops, knob, mats)
    ops.check()
    judged = JUDGED if M <= 62 else ((M % F), (M + 3) % F)
    _judge(KERNEL[2], mats, out, M, judged, forward=M in FORWARD_SIZES)


@pytest.mark.parametrize("M,nv", [(125, 2), (119, 8), (6, 2), (6, 8)])
def test_backward_error_several_components(ops, M, nv):
    """nv > 1 at the row limit M + 1 + nv = 128 and at a small M; Q symmetric bit for bit."""
    mats = _launch_mats(M, nv, n=F + 1)
    out = _solve(ops, 0, mats)
    ops.check()
    assert out["m"].shape == (F + 1, nv) and out["q"].shape == (F + 1, nv, nv) and out["L"].shape == (F + 1, mc.tri(M + 1 + nv))
    assert np.array_equal(out["q"], out["q"].transpose(0, 2, 1))
    _judge(KERNEL[2], mats, out, M, (1, 3) if M > 62 else range(F + 1), nv)
    if M <= 62:
        gen, parts = _general_case(ops, 0, M, nv, n=F + 1)
        for p in range(F + 1):
            B, slack = mc.augmented_affine(*parts[p])
            r = mc.backward_ratio(B, gen["L"][p], M, nv, slack=slack)
            _note(KERNEL[2], "general", r)
            assert r <= mc.BACKWARD_LIMIT, (M, nv, p, r)
            assert max(mc.scalar_ratios(gen["L"][p], gen["c"][p], gen["m"][p], gen["q"][p], gen["logdet"][p], M, nv).values()) <= mc.SCALAR_LIMIT


@pytest.mark.parametrize("knob", [0, 1, 2])
def test_pivot_sweep(ops, knob):
    """M = 1: rsqrt_newton alone through the public entry point, 4096 pivots over 2^-600 ... 2^600.  The backward ratio is |d^2 a - 1| / 2u:
    1 for a correctly rounded 1 / sqrt(a), 128 with one Newton step too few."""
    a, phi, eta0 = mc.pivot_sweep()
    out = _solve(ops, knob, [(a.reshape(-1, 1, 1)[i], phi[i:i + 1], eta0[i:i + 1]) for i in range(a.size)])
    ops.check()
    assert out["L"].shape == (a.size, 6)
    worst = 0.0
    for i in range(a.size):
        r = mc.backward_ratio(np.array([[a[i]], [phi[i]], [eta0[i]]]), out["L"][i], 1)
        s = mc.scalar_ratios(out["L"][i], out["c"][i], out["m"][i], out["q"][i], out["logdet"][i], 1)
        worst = max(worst, r)
        _note(KERNEL[knob], "scalars", max(s.values()))
        assert r <= mc.BACKWARD_LIMIT, (knob, i, float(a[i]).hex(), r)
        assert max(s.values()) <= mc.SCALAR_LIMIT, (knob, i, float(a[i]).hex(), s)
    _note(KERNEL[knob], "pivot", worst)


ILL = ("graded", "graded_rev", "near_singular", "scaled_up", "scaled_down")


def _non_corner(M, nv=1):
    keep = np.zeros(mc.tri(M + 1 + nv), bool)
    for r in range(M + 1 + nv):
        keep[mc.tri(r):mc.tri(r) + min(r + 1, M)] = True
    return keep


@pytest.mark.parametrize("M", [15, 31, 47, 62])
def test_wide_equals_row_per_lane_on_ill_conditioned_inputs(ops, M):
    """Option 6 = 1 against = 2: the same operations in the same order, so the same bits -- also where rounding errors are amplified 1e12-fold."""
    mats = [mc.family(ILL[p % len(ILL)], M, 10 + p) for p in range(11)]
    a, b = _solve(ops, 1, mats), _solve(ops, 2, mats)
    ops.check()
    for k in ("m", "c", "q", "logdet"):
        assert np.array_equal(a[k], b[k]), k
    keep = _non_corner(M)
    assert np.array_equal(a["L"][:, keep], b["L"][:, keep])


@pytest.mark.parametrize("M,knob", [(15, 0), (15, 1), (15, 2), (62, 0), (62, 1), (62, 2), (65, 0)])
def test_outputs_do_not_depend_on_what_else_is_asked_or_launched(ops, M, knob):
    """keep_factor or not, any subset of `want`, another particle index, another launch size (n = 1, 2, 3, 5: other waves, other workgroups):
    the same bits for the same matrix."""
    mats = [mc.family(ILL[p % len(ILL)], M, 20 + p) for p in range(7)]
    full = _solve(ops, knob, mats)
    bare = _solve(ops, knob, mats, keep_factor=False)
    assert "L" not in bare
    for k in ("m", "c", "q", "logdet"):
        assert np.array_equal(full[k], bare[k]), k
    for want in (("m",), ("c", "logdet"), ("q",), ("logdet",), ("q", "m")):
        for keep in (False, True):
            part = _solve(ops, knob, mats, want=want, keep_factor=keep)
            assert set(part) == set(want) | ({"L"} if keep else set())
            for k in want:
                assert np.array_equal(full[k], part[k]), (want, k)
            if keep:
                assert np.array_equal(full["L"][:, _non_corner(M)], part["L"][:, _non_corner(M)])
    keep = _non_corner(M)
    for n in (1, 2, 3, 5):
        for at in range(n):
            sub = [mats[(at + 1 + i) % 7] for i in range(n)]
            sub[at] = mats[6]
            one = _solve(ops, knob, sub)
            for k in ("m", "c", "q", "logdet"):
                assert one[k][at] == full[k][6], (n, at, k)
            assert np.array_equal(one["L"][at][keep], full["L"][6][keep]), (n, at)
    ops.check()


@pytest.mark.parametrize("M,nv,knob", [(1, 1, 0), (15, 1, 0), (61, 1, 1), (62, 1, 0), (63, 1, 0), (126, 1, 0), (20, 2, 0), (15, 1, 2)])
def test_stored_factor_solves(ops, M, nv, knob):
    """mniw_trisolve on `graded` and `near_singular` factors through a gathering anc, against a 512-bit substitution that takes the DEVICE's
    packed factor as exact input; tolerance = the first-order bound of Higham Thm 8.5 (mniw_cases.trisolve_bounds).  M = 62 asks
    k_mniw_trisolve for 4 x 2080 doubles = 66 560 bytes of dynamic LDS without a size attribute on the function (the wide path sets one):
    that launch is covered here."""
    n = 6
    mats = [mc.family(("graded", "near_singular")[p % 2], M, 30 + p, nv) for p in range(n)]
    T1, phi, T0 = (np.stack([m[i] for m in mats]) for i in (0, 1, 2))
    anc = np.array([3, 0, 5, 1, 1, 2])
    phi2 = np.random.default_rng([M, nv, 5]).standard_normal((n, M))
    ops.eng.set_option(6, knob)
    try:
        fac = ops.mniw_solve(_dev(np.zeros(T0.shape[1:]), ops), _dev(np.zeros((M, M)), ops), _dev(T0, ops), _dev(T1, ops), scale=1.0, phi=_dev(phi, ops),
                             keep_factor=True)
        tri = ops.mniw_trisolve(fac, torch.as_tensor(anc, device=ops.device), _dev(phi2, ops))
        same = ops.mniw_trisolve(fac, None, _dev(phi, ops))
    finally:
        ops.eng.set_option(6, 0)
    ops.check()
    L = fac["L"].cpu().numpy()
    kern = "k_mniw_trisolve_wide" if (M > 62 or nv > 1 or knob == 2) else "k_mniw_trisolve"
    for got, rhs, src in ((tri, phi2, anc), (same, phi, np.arange(n))):
        gc, gm = got["c"].cpu().numpy(), got["m"].cpu().numpy().reshape(n, nv)
        for p in (range(n) if M <= 62 else (0, 1)):
            c, m, v = mc.reference_trisolve(L[src[p]], rhs[p], M, nv)
            dc, dm = mc.trisolve_bounds(L[src[p]], v, M, nv)
            _note(kern, "c / bound", abs(gc[p] - c) / dc)
            _note(kern, "m / bound", np.max(np.abs(gm[p] - m) / dm))
            assert abs(gc[p] - c) <= dc, (M, p, gc[p], c, dc)
            assert np.all(np.abs(gm[p] - m) <= dm), (M, p, gm[p], m, dm)


BAD_K = (0, 3, 4, 15, 16, 32)          # panel start, panel interior, tile boundary on both sides, the last pivot (M = 33)


@pytest.mark.parametrize("knob", [0, 1, 2])
@pytest.mark.parametrize("kind", ["zero", "minus", "coupled", "nonfinite"])
def test_failure_detection(ops, kind, knob):
    """Three matrices that are not positive definite among six of the `graded` family: check() names exactly three, a second check() passes,
    the good particles' outputs are those of a launch without the bad ones bit for bit, the bad ones' logdet is not finite.  The failing
    pivot is exact whatever the rounding before it (mniw_cases.bad_matrix): an exact zero (v_rsq gives inf, the Newton step turns it into
    NaN), a decoupled -1, a coupled 1/4 - 1, a NaN or +inf in the lower triangle."""
    from pgas_amd._lib import PgasError

    M = 33
    good = [mc.family("graded", M, 40 + p) for p in range(6)]
    clean = _solve(ops, knob, good)
    ops.check()
    at = (1, 4, 8)                     # 1, 4: between good neighbours of their workgroup; 8: alone in the last one (blocks of 4 and 2 waves)
    if kind == "nonfinite":
        rounds = [(("nan", 3), ("inf", 16), ("nan", 32)), (("inf", 0), ("nan", 15), ("inf", 32))]
    else:
        rounds = [tuple((kind, k) for k in BAD_K[:3]), tuple((kind, k) for k in BAD_K[3:])]
    for bads in rounds:
        mats, it = [], iter(good)
        for p in range(9):
            if p in at:
                kd, k = bads[at.index(p)]
                mats.append((mc.bad_matrix(kd, M, k, seed=p),) + good[0][1:])
            else:
                mats.append(next(it))
        out = _solve(ops, knob, mats)
        with pytest.raises(PgasError, match=r"\b3 matrices"):
            ops.check()
        ops.check()                    # the counter is cleared by the failed check
        ok = [p for p in range(9) if p not in at]
        for k in ("m", "c", "q", "logdet"):
            assert np.array_equal(out[k][ok], clean[k]), (bads, k)
            assert np.all(np.isfinite(out[k][ok]))
        assert np.array_equal(out["L"][ok][:, _non_corner(M)], clean["L"][:, _non_corner(M)]), bads
        assert not np.any(np.isfinite(out["logdet"][list(at)])), (bads, out["logdet"][list(at)])


def test_failure_detection_wide_native(ops):
    """The same through k_mniw_solve_wide at M = 70 (pivots held by the second row of a lane: k >= 64) and at the last pivot."""
    from pgas_amd._lib import PgasError

    M = 70
    good = [mc.family("graded", M, 50 + p) for p in range(2)]
    clean = _solve(ops, 0, good)
    ops.check()
    mats = [good[0], (mc.bad_matrix("zero", M, 64),) + good[0][1:], (mc.bad_matrix("coupled", M, 69),) + good[0][1:], good[1],
            (mc.bad_matrix("minus", M, 63),) + good[0][1:]]
    out = _solve(ops, 0, mats)
    with pytest.raises(PgasError, match=r"\b3 matrices"):
        ops.check()
    ops.check()
    for k in ("m", "c", "q", "logdet"):
        assert np.array_equal(out[k][[0, 3]], clean[k]), k
    assert not np.any(np.isfinite(out["logdet"][[1, 2, 4]]))
    assert math.isfinite(float(clean["logdet"].sum()))
