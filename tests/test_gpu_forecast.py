"""h-step-ahead forecasts from the held-out filter's trace, every origin row of every draw in one launch (pgas_amd.HeldOutFilter.forecast,
pgas_forecast, csrc/pgas_forecast.hip.h) against the NumPy restatement of the definition from the canonical oracle's primitives
(tests/forecast_numpy.py), which tests/test_forecast_host.py pins to plain float arithmetic.  Every comparison against the restatement is
np.array_equal.  Independent of the restatement: horizon 1 against k_filter's own outputs, and a linear-Gaussian model whose h-step-ahead
log score is known in closed form."""
import functools

import numpy as np
import pytest
import torch

import filter_numpy as fn
import forecast_numpy as fc
from common import canon_model, experiments, pgas_amd
from pgas_amd import chains as ch
from pgas_amd import random as prng
from pgas_amd._lib import PgasError, load
from test_forecast_host import KEYS, closed_form_keys, closed_form_z, linear_gaussian_case
from test_gpu_rollout import MODELS, _draws, _np, _problem

pytestmark = pytest.mark.gpu

K, H = 3, 4
NS = [1, 2, 255, 256, 257, 512, 513, 1024]   # every NR (1, 2, 4 register rows) and both sides of each row boundary
OUT = ("sum", "sumsq", "lpd")


def _y(pb):
    return np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1)


def _with_obs(pb, y):
    return type(pb)(**{**pb.__dict__, "observations": y})


def _filter_for(pb, N, obs=None):
    return pgas_amd.HeldOutFilter(pb.observations if obs is None else obs, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, pb.nx, N,
                                  pb.init_state_mean, pb.init_state_cov)


def _restate_filter(pb, N, keys, As, Ss, y=None):
    y = _y(pb) if y is None else y
    cm1 = canon_model(_with_obs(pb, y), N + 1)
    L0 = np.linalg.cholesky(pb.init_state_cov)
    return [fn.run(cm1, N, keys[k], As[k], Ss[k], pb.init_state_mean, L0, pb.likelihood_fcn, y) for k in range(len(keys))]


def _restate(pb, N, keys, As, Ss, x, Hn, y=None, score=True):
    """The restatement of every draw from the trace x (K, T, N, nx), stacked: dict of (K, H, ...) arrays."""
    y = _y(pb) if y is None else y
    cm1 = canon_model(_with_obs(pb, y), N + 1)
    rs_ = [fc.run(cm1, N, keys[k], As[k], Ss[k], pb.likelihood_fcn, y, x[k], Hn, score) for k in range(len(keys))]
    return {f: np.stack([r[f] for r in rs_]) for f in (OUT if score else OUT[:2])}


def _assert_equal(res, want, what):
    for f in want:
        got = _np(getattr(res, f))
        assert got.shape == want[f].shape, f"{what}: {f} shape {got.shape} != {want[f].shape}"
        assert np.array_equal(got, want[f], equal_nan=True), f"{what}: {f}"


def _assert_undefined_are_nan(res, Hn):
    for f in OUT:
        got = _np(getattr(res, f))
        for h in range(Hn):
            assert np.isnan(got[:, h, :h]).all() and not np.isnan(got[:, h, h:]).any(), (f, h)


@functools.lru_cache(maxsize=None)
def _device(name, N):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    return _filter_for(pb, N).forecast(As, Ss, keys, H)


# ---- 1. the restated definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", MODELS)
def test_forecast_equals_the_restated_definition(name, N):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    drawn = _device(name, N)
    nv = pb.nx + _y(pb).shape[1]
    assert drawn.horizon == H and tuple(drawn.sum.shape) == (K, H, pb.T, nv) and tuple(drawn.lpd.shape) == (K, H, pb.T)
    x = _np(drawn.filter.x)
    flt = _restate_filter(pb, N, keys, As, Ss)
    assert np.array_equal(x, np.stack([r["x"] for r in flt])), "the device's trace is not the filter restatement's"
    want = _restate(pb, N, keys, As, Ss, x, H)
    _assert_equal(drawn, want, "drawn x_0")
    _assert_undefined_are_nan(drawn, H)
    given = _filter_for(pb, N).forecast(As, Ss, keys, H, init_state=x[:, 0].copy())
    _assert_equal(given, want, "given x_0 (K, N, nx)")
    assert not np.array_equal(want["lpd"][0], want["lpd"][1])


# ---- 2. horizon 1 against k_filter, independent of the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", MODELS)
def test_horizon_one_is_the_filters_own_prediction(name, N):
    res = _device(name, N)
    assert torch.equal(res.sum[:, 0], res.filter.pred_sum) and torch.equal(res.sumsq[:, 0], res.filter.pred_sumsq)
    ell = _np(res.filter.ell)
    assert np.isfinite(ell).all()
    assert np.abs(_np(res.lpd)[:, 0] - ell).max() <= 1e-12


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 300])
def test_a_record_of_one_row(N):
    pb = experiments.smo_pgas(T=1)
    keys, As, Ss = _draws(_problem("smo"), K)
    res = _filter_for(pb, N).forecast(As, Ss, keys, 1)
    _assert_equal(res, _restate(pb, N, keys, As, Ss, _np(res.filter.x), 1), "T = 1, H = 1")
    assert torch.equal(res.sum[:, 0], res.filter.pred_sum) and not bool(torch.isnan(res.lpd).any())


def test_horizon_one_propagates_nothing_and_horizon_T_reaches_one_row():
    pb = experiments.smo_pgas(T=6)
    keys, As, Ss = _draws(_problem("smo"), K)
    N, T = 257, 6
    flt = _filter_for(pb, N)
    one = flt.forecast(As, Ss, keys, 1)
    assert torch.equal(one.sum[:, 0], one.filter.pred_sum) and torch.equal(one.sumsq[:, 0], one.filter.pred_sumsq)
    _assert_equal(one, _restate(pb, N, keys, As, Ss, _np(one.filter.x), 1), "H = 1")
    full = flt.forecast(As, Ss, keys, T)
    _assert_equal(full, _restate(pb, N, keys, As, Ss, _np(full.filter.x), T), "H = T")
    _assert_undefined_are_nan(full, T)
    last = _np(full.lpd)[:, T - 1]
    assert np.isnan(last[:, :T - 1]).all() and np.isfinite(last[:, T - 1]).all()
    assert torch.equal(full.sum[:, :1], one.sum) and torch.equal(full.lpd[:, :1], one.lpd)


def test_record_lengths_around_the_origins_per_workgroup():
    TB = int(load().pgas_forecast_origins_per_block())
    assert TB >= 2
    keys, As, Ss = _draws(_problem("smo"), K)
    N = 70
    for T in (TB - 1, TB + 1, 2 * TB + 3):   # below TB (one ragged chunk), exactly one row into the second chunk, ragged third chunk
        pb = experiments.smo_pgas(T=T)
        Hn = min(H, T)
        res = _filter_for(pb, N).forecast(As, Ss, keys, Hn)
        _assert_equal(res, _restate(pb, N, keys, As, Ss, _np(res.filter.x), Hn), f"T = {T}")
        _assert_undefined_are_nan(res, Hn)


@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_nan_row_and_outlier_row(name):
    pb = _problem(name)
    N = 257
    keys, As, Ss = _draws(pb, K)
    y = _y(pb).copy()
    y[7, -1] = np.nan      # one component of one row
    y[12] = 1e200          # the quadratic form overflows: every l_i is -inf
    res = _filter_for(pb, N, obs=y).forecast(As, Ss, keys, H)
    x = _np(res.filter.x)
    assert np.array_equal(x, np.stack([r["x"] for r in _restate_filter(pb, N, keys, As, Ss, y=y)]))
    want = _restate(pb, N, keys, As, Ss, x, H, y=y)
    lpd = _np(res.lpd)
    assert np.isnan(lpd[:, :, 7]).all() and (lpd[:, :, 12] == -np.inf).all()
    for h in range(H):
        rest = np.setdiff1d(np.arange(h, pb.T), [7, 12])
        assert np.isfinite(lpd[:, h, rest]).all()
        assert np.isfinite(_np(res.sum)[:, h, h:]).all() and np.isfinite(_np(res.sumsq)[:, h, h:]).all()
    _assert_equal(res, want, "NaN and outlier rows")   # the sums of those rows and the later targets included


# ---- 4. addressing ------------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_number_of_horizons():
    pb = _problem("veh27")
    N = 300
    keys, As, Ss = _draws(pb, K)
    flt = _filter_for(pb, N)
    four, two = flt.forecast(As, Ss, keys, 4), flt.forecast(As, Ss, keys, 2)
    for f in OUT:
        a, b = _np(getattr(four, f)), _np(getattr(two, f))
        assert b.shape[1] == 2 and np.array_equal(a[:, :2], b, equal_nan=True), f
    assert not np.array_equal(_np(four.sum)[:, 1, 5], _np(four.sum)[:, 2, 5])


def test_more_draws_than_the_gpu_holds_at_once_in_chunks_and_reversed():
    Kb, N, T, Hn = 2000, 64, 8, 3
    pb = experiments.smo_pgas(T=T)
    keys, As, Ss = _draws(pb, Kb)
    As = np.stack([As[0] * (1.0 + 1e-4 * k) for k in range(Kb)])
    Ss = np.stack([Ss[0] * (1.0 + 1e-3 * k) for k in range(Kb)])
    flt = _filter_for(pb, N)
    whole = flt.forecast(As, Ss, keys, Hn)
    got = {f: _np(getattr(whole, f)) for f in OUT}
    assert np.isfinite(got["lpd"][:, 0]).all()
    for lo in range(0, Kb, 700):    # chunks of 700, 700, 600
        part = flt.forecast(As[lo:lo + 700], Ss[lo:lo + 700], keys[lo:lo + 700], Hn)
        for f in got:
            assert np.array_equal(_np(getattr(part, f)), got[f][lo:lo + 700], equal_nan=True), f"chunk at {lo}: {f}"
    rev = flt.forecast(As[::-1].copy(), Ss[::-1].copy(), keys[::-1], Hn)
    for f in got:
        assert np.array_equal(_np(getattr(rev, f))[::-1], got[f], equal_nan=True), f"reversed: {f}"
    want = _restate(pb, N, keys[-2:], As[-2:], Ss[-2:], _np(whole.filter.x)[-2:], Hn)
    for f in got:
        assert np.array_equal(got[f][-2:], want[f], equal_nan=True), f"last draws: {f}"


def test_equal_draws_give_equal_outputs_and_the_log_score_changes_nothing_else():
    pb = _problem("veh27")
    N = 300
    keys, As, Ss = _draws(pb, K)
    flt = _filter_for(pb, N)
    full = flt.forecast(As, Ss, keys, H)
    idx = [0, 2, 0, 2, 1]
    dup = flt.forecast(As[idx], Ss[idx], [keys[i] for i in idx], H)
    for f in OUT:
        d, g = _np(getattr(dup, f)), _np(getattr(full, f))
        assert np.array_equal(d[0], d[2], equal_nan=True) and np.array_equal(d[1], d[3], equal_nan=True) and np.array_equal(d, g[idx], equal_nan=True), f
    assert not np.array_equal(_np(dup.lpd)[0], _np(dup.lpd)[1], equal_nan=True)
    bare = flt.forecast(As, Ss, keys, H, log_score=False)
    assert bare.lpd is None
    assert torch.equal(bare.sum.view(torch.int64), full.sum.view(torch.int64)) and torch.equal(bare.sumsq.view(torch.int64), full.sumsq.view(torch.int64))
    assert torch.equal(bare.filter.ell, full.filter.ell) and torch.equal(bare.filter.x, full.filter.x)


# ---- 5. host contract ---------------------------------------------------------------------------------------------------------------------
def test_forecast_calls_make_no_host_round_trip():
    pb = experiments.smo_pgas(T=16)
    Kc, N = 4, 300
    keys, As, Ss = _draws(pb, Kc)
    flt = _filter_for(pb, N)
    dev = flt.engine.device
    kd = ch.keys_tensor(keys, dev)
    Ad, Sd = torch.as_tensor(As, device=dev), torch.as_tensor(Ss, device=dev)
    x0 = torch.as_tensor(np.repeat(pb.X_true[:1], Kc, axis=0), device=dev)
    calls = [lambda: flt.forecast(Ad, Sd, kd, H), lambda: flt.forecast(Ad, Sd, kd, 2, init_state=x0), lambda: flt.forecast(Ad, Sd, kd, H, log_score=False)]
    warm = [c() for c in calls]   # allocations may synchronise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a.sum.view(torch.int64), b.sum.view(torch.int64)) and torch.equal(a.filter.ell, b.filter.ell)
        assert bool(torch.isfinite(a.sum[:, 0]).all())
    summary = pgas_amd.forecast_summary(outs[0], y=pb.observations)
    assert summary["rmse"].shape == (H,) and bool(torch.isfinite(summary["rmse"]).all()) and bool(torch.isfinite(summary["log_score"]).all())


def test_in_sample_forecast_leaves_single_chain_and_chains_state_as_it_was():
    pb = _problem("smo")
    Cn, N = 3, 200
    keys, As, Ss = _draws(pb, Cn)
    refs = np.stack([pb.X_true * (1.0 + 0.01 * c) for c in range(Cn)])
    chs = ch.condSequentialMonteCarloChains(Cn, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    eng, dev = chs.engine, chs.device
    Sd = torch.as_tensor(Ss[1], device=dev)

    def sweeps(set_params):
        if set_params:
            t1 = chs.single(4242, pb.X_true, As[1], Sd).clone()
            tc = chs(keys, refs, As, Ss).clone()
        else:   # the parameters packed before the forecast call must still be there
            t1 = eng.sweep(prng.as_key(4242), torch.as_tensor(pb.X_true, device=dev)).clone()
            tc = eng.chains_sweep(ch.keys_tensor(keys, dev), torch.as_tensor(refs, device=dev)).clone()
        single = [t.clone() for t in eng.traces()[:3]]
        return [t1, tc] + single + [t.clone() for t in chs.traces()]

    before = sweeps(True)
    views = list(eng.traces()[:3]) + list(chs.traces())
    fk, fA, fS = _draws(pb, 4)
    fkeys = [k + 5 for k in fk]
    res = chs.forecast(fA * 1.01, fS * 2.0, fkeys, H)
    one = chs.single.forecast(fA * 1.01, fS * 2.0, fkeys, H)
    want = _restate(pb, N, fkeys, fA * 1.01, fS * 2.0, _np(res.filter.x), H)
    _assert_equal(res, want, "chains context")
    _assert_equal(one, want, "single-chain context")
    for a, b in zip(before[2:], views):
        assert torch.equal(a, b), "a forecast call wrote into a trace buffer"
    for a, b in zip(before, sweeps(False)):
        assert torch.equal(a, b), "sweeps after a forecast call (parameters not set again) differ"
    for a, b in zip(before, sweeps(True)):
        assert torch.equal(a, b)


def test_refusals_are_clean_and_leave_the_context_usable():
    pb = experiments.smo_pgas(T=16)
    Kc, N, T = 2, 40, 16
    keys, As, Ss = _draws(pb, Kc)
    flt = _filter_for(pb, N)
    eng = flt.engine
    good = flt.forecast(As, Ss, keys, H)
    Ad, Sd, kd = torch.as_tensor(As, device=eng.device), torch.as_tensor(Ss, device=eng.device), ch.keys_tensor(keys, eng.device)
    xd = good.filter.x
    f = lambda *s: torch.empty(s, dtype=torch.float64, device=eng.device)  # noqa: E731
    s1, s2, lp = f(Kc, H, T, 3), f(Kc, H, T, 3), f(Kc, H, T)
    PGAS_E_ARG = -1

    def call(Kn=Kc, Hn=H, seeds=kd, S=Sd, x=xd, a=s1, b=s2, lpd=lp):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = eng.lib.pgas_forecast(eng._h, Kn, Hn, p(seeds), Ad.data_ptr(), p(S), p(x), p(a), p(b), p(lpd), eng._stream())
        return rc, eng.lib.pgas_last_error(eng._h).decode()

    for kw, msg in [(dict(Kn=0), "K = 0"), (dict(Hn=0), "H = 0"), (dict(Hn=-3), "H = -3"), (dict(Hn=T + 1), f"H = {T + 1}"), (dict(x=None), "NULL"),
                    (dict(a=None), "NULL"), (dict(b=None), "NULL"), (dict(seeds=None), "seeds and S"), (dict(S=None), "seeds and S")]:
        rc, err = call(**kw)
        assert rc == PGAS_E_ARG and "pgas_forecast" in err and msg in err, (kw, rc, err)
        again = flt.forecast(As, Ss, keys, H)
        assert torch.equal(again.lpd.view(torch.int64), good.lpd.view(torch.int64)), f"forecast after refusing {kw}"
    rc, _ = call(lpd=None)
    assert rc == 0
    with pytest.raises(PgasError, match="seeds and S"):
        eng.forecast(Ad, None, kd, xd, H)
    with pytest.raises(PgasError, match="H = 17"):
        eng.forecast(Ad, Sd, kd, xd, T + 1)
    # a context of more than one segment of particles has no one-workgroup variant
    big = pgas_amd.condSequentialMonteCarlo(5000, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    with pytest.raises(PgasError, match="no one-workgroup variant"):
        big.engine.forecast(Ad, Sd, kd, torch.zeros((Kc, T, 5000, pb.nx), dtype=torch.float64, device=eng.device), H)
    with pytest.raises(ValueError, match="particles"):
        big.forecast(As, Ss, keys, H)
    traj = big(77, pb.X_true, As[0], Sd[0])
    assert bool(torch.isfinite(traj).all())


# ---- 6. analytic check, independent of the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smo", "toy", "veh27"])
def test_log_score_of_a_linear_gaussian_model_is_the_closed_form(name):
    """With A = 0 the h-step-ahead cloud (h >= 2) is iid N(0, S) whatever the filter did, so sum_{tau >= h - 1} lpd[k, h - 1, tau]
    estimates sum_{tau >= h - 1} log N(y_tau; 0, H S H^T + R).  For each h in {2, 3, 4} the mean over 16 keys must lie within 4 standard
    errors (std_k / sqrt(16)) of the closed form: test_evidence_of_a_linear_gaussian_model_is_the_closed_form's construction and bound.
    The engine equals its restatement bit for bit, so z is fixed by the keys; plain float64 arithmetic on the oracle's stream-7
    normals gives z = 3.07, 1.65, 0.52 (smo), -0.82, -1.40, -0.43 (toy), -1.52, 0.79, 0.80 (veh27)."""
    pb = _problem(name)
    S, y, analytic = linear_gaussian_case(pb)
    A = np.zeros((KEYS, pb.nx, pb.basis_fcn.basis.M))
    res = _filter_for(pb, 1024, obs=y).forecast(A, np.repeat(S[None], KEYS, axis=0), closed_form_keys(), H)
    z = closed_form_z(_np(res.lpd), analytic, name)
    assert (np.abs(z[2:]) <= 4.0).all()
    summary = pgas_amd.forecast_summary(res, y=y)
    assert bool(torch.isfinite(summary["log_score"]).all()) and bool(torch.isfinite(summary["rmse"]).all())
