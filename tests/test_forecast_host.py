"""Host side of the h-step-ahead forecast (pgas_amd/heldout.py), no GPU: the NumPy restatement of the definition
(tests/forecast_numpy.py) on the filter restatement's trace against that restatement's own one-step-ahead outputs and against a plain
float64 log predictive density, the shape checks of HeldOutFilter.forecast, forecast_summary on hand-made numbers, and the closed-form
statistic of tests/test_gpu_forecast.py evaluated on the restatement."""
import functools

import numpy as np
import pytest
import torch

import filter_numpy as fn
import forecast_numpy as fc
from common import canon, canon_model, experiments, pgas_amd
from pgas_amd import heldout
from pgas_amd import random as prng

H = 4


@functools.lru_cache(maxsize=None)
def _problem(name):
    return {"smo": lambda: experiments.smo_pgas(T=40), "toy": lambda: experiments.toy(T=40),
            "veh27": lambda: experiments.vehicle_pgas(T=30, M=27)}[name]()


def _y(pb):
    return np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1)


# ---- 0. the stream of the forecast's noise -----------------------------------------------------------------------------------------------
def test_forecast_noise_counters_are_distinct():
    key = prng.key(1000)
    a, b = fc.noise(key, 5, 1, 6, 2), fc.noise(key, 5, 2, 6, 2)
    prop = canon.normals(key, canon.STREAM_PROP, 5, 0, 6, 2)
    assert not np.array_equal(a, b) and not np.array_equal(a, prop) and not np.array_equal(fc.noise(key, 5, 0, 6, 2), prop)
    assert np.array_equal(fc.noise(key, 5, 1, 6, 2)[2:], canon.normals(key, fc.STREAM_FORECAST, 5, (1 << 32) + 2, 4, 2))   # particle = lead << 32 | i
    assert not np.array_equal(a, fc.noise(key, 6, 1, 6, 2))


# ---- 1. the restatement on the filter restatement's trace -------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 200, 257, 1024])
@pytest.mark.parametrize("name", ["smo", "toy"])
def test_restatement_on_the_filter_trace(name, N):
    pb = _problem(name)
    A, S = experiments.initial_params(pb)
    lik, y, T = pb.likelihood_fcn, _y(pb), pb.T
    cm1 = canon_model(pb, N + 1)
    key = prng.key(1000)
    flt = fn.run(cm1, N, key, A, S, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), lik, y)
    res = fc.run(cm1, N, key, A, S, lik, y, flt["x"], H)
    nv = pb.nx + y.shape[1]
    assert res["sum"].shape == (H, T, nv) and res["sumsq"].shape == (H, T, nv) and res["lpd"].shape == (H, T)
    # h = 1 is the filter's own predictive cloud: the same operation sequence
    assert np.array_equal(res["sum"][0], flt["pred_sum"]) and np.array_equal(res["sumsq"][0], flt["pred_sumsq"])
    assert np.isfinite(flt["ell"]).all()
    assert np.abs(res["lpd"][0] - flt["ell"]).max() <= 1e-12
    # every horizon against a plain float64 logsumexp - log N on the same clouds
    plain = fc.float_lpd(res["cloud"], lik, y)
    for h in range(H):
        assert np.isfinite(res["lpd"][h, h:]).all() and np.isfinite(res["sum"][h, h:]).all() and np.isfinite(res["sumsq"][h, h:]).all()
        assert np.abs(res["lpd"][h, h:] - plain[h, h:]).max() <= 1e-12
        # rows without an origin are NaN
        assert np.isnan(res["lpd"][h, :h]).all() and np.isnan(res["sum"][h, :h]).all() and np.isnan(res["sumsq"][h, :h]).all()
    # the moments are the plain sums of the clouds' channels
    v = np.concatenate([res["cloud"], res["cloud"] @ np.atleast_2d(lik.H).T], axis=-1)
    for h in range(H):
        assert np.allclose(res["sum"][h, h:], v[h, h:].sum(axis=1), rtol=1e-12, atol=1e-300)
        assert np.allclose(res["sumsq"][h, h:], (v[h, h:] ** 2).sum(axis=1), rtol=1e-12, atol=1e-300)
    if N >= 200:   # the clouds of different horizons for the same target row differ (the noise of each lead is its own)
        assert not np.array_equal(res["cloud"][1, 5], res["cloud"][2, 5])
    bare = fc.run(cm1, N, key, A, S, lik, y, flt["x"], 2, score=False)
    assert bare["lpd"] is None and np.array_equal(bare["sum"], res["sum"][:2], equal_nan=True)   # independent of H and of the score


def test_restatement_nan_row_and_outlier_row():
    pb = _problem("toy")
    N = 65
    A, S = experiments.initial_params(pb)
    lik = pb.likelihood_fcn
    y = _y(pb).copy()
    y[5] = np.nan
    y[9] = 1e200
    toy = experiments.toy(T=40)
    toy.observations = y
    cm1 = canon_model(toy, N + 1)
    flt = fn.run(cm1, N, prng.key(3), A, S, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), lik, y)
    res = fc.run(cm1, N, prng.key(3), A, S, lik, y, flt["x"], H)
    for h in range(H):
        assert np.isnan(res["lpd"][h, 5]) and res["lpd"][h, 9] == -np.inf
        rest = np.delete(np.arange(h, pb.T), [5 - h, 9 - h])
        assert np.isfinite(res["lpd"][h, rest]).all() and np.isfinite(res["sum"][h, h:]).all()


# ---- 2. every argument error is a ValueError before a device is touched --------------------------------------------------------------
def test_forecast_refusals_touch_no_device():
    pb = _problem("smo")
    flt = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, pb.nx, 32, init_state_mean=pb.init_state_mean,
                                 init_state_cov=pb.init_state_cov)
    nx, M, K, N, T = pb.nx, pb.basis_fcn.basis.M, 3, 32, pb.T
    A, S, keys = np.zeros((K, nx, M)), np.stack([np.eye(nx)] * K), [1, 2, 3]
    bad = [
        (dict(horizon=0), "horizon"),
        (dict(horizon=-1), "horizon"),
        (dict(horizon=T + 1), "horizon"),
        (dict(horizon=2.0), "horizon"),
        (dict(horizon=None), "horizon"),
        (dict(horizon=True), "horizon"),
        (dict(coeff_mat=np.zeros((nx, M))), "coeff_mat"),
        (dict(coeff_mat=np.zeros((K, nx, M + 1))), "coeff_mat"),
        (dict(coeff_mat=np.zeros((0, nx, M)), error_cov=np.zeros((0, nx, nx)), keys=[]), "K must be"),
        (dict(error_cov=None), "error_cov"),
        (dict(error_cov=np.zeros((K + 1, nx, nx))), "error_cov"),
        (dict(keys=None), "keys"),
        (dict(keys=[1, 2]), "keys"),
        (dict(keys=torch.zeros(K, dtype=torch.int32)), "keys"),
        (dict(init_state=np.zeros((K, N + 1, nx))), "init_state"),
        (dict(init_state=np.zeros(nx + 1)), "init_state"),
    ]
    for kw, match in bad:
        args = dict(coeff_mat=A, error_cov=S, keys=keys, horizon=H)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            flt.forecast(**args)
    assert flt._engine is None
    bare = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, pb.nx, 32)
    with pytest.raises(ValueError, match="init_state=None"):
        bare.forecast(A, S, keys, H)
    assert bare._engine is None
    assert heldout.check_forecast(nx, M, N, T, True, A, S, keys, 1) == (K, 0, 1)
    assert heldout.check_forecast(nx, M, N, T, True, A, S, keys, np.int64(T)) == (K, 0, T)
    assert heldout.check_forecast(nx, M, N, T, False, A, S, keys, 3, np.zeros((K, N, nx))) == (K, 3, 3)
    with pytest.raises(ValueError, match="particles"):
        heldout.check_forecast(nx, M, 2048, T, True, A, S, keys, H)


# ---- 3. forecast_summary on hand-made numbers -------------------------------------------------------------------------------------------
def test_forecast_summary_by_hand():
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    nan = float("nan")
    # K = 2 draws, n = 2 particles, H = 2, T = 3, nx = 1, ny = 1 (yhat = x).  Clouds at h = 1: {1, 3}, {5, 7} | {0, 0}, {2, 2} | {1, 1}, {1, 1};
    # at h = 2 (row 0 undefined): {0, 2}, {2, 4} | {3, 3}, {3, 3}
    s1 = t([[[[4.0, 4.0], [0.0, 0.0], [2.0, 2.0]], [[nan, nan], [2.0, 2.0], [6.0, 6.0]]],
            [[[12.0, 12.0], [4.0, 4.0], [2.0, 2.0]], [[nan, nan], [6.0, 6.0], [6.0, 6.0]]]])
    s2 = t([[[[10.0, 10.0], [0.0, 0.0], [2.0, 2.0]], [[nan, nan], [4.0, 4.0], [18.0, 18.0]]],
            [[[74.0, 74.0], [8.0, 8.0], [2.0, 2.0]], [[nan, nan], [20.0, 20.0], [18.0, 18.0]]]])
    lpd = t([[[np.log(0.2), np.log(0.1), nan], [nan, np.log(0.3), nan]],
             [[np.log(0.6), np.log(0.3), nan], [nan, np.log(0.5), nan]]])
    flt = heldout.FilterResult(2, 1, loglik=t([0.0, 0.0]), ell=lpd[:, 0])
    res = heldout.ForecastResult(flt, 2, s1, s2, lpd)
    out = pgas_amd.forecast_summary(res, y=np.array([5.0, 2.0, np.nan]))
    assert out["y_pred_mean"].shape == (2, 3, 1) and out["x_pred_mean"].shape == (2, 3, 1) and out["log_score"].shape == (2,)
    assert np.array_equal(out["x_pred_mean"].numpy()[0], [[4.0], [1.0], [1.0]]) and np.array_equal(out["y_pred_mean"].numpy()[0], [[4.0], [1.0], [1.0]])
    assert np.array_equal(out["y_pred_mean"].numpy()[1], [[nan], [2.0], [3.0]], equal_nan=True)
    assert np.allclose(out["x_pred_std"].numpy()[0], [[np.sqrt(5.0)], [1.0], [0.0]], rtol=1e-15)
    assert np.allclose(out["y_pred_std"].numpy()[1, 1:], [[np.sqrt(2.0)], [0.0]], rtol=1e-15) and np.isnan(out["y_pred_std"].numpy()[1, 0])
    # log score: h = 1 over rows 0, 1 (row 2 holds a NaN observation), h = 2 over row 1 only
    want = [0.5 * (np.log(0.4) + np.log(0.2)), np.log(0.4)]
    assert np.allclose(out["log_score"].numpy(), want, rtol=0, atol=1e-15)
    # rmse: h = 1 over rows 0, 1: errors -1, -1; h = 2 over row 1: error 0
    assert np.array_equal(out["rmse"].numpy(), [1.0, 0.0])
    bare = heldout.ForecastResult(flt, 2, s1, s2, None)
    assert set(pgas_amd.forecast_summary(bare)) == {"x_pred_mean", "x_pred_std", "y_pred_mean", "y_pred_std"}
    with pytest.raises(ValueError):
        pgas_amd.forecast_summary(res, y=np.zeros(4))
    # a horizon without a defined, non-NaN row has no score
    empty = heldout.ForecastResult(flt, 2, s1, s2, torch.full((2, 2, 3), nan, dtype=torch.float64))
    assert np.isnan(pgas_amd.forecast_summary(empty)["log_score"].numpy()).all()


# ---- 4. the closed-form statistic of the device test, on the restatement ---------------------------------------------------------------
def _mvn_logpdf(e, C):
    C = np.atleast_2d(C)
    return float(-0.5 * (len(e) * np.log(2 * np.pi) + np.linalg.slogdet(C)[1] + e @ np.linalg.solve(C, e)))


def linear_gaussian_case(pb):
    """test_evidence_of_a_linear_gaussian_model_is_the_closed_form's construction (tests/test_gpu_filter.py): A = 0, S scaled so that
    tr(H S H^T) = tr(R), y drawn from that model -> (S, y, analytic (H + 1,)) with analytic[h] = sum_{tau >= h - 1} log N(y_tau; 0, H S H^T
    + R) for h >= 2 (the h-step-ahead cloud of a model with A = 0 is N(0, S) whatever the origin's cloud was)."""
    lik, T, nx = pb.likelihood_fcn, pb.T, pb.nx
    Hm, R = np.atleast_2d(lik.H), np.atleast_2d(lik.R)
    _, S = experiments.initial_params(pb)
    S = S * (np.trace(R) / np.trace(Hm @ S @ Hm.T))
    assert np.isclose(np.trace(Hm @ S @ Hm.T), np.trace(R))
    rng = np.random.default_rng(20240607)
    m0, P0 = pb.init_state_mean, pb.init_state_cov
    xs = rng.standard_normal((T, nx)) @ np.linalg.cholesky(S).T
    xs[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(nx)
    y = xs @ Hm.T + rng.standard_normal((T, lik.ny)) @ np.atleast_2d(lik.LR).T
    analytic = np.full(H + 1, np.nan)
    for h in range(2, H + 1):
        analytic[h] = sum(_mvn_logpdf(y[t], Hm @ S @ Hm.T + R) for t in range(h - 1, T))
    return S, y, analytic


KEYS = 16


def closed_form_keys():
    return [prng.key(1000 + 7919 * k) for k in range(KEYS)]


def closed_form_z(lpd, analytic, name):
    """lpd (16, H, T) -> z (H + 1,) for h = 2 .. H: (mean_k sum_{tau >= h - 1} lpd[k, h - 1, tau] - analytic[h]) / (std_k / sqrt(16))."""
    z = np.full(H + 1, np.nan)
    for h in range(2, H + 1):
        tot = lpd[:, h - 1, h - 1:].sum(axis=1)
        assert np.isfinite(tot).all()
        se = tot.std() / np.sqrt(len(tot))
        z[h] = (tot.mean() - analytic[h]) / se
        print(f"{name}: h = {h}, analytic {analytic[h]:.6f}, mean {tot.mean():.6f}, std {tot.std():.6f}, z = {z[h]:.3f}")
    return z


@pytest.mark.parametrize("name", ["smo", "toy", "veh27"])
def test_closed_form_statistic_on_the_restatement(name):
    """With A = 0 the clouds at h >= 2 do not depend on the trace they start from, so the restatement runs from a trace of zeros: the
    figures are the ones the device test must reproduce (the engine equals its restatement bit for bit)."""
    pb = _problem(name)
    S, y, analytic = linear_gaussian_case(pb)
    N = 1024
    pbs = type(pb)(**{**pb.__dict__, "observations": y})
    cm1 = canon_model(pbs, N + 1)
    A = np.zeros((pb.nx, pb.basis_fcn.basis.M))
    x = np.zeros((pb.T, N, pb.nx))
    lpd = np.stack([fc.run(cm1, N, key, A, S, pb.likelihood_fcn, y, x, H)["lpd"] for key in closed_form_keys()])
    z = closed_form_z(lpd, analytic, name)
    assert (np.abs(z[2:]) <= 4.0).all()
