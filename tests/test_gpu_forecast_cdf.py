"""CDF counts of the h-step-ahead clouds (pgas_amd.HeldOutFilter.forecast_cdf, pgas_forecast_cdf, csrc/pgas_forecast_cdf.hip.h, DESIGN.md
section 19) against the NumPy restatement (tests/rollout_cdf_numpy.py) applied to the clouds of tests/forecast_numpy.py, fed the device's
own filter trace (which tests/test_gpu_forecast.py pins to the filter restatement).  Every comparison with the restatement is
np.array_equal.  Independent of the restatement: +inf thresholds against pgas_forecast's own sums, and a model with A = 0 whose pooled
counts are binomial."""
import functools

import numpy as np
import pytest
import torch

import forecast_numpy as fc
import rollout_cdf_numpy as rc
from common import canon_model, experiments, pgas_amd
from pgas_amd import chains as ch
from test_gpu_forecast import _filter_for, _with_obs, _y
from test_gpu_rollout import _draws, _np, _problem
from test_gpu_rollout_stats import _noise_lik
from test_rollout_cdf_host import TAUS, binomial_z

pytestmark = pytest.mark.gpu

K, H = 3, 5
NS = [1, 2, 255, 256, 257, 513, 1024]   # every NR (1, 2, 4 register rows) and both sides of a row boundary
INF, NAN = float("inf"), float("nan")


def _noise_pb(name):
    pb = _problem(name)
    return type(pb)(**{**pb.__dict__, "likelihood_fcn": _noise_lik(name)})


def _clouds(pb, N, keys, As, Ss, x, Hn, y=None):
    """forecast_numpy.run's clouds (K, H, T, N, nx) from the trace x (K, T, N, nx)."""
    y = _y(pb) if y is None else y
    cm1 = canon_model(_with_obs(pb, y), N + 1)
    return np.stack([fc.run(cm1, N, keys[k], As[k], Ss[k], pb.likelihood_fcn, y, x[k], Hn, score=False)["cloud"] for k in range(len(keys))])


def _want(pb, clouds, thr, keys=None):
    return np.stack([rc.forecast_counts(clouds[k], pb.likelihood_fcn, thr, None if keys is None else keys[k]) for k in range(clouds.shape[0])])


def _grid(clouds, lik, J):
    """threshold_grid of the clouds' pooled moments over draws, horizons and particles, per target row; the predicted observations'
    spread with the measurement noise's variance added (it is there when the noise is on, and keeps a cloud of one particle off zero)."""
    v = rc.channels(clouds, lik.H)                                          # (K, H, T, N, nv), NaN where undefined
    nx = clouds.shape[-1]
    mean, var = np.nanmean(v, axis=(0, 1, 3)), np.nanvar(v, axis=(0, 1, 3))
    var[:, nx:] += np.diag(np.atleast_2d(lik.R))[None, :]
    std = np.sqrt(var) + 1e-3 * np.abs(mean)
    return pgas_amd.threshold_grid(torch.as_tensor(mean), torch.as_tensor(std), J, width=2.0 if J > 1 else 0.5).numpy()


@functools.lru_cache(maxsize=None)
def _case(name, N):
    """(filter, trace (K, T, N, nx), restated clouds (K, H, T, N, nx)): computed once per (model, N) and never changed."""
    pb = _noise_pb(name)
    keys, As, Ss = _draws(pb, K)
    flt = _filter_for(pb, N)
    x = _np(flt(As, Ss, keys, traces=True).x)
    clouds = _clouds(pb, N, keys, As, Ss, x, H)
    clouds.setflags(write=False)
    return flt, x, clouds


# ---- 1. the restated counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", [("toy", N) for N in NS] + [("veh27", 257)])
def test_counts_equal_the_restated_counts_of_the_forecast_clouds(name, N):
    pb = _noise_pb(name)
    keys, As, Ss = _draws(pb, K)
    flt, x, clouds = _case(name, N)
    nv = pb.nx + pb.likelihood_fcn.ny
    for J in (1, 16):
        thr = _grid(clouds, pb.likelihood_fcn, J)
        for noise in (False, True):
            res = flt.forecast_cdf(As, Ss, keys, H, thresholds=thr, observation_noise=noise)
            got = _np(res.count)
            assert res.n == N and got.dtype == np.int32 and got.shape == (K, H, pb.T, nv, J)
            want = _want(pb, clouds, thr, keys if noise else None)
            assert np.array_equal(got, want), f"J = {J}, noise = {noise}"
            for h in range(H):   # -1 exactly where the target row has no origin
                assert (got[:, h, :h] == -1).all() and (got[:, h, h:] >= 0).all() and (got[:, h, h:] <= N).all()
            if J == 16 and N >= 255:   # the grid sits inside the clouds: every channel has counts that are neither 0 nor N
                assert ((want > 0) & (want < N)).any(axis=(0, 1, 2, 4)).all()
    # counts do not depend on H: fewer horizons are the leading horizons
    for Hn in (1, 2):
        part = _np(flt.forecast_cdf(As, Ss, keys, Hn, thresholds=thr, observation_noise=True).count)
        assert np.array_equal(part, got[:, :Hn])


def test_every_horizon_of_a_short_record():
    pb0 = experiments.smo_pgas(T=6)
    pb = type(pb0)(**{**pb0.__dict__, "likelihood_fcn": _noise_lik("smo")})
    keys, As, Ss = _draws(_problem("smo"), K)
    N, T = 257, 6
    flt = _filter_for(pb, N)
    x = _np(flt(As, Ss, keys, traces=True).x)
    clouds = _clouds(pb, N, keys, As, Ss, x, T)
    thr = _grid(clouds, pb.likelihood_fcn, 16)
    got = _np(flt.forecast_cdf(As, Ss, keys, T, thresholds=thr).count)
    assert np.array_equal(got, _want(pb, clouds, thr, keys))
    assert (got[:, T - 1, :T - 1] == -1).all() and (got[:, T - 1, T - 1] >= 0).all()
    one = _np(flt.forecast_cdf(As, Ss, keys, 1, thresholds=thr).count)
    assert np.array_equal(one, got[:, :1]) and (one >= 0).all()


# ---- 2. against pgas_forecast's own outputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 300, 1024])
def test_an_infinite_threshold_counts_every_particle_where_the_forecast_sum_is_finite(N):
    pb = _noise_pb("smo")
    keys, As, Ss = _draws(pb, K)
    flt = _filter_for(pb, N)
    res = flt.forecast(As, Ss, keys, H, log_score=False)
    thr = np.full((pb.T, pb.nx + 1, 3), INF)
    thr[..., 0], thr[..., 1] = -INF, NAN
    cnt = flt.forecast_cdf(As, Ss, keys, H, thresholds=thr, observation_noise=False).count
    finite = torch.isfinite(res.sum)
    assert bool(finite.any()) and torch.equal(finite, ~torch.isnan(res.sum))
    assert bool((cnt[..., 2][finite] == N).all()) and bool((cnt[..., 2][~finite] == -1).all())
    assert bool((cnt[..., 0][finite] == 0).all()) and bool((cnt[..., 1][finite] == 0).all())


def test_counts_do_not_depend_on_which_draws_share_the_launch():
    name, N = "toy", 257
    pb = _noise_pb(name)
    keys, As, Ss = _draws(pb, K)
    flt, _, clouds = _case(name, N)
    thr = _grid(clouds, pb.likelihood_fcn, 16)
    whole = flt.forecast_cdf(As, Ss, keys, H, thresholds=thr).count
    idx = [2, 0, 2, 1]
    mixed = flt.forecast_cdf(As[idx], Ss[idx], [keys[i] for i in idx], H, thresholds=thr).count
    for j, i in enumerate(idx):
        assert torch.equal(mixed[j], whole[i])
    one = flt.forecast_cdf(As[1:2], Ss[1:2], keys[1:2], H, thresholds=thr).count
    assert torch.equal(one[0], whole[1]) and not torch.equal(whole[0], whole[1])


def test_a_nan_observation_row_and_the_pit_of_the_record():
    name, N = "toy", 300
    pb = _noise_pb(name)
    keys, As, Ss = _draws(pb, K)
    y = _y(pb).copy()
    y[7] = NAN
    flt = _filter_for(pb, N, obs=y)
    x = _np(flt(As, Ss, keys, traces=True).x)
    clouds = _clouds(pb, N, keys, As, Ss, x, H, y=y)
    pit = flt.forecast_cdf(As, Ss, keys, H)                     # thresholds=None: the record's observations, measurement noise on
    assert pit.pit and tuple(pit.count.shape) == (K, H, pb.T, pb.nx + 1, 1)
    full = np.concatenate([np.full((pb.T, pb.nx, 1), NAN), y[:, :, None]], axis=1)
    assert np.array_equal(_np(pit.thresholds), full, equal_nan=True)
    got = _np(pit.count)
    assert np.array_equal(got, _want(pb, clouds, full, keys))
    assert (got[:, :, 7][got[:, :, 7] >= 0] == 0).all() and got.max() <= N   # a NaN threshold counts nothing
    assert torch.equal(flt.forecast_cdf(As, Ss, keys, H, thresholds=y).count, pit.count)
    s = pgas_amd.calibration_summary(pit)
    assert tuple(s["pit"].shape) == (H, pb.T, 1) and tuple(s["ks"].shape) == (H,) and tuple(s["hist"].shape) == (H, 10)
    for h in range(H):
        assert bool(torch.isnan(s["pit"][h, :h]).all()) and float(s["hist"][h].sum()) == pb.T - h - (1 if h <= 7 else 0)
        assert 0.0 <= float(s["ks"][h]) <= 1.0


# ---- 3. side effects ------------------------------------------------------------------------------------------------------------------------
def test_forecast_cdf_makes_no_host_round_trip():
    pb = experiments.smo_pgas(T=16)
    Kd, N = 4, 300
    keys, As, Ss = _draws(pb, Kd)
    flt = _filter_for(pb, N)
    dev = flt.engine.device
    kd = ch.keys_tensor(keys, dev)
    Ad, Sd = torch.as_tensor(As, device=dev), torch.as_tensor(Ss, device=dev)
    thr = torch.linspace(-1.0, 1.0, 16, dtype=torch.float64, device=dev).expand(16, 3, 16).contiguous()
    calls = [lambda: flt.forecast_cdf(Ad, Sd, kd, 4, thresholds=thr), lambda: flt.forecast_cdf(Ad, Sd, kd, 16, thresholds=thr[:, 2:].contiguous(), observation_noise=False)]
    warm = [c() for c in calls]   # allocations may synchronise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a.count, b.count) and bool((a.count >= -1).all()) and bool((a.count > 0).any())


def test_refusals_are_clean_and_leave_the_context_usable():
    pb = experiments.smo_pgas(T=16)
    Kd, N, T = 2, 64, 16
    keys, As, Ss = _draws(pb, Kd)
    flt = _filter_for(pb, N)
    eng = flt.engine
    thr = torch.linspace(-1.0, 1.0, 16, dtype=torch.float64, device=eng.device).expand(T, 3, 16).contiguous()
    good = flt.forecast_cdf(As, Ss, keys, 3, thresholds=thr).count.clone()
    Ad, Sd, kd = torch.as_tensor(As, device=eng.device), torch.as_tensor(Ss, device=eng.device), ch.keys_tensor(keys, eng.device)
    x = flt(As, Ss, keys, traces=True).x
    out = torch.empty((Kd, T, T, 3, 16), dtype=torch.int32, device=eng.device)
    PGAS_E_ARG = -1

    def call(Kc, Hc, seeds=kd, S=Sd, xt=x, th=thr, J=16, cnt=out):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc_ = eng.lib.pgas_forecast_cdf(eng._h, Kc, Hc, p(seeds), Ad.data_ptr(), p(S), p(xt), None, p(th), J, p(cnt), eng._stream())
        return rc_, eng.lib.pgas_last_error(eng._h).decode()

    for args, kw, msg in [((Kd, 0), {}, "H = 0"), ((Kd, T + 1), {}, "H = 17"), ((0, 3), {}, "K = 0"), ((Kd, 3, None), {}, "seeds and S are needed"),
                          ((Kd, 3, kd, None), {}, "seeds and S are needed"), ((Kd, 3), dict(xt=None), "NULL"), ((Kd, 3), dict(J=0), "J = 0"),
                          ((Kd, 3), dict(J=17), "J = 17"), ((Kd, 3), dict(th=None), "NULL"), ((Kd, 3), dict(cnt=None), "NULL")]:
        rc_, err = call(*args, **kw)
        assert rc_ == PGAS_E_ARG and msg in err, (args, kw, rc_, err)
        assert torch.equal(flt.forecast_cdf(As, Ss, keys, 3, thresholds=thr).count, good), f"forecast_cdf after refusing {args} {kw}"
    # in-sample on a training context: the same counts
    smc = pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    assert torch.equal(smc.forecast_cdf(As, Ss, keys, 3, thresholds=thr).count, good)


# ---- 4. independent of the restatement: a model whose predictive is known ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_pooled_counts_of_a_model_with_A_zero_are_binomial(name):
    """A = 0: every cloud at a target row tau >= 1 is iid N(0, S) whatever the horizon (lead 0 is the filter's propagated row, leads >= 1
    the forecast's own noise), and yhat + noise ~ N(0, H S H^T + R).  The count pooled over draws, horizons, rows and particles at the
    thresholds sigma_c * TAUS is Binomial(n, Phi(TAUS)): |z| <= 4, the bound of the project's other closed-form tests."""
    pb = _noise_pb(name)
    Kd, N, Hn = 3, 1024, 4
    keys, _, Ss = _draws(pb, Kd)
    S, lik = Ss[0], pb.likelihood_fcn
    Hm = np.atleast_2d(lik.H)
    sig = np.sqrt(np.concatenate([np.diag(S), np.diag(Hm @ S @ Hm.T + np.atleast_2d(lik.R))]))
    thr = np.broadcast_to(sig[:, None] * np.array(TAUS)[None, :], (pb.T, len(sig), len(TAUS))).copy()
    A0 = np.zeros((Kd, pb.nx, pb.basis_fcn.basis.M))
    cnt = _np(_filter_for(pb, N).forecast_cdf(A0, np.stack([S] * Kd), keys, Hn, thresholds=thr, observation_noise=True).count).astype(np.int64)
    defined = (np.arange(pb.T)[None, :] >= np.maximum(np.arange(Hn), 1)[:, None])       # tau >= max(h - 1, 1)
    assert (cnt[:, defined] >= 0).all()
    tot = cnt[:, defined].sum(axis=(0, 1))                                               # (nv, 7)
    n = Kd * int(defined.sum()) * N
    for c in range(len(sig)):
        z = binomial_z(tot[c], n)
        print(f"{name}: channel {c}, n = {n}, z = {np.round(z, 3).tolist()}")
        assert (np.abs(z) <= 4.0).all()
