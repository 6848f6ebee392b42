"""Host side of the predictive CDF counts (pgas_amd/calibration.py, Rollout.cdf, HeldOutFilter.forecast_cdf), no
GPU: the NumPy restatement of the counts (tests/rollout_cdf_numpy.py) on hand-made clouds, the refusals from shapes alone, the plain-torch
summaries on constructed counts, and the closed-form binomial statistic of the GPU tests evaluated on the generator's own normals."""
import math

import numpy as np
import pytest
import torch

import rollout_cdf_numpy as rc
from common import canon, experiments, pgas_amd
from pgas_amd import calibration as cal
from pgas_amd import random as prng

INF, NAN = float("inf"), float("nan")


# ---- 1. the restatement on hand-made clouds ------------------------------------------------------------------------------------------
def test_counts_on_a_hand_made_cloud_ties_nan_and_infinite_thresholds():
    # one row, five replicates, one channel: values with a tie at 1.0 and a NaN
    v = np.array([0.5, 1.0, 1.0, NAN, -2.0]).reshape(1, 5, 1)
    thr = np.array([-INF, -2.0, 0.75, 1.0, np.nextafter(1.0, 0.0), NAN, INF]).reshape(1, 1, 7)
    got = rc.counts(v, thr)
    assert got.dtype == np.int32 and got.shape == (1, 1, 7)
    #                                 -inf  -2 (tie counts)  0.75  1.0 (both ties)  just below 1  NaN  +inf (the NaN value never counts)
    assert got[0, 0].tolist() == [0, 1, 2, 4, 2, 0, 4]
    # an infinite value: -inf <= -inf and +inf <= +inf hold
    w = np.array([-INF, INF, 0.0]).reshape(1, 3, 1)
    assert rc.counts(w, np.array([-INF, 0.0, INF]).reshape(1, 1, 3))[0, 0].tolist() == [1, 2, 3]
    # leading axes, rows and channels keep their places: thr is indexed by (row, channel)
    v2 = np.arange(2 * 3 * 4 * 2, dtype=np.float64).reshape(2, 3, 4, 2)
    thr2 = np.stack([np.full((2, 1), 8.0 * t + 3.0) for t in range(3)])   # (3, 2, 1)
    want = np.array([[[(v2[k, t, :, c] <= thr2[t, c, 0]).sum() for c in range(2)] for t in range(3)] for k in range(2)])
    assert np.array_equal(rc.counts(v2, thr2)[..., 0], want)


def test_channels_are_the_state_then_the_predicted_observation_with_the_noise_chain():
    rng = np.random.default_rng(5)
    cloud, e = rng.standard_normal((2, 3, 7, 2)), rng.standard_normal((2, 3, 7, 2))
    sel = np.array([[0.0, 1.0], [1.0, 0.0]])
    LR = np.array([[0.3, 0.0], [-0.07, 0.4]])
    import rollout_stats_numpy as rs

    for H in (sel, np.array([[0.3, -1.7], [1.0, 0.25]])):
        for noise in (False, True):
            got = rc.channels(cloud, H, LR if noise else None, e if noise else None)
            want = np.concatenate([cloud, rs.predicted_obs(cloud, H, LR if noise else None, e if noise else None)], axis=-1)
            assert np.array_equal(got, want)
    assert np.array_equal(rc.channels(cloud, sel)[..., 2:], cloud[..., ::-1])


def test_forecast_counts_mark_the_entries_without_an_origin_row():
    lik = pgas_amd.GaussianLikelihood(np.array([[1.0]]), np.array([[0.04]]))
    Hn, T, N = 3, 4, 5
    cloud = np.full((Hn, T, N, 1), NAN)
    for h in range(Hn):
        cloud[h, h:] = np.arange(N, dtype=np.float64)[None, :, None]
    thr = np.full((T, 2, 2), 1.0)   # a tie with particle 1: the noise decides it
    thr[..., 1] = INF
    got = rc.forecast_counts(cloud, lik, thr)
    assert got.shape == (Hn, T, 2, 2) and got.dtype == np.int32
    for h in range(Hn):
        assert (got[h, :h] == -1).all() and (got[h, h:, :, 0] == 2).all() and (got[h, h:, :, 1] == N).all()
    # the noise of lead l sits on particle offset (l + 1) << 32 of the observation stream: distinct from the open loop's
    key = prng.key(1000)
    a = canon.normals(key, rc.STREAM_OBS, 2, 1 << 32, 4, 1)
    assert not np.array_equal(a, canon.normals(key, rc.STREAM_OBS, 2, 0, 4, 1)) and not np.array_equal(a, canon.normals(key, rc.STREAM_OBS, 2, 2 << 32, 4, 1))
    noisy = rc.forecast_counts(cloud, lik, thr, key=key)
    assert (noisy[..., :1, :] == got[..., :1, :]).all() and not np.array_equal(noisy[..., 1:, 0], got[..., 1:, 0])


# ---- 2. every argument error is a ValueError before a device is touched --------------------------------------------------------------
def test_cdf_refusals_touch_no_device():
    pb = experiments.smo_pgas(T=16)
    nx, M, K, T = pb.nx, pb.basis_fcn.basis.M, 3, pb.T
    sim = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, nx, pb.init_state_mean, pb.init_state_cov, likelihood_fcn=pb.likelihood_fcn, observations=pb.observations)
    A, S, keys = np.zeros((K, nx, M)), np.stack([np.eye(nx)] * K), [1, 2, 3]
    bad = [
        (dict(thresholds=np.zeros((T, nx + 1, 17))), "J = 17"),
        (dict(thresholds=np.zeros((T, 1, 0))), "J = 0"),
        (dict(thresholds=np.zeros((T + 1, nx + 1, 2))), "thresholds"),
        (dict(thresholds=np.zeros((T, nx, 2))), "thresholds"),
        (dict(thresholds=np.zeros((T, nx + 1))), "thresholds"),
        (dict(thresholds=np.zeros(T + 1)), "thresholds"),
        (dict(replicates=0), "replicates"),
        (dict(replicates=(1 << 20) + 1), "replicates"),
        (dict(keys=None), "needs keys"),
        (dict(keys=[1, 2]), "keys"),
        (dict(coeff_mat=np.zeros((K, nx, M + 1))), "coeff_mat"),
        (dict(error_cov=np.zeros((K + 1, nx, nx))), "error_cov"),
        (dict(init_state=np.zeros(nx + 1)), "init_state"),
    ]
    for kw, match in bad:
        args = dict(coeff_mat=A, error_cov=S, keys=keys, replicates=10)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            sim.cdf(**args)
    with pytest.raises(ValueError, match="observation_noise needs keys"):
        sim.cdf(A, init_state=np.zeros(nx), observation_noise=True)
    bare = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, nx, pb.init_state_mean, pb.init_state_cov)
    with pytest.raises(ValueError, match="has none"):
        bare.cdf(A, S, keys, replicates=10)
    assert sim._engine is None and bare._engine is None
    # the accepted forms
    assert cal.check_thresholds(T, nx, 1, None, True) == (1, "pit")
    assert cal.check_thresholds(T, nx, 1, np.zeros(T), False) == (1, "obs")
    assert cal.check_thresholds(T, nx, 2, np.zeros((T, 2)), False) == (1, "obs")
    assert cal.check_thresholds(T, nx, 1, np.zeros((T, 1, 16)), False) == (16, "obs")
    assert cal.check_thresholds(T, nx, 1, np.zeros((T, nx + 1, 5)), False) == (5, "all")

    flt = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, nx, 32, init_state_mean=pb.init_state_mean,
                                 init_state_cov=pb.init_state_cov)
    for kw, match in [(dict(horizon=0), "horizon"), (dict(horizon=T + 1), "horizon"), (dict(thresholds=np.zeros((T, nx + 1, 17))), "J = 17"),
                      (dict(thresholds=np.zeros((T, 5, 2))), "thresholds"), (dict(keys=None), "keys"), (dict(error_cov=None), "error_cov")]:
        args = dict(coeff_mat=A, error_cov=S, keys=keys, horizon=2)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            flt.forecast_cdf(**args)
    assert flt._engine is None


# ---- 3. the summaries on constructed counts ------------------------------------------------------------------------------------------
def test_pooled_cdf_is_one_integer_sum_and_one_division_and_minus_one_is_nan():
    K, n = 3, 7
    count = torch.tensor([[[[1, 7]], [[0, 3]]], [[[2, 7]], [[5, 3]]], [[[7, 7]], [[1, 4]]]], dtype=torch.int32)   # (K, T = 2, C = 1, J = 2)
    out = pgas_amd.calibration_summary(pgas_amd.CdfCounts(n, count, torch.zeros(2, 1, 2, dtype=torch.float64)))
    assert set(out) == {"F"} and out["F"].dtype == torch.float64
    assert torch.equal(out["F"], torch.tensor([[[10, 21]], [[6, 10]]], dtype=torch.float64) / 21.0)
    big = torch.full((600, 1, 1, 1), 2 ** 20, dtype=torch.int32)   # the int32 sum would overflow
    assert float(pgas_amd.calibration_summary(pgas_amd.CdfCounts(2 ** 20, big, torch.zeros(1, 1, 1)))["F"][0, 0, 0]) == 1.0
    fc = torch.tensor([[[[[3]], [[4]]], [[[-1]], [[2]]]]], dtype=torch.int32)   # (K = 1, H = 2, T = 2, C = 1, J = 1)
    s = pgas_amd.calibration_summary(pgas_amd.CdfCounts(4, fc, torch.zeros(2, 1, 1, dtype=torch.float64)))
    assert torch.equal(torch.isnan(s["F"][..., 0, 0]), torch.tensor([[False, False], [True, False]]))
    assert s["pit"].shape == (2, 2, 1) and s["ks"].shape == (2,) and s["hist"].shape == (2, 10)
    assert float(s["hist"][1].sum()) == 1.0 and float(s["hist"][0].sum()) == 2.0   # the undefined entry takes no part


def test_a_uniform_pit_is_calibrated_and_a_narrow_one_is_not():
    T, n, nx = 1000, 2000, 2
    obs = torch.zeros(T, nx + 1, 1, dtype=torch.float64)
    obs[:, :nx] = NAN
    count = torch.zeros((1, T, nx + 1, 1), dtype=torch.int32)
    count[0, :, nx, 0] = 2 * torch.arange(1, T + 1, dtype=torch.int32) - 1   # pit = (2 i - 1) / (2 T): the midpoints, off every edge
    s = pgas_amd.calibration_summary(pgas_amd.CdfCounts(n, count, obs, nx=nx, pit=True))
    assert s["pit"].shape == (T, 1) and torch.equal(s["pit"][:, 0], (2 * torch.arange(1, T + 1, dtype=torch.float64) - 1) / n)
    for lv, share in s["coverage"].items():
        assert abs(float(share) - lv) <= 1e-12, (lv, float(share))         # (a, 1 - a] holds exactly level * T of the T values
    assert torch.equal(s["hist"], torch.full((10,), 100.0, dtype=s["hist"].dtype))
    assert abs(float(s["ks"]) - 0.5 / T) <= 1e-12
    # a NaN observation row takes no part
    obs2 = obs.clone()
    obs2[10, nx, 0] = NAN
    s2 = pgas_amd.calibration_summary(pgas_amd.CdfCounts(n, count, obs2, nx=nx, pit=True))
    assert float(s2["hist"].sum()) == T - 1
    # every observation in the middle of its predictive: the intervals over-cover, the KS distance is 1/2
    mid = torch.full((1, T, nx + 1, 1), n // 2, dtype=torch.int32)
    s3 = pgas_amd.calibration_summary(pgas_amd.CdfCounts(n, mid, obs, nx=nx, pit=True), levels=(0.5, 0.9))
    assert float(s3["coverage"][0.5]) == 1.0 and float(s3["coverage"][0.9]) == 1.0 and abs(float(s3["ks"]) - 0.5) <= 1e-12


def test_threshold_grid_and_bands_invert_a_known_gaussian_cdf_to_the_grid_spacing():
    T, C, J, K, n = 4, 2, 16, 2, 50000
    mean = torch.tensor([[0.0, 1.0], [2.0, -1.0], [0.5, 0.0], [-3.0, 10.0]], dtype=torch.float64)
    std = torch.tensor([[1.0, 2.0], [0.5, 1.0], [3.0, 0.1], [1.0, 4.0]], dtype=torch.float64)
    thr = pgas_amd.threshold_grid(mean, std, J, width=3.0)
    assert thr.shape == (T, C, J)
    z = torch.linspace(-3.0, 3.0, J, dtype=torch.float64)
    assert torch.equal(thr, mean[..., None] + std[..., None] * z)
    with pytest.raises(ValueError, match="J = 17"):
        pgas_amd.threshold_grid(mean, std, 17)
    Phi = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    count = torch.round(Phi * n).to(torch.int32).expand(K, T, C, J).contiguous()
    cdf = pgas_amd.CdfCounts(n, count, thr)
    levels = (0.025, 0.25, 0.5, 0.75, 0.975)
    q = pgas_amd.predictive_bands(cdf, levels)
    assert q.shape == (T, C, len(levels))
    zq = torch.tensor([-1.959963984540054, -0.6744897501960817, 0.0, 0.6744897501960817, 1.959963984540054], dtype=torch.float64)
    want = mean[..., None] + std[..., None] * zq
    spacing = std[..., None] * (6.0 / (J - 1))
    assert bool(((q - want).abs() <= spacing).all())
    assert bool(((q - want).abs() <= 0.06 * std[..., None]).all())          # linear interpolation of Phi on a 0.4 sigma grid
    # a level outside the grid's range, and an undefined count, give NaN
    out = pgas_amd.predictive_bands(cdf, (0.0005, 0.9995))
    assert bool(torch.isnan(out).all())
    hole = count.clone()
    hole[0, 1] = -1
    q2 = pgas_amd.predictive_bands(pgas_amd.CdfCounts(n, hole, thr), levels)
    assert bool(torch.isnan(q2[1]).all()) and torch.equal(q2[[0, 2, 3]], q[[0, 2, 3]])


# ---- 4. the closed-form statistic of the GPU tests on the generator's own normals ----------------------------------------------------
TAUS = (-2.0, -1.0, -0.25, 0.0, 0.5, 1.5, 2.5)


def binomial_z(count, n, sigma_units=TAUS):
    """count (len(TAUS),) pooled over n values of N(0, sigma^2) at the thresholds sigma * TAUS -> z = (count - n Phi) / sqrt(n Phi (1 - Phi))."""
    Phi = np.array([0.5 * math.erfc(-t / math.sqrt(2.0)) for t in sigma_units])
    return (np.asarray(count, dtype=np.float64) - n * Phi) / np.sqrt(n * Phi * (1.0 - Phi))


def test_closed_form_binomial_statistic_on_the_generators_normals():
    """A = 0, nx = ny = 1: x_t = LS z_t and yhat_t = x_t + LR e_t are iid N(0, S) and N(0, S + R) for t >= 1, so the pooled count at
    sigma * TAUS is Binomial(n, Phi(TAUS))."""
    keys, T, P = [prng.key(1000 + 7919 * k) for k in range(4)], 33, 4096
    LS, LR = math.sqrt(0.37), math.sqrt(0.21)
    sig = np.array([LS, math.sqrt(LS * LS + LR * LR)])
    thr = np.broadcast_to(sig[:, None] * np.array(TAUS)[None, :], (T, 2, len(TAUS)))
    tot = np.zeros((2, len(TAUS)), dtype=np.int64)
    for key in keys:
        x = np.stack([LS * canon.normals(key, canon.STREAM_PROP, t, 0, P, 1) for t in range(T)])           # (T, P, 1)
        e = np.stack([canon.normals(key, rc.STREAM_OBS, t, 0, P, 1) for t in range(T)])
        v = np.concatenate([x, x + LR * e], axis=-1)
        tot += rc.counts(v, thr)[1:].sum(axis=0)
    n = len(keys) * (T - 1) * P
    for c, name in enumerate(("x", "yhat")):
        z = binomial_z(tot[c], n)
        print(f"{name}: z = {np.round(z, 3).tolist()}")
        assert (np.abs(z) <= 4.0).all()
