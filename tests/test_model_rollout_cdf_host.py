"""Host side of the grey-box predictive CDF counts (pgas_amd.ModelRollout.cdf / forecast_cdf, pgas_m_rollout_cdf, pgas_m_forecast_cdf,
DESIGN.md section 20), no GPU: the NumPy restatement (tests/model_rollout_cdf_numpy.py) on hand-made clouds, every refusal of
``check_cdf`` / ``check_forecast_cdf`` before a device is touched, the C ABI binding, calibration_summary on a constructed grey-box
CdfCounts, and the closed-form binomial statistic of the GPU tests evaluated on the CPU with the generator's own normals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import model_cdf_cases as mc
import model_filter_cases as cases
import model_rollout_cdf_numpy as mrc
import model_rollout_stats_numpy as ms
from common import ROOT, canon, pgas_amd
from pgas_amd import calibration as cal
from test_model_rollout_stats_host import _c_struct_layout

K, T, KEYS = cases.K, cases.T, cases.KEYS
INF, NAN = float("inf"), float("nan")


# ---- 1. the restatement on hand-made clouds ------------------------------------------------------------------------------------------------
def test_counts_on_a_hand_made_cloud_ties_nan_and_infinite_thresholds():
    v = np.array([0.5, 1.0, 1.0, NAN, -2.0]).reshape(1, 5, 1)   # one row, five replicates, one channel: a tie at 1.0 and a NaN value
    thr = np.array([-INF, -2.0, 0.75, 1.0, np.nextafter(1.0, 0.0), NAN, INF]).reshape(1, 1, 7)
    got = mrc.counts(v, thr)
    assert got.dtype == np.int32 and got.shape == (1, 1, 7)
    #                              -inf  -2 (the tie counts)  0.75  1.0 (both ties)  just below 1  NaN  +inf (the NaN value never counts)
    assert got[0, 0].tolist() == [0, 1, 2, 4, 2, 0, 4]
    w = np.array([-INF, INF, 0.0]).reshape(1, 3, 1)             # -inf <= -inf and +inf <= +inf hold
    assert mrc.counts(w, np.array([-INF, 0.0, INF]).reshape(1, 1, 3))[0, 0].tolist() == [1, 2, 3]


def test_channels_are_the_state_then_g_with_the_noise_chain_and_undefined_forecast_entries_are_minus_one():
    rng = np.random.default_rng(5)
    x, g, e = rng.standard_normal((2, 3, 7, 3)), rng.standard_normal((2, 3, 7, 2)), rng.standard_normal((2, 3, 7, 2))
    LR = np.array([[0.3, 0.0], [-0.07, 0.4]])
    assert np.array_equal(mrc.channels(x, g), np.concatenate([x, g], axis=-1))
    noisy = mrc.channels(x, g, LR, e)
    assert np.array_equal(noisy[..., :3], x) and np.array_equal(noisy[..., 3:], ms.predicted_obs(g, LR, e))
    assert np.abs(noisy[..., 3:] - (g + e @ LR.T)).max() <= 1e-15 and not np.array_equal(noisy[..., 3:], g)
    thr = np.zeros((3, 5, 2))
    thr[..., 1] = INF
    got = mrc.rollout_counts(x, g, thr)                       # (K = 2, T = 3, P = 7): leading axes, rows and channels keep their places
    want = np.array([[[(np.concatenate([x, g], -1)[k, t, :, c] <= 0.0).sum() for c in range(5)] for t in range(3)] for k in range(2)])
    assert np.array_equal(got[..., 0], want) and (got[..., 1] == 7).all()
    Hn, Tn, N = 3, 4, 5                                       # forecasts: -1 exactly where the target row is < h - 1
    cx = np.full((Hn, Tn, N, 1), NAN)
    for h in range(Hn):
        cx[h, h:] = np.arange(N, dtype=np.float64)[None, :, None]
    th = np.full((Tn, 2, 2), 1.0)
    th[..., 1] = INF
    fc = mrc.forecast_counts(cx, 2.0 * cx, th)
    assert fc.shape == (Hn, Tn, 2, 2) and fc.dtype == np.int32
    for h in range(Hn):
        assert (fc[h, :h] == -1).all() and (fc[h, h:, 0, 0] == 2).all() and (fc[h, h:, 1, 0] == 1).all() and (fc[h, h:, :, 1] == N).all()


# ---- 2. every refusal is a ValueError before a device is touched -----------------------------------------------------------------------------
def test_every_cdf_refusal_is_raised_without_a_device():
    pb, ssm, sim = cases.rollout("vehicle")                    # nx = ny = 2: 16 thresholds fill the wave exactly
    A = cases.coeffs(pb)
    keys, P, nx, ny = [1, 2, 3], 10, 2, 2
    assert sim.max_thresholds() == 16
    assert sim.check_cdf(A, keys, P) == (3, P, 0, True, False, 1, "pit")
    assert sim.check_cdf(A, keys, P, thresholds=np.zeros((T, 4, 16)), observation_noise=True, p0=64) == (3, P, 0, True, False, 16, "all")
    assert sim.check_cdf(A, keys, P, thresholds=np.zeros((T, 2, 5)))[5:] == (5, "obs")
    assert sim.check_cdf(A, keys, P, thresholds=np.zeros((T, 2)))[5:] == (1, "obs")
    bad = [
        (dict(thresholds=np.zeros((T, 4, 17))), "J = 17"),
        (dict(thresholds=np.zeros((T, 2, 0))), "J = 0"),
        (dict(thresholds=np.zeros((T + 1, 4, 2))), "thresholds"),
        (dict(thresholds=np.zeros((T, 3, 2))), "thresholds"),
        (dict(thresholds=np.zeros(T)), "thresholds"),           # (T,) is the ny == 1 form
        (dict(replicates=0), "replicates"),
        (dict(replicates=(1 << 20) + 1), "replicates"),
        (dict(p0=-1), "p0"),
        (dict(keys=None), "needs keys"),
        (dict(keys=[1, 2]), "expected 3 keys"),
        (dict(coeffs=A[0]), "list of 2"),
        (dict(coeffs=[A[0][:, :, :-1], A[1]]), r"coeffs\[0\]"),
        (dict(init_state=np.zeros(3)), "init_state"),
        (dict(row_cov=[np.zeros((3, 2, 2)), np.zeros((3, 1, 1))]), r"row_cov\[0\]"),
        (dict(init_state=np.zeros(2), process_noise=False), "copies"),
    ]
    for kw, msg in bad:
        args = dict(coeffs=A, keys=keys, replicates=P)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            sim.check_cdf(**args)
        with pytest.raises(ValueError, match=msg):
            sim.cdf(**args)
    with pytest.raises(ValueError, match="observation_noise needs keys"):
        sim.cdf(A, None, 3, init_state=np.zeros((3, 3, 2)), process_noise=False, observation_noise=True)
    _, _, bare = cases.rollout("vehicle", has_obs=False)
    with pytest.raises(ValueError, match="has none"):
        bare.cdf(A, keys, P)
    assert bare.check_cdf(A, keys, P, thresholds=np.zeros((T, 4, 3)))[5:] == (3, "all")      # explicit thresholds need no observations
    fbad = [
        (dict(horizon=0), "horizon"),
        (dict(horizon=T + 1), "horizon"),
        (dict(horizon=2.0), "horizon"),
        (dict(particles=0), "particles"),
        (dict(particles=sim.max_particles() + 1), "particles"),
        (dict(keys=None), "keys"),
        (dict(thresholds=np.zeros((T, 4, 17))), "J = 17"),
        (dict(thresholds=np.zeros((T, 5, 2))), "thresholds"),
        (dict(coeffs=A[0]), "list of 2"),
    ]
    assert sim.check_forecast_cdf(A, keys, 70, 4) == (3, 70, 0, True, False, 4, 1, "pit")
    assert sim.check_forecast_cdf(A, keys, 70, T, np.zeros((T, 4, 16)), False, np.zeros(2))[-4:] == (False, T, 16, "all")
    for kw, msg in fbad:
        args = dict(coeffs=A, keys=keys, particles=70, horizon=4)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            sim.check_forecast_cdf(**args)
        with pytest.raises(ValueError, match=msg):
            sim.forecast_cdf(**args)
    with pytest.raises(ValueError, match="needs observations"):
        bare.forecast_cdf(A, keys, 70, 4, thresholds=np.zeros((T, 4, 2)))
    # the slot limit on five channels: J = 13 needs 65 slots
    wssm, wide, WA, wy = mc.wide_rollout()
    assert (wide.nx, wide.ny, wide.max_thresholds()) == (3, 2, 12)
    for call in (lambda th: wide.cdf(WA, keys, P, thresholds=th), lambda th: wide.check_cdf(WA, keys, P, thresholds=th),
                 lambda th: wide.forecast_cdf(WA, keys, 70, 2, thresholds=th), lambda th: wide.check_forecast_cdf(WA, keys, 70, 2, th)):
        with pytest.raises(ValueError, match="J_max = 12"):
            call(np.zeros((T, 5, 13)))
        with pytest.raises(ValueError, match="J_max = 12"):
            call(np.zeros((T, 2, 13)))                           # the "obs" form still occupies the state channels' slots
    assert wide.check_cdf(WA, keys, P, thresholds=np.zeros((T, 5, 12)))[5:] == (12, "all")
    assert wide.check_forecast_cdf(WA, keys, 70, 2, np.zeros((T, 5, 12)))[-2:] == (12, "all")
    for s in (sim, bare, wide):
        assert s._ops is None and s._dev_cache is None, "a refused call created the device context"


def test_device_thresholds_still_serves_an_engine_like_object_unchanged():
    """What existing callers receive does not change: an object with _dev is used as it is (here a stand-in on the CPU)."""

    class Eng:
        T, nx, ny, device = 3, 2, 1, torch.device("cpu")

        def _dev(self, t, dtype=torch.float64, shape=None):
            return torch.as_tensor(np.asarray(t), dtype=dtype).reshape(shape).contiguous()

    e = Eng()
    full = cal.device_thresholds(e, np.arange(3.0), 1, "obs")
    assert full.shape == (3, 3, 1) and torch.isnan(full[:, :2]).all() and torch.equal(full[:, 2, 0], torch.arange(3, dtype=torch.float64))
    assert torch.equal(cal.device_thresholds(e, np.ones((3, 3, 2)), 2, "all"), torch.ones(3, 3, 2, dtype=torch.float64))
    pit = cal.device_thresholds(e, None, 1, "pit", np.array([[5.0], [6.0], [7.0]]))
    assert torch.equal(pit[:, 2, 0], torch.tensor([5.0, 6.0, 7.0], dtype=torch.float64))

    class Sim:   # a ModelRollout-like object: dimensions of its own, the utility context behind ops.eng
        T, nx, ny = 3, 2, 1

        class ops:
            eng = e

    assert torch.equal(torch.nan_to_num(cal.device_thresholds(Sim(), np.arange(3.0), 1, "obs"), nan=-1.0), torch.nan_to_num(full, nan=-1.0))


# ---- 3. C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound_and_the_ctypes_structs_are_the_c_structs():
    from pgas_amd import _lib

    txt = open(os.path.join(ROOT, "include", "pgas_marginal.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for fn, desc in (("pgas_m_rollout_cdf", "pgas_m_rollout_cdf_desc"), ("pgas_m_forecast_cdf", "pgas_m_forecast_cdf_desc")):
        m = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{fn} is not declared in include/pgas_marginal.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == 4 and "pgas_m_rollout_desc" in params[1] and desc in params[2]
    fields, size = _c_struct_layout(txt, "pgas_m_rollout_cdf_desc")
    S = _lib.ModelRolloutCdfDesc
    assert C.sizeof(S) == size == 2 * 8 + 2 * 4 + 64 * 8
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == fields
    assert [n for n, _ in S._fields_] == ["thr_dev", "count_dev", "J", "noise", "LR"]
    fields, size = _c_struct_layout(txt, "pgas_m_forecast_cdf_desc")
    S = _lib.ModelForecastCdfDesc
    assert C.sizeof(S) == size == 3 * 8 + 4 * 4 + 64 * 8
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == fields
    assert [n for n, _ in S._fields_] == ["x_dev", "thr_dev", "count_dev", "H", "J", "noise", "reserved", "LR"]
    assert "pgas_m_rollout_cdf" in _lib.EXPORTS and "pgas_m_forecast_cdf" in _lib.EXPORTS
    L = _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "pgas_m_rollout_cdf") and hasattr(lib, "pgas_m_forecast_cdf")
    assert L.pgas_m_rollout_cdf.restype is C.c_int and len(L.pgas_m_rollout_cdf.argtypes) == 4
    assert L.pgas_m_forecast_cdf.restype is C.c_int and len(L.pgas_m_forecast_cdf.argtypes) == 4
    assert callable(_lib.MarginalOps.model_rollout_cdf) and callable(_lib.MarginalOps.model_forecast_cdf)
    assert pgas_amd.model_rollout.STREAM_ROLLOUT_OBS == mrc.STREAM_OBS == 200 and pgas_amd.model_rollout.CDF_SLOTS == 64


# ---- 4. calibration_summary on a constructed grey-box CdfCounts -----------------------------------------------------------------------------
def test_calibration_summary_takes_a_grey_box_result_as_it_is():
    nx, ny, n, Kc, Tn = 3, 2, 8, 2, 4                        # the wide model's channels: PIT over the two predicted observations
    thr = torch.full((Tn, nx + ny, 1), NAN, dtype=torch.float64)
    thr[:, nx:, 0] = torch.tensor([[0.1, 0.2], [0.3, NAN], [0.5, 0.6], [0.7, 0.8]], dtype=torch.float64)
    count = torch.zeros((Kc, Tn, nx + ny, 1), dtype=torch.int32)
    count[0, :, nx:, 0] = torch.tensor([[1, 8], [2, 0], [3, 4], [8, 0]], dtype=torch.int32)
    count[1, :, nx:, 0] = torch.tensor([[3, 8], [2, 0], [5, 4], [8, 2]], dtype=torch.int32)
    s = pgas_amd.calibration_summary(pgas_amd.CdfCounts(n, count, thr, nx=nx, pit=True), levels=(0.5,))
    assert s["F"].shape == (Tn, nx + ny, 1) and s["pit"].shape == (Tn, ny)
    assert torch.equal(s["pit"], torch.tensor([[4, 16], [4, 0], [8, 8], [16, 2]], dtype=torch.float64) / 16.0)
    assert float(s["hist"].sum()) == 7.0                      # the NaN observation takes no part
    assert abs(float(s["coverage"][0.5]) - 2.0 / 7.0) <= 1e-15   # 0.25 < pit <= 0.75 holds the two 0.5 of the seven: 0.25 lies outside
    # a forecast result: a leading horizon axis, -1 becomes NaN
    fc = torch.full((Kc, 2, Tn, nx + ny, 1), 4, dtype=torch.int32)
    fc[:, 1, 0] = -1
    f = pgas_amd.calibration_summary(pgas_amd.CdfCounts(n, fc, thr, nx=nx, pit=True))
    assert f["pit"].shape == (2, Tn, ny) and f["ks"].shape == (2,) and bool(torch.isnan(f["pit"][1, 0]).all()) and float(f["hist"][1].sum()) == 5.0
    # J > 1: the pooled CDF and the bands
    grid = pgas_amd.threshold_grid(torch.zeros(Tn, nx + ny), torch.ones(Tn, nx + ny), 12)
    cnt = torch.arange(12, dtype=torch.int32).expand(Kc, Tn, nx + ny, 12).contiguous()
    q = pgas_amd.predictive_bands(pgas_amd.CdfCounts(11, cnt, grid, nx=nx), (0.5,))
    assert q.shape == (Tn, nx + ny, 1) and bool((q.abs() <= 8.0 / 11).all())


# ---- 5. the closed-form statistic of the GPU tests on the generator's own normals ------------------------------------------------------------
def test_closed_form_binomial_statistic_on_the_generators_normals():
    """The memoryless model with A = 0: x_t = sqrt(q) z_t (t >= 1) and yhat_t + e_t = x_t + sqrt(r) e_t are iid N(0, q) and N(0, q + r), so
    the count at sigma * TAUS pooled over draws, rows and replicates is Binomial(n, Phi(TAUS)).  Here the kernels' clouds are rebuilt on
    the CPU from oracle.canon.normals with the kernels' counters -- open loop: z on (PGAS_STREAM_M_STATE, t, p), e on (200, t, p);
    forecasts: lead 0 is the filter's own cloud z on (17, tau, i), lead l >= 1 z on (17, tau, l << 32 | i), e on (200, tau, (l + 1) << 32 | i)
    -- so the statistic shows the generator alone stays inside the project's bound |z| <= 4.
    Measured: open loop (K = 3, P = 4096, rows 1 .. 11, n = 135168) max |z| = 1.425 (x), 1.643 (yhat); forecasts (K = 3, N = 1024, H = 4,
    n = 125952) max |z| = 1.762 (x), 1.879 (yhat)."""
    sq, sr = np.sqrt(mc.MEM["q"]), np.sqrt(mc.MEM["r"])
    thr = mc.closed_thresholds(T)
    P, N, H = mc.CLOSED_P, mc.CLOSED_N, mc.CLOSED_H
    # ---- open loop
    cnt = np.zeros((K, T, 2, len(mc.TAUS)), dtype=np.int32)
    for k, key in enumerate(KEYS):
        x = np.stack([sq * canon.normals(key, canon.STREAM_M_STATE, t, 0, P, 1) for t in range(T)])    # row 0 stands in for x_0: not pooled
        e = np.stack([canon.normals(key, mrc.STREAM_OBS, t, 0, P, 1) for t in range(T)])
        cnt[k] = mrc.counts(np.concatenate([x, x + sr * e], axis=-1), thr)
    tot, rows = mc.pool_rollout(cnt)
    assert rows == K * (T - 1)
    za = mc.binomial_z(tot, rows * P)
    print(f"open loop: n = {rows * P}, max |z| x = {np.abs(za[0]).max():.3f}, yhat = {np.abs(za[1]).max():.3f}")
    assert (np.abs(za) <= 4.0).all()
    # ---- forecasts
    fc = np.full((K, H, T, 2, len(mc.TAUS)), -1, dtype=np.int32)
    for k, key in enumerate(KEYS):
        for lead in range(H):
            x = np.stack([sq * canon.normals(key, canon.STREAM_M_STATE, t, lead << 32, N, 1) for t in range(T)])
            e = np.stack([canon.normals(key, mrc.STREAM_OBS, t, (lead + 1) << 32, N, 1) for t in range(T)])
            c = mrc.counts(np.concatenate([x, x + sr * e], axis=-1), thr)
            fc[k, lead, lead:] = c[lead:]
    tot, rows = mc.pool_forecast(fc)
    assert rows == K * sum(T - max(h - 1, 1) for h in range(1, H + 1))
    zb = mc.binomial_z(tot, rows * N)
    print(f"forecasts: n = {rows * N}, max |z| x = {np.abs(zb[0]).max():.3f}, yhat = {np.abs(zb[1]).max():.3f}")
    assert (np.abs(zb) <= 4.0).all()
