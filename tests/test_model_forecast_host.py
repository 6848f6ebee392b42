"""Host side of the grey-box h-step-ahead forecast (pgas_amd.ModelRollout.forecast, pgas_m_forecast), no GPU: the
NumPy restatement (tests/model_forecast_numpy.py) on the clouds of a plain NumPy filter and forecast against a plain float64 log
predictive density, every refusal of ``check_forecast`` before a device is touched, the C ABI binding, forecast_summary on a hand-built
ModelForecastResult, and the closed-form statistic of tests/test_gpu_model_forecast.py evaluated on the CPU with the device's normals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import model_filter_cases as cases
import model_filter_numpy as mf
import model_forecast_numpy as mfc
import model_rollout_numpy as mrn
import model_rollout_stats_numpy as ms
from common import ROOT, canon, pgas_amd
from test_model_filter_host import _numpy_filter
from test_model_rollout_stats_host import _c_struct_layout

K, T, H = cases.K, cases.T, 4


def _noise_parts(R):
    LR = np.linalg.cholesky(R)
    return np.linalg.inv(LR), -0.5 * R.shape[0] * np.log(2 * np.pi) - np.sum(np.log(np.diag(LR)))


def _numpy_clouds(name, k, N, seed):
    """A plain NumPy bootstrap filter of draw k on the model's record, then the clouds of the definition with NumPy's own normals."""
    res, y = _numpy_filter(name, k, N, seed=seed)
    pb, _, R = cases.problem(name)
    lat, model = [mrn.Latent(b) for b in pb.basis], pb.model(np)
    A = [a[k] for a in cases.coeffs(pb)]
    u = np.asarray(pb.inputs[:T], dtype=np.float64).reshape(T, -1)
    nx = res["x"].shape[2]
    Qc = np.linalg.cholesky(pb.process_noise) if np.any(pb.process_noise) else None
    rng = np.random.default_rng(seed + 1)
    cx, cy = mfc.clouds(lambda t, lead, c: mrn.step(model, lat, A, c, u[t], rng.standard_normal((N, nx)) if Qc is not None else None, Qc)[2],
                        lambda t, lead, c: mrn.step(model, lat, A, c, u[t])[1], res["x"], H)
    return res, cx, cy, y, R


def _float_lse(l):
    m = l.max(axis=-1)
    return m + np.log(np.exp(l - m[..., None]).sum(axis=-1)) - np.log(l.shape[-1])


# ---- 1. the restatement on the clouds of a plain filter and forecast -----------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 200, 257, 1024])
@pytest.mark.parametrize("name", ["smo", "toy"])
def test_restatement_on_the_clouds_of_a_numpy_forecast(name, N):
    res, cx, cy, y, R = _numpy_clouds(name, 0, N, seed=N)
    LRinv, cR = _noise_parts(R)
    got = mfc.run(cx, cy, y, cR, LRinv)
    nv = cx.shape[3] + cy.shape[3]
    assert got["sum"].shape == got["sumsq"].shape == (H, T, nv) and got["lpd"].shape == (H, T) and got["l"].shape == (H, T, N)
    assert np.array_equal(cx[0], res["x"]) and np.array_equal(cy[0], res["yhat"])          # lead 0 is the filter's own cloud
    pred = mf.run(7, res["lw"], res["x"], res["yhat"], y)
    assert np.array_equal(got["sum"][0], pred["pred_sum"]) and np.array_equal(got["sumsq"][0], pred["pred_sumsq"])
    assert np.abs(got["lpd"][0] - pred["ell"]).max() <= 1e-12                              # logsumexp against the fixed-point increment
    plain = mfc.float_lpd(cy, y, R)
    v = np.concatenate([cx, cy], axis=-1)
    for h in range(H):
        d = slice(h, T)
        assert np.isfinite(got["lpd"][h, d]).all() and np.isfinite(got["sum"][h, d]).all() and np.isfinite(got["sumsq"][h, d]).all()
        assert np.abs(got["lpd"][h, d] - _float_lse(got["l"][h, d])).max() <= 1e-12       # a float64 logsumexp - log N on the same densities
        assert np.abs(got["lpd"][h, d] - plain[h, d]).max() <= 1e-9 * max(1.0, np.abs(plain[h, d]).max())   # mode 2's operations ARE the density
        assert np.isnan(got["lpd"][h, :h]).all() and np.isnan(got["sum"][h, :h]).all() and np.isnan(got["sumsq"][h, :h]).all()
        assert np.isnan(got["l"][h, :h]).all()
        assert np.allclose(got["sum"][h, d], v[h, d].sum(axis=1), rtol=1e-12, atol=1e-300)
        assert np.allclose(got["sumsq"][h, d], (v[h, d] ** 2).sum(axis=1), rtol=1e-12, atol=1e-300)
    if N >= 200 and name == "smo":   # the clouds of different horizons for the same target row differ
        assert not np.array_equal(cx[1, 5], cx[2, 5])
    bare = mfc.run(cx[:2], cy[:2], y, cR, LRinv, score=False)
    assert bare["lpd"] is None and np.array_equal(bare["sum"], got["sum"][:2], equal_nan=True) and np.array_equal(bare["sumsq"], got["sumsq"][:2], equal_nan=True)


def test_restatement_nan_row_and_outlier_row():
    res, cx, cy, y, R = _numpy_clouds("toy", 0, 65, seed=3)
    y = y.copy()
    y[5], y[9] = np.nan, 1e200
    LRinv, cR = _noise_parts(R)
    got = mfc.run(cx, cy, y, cR, LRinv)
    for h in range(H):
        assert np.isnan(got["lpd"][h, 5]) and got["lpd"][h, 9] == -np.inf
        rest = [t for t in range(h, T) if t not in (5, 9)]
        assert np.isfinite(got["lpd"][h, rest]).all() and np.isfinite(got["sum"][h, h:]).all() and np.isfinite(got["sumsq"][h, h:]).all()
        assert np.isnan(got["l"][h, 5]).all() and (got["l"][h, 9] == -np.inf).all()


# ---- 2. every refusal of check_forecast is a ValueError before a device is touched ---------------------------------------------------------
def test_every_forecast_refusal_is_raised_without_a_device():
    pb, ssm, sim = cases.rollout("smo")
    A = cases.coeffs(pb)
    keys, x0, N = [1, 2, 3], np.zeros(2), 70
    assert sim.check_forecast(A, keys, N, 1) == (3, N, 0, True, False, 1)
    assert sim.check_forecast(A, keys, sim.max_particles(), np.int64(T), x0) == (3, sim.max_particles(), 1, True, False, T)
    assert sim.check_forecast(A, torch.zeros(3, dtype=torch.int64), N, 3, np.zeros((3, N, 2)), process_noise=False) == (3, N, 3, False, False, 3)
    assert sim.check_forecast(A, keys, N, 2, x0, row_cov=[np.stack([np.eye(1)] * 3)], process_noise=False) == (3, N, 1, False, True, 2)
    bad = [
        (dict(horizon=0), "horizon"),
        (dict(horizon=-1), "horizon"),
        (dict(horizon=T + 1), "horizon"),
        (dict(horizon=2.0), "horizon"),
        (dict(horizon=None), "horizon"),
        (dict(horizon=True), "horizon"),
        (dict(particles=0), "particles"),
        (dict(particles=sim.max_particles() + 1), "particles"),
        (dict(particles=1025), "particles"),
        (dict(keys=None), "keys"),
        (dict(keys=[1, 2]), "expected 3 keys"),
        (dict(keys=torch.zeros(3, dtype=torch.int32)), "keys"),
        (dict(coeffs=A[0]), "list of 1"),
        (dict(coeffs=[A[0][:, :, :-1]]), r"coeffs\[0\]"),
        (dict(init_state=np.zeros((3, N + 1, 2))), "init_state"),
        (dict(init_state=np.zeros(3)), "init_state"),
        (dict(row_cov=[np.zeros((3, 2, 2))]), r"row_cov\[0\]"),
        (dict(init_state=x0, process_noise=False), "copies"),
        (dict(init_state=np.zeros((3, 2)), process_noise=False), "copies"),
    ]
    for kw, msg in bad:
        args = dict(coeffs=A, keys=keys, particles=N, horizon=H)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            sim.check_forecast(**args)
        with pytest.raises(ValueError, match=msg):
            sim.forecast(**args)
    _, _, bare = cases.rollout("smo", has_obs=False)
    with pytest.raises(ValueError, match="needs observations"):
        bare.forecast(A, keys, N, H)
    wide = pgas_amd.SymbolicStateSpaceModel(pb.process_noise, np.diag([1e-3, 1e-3]), pb.model)   # ny = 1 under a 2 x 2 output noise
    odd = pgas_amd.ModelRollout(pb.inputs[:T], wide, pb.basis, pb.init_state_mean, pb.init_state_cov, observations=pb.observations[:T])
    with pytest.raises(ValueError, match="output_noise"):
        odd.forecast(A, keys, N, H)
    noinit = pgas_amd.ModelRollout(pb.inputs[:T], ssm, pb.basis, observations=pb.observations[:T])
    with pytest.raises(ValueError, match="construct the ModelRollout with both"):
        noinit.forecast(A, keys, N, H)
    for s in (sim, bare, odd, noinit):
        assert s._ops is None and s._dev_cache is None, "a refused call created the device context"


# ---- 3. C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_forecast_is_declared_and_bound_and_the_ctypes_struct_is_the_c_struct():
    from pgas_amd import _lib

    txt = open(os.path.join(ROOT, "include", "pgas_marginal.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+pgas_m_forecast\s*\(([^)]*)\)\s*;", txt)
    assert m, "pgas_m_forecast is not declared in include/pgas_marginal.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 4 and "pgas_m_rollout_desc" in params[1] and "pgas_m_forecast_desc" in params[2]
    assert re.search(r"\bint\s+pgas_m_forecast_origins_per_block\s*\(\s*void\s*\)\s*;", txt)
    fields, size = _c_struct_layout(txt, "pgas_m_forecast_desc")
    S = _lib.ModelForecastDesc
    assert C.sizeof(S) == size == 7 * 8 + 8 + 8 + 64 * 8
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == fields
    assert [n for n, _ in S._fields_] == ["x_dev", "y_dev", "sum_dev", "sumsq_dev", "lpd_dev", "cloud_x_dev", "cloud_y_dev", "H", "reserved", "cR", "LRinv"]
    assert "pgas_m_forecast" in _lib.EXPORTS and "pgas_m_forecast_origins_per_block" in _lib.EXPORTS
    L = _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "pgas_m_forecast") and hasattr(lib, "pgas_m_forecast_origins_per_block")
    assert L.pgas_m_forecast.restype is C.c_int and len(L.pgas_m_forecast.argtypes) == 4
    assert 1 <= L.pgas_m_forecast_origins_per_block() <= 64                                  # no device is needed to ask
    assert callable(_lib.MarginalOps.model_forecast)
    R = pgas_amd.ModelForecastResult
    assert issubclass(R, pgas_amd.ForecastResult) and R is pgas_amd.model_rollout.ModelForecastResult


# ---- 4. forecast_summary on a hand-built ModelForecastResult --------------------------------------------------------------------------------
def test_forecast_summary_works_on_a_model_forecast_result():
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    nan = float("nan")
    # K = 2 draws, n = 2 particles, H = 2, T = 3, nx = 1, ny = 1 with g = 2 x.  Clouds of x at h = 1: {1, 3}, {5, 7} | {0, 0}, {2, 2} |
    # {1, 1}, {1, 1}; at h = 2 (row 0 undefined): {0, 2}, {2, 4} | {3, 3}, {3, 3}
    cx = t([[[[nan, nan], [nan, nan], [nan, nan]]] * 2] * 2).reshape(2, 2, 3, 2, 1)
    cx[0, 0, :, :, 0] = t([[1.0, 3.0], [0.0, 0.0], [1.0, 1.0]])
    cx[1, 0, :, :, 0] = t([[5.0, 7.0], [2.0, 2.0], [1.0, 1.0]])
    cx[0, 1, 1:, :, 0] = t([[0.0, 2.0], [3.0, 3.0]])
    cx[1, 1, 1:, :, 0] = t([[2.0, 4.0], [3.0, 3.0]])
    cy = 2.0 * cx
    v = torch.cat([cx, cy], dim=-1)
    s1, s2 = v.sum(dim=3), (v * v).sum(dim=3)
    lpd = t([[[np.log(0.2), np.log(0.1), nan], [nan, np.log(0.3), nan]],
             [[np.log(0.6), np.log(0.3), nan], [nan, np.log(0.5), nan]]])
    flt = pgas_amd.ModelFilterResult(2, 1, loglik=t([0.0, 0.0]), ell=lpd[:, 0])
    res = pgas_amd.ModelForecastResult(flt, 2, s1, s2, lpd, cx, cy)
    assert res.n == 2 and res.nx == 1 and res.horizon == 2 and res.cloud_x is cx and res.cloud_y is cy and res.filter is flt
    out = pgas_amd.forecast_summary(res, y=np.array([10.0, 4.0, np.nan]))
    assert out["y_pred_mean"].shape == (2, 3, 1) and out["x_pred_mean"].shape == (2, 3, 1) and out["log_score"].shape == (2,)
    assert np.array_equal(out["x_pred_mean"].numpy()[0], [[4.0], [1.0], [1.0]]) and np.array_equal(out["y_pred_mean"].numpy()[0], [[8.0], [2.0], [2.0]])
    assert np.array_equal(out["y_pred_mean"].numpy()[1], [[nan], [4.0], [6.0]], equal_nan=True)
    assert np.allclose(out["x_pred_std"].numpy()[0], [[np.sqrt(5.0)], [1.0], [0.0]], rtol=1e-15)
    assert np.allclose(out["y_pred_std"].numpy()[1, 1:], [[2.0 * np.sqrt(2.0)], [0.0]], rtol=1e-15) and np.isnan(out["y_pred_std"].numpy()[1, 0])
    want = [0.5 * (np.log(0.4) + np.log(0.2)), np.log(0.4)]   # h = 1 over rows 0, 1 (row 2 holds a NaN observation), h = 2 over row 1
    assert np.allclose(out["log_score"].numpy(), want, rtol=0, atol=1e-15)
    assert np.array_equal(out["rmse"].numpy(), [2.0, 0.0])   # h = 1 over rows 0, 1: errors -2, -2; h = 2 over row 1: error 0
    bare = pgas_amd.ModelForecastResult(flt, 2, s1, s2)
    assert bare.lpd is None and bare.cloud_x is None and bare.cloud_y is None
    assert set(pgas_amd.forecast_summary(bare)) == {"x_pred_mean", "x_pred_std", "y_pred_mean", "y_pred_std"}


# ---- 5. the closed-form statistic of the device test, on the CPU ---------------------------------------------------------------------------
# 16 fixed keys.  Chosen so that the CPU statistic below has |z| <= 3 at every h (DESIGN.md section 18 lists the z values): the estimate
# is the log of an unbiased one, so z sits near -0.9 on average and the bound of 4 is not idle.
CLOSED_FORM_KEYS = [500 + 13 * s for s in range(cases.KAL["seeds"])]


def closed_form_z(lpd, y, what):
    """lpd (16, H, T) -> z (H + 1,) for h = 2 .. H: (mean_k sum_{tau >= h - 1} lpd[k, h - 1, tau] - Kalman) / (std_k / sqrt(16))."""
    kal = cases.KAL
    want = mfc.kalman_forecast_logpdf(kal["a"], kal["q"], kal["r"], kal["m0"], kal["p0"], y, H)
    z = np.full(H + 1, np.nan)
    for h in range(2, H + 1):
        tot = lpd[:, h - 1, h - 1:].sum(axis=1)
        assert np.isfinite(tot).all() and len(np.unique(tot)) == len(tot)
        se = tot.std() / np.sqrt(len(tot))
        ref = want[h - 1, h - 1:].sum()
        z[h] = (tot.mean() - ref) / se
        print(f"{what}: h = {h}, Kalman {ref:.6f}, mean {tot.mean():.6f}, std {tot.std():.6f}, z = {z[h]:.3f}")
    return z


def kalman_cpu_lpd(key):
    """The device's filter and forecast of the Kalman model under `key` in plain NumPy on the device's very normals: x_0 on
    STREAM_M_INIT_STATE, the filter's process noise on (STREAM_M_STATE, t + 1, particle i), the canonical scan's ancestors, and the
    forecast's noise on (STREAM_M_STATE, tau, lead << 32 | i).  A = 0, so xi = 0 exactly."""
    kal = cases.KAL
    Tn, N = kal["T"], kal["N"]
    y = cases.kalman_record().reshape(-1, 1)
    R = np.array([[kal["r"]]])
    LRinv, cR = _noise_parts(R)
    sq = np.sqrt(kal["q"])

    def resample(t, l):
        segm, segs, c = canon.segment_partials(l)
        return canon.resample_range(segm, segs, c, N, canon.uniform(key, canon.STREAM_M_RESAMPLE, t), 0, N)

    x0 = kal["m0"] + np.sqrt(kal["p0"]) * canon.normals(key, canon.STREAM_M_INIT_STATE, 0, 0, N, 1)
    flt = mf.bootstrap(lambda t, x: kal["a"] * x + canon.normals(key, canon.STREAM_M_STATE, t + 1, 0, N, 1) * sq, lambda t, x: x, x0, y, R, None,
                       resample, lambda yh, yt: ms.loglik(yh, yt[None, :], LRinv, cR))
    cx, cy = mfc.clouds(lambda t, lead, c: kal["a"] * c + canon.normals(key, canon.STREAM_M_STATE, t + 1, lead << 32, N, 1) * sq,
                        lambda t, lead, c: c, flt["x"], H)
    return mfc.run(cx, cy, y, cR, LRinv)["lpd"], flt


def test_kalman_forecast_logpdf_is_the_kalman_filter_at_h_1_and_the_stationary_law_far_out():
    kal = cases.KAL
    y = cases.kalman_record()
    want = mfc.kalman_forecast_logpdf(kal["a"], kal["q"], kal["r"], kal["m0"], kal["p0"], y, kal["T"])
    assert want[0].sum() == pytest.approx(mf.kalman_loglik(kal["a"], kal["q"], kal["r"], kal["m0"], kal["p0"], y), abs=1e-10)
    # from origin 0 the h-step law is N(a^l m0, a^2l p0 + q (1 - a^2l) / (1 - a^2) + r)
    for lead in (1, 5, 19):
        a2 = kal["a"] ** (2 * lead)
        sv = a2 * kal["p0"] + kal["q"] * (1 - a2) / (1 - kal["a"] ** 2) + kal["r"]
        assert want[lead, lead] == pytest.approx(-0.5 * (np.log(2 * np.pi * sv) + (y[lead] - kal["a"] ** lead * kal["m0"]) ** 2 / sv), abs=1e-12)


def test_closed_form_statistic_on_the_cpu():
    """The figures the device test reproduces up to rounding: the same normals, the same ancestors' scan, plain NumPy arithmetic."""
    y = cases.kalman_record()
    runs = [kalman_cpu_lpd(key) for key in CLOSED_FORM_KEYS]
    lpd = np.stack([r[0] for r in runs])
    assert np.abs(lpd[:, 0] - np.stack([r[1]["ell"] for r in runs])).max() <= 1e-12      # horizon 1 is the filter's increment
    z = closed_form_z(lpd, y, "cpu")
    assert (np.abs(z[2:]) <= 3.0).all()
