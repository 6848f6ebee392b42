"""NumPy restatement of the counts of pgas_m_rollout_cdf and pgas_m_forecast_cdf (csrc/pgas_marginal_rollout_cdf.hip.h,
csrc/pgas_marginal_forecast_cdf.hip.h) from given clouds: count[..., c, j] = (v_c <= thr[t, c, j]).sum over the
replicate (particle) axis, the IEEE comparison, so a NaN on either side counts nothing.  Value channels: the state x, then yhat = g, with
observation noise g continued by the exactly rounded fma chain acc = fma(LR[j,l], e_l, acc), l = 0 .. j
(model_rollout_stats_numpy.predicted_obs, on rollout_stats_numpy.fma).  The forecasts' entries without an origin row
(model_forecast_numpy.defined) are -1.  Counts are integers: there is no order to restate.

Where the normals e come from is the caller's business: PGAS_STREAM_M_ROLLOUT_OBS = 200 at the (target) row, particle p0 + p for the open
loop and (lead + 1) << 32 | i for the forecasts."""
import numpy as np

import model_forecast_numpy as mfc
import model_rollout_stats_numpy as ms

STREAM_OBS = 200   # include/pgas_marginal.h: PGAS_STREAM_M_ROLLOUT_OBS


def counts(v, thr):
    """v (..., T, P, C) values, thr (T, C, J) -> (..., T, C, J) int32."""
    v, thr = np.asarray(v, dtype=np.float64), np.asarray(thr, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        le = v[..., :, :, :, None] <= thr[:, None, :, :]   # (..., T, P, C, J)
    return le.sum(axis=-3).astype(np.int32)


def channels(x, g, LR=None, e=None):
    """x (..., P, nx), g (..., P, ny) -> (..., P, nx + ny): the state, then yhat = g (+ LR e through the fma chain, e (..., P, ny))."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        yh = ms.predicted_obs(g, None if LR is None else np.asarray(LR, dtype=np.float64), e)
    return np.concatenate([x, yh], axis=-1)


def rollout_counts(x, g, thr, LR=None, e=None):
    """Clouds x (K, T, P, nx), g (K, T, P, ny) as ModelRollout.__call__(outputs=True) returns them, thr (T, nx + ny, J) ->
    (K, T, nx + ny, J).  LR, e (K, T, P, ny): the observation noise, or None for none."""
    return counts(channels(x, g, LR, e), thr)


def forecast_counts(cloud_x, cloud_y, thr, LR=None, e=None):
    """Clouds (..., H, T, N, nx) and (..., H, T, N, ny) as ModelRollout.forecast(clouds=True) returns them (NaN where the target row is
    < h - 1), thr (T, nx + ny, J) -> (..., H, T, nx + ny, J) with -1 at the undefined entries.  LR, e (..., H, T, N, ny) or None."""
    cx = np.asarray(cloud_x, dtype=np.float64)
    Hn, T = cx.shape[-4], cx.shape[-3]
    out = counts(channels(cx, cloud_y, LR, e), thr)
    ok = mfc.defined(Hn, T)
    return np.where(ok[:, :, None, None], out, np.int32(-1)).astype(np.int32)
