"""NumPy restatement of the counts of pgas_rollout_cdf and pgas_forecast_cdf (csrc/pgas_rollout_cdf.hip.h, csrc/pgas_forecast_cdf.hip.h,
DESIGN.md section 19) from clouds: count[..., c, j] = (v_c <= thr[t, c, j]).sum over the replicate (particle) axis, the IEEE comparison,
so a NaN on either side counts nothing.  Value channels: the state, then rollout_stats_numpy.predicted_obs (the exactly rounded fma
chain, with the measurement noise LR e when asked for).  The noise is oracle.canon.normals(key, 6, t, offset, P, ny): offset p0 for the
open loop, (lead + 1) << 32 for the forecasts.  Counts are integers: there is no order to restate."""
import numpy as np

import rollout_stats_numpy as rs
from common import canon

STREAM_OBS = 6   # include/pgas_canon.h: PGAS_STREAM_OBS


def counts(v, thr):
    """v (..., T, P, C) values, thr (T, C, J) -> (..., T, C, J) int32."""
    v, thr = np.asarray(v, dtype=np.float64), np.asarray(thr, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        le = v[..., :, :, :, None] <= thr[:, None, :, :]   # (..., T, P, C, J)
    return le.sum(axis=-3).astype(np.int32)


def channels(cloud, H, LR=None, e=None):
    """cloud (..., P, nx) -> (..., P, nx + ny): the state, then yhat = H x (+ LR e, e (..., P, ny)).  Under a 0/1 selector H the chain
    sum_k H[j,k] x_k adds one exact product to zeros, so x @ H.T is its value (up to the sign of a zero, which no comparison sees) and
    only the noise chain goes through the exactly rounded fma."""
    H = np.atleast_2d(np.asarray(H, dtype=np.float64))
    if not (np.all((H == 0) | (H == 1)) and np.all(H.sum(axis=1) == 1)):
        return np.concatenate([cloud, rs.predicted_obs(cloud, H, LR, e)], axis=-1)
    with np.errstate(invalid="ignore"):
        yh = np.stack([cloud[..., int(np.argmax(H[j]))] + 0.0 for j in range(H.shape[0])], axis=-1)
    if LR is not None:
        for j in range(H.shape[0]):
            acc = yh[..., j]
            for l in range(j + 1):
                acc = np.asarray(rs.fma(LR[j, l], e[..., l], acc), dtype=np.float64)
            yh[..., j] = acc
    return np.concatenate([cloud, yh], axis=-1)


def obs_normals(keys, T, p0, P, ny):
    """e (K, T, P, ny) of the open loop: replicate p0 + p at row t."""
    return np.stack([np.stack([canon.normals(int(k), STREAM_OBS, t, p0, P, ny) for t in range(T)]) for k in keys])


def rollout_counts(cloud, lik, thr, keys=None, p0=0):
    """cloud (K, T, P, nx) as Rollout.__call__ returns it (replicates p0 .. p0 + P - 1), thr (T, nx + ny, J) -> (K, T, nx + ny, J).
    keys: the draws' keys when measurement noise is on, None for none."""
    K, T, P, _ = cloud.shape
    e = None if keys is None else obs_normals(keys, T, p0, P, lik.ny)
    return counts(channels(cloud, lik.H, None if keys is None else lik.LR, e), thr)


def forecast_counts(cloud, lik, thr, key=None):
    """cloud (H, T, N, nx) of one draw as forecast_numpy.run returns it (NaN where the target row is < h - 1), thr (T, nx + ny, J) ->
    (H, T, nx + ny, J) with -1 at the undefined entries.  key: the draw's key when measurement noise is on (particle offset (lead + 1) << 32)."""
    Hn, T, N, _ = cloud.shape
    e = None
    if key is not None:
        e = np.stack([np.stack([canon.normals(int(key), STREAM_OBS, t, (lead + 1) << 32, N, lik.ny) for t in range(T)]) for lead in range(Hn)])
    out = counts(channels(cloud, lik.H, None if key is None else lik.LR, e), thr)
    defined = np.arange(T)[None, :] >= np.arange(Hn)[:, None]
    return np.where(defined[:, :, None, None], out, np.int32(-1)).astype(np.int32)
