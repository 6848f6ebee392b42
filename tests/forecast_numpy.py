"""NumPy restatement of pgas_forecast (csrc/pgas_forecast.hip.h) from the canonical oracle's primitives: the
h-step-ahead clouds of one draw (A, S, key) from a filter trace x (T, N, nx), origin by origin in the order of the definition.

    cloud        lead 0: row s of the trace.  lead l >= 1: the transition mean is the `aux` array of CanonModel.step(t = s + l, debug=True)
                 on a model of N + 1 particles (the cloud padded with its last row, rows 0 .. N - 1 kept: filter_numpy.run's trick), the
                 noise is canon.normals(key, STREAM_FORECAST, s + l, l << 32, N, nx) through the ascending fma chain of LS z
    channels     the state, then filter_numpy.predicted_obs (fma chain from +0.0, no measurement noise)
    moments      rollout_stats_numpy.moments: levels 1-2 of the defined summation order
    log score    filter_numpy.loglik per particle, rollout_stats_numpy.lpd with the library's exp and log (one block: N <= 1024)
    undefined    target rows tau < h - 1 have no origin row: NaN
"""
import numpy as np

import filter_numpy as fn
import rollout_stats_numpy as rs
from common import canon

STREAM_FORECAST = 7   # include/pgas_canon.h: PGAS_STREAM_FORECAST


def noise(key, t, lead, N, nx):
    """The normals of target row t at lead `lead` for particles 0 .. N - 1: the lead sits in the high word of the particle counter."""
    return canon.normals(key, STREAM_FORECAST, t, lead << 32, N, nx)


def run(cm1, N, key, A, S, lik, y, x, H, score=True):
    """cm1: the CanonModel of the problem with N + 1 particles; A (nx, M), S (nx, nx); lik: the GaussianLikelihood; y (T, ny) the
    observations the model was built with; x (T, N, nx) the filter's trace; H horizons -> dict of sum, sumsq (H, T, nx + ny), lpd (H, T)
    (None without score), cloud (H, T, N, nx) and l (H, T, N), at [h - 1, target row]; NaN where the target row is < h - 1."""
    T, nx = cm1.T, cm1.nx
    assert cm1.N == N + 1 and 1 <= H <= T
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    ny = y.shape[1]
    x = np.asarray(x, dtype=np.float64).reshape(T, N, nx)
    LS, LSinv, cS = cm1.chol_parts_dev(S)
    ref = np.zeros(nx)
    out = dict(sum=np.full((H, T, nx + ny), np.nan), sumsq=np.full((H, T, nx + ny), np.nan), cloud=np.full((H, T, N, nx), np.nan),
               l=np.full((H, T, N), np.nan), lpd=None)
    for s in range(T):
        c = x[s].copy()
        for lead in range(min(H, T - s)):
            t = s + lead
            if lead > 0:
                pad = np.concatenate([c, c[-1:]], axis=0)
                mean = cm1.step(t, key, pad, None, A, LS, LSinv, cS, ref, debug=True)[3]["aux"][:N]
                z = noise(key, t, lead, N, nx)
                c = np.empty((N, nx))
                for k in range(nx):
                    v = mean[:, k].copy()
                    for q in range(k + 1):
                        v = fn.fma(LS[k, q], z[:, q], v)
                    c[:, k] = v
            out["cloud"][lead, t] = c
            v = np.concatenate([c, fn.predicted_obs(c, lik.H)], axis=1)
            out["sum"][lead, t], out["sumsq"][lead, t] = rs.moments(v.T)
            if score:
                out["l"][lead, t] = fn.loglik(c, y[t], lik.H, lik.LRinv, lik.cR)
    if score:
        defined = np.arange(T)[None, :] >= np.arange(H)[:, None]
        with np.errstate(all="ignore"):
            # an undefined row holds NaN log-likelihoods, which take no part: its value is replaced below
            lpd = rs.lpd(out["l"], y, canon.det_exp, canon.det_log)
        out["lpd"] = np.where(defined, lpd, np.nan)
    return out


def float_lpd(cloud, lik, y):
    """A plain float64 log predictive density of the restatement's clouds (H, T, N, nx): logsumexp of the Gaussian log density - log N."""
    Hn, T, N, _ = cloud.shape
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    R = np.atleast_2d(lik.R)
    Rinv, ny = np.linalg.inv(R), R.shape[0]
    c = -0.5 * (ny * np.log(2 * np.pi) + np.linalg.slogdet(R)[1])
    out = np.full((Hn, T), np.nan)
    for h in range(Hn):
        for t in range(h, T):
            e = y[t][None, :] - cloud[h, t] @ np.atleast_2d(lik.H).T
            l = c - 0.5 * np.einsum("ij,jk,ik->i", e, Rinv, e)
            m = l.max()
            out[h, t] = m + np.log(np.exp(l - m).sum()) - np.log(N)
    return out
