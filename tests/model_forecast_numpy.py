"""NumPy restatement of what pgas_m_forecast (csrc/pgas_marginal_forecast.hip.h) computes DOWNSTREAM of the
h-step-ahead clouds: fed one draw's clouds cloud_x (H, T, N, nx) and cloud_y (H, T, N, ny) at [h - 1, target row], it restates steps 3 - 5
of the definition.

    moments      rollout_stats_numpy.moments of x_j and g_j (model_filter_numpy's order: lane-local ascending particle row, the balanced
                 adjacent-pair tree over 256 lanes -- wave_sum_tree and (w0 + w1) + (w2 + w3))
    log score    model_rollout_stats_numpy.loglik per particle (k_expr mode 2's operations), then the one-block logsumexp of
                 rollout_stats_numpy.lpd with the library's exp and log: (m + log S) - log N, -inf when S == 0, NaN where y_tau holds a NaN
    undefined    target rows tau < h - 1 have no origin row: NaN in every output

What the restatement cannot see -- that the clouds are the propagation of the filter's trace -- is checked against the per-step primitives
and against ModelRollout.__call__ in tests/test_gpu_model_forecast.py."""
import numpy as np

import model_rollout_stats_numpy as ms
import rollout_stats_numpy as rs
from common import canon


def defined(H, T):
    """(H, T) bool: target row tau has an origin row at horizon index h - 1."""
    return np.arange(T)[None, :] >= np.arange(H)[:, None]


def run(cloud_x, cloud_y, y, cR, LRinv, score=True):
    """One draw: cloud_x (H, T, N, nx), cloud_y (H, T, N, ny), y (T, ny) -> dict of sum, sumsq (H, T, nx + ny), l (H, T, N), lpd (H, T)
    (None without score)."""
    cx, cy = np.asarray(cloud_x, dtype=np.float64), np.asarray(cloud_y, dtype=np.float64)
    H, T, N, _ = cx.shape
    assert N <= rs.BLOCK and cy.shape[:3] == (H, T, N)
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    ok = defined(H, T)
    v = np.concatenate([cx, cy], axis=-1)                     # (H, T, N, nv)
    with np.errstate(all="ignore"):
        s1, s2 = rs.moments(np.moveaxis(v, 2, 3))                # over the particles
    out = dict(sum=np.where(ok[..., None], s1, np.nan), sumsq=np.where(ok[..., None], s2, np.nan), l=None, lpd=None)
    if score:
        with np.errstate(all="ignore"):
            l = ms.loglik(cy, y[None, :, None, :], LRinv, cR)    # (H, T, N)
            lpd = rs.lpd(l, y, canon.det_exp, canon.det_log)     # an undefined row's NaN log-densities take no part: replaced below
        out["l"], out["lpd"] = np.where(ok[..., None], l, np.nan), np.where(ok, lpd, np.nan)
    return out


def float_lpd(cloud_y, y, R):
    """A plain float64 log predictive density of the clouds' outputs (H, T, N, ny): logsumexp of the Gaussian log density - log N."""
    cy = np.asarray(cloud_y, dtype=np.float64)
    H, T, N, ny = cy.shape
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    Rinv = np.linalg.inv(R)
    c = -0.5 * (ny * np.log(2 * np.pi) + np.linalg.slogdet(R)[1])
    out = np.full((H, T), np.nan)
    for h in range(H):
        for t in range(h, T):
            e = y[t][None, :] - cy[h, t]
            l = c - 0.5 * np.einsum("ij,jk,ik->i", e, Rinv, e)
            m = l.max()
            out[h, t] = m + np.log(np.exp(l - m).sum()) - np.log(N)
    return out


def clouds(step, output, x, H):
    """The clouds of the definition from a trace x (T, N, nx) by plain callables: step(t, lead, c) -> the cloud of row t + 1 at that lead
    (noise included) from the cloud c of row t; output(t, lead, c) -> g (N, ny) -> cloud_x (H, T, N, nx), cloud_y (H, T, N, ny)."""
    x = np.asarray(x, dtype=np.float64)
    T, N, nx = x.shape
    cx, cy = np.full((H, T, N, nx), np.nan), None
    for s in range(T):
        c = x[s].copy()
        for lead in range(min(H, T - s)):
            t = s + lead
            if lead > 0:
                c = np.asarray(step(t - 1, lead, c), dtype=np.float64).reshape(N, nx)
            g = np.asarray(output(t, lead, c), dtype=np.float64).reshape(N, -1)
            if cy is None:
                cy = np.full((H, T, N, g.shape[1]), np.nan)
            cx[lead, t], cy[lead, t] = c, g
    return cx, cy


def kalman_forecast_logpdf(a, q, r, m0, p0, y, H):
    """x_0 ~ N(m0, p0), x' = a x + N(0, q), y = x + N(0, r): out[h - 1, tau] = log p(y_tau | y_{0:tau-h}) for h = 1 .. H, NaN where
    tau < h - 1 -- the scalar Kalman filter's prediction of row s propagated h - 1 more steps without an update."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    T = len(y)
    out = np.full((H, T), np.nan)
    m, p = float(m0), float(p0)
    for s in range(T):
        mm, pp = m, p                                  # p(x_s | y_{0:s-1})
        for lead in range(min(H, T - s)):
            if lead > 0:
                mm, pp = a * mm, a * a * pp + q
            sv = pp + r
            out[lead, s + lead] = -0.5 * (np.log(2 * np.pi * sv) + (y[s + lead] - mm) ** 2 / sv)
        k = p / (p + r)
        m, p = m + k * (y[s] - m), (1 - k) * p
        m, p = a * m, a * a * p + q
    return out
