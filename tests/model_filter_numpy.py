"""NumPy restatement of what pgas_m_filter (csrc/pgas_marginal_filter.hip.h) computes DOWNSTREAM of the particles'
log-likelihoods: fed one draw's own traces lw (T, N), x (T, N, nx) and yhat (T, N, ny), it restates everything else the kernel returns.

    predictive   rollout_stats_numpy.moments of x_j and yhat_j over the unweighted cloud (lane-local ascending particle row, the
                 balanced adjacent-pair tree over 256 lanes -- wave_sum_tree and (w0 + w1) + (w2 + w3))
    scan         canon.segment_partials: k = ceil(max l log2 e), integer cumsum c, total s; S = double(s) 2^-51
    ell          filter_numpy.ell_from_scan: fma(k, LN2_LO, fma(k, LN2_HI, log S)) - log N; -inf when S == 0; NaN when y_t holds a NaN
    filtered     w_i = q_i 2^-51, sum (w_i x_ij) and sum (w_i w_i) in the order of the predictive sums; ess = (S S) / sum w w, 0 if not valid
    resampling   canon.resample_range with canon.uniform(key, STREAM_M_RESAMPLE, t): the identity when S is not in (0, inf)
    loglik       sum_t ell, ascending t from +0.0, over the rows whose y_t holds no NaN

What the restatement cannot see -- that x_{t+1}[i] descends from particle anc_t[i], that lw and yhat belong to x -- is checked against the
per-step primitives in tests/test_gpu_model_filter.py."""
import numpy as np

import filter_numpy as fn
import rollout_stats_numpy as rs
from common import canon

FIX_INV = 2.0 ** -51


def run(key, lw, x, yhat, y):
    """One draw: key, lw (T, N), x (T, N, nx), yhat (T, N, ny), y (T, ny) -> dict of anc (T, N) int32, ell, ess, wtot (T), pred_sum,
    pred_sumsq (T, nx + ny), filt_sum (T, nx), loglik."""
    lw, x, yhat = (np.asarray(a, dtype=np.float64) for a in (lw, x, yhat))
    T, N, nx = x.shape
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    ny = yhat.shape[2]
    u64 = canon.lib().oc_u64_to_double
    out = dict(anc=np.empty((T, N), np.int32), ell=np.empty(T), ess=np.empty(T), wtot=np.empty(T), pred_sum=np.empty((T, nx + ny)),
               pred_sumsq=np.empty((T, nx + ny)), filt_sum=np.empty((T, nx)))
    total = 0.0
    for t in range(T):
        v = np.concatenate([x[t], yhat[t]], axis=1)
        out["pred_sum"][t], out["pred_sumsq"][t] = rs.moments(v.T)
        segm, segs, c = canon.segment_partials(lw[t])
        kref, S = float(segm[0]), float(u64(int(segs[0]))) * FIX_INV
        valid = 0.0 < S < np.inf
        ynan = bool(np.isnan(y[t]).any())
        ell = np.nan if ynan else fn.ell_from_scan(kref, S, N)
        out["ell"][t] = ell
        if not ynan:
            total = total + ell
        q = np.diff(np.concatenate([np.zeros(1, np.uint64), c]))
        w = q.astype(np.float64) * FIX_INV   # q <= 2^51: exact
        out["wtot"][t] = S
        out["filt_sum"][t] = rs.reduce_sum((w[:, None] * x[t]).T)
        sw = float(rs.reduce_sum(w * w))
        out["ess"][t] = (S * S) / sw if valid else 0.0
        out["anc"][t] = canon.resample_range(segm, segs, c, N, canon.uniform(key, canon.STREAM_M_RESAMPLE, t), 0, N)
    out["loglik"] = total
    return out


def float_filter(lw, x):
    """A plain float64 bootstrap filter on the same particles and log-likelihoods: per step logsumexp(l) - log N, the self-normalised
    filtered mean and 1 / sum W^2 -> (ell (T), mean (T, nx), ess (T))."""
    lw, x = np.asarray(lw, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T, N, nx = x.shape
    ell, mean, ess = np.empty(T), np.empty((T, nx)), np.empty(T)
    for t in range(T):
        m = lw[t].max()
        p = np.exp(lw[t] - m)
        ell[t] = m + np.log(p.sum()) - np.log(N)
        W = p / p.sum()
        mean[t] = W @ x[t]
        ess[t] = 1.0 / np.sum(W * W)
    return ell, mean, ess


def gauss_loglik(yhat, y, R):
    """Plain float64 Gaussian log-density of y (ny,) at means yhat (..., ny) under covariance R."""
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    e = np.asarray(y, dtype=np.float64) - np.asarray(yhat, dtype=np.float64)
    return -0.5 * (R.shape[0] * np.log(2 * np.pi) + np.linalg.slogdet(R)[1]) - 0.5 * np.einsum("...j,jk,...k->...", e, np.linalg.inv(R), e)


def bootstrap(step, output, x0, y, R, uniforms, resample=None, loglik=None):
    """A plain NumPy bootstrap filter resampling at every step: x0 (N, nx); step(t, x) -> x_{t+1} (noise included); output(t, x) ->
    yhat (N, ny); systematic resampling with uniforms[t], or resample(t, l) -> ancestors; loglik(yhat, y_t) replaces the plain Gaussian
    log-density -> dict of x, yhat, lw, anc, ell (T), loglik."""
    x = np.array(x0, dtype=np.float64)
    N, T = x.shape[0], len(y)
    out = dict(x=[], yhat=[], lw=[], anc=[], ell=[])
    for t in range(T):
        yh = np.asarray(output(t, x), dtype=np.float64).reshape(N, -1)
        l = gauss_loglik(yh, y[t], R) if loglik is None else loglik(yh, y[t])
        m = l.max()
        p = np.exp(l - m)
        W = p / p.sum()
        if resample is not None:
            a = np.asarray(resample(t, l))
        else:
            a = np.minimum(np.searchsorted(np.cumsum(W), (uniforms[t] + np.arange(N)) / N, side="left"), N - 1)
        for k, v in zip(("x", "yhat", "lw", "anc", "ell"), (x, yh, l, a, m + np.log(p.sum()) - np.log(N))):
            out[k].append(v)
        if t < T - 1:
            x = step(t, x[a])
    out = {k: np.array(v) for k, v in out.items()}
    out["loglik"] = float(out["ell"].sum())
    return out


def kalman_loglik(a, q, r, m0, p0, y):
    """log p(y_0 .. y_T-1) of x_0 ~ N(m0, p0), x' = a x + N(0, q), y = x + N(0, r): the scalar Kalman filter."""
    m, p, ll = float(m0), float(p0), 0.0
    for yt in np.asarray(y, dtype=np.float64).reshape(-1):
        s = p + r
        ll += -0.5 * (np.log(2 * np.pi * s) + (yt - m) ** 2 / s)
        k = p / s
        m, p = m + k * (yt - m), (1 - k) * p
        m, p = a * m, a * a * p + q
    return ll
