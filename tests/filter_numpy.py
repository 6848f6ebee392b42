"""NumPy restatement of pgas_filter (csrc/pgas_filter.hip.h) from the canonical oracle's primitives: a bootstrap
particle filter of one draw (A, S, key), step by step in the order of the definition.

    state        CanonModel.init_state / CanonModel.step on a model of N + 1 particles: rows 0 .. N - 1 of its x_new are
                 eval_mean(x_prev[i]) + LS z(key, PROP, t, i) for whatever x_prev holds -- here the RESAMPLED state -- and row N is the
                 oracle's conditioned particle, which is dropped
    l_i          loglik<NX>'s fma chains, every fma exactly rounded (fma below: rollout_stats_numpy.fma, vectorised)
    predictive   rollout_stats_numpy.moments of x_j and yhat_j = sum_k H[j,k] x_k over the unweighted cloud
    scan         canon.segment_partials: k = ceil(max l log2 e), integer cumsum c, total s; S = double(s) 2^-51
    ell          fma(k, LN2_LO, fma(k, LN2_HI, log S)) - log N with the library's log; -inf when S == 0; NaN when y_t holds a NaN
    filtered     w_i = q_i 2^-51, sum (w_i x_ij) and sum (w_i w_i) in the order of the predictive sums; ess = (S S) / sum w w, 0 if not valid
    resampling   canon.resample_range with canon.uniform(key, RESAMPLE, t): the identity when S is not in (0, inf)
"""
import numpy as np

import rollout_stats_numpy as rs
from common import canon

LN2_HI = float.fromhex("0x1.62e42fefa39efp-1")   # include/pgas_canon.h: PGAS_SEG_LN2_HI / _LO
LN2_LO = float.fromhex("0x1.abc9e3b39803fp-56")
FIX_INV = 2.0 ** -51


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = 134217729.0 * a   # 2^27 + 1: Veltkamp's splitting
    hi = t - (t - a)
    return hi, a - hi


def fma(a, b, c):
    """The correctly rounded a * b + c of rollout_stats_numpy.fma, vectorised: the exact product (Dekker), the exact sum of its head with
    c (Knuth), the two tails added with rounding to odd, one final rounding to nearest (Boldo and Melquiond, "Emulation of a FMA and
    correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 57(4), 2008).  The error-free transformations need their
    operands and results away from overflow and underflow: every element outside that range, or not finite, goes through
    rollout_stats_numpy.fma (exact rational arithmetic) instead."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    a, b, c = a.copy(), b.copy(), c.copy()
    with np.errstate(all="ignore"):
        p = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        pl = (((ah * bh - p) + ah * bl) + al * bh) + al * bl
        th, tl = _two_sum(c, p)
        vh, vl = _two_sum(tl, pl)
        even = (vh.view(np.int64) & 1) == 0
        v = np.where((vl != 0.0) & even, np.nextafter(vh, np.where(vl > 0, np.inf, -np.inf)), vh)
        out = th + v
        big = lambda z: np.abs(z) > 1e140  # noqa: E731
        slow = ~(np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(out)) | big(a) | big(b) | big(c) | ((p != 0.0) & (np.abs(p) < 1e-200))
        slow |= (out != 0.0) & (np.abs(out) < 1e-280)
        if slow.any():
            out[slow] = np.asarray(rs.fma(a[slow], b[slow], c[slow]), dtype=np.float64)
    return out


def loglik(x, y, H, LRinv, cR):
    """rollout_stats_numpy.loglik (the device function loglik<NX>) with the vectorised fma, for one observation row y (ny,)."""
    H, LRinv = np.atleast_2d(H), np.atleast_2d(LRinv)
    ny, nx = H.shape
    e = []
    for j in range(ny):
        ej = np.full(x.shape[:-1], float(y[j]))
        for k in range(nx):
            ej = fma(-H[j, k], x[..., k], ej)
        e.append(ej)
    quad = np.zeros(x.shape[:-1])
    for j in range(ny):
        w = np.zeros(x.shape[:-1])
        for l in range(j + 1):
            w = fma(LRinv[j, l], e[l], w)
        quad = fma(w, w, quad)
    return fma(-0.5, quad, cR)


def _selector(H):
    H = np.atleast_2d(H)
    return bool(np.all((H == 0) | (H == 1)) and np.all(H.sum(axis=1) == 1))


def ell_from_scan(kref, S, N):
    """The evidence increment from the scan's exact pair (k, S) and N: the expression of filter_ell (csrc/pgas_filter.hip.h)."""
    if S == 0.0:
        return -np.inf
    logS = float(canon.det_log(np.array([S]))[0])
    logN = float(canon.det_log(np.array([float(N)]))[0])
    return rs._fma1(kref, LN2_LO, rs._fma1(kref, LN2_HI, logS)) - logN


def predicted_obs(x, H):
    return x @ np.atleast_2d(H).T if _selector(H) else rs.predicted_obs(x, H)   # a 0/1 selector: the fma chain from +0.0 is exact


def run(cm1, N, key, A, S, m0, L0, lik, y, x0=None):
    """cm1: the CanonModel of the problem with N + 1 particles; A (nx, M), S (nx, nx); lik: the GaussianLikelihood; y (T, ny) the
    observations the model was built with; x0 (N, nx) or None (drawn) -> dict of x (T, N, nx), anc (T, N) int32, l (T, N), ell, ess, wtot
    (T), pred_sum, pred_sumsq (T, nx + ny), filt_sum (T, nx), loglik."""
    T, nx = cm1.T, cm1.nx
    assert cm1.N == N + 1
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    ny = y.shape[1]
    LS, LSinv, cS = cm1.chol_parts_dev(S)
    ref = np.zeros(nx)
    u64 = canon.lib().oc_u64_to_double
    out = dict(x=np.empty((T, N, nx)), anc=np.empty((T, N), np.int32), l=np.empty((T, N)), ell=np.empty(T), ess=np.empty(T), wtot=np.empty(T),
               pred_sum=np.empty((T, nx + ny)), pred_sumsq=np.empty((T, nx + ny)), filt_sum=np.empty((T, nx)))
    total = 0.0
    x = cm1.init_state(key, m0, L0, ref)[:N].copy() if x0 is None else np.array(x0, dtype=np.float64).reshape(N, nx)
    for t in range(T):
        if t > 0:
            prev = x[out["anc"][t - 1]]
            pad = np.concatenate([prev, prev[-1:]], axis=0)
            x = cm1.step(t, key, pad, None, A, LS, LSinv, cS, ref)[1][:N].copy()
        out["x"][t] = x
        l = loglik(x, y[t], lik.H, lik.LRinv, lik.cR)
        out["l"][t] = l
        v = np.concatenate([x, predicted_obs(x, lik.H)], axis=1)
        out["pred_sum"][t], out["pred_sumsq"][t] = rs.moments(v.T)
        segm, segs, c = canon.segment_partials(l)
        kref, Ssum = float(segm[0]), float(u64(int(segs[0]))) * FIX_INV
        valid = 0.0 < Ssum < np.inf
        ynan = bool(np.isnan(y[t]).any())
        ell = np.nan if ynan else ell_from_scan(kref, Ssum, N)
        out["ell"][t] = ell
        if not ynan:
            total = total + ell
        q = np.diff(np.concatenate([np.zeros(1, np.uint64), c]))
        w = q.astype(np.float64) * FIX_INV   # q <= 2^51: exact
        out["wtot"][t] = Ssum
        out["filt_sum"][t] = rs.reduce_sum((w[:, None] * x).T)
        sw = float(rs.reduce_sum(w * w))
        out["ess"][t] = (Ssum * Ssum) / sw if valid else 0.0
        u = canon.uniform(key, canon.STREAM_RESAMPLE, t)
        out["anc"][t] = canon.resample_range(segm, segs, c, N, u, 0, N)
    out["loglik"] = total
    return out


def float_filter(res, lik, y):
    """A plain float64 filter on the restatement's particles (the same ancestors): per step logsumexp(l) - log N with l the Gaussian log
    density, the self-normalised filtered mean and 1 / sum W^2 -> (ell (T), mean (T, nx), ess (T))."""
    x = res["x"]
    T, N, nx = x.shape
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    R = np.atleast_2d(lik.R)
    Rinv, ny = np.linalg.inv(R), R.shape[0]
    c = -0.5 * (ny * np.log(2 * np.pi) + np.linalg.slogdet(R)[1])
    ell, mean, ess = np.empty(T), np.empty((T, nx)), np.empty(T)
    for t in range(T):
        e = y[t][None, :] - x[t] @ np.atleast_2d(lik.H).T
        l = c - 0.5 * np.einsum("ij,jk,ik->i", e, Rinv, e)
        m = l.max()
        p = np.exp(l - m)
        ell[t] = m + np.log(p.sum()) - np.log(N)
        W = p / p.sum()
        mean[t] = W @ x[t]
        ess[t] = 1.0 / np.sum(W * W)
    return ell, mean, ess
