"""NumPy restatement of pgas_m_smooth (csrc/pgas_marginal_smooth.hip.h) DOWNSTREAM of one draw's own traces: fed
the filter's x (T, N, nx), anc (T, N), lw (T, N), yhat (T, N, ny) and the smoother's fmean (T, N, nx) = f(x_t^i, u_t, xi_t^i) and
xi (T, N, n_xi), it restates everything else the kernel returns, row by row from T - 1 down to 0, vectorised over the trajectories.

    l_i          lw[t]; +0.0 on a row whose y_t holds a NaN
    h_i          pgas_m_expr_eval mode 2's operations: e_j = sum_l (xt_{t+1,l} - f_{i,l}) LQinv[j,l] ascending l from 0.0,
                 q = sum_j e_j e_j ascending j from 0.0, h = cQ - 0.5 q, every product and sum rounded on its own; v_i = l_i + h_i
                 (row T - 1: v_i = l_i)
    scan         canon.segment_partials(v): k, the integer cumsum c, the total s; S = oc_u64_to_double(s) 2^-51
    u            smooth_numpy.uniform on STREAM_M_SMOOTH = 201: pgas_u52 of words 0, 1 of the Philox block of (key, stream, 0, t, g)
    j_t          min(#{i : double(c_i) 2^-51 < u S}, N - 1); S not in (0, inf): g mod N at T - 1, anc[t, j_{t+1}] clamped below
    moments      rollout_stats_numpy.moments over the trajectories of a call (<= 256: one register row of the 256-position tree) of
                 x[t, j_t] then yhat[t, j_t], and on their own of xi[t, j_t]

What the restatement cannot see -- that fmean and xi belong to x -- is checked against the per-step primitives in
tests/test_gpu_model_smooth.py."""
import numpy as np

import rollout_stats_numpy as rs
import smooth_numpy as sn
from common import canon

STREAM_M_SMOOTH = 201   # include/pgas_marginal.h: PGAS_STREAM_M_SMOOTH
CHUNK = 256             # trajectories per pgas_m_smooth call
FIX_INV = 2.0 ** -51


def transition_constants(Q):
    """(LQinv, cQ) as SymbolicStateSpaceModel.transition_logpdf forms them."""
    Lq = np.linalg.cholesky(np.atleast_2d(np.asarray(Q, dtype=np.float64)))
    return np.linalg.inv(Lq), -0.5 * Lq.shape[0] * np.log(2 * np.pi) - float(np.sum(np.log(np.diag(Lq))))


def transition_logdensity(xn, f, LQinv, cQ):
    """h (B, N) of next states xn (B, nx) against means f (N, nx); NumPy rounds every elementwise product and sum on its own."""
    B, nx = xn.shape
    d = xn[:, None, :] - f[None, :, :]
    q = np.zeros((B, f.shape[0]))
    for j in range(nx):
        e = np.zeros_like(q)
        for l in range(nx):
            e = e + d[:, :, l] * LQinv[j, l]
        q = q + e * e
    return cQ - 0.5 * q


def run(key, x, anc, lw, yhat, fmean, xi, y, LQinv, cQ, B, b0=0):
    """One pgas_m_smooth call for one draw -> dict of idx (B, T) int32, xs (B, T, nx), xis (B, T, n_xi), sum, sumsq (T, nx + ny), xi_sum,
    xi_sumsq (T, n_xi), u (B, T), S (B, T)."""
    assert 1 <= B <= CHUNK
    x, lw, yhat, xi = (np.asarray(a, dtype=np.float64) for a in (x, lw, yhat, xi))
    T, N, nx = x.shape
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    ny, nxi = yhat.shape[2], xi.shape[2]
    u64 = canon.lib().oc_u64_to_double
    out = dict(idx=np.empty((B, T), np.int32), xs=np.empty((B, T, nx)), xis=np.empty((B, T, nxi)), sum=np.empty((T, nx + ny)),
               sumsq=np.empty((T, nx + ny)), xi_sum=np.empty((T, nxi)), xi_sumsq=np.empty((T, nxi)), u=np.empty((B, T)), S=np.empty((B, T)))
    for t in range(T - 1, -1, -1):
        l = np.zeros(N) if np.isnan(y[t]).any() else lw[t]
        same = t == T - 1
        v = np.broadcast_to(l, (B, N)) if same else l[None, :] + transition_logdensity(out["xs"][:, t + 1], np.asarray(fmean[t], dtype=np.float64), LQinv, cQ)
        part = None
        for b in range(B):
            g = b0 + b
            if part is None or not same:
                segm, segs, c = canon.segment_partials(v[b])
                part = (float(u64(int(segs[0]))) * FIX_INV, sn.u64_to_double(c) * FIX_INV)
            Ssum, cdf = part
            uu = sn.uniform(key, t, g, STREAM_M_SMOOTH)
            out["u"][b, t], out["S"][b, t] = uu, Ssum
            if 0.0 < Ssum < np.inf:
                j = min(int(np.count_nonzero(cdf < uu * Ssum)), N - 1)
            else:
                j = g % N if same else min(max(int(anc[t, out["idx"][b, t + 1]]), 0), N - 1)
            out["idx"][b, t] = j
        jt = out["idx"][:, t]
        out["xs"][:, t], out["xis"][:, t] = x[t][jt], xi[t][jt]
        out["sum"][t], out["sumsq"][t] = rs.moments(np.concatenate([x[t][jt], yhat[t][jt]], axis=1).T)
        out["xi_sum"][t], out["xi_sumsq"][t] = rs.moments(xi[t][jt].T)
    return out


def run_chunks(key, x, anc, lw, yhat, fmean, xi, y, LQinv, cQ, n_traj):
    """n_traj trajectories as the Python layer issues them: calls of <= 256 at b0 = 0, 256, ...; idx, xs and xis concatenated, the
    chunks' sums added elementwise in ascending chunk order starting from the first chunk's."""
    parts = [run(key, x, anc, lw, yhat, fmean, xi, y, LQinv, cQ, min(CHUNK, n_traj - b0), b0) for b0 in range(0, n_traj, CHUNK)]
    out = {f: np.concatenate([p[f] for p in parts], axis=0) for f in ("idx", "xs", "xis", "u", "S")}
    for f in ("sum", "sumsq", "xi_sum", "xi_sumsq"):
        acc = parts[0][f]
        for p in parts[1:]:
            acc = acc + p[f]
        out[f] = acc
    return out


# ---- plain float64 counterparts, for the host tests ---------------------------------------------------------------------------------------
def float_transition(xn, f, Q):
    """log N(xn_b; f_i, Q) (B, N) written with NumPy's linear algebra: transition_logpdf's expression in float64."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    d = xn[:, None, :] - f[None, :, :]
    return -0.5 * (Q.shape[0] * np.log(2 * np.pi) + np.linalg.slogdet(Q)[1]) - 0.5 * np.einsum("bij,jk,bik->bi", d, np.linalg.inv(Q), d)


def float_indices(lw, fmean, y, Q, res):
    """A plain float64 FFBSi on the same trace and uniforms, row by row given the restatement's next state: log-sum-exp weights, their
    cumulative sum, searchsorted -> idx (B, T)."""
    T, N = lw.shape
    B = res["idx"].shape[0]
    out = np.empty((B, T), np.int64)
    for t in range(T - 1, -1, -1):
        l = np.zeros(N) if np.isnan(y[t]).any() else lw[t]
        v = np.broadcast_to(l, (B, N)) if t == T - 1 else l[None, :] + float_transition(res["xs"][:, t + 1], fmean[t], Q)
        w = np.exp(v - v.max(axis=1, keepdims=True))
        cdf = np.cumsum(w / w.sum(axis=1, keepdims=True), axis=1)
        for b in range(B):
            out[b, t] = min(int(np.searchsorted(cdf[b], res["u"][b, t], side="left")), N - 1)
    return out


def smoother_marginals(x, lw, fmean, y, Q):
    """The O(N^2) float64 forward-filter / backward-smoother weights w_{t|T} (T, N) on the trace: conditionally on the trace, the
    marginal of j_t under backward simulation.  The filter resamples at every step, so its weights at row t are softmax(l(t))."""
    T, N = lw.shape
    W = np.empty((T, N))
    for t in range(T):
        l = np.zeros(N) if np.isnan(y[t]).any() else lw[t]
        W[t] = np.exp(l - l.max())
        W[t] /= W[t].sum()
    out = np.empty((T, N))
    out[T - 1] = W[T - 1]
    for t in range(T - 2, -1, -1):
        lf = float_transition(x[t + 1], fmean[t], Q)            # (j, i): log f(x_{t+1,j} | x_{t,i}, xi_{t,i})
        num = W[t][None, :] * np.exp(lf - lf.max(axis=1, keepdims=True))
        out[t] = (out[t + 1][:, None] * num / num.sum(axis=1, keepdims=True)).sum(axis=0)
    return out


def rts_smoother(a, q, r, m0, p0, y):
    """The smoothed means E[x_t | y_0 .. y_T-1] (T) of x_0 ~ N(m0, p0), x' = a x + N(0, q), y = x + N(0, r): the scalar Kalman filter
    and the Rauch-Tung-Striebel backward pass."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Tn = len(y)
    mp, pp, mf, pf = np.empty(Tn), np.empty(Tn), np.empty(Tn), np.empty(Tn)
    m, p = float(m0), float(p0)
    for t in range(Tn):
        mp[t], pp[t] = m, p
        k = p / (p + r)
        mf[t], pf[t] = m + k * (y[t] - m), (1 - k) * p
        m, p = a * mf[t], a * a * pf[t] + q
    ms = mf.copy()
    for t in range(Tn - 2, -1, -1):
        ms[t] = mf[t] + pf[t] * a / pp[t + 1] * (ms[t + 1] - mp[t + 1])
    return ms
