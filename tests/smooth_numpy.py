"""NumPy restatement of pgas_smooth (csrc/pgas_smooth.hip.h) from the canonical oracle's primitives: backward
simulation (FFBSi) of B trajectories of one draw (A, S, key) over the trace filter_numpy.run returns, row by row from T - 1 down to 0, in
the order of the definition, vectorised over the trajectories.

    l_i          the filter's own l (filter_numpy.run's "l"); +0.0 on a row whose y_t holds a NaN
    mu_i         CanonModel.step(t + 1, ..., debug=True)["aux"] on the model of N + 1 particles: eval_mean(x[t, i], u_{t+1})
    h_i          the chain of propagate_particles with filter_numpy.fma: w_k = sum_{l <= k} LSinv[k,l] (xt_{t+1,l} - mu_{i,l}) from +0.0,
                 quad = fma(w_k, w_k, quad), h = fma(-0.5, quad, cS); v_i = l_i + h_i (row T - 1: v_i = l_i)
    scan         canon.segment_partials(v): k, the integer cumsum c, the total s; S = oc_u64_to_double(s) 2^-51
    u            pgas_u52 (transcribed below) of words 0, 1 of canon.philox on (g lo, g hi, t, PGAS_STREAM_SMOOTH), key (seed lo, seed hi)
    j_t          min(#{i : double(c_i) 2^-51 < u S}, N - 1); S not in (0, inf): g mod N at T - 1, anc[t, j_{t+1}] below
    moments      rollout_stats_numpy.moments over the trajectories of a call (<= 256: one register row of the 256-position tree)
"""
import numpy as np

import filter_numpy as fn
import rollout_stats_numpy as rs
from common import canon

STREAM_SMOOTH = 8   # include/pgas_canon.h: PGAS_STREAM_SMOOTH
CHUNK = 256         # trajectories per pgas_smooth call
FIX_INV = 2.0 ** -51
MASK32 = 0xFFFFFFFF


def u52(lo, hi):
    """include/pgas_detmath.h: pgas_u52.  Every operation is exact but the last product, a scaling by a power of two."""
    n = ((int(hi) << 32) | int(lo)) >> 12
    return (float(n >> 32) * 4294967296.0 + float(n & MASK32) + 0.5) * 2.0 ** -52


def uniform(key, t, g, stream=STREAM_SMOOTH):
    """The uniform of (key, stream, t, particle = g): pgas_rng_uniform's formation on pgas_rng_block(key, stream, 0, t, g)."""
    key, g = int(key) & 0xFFFFFFFFFFFFFFFF, int(g)
    w = canon.philox((g & MASK32, (g >> 32) & MASK32, int(t), int(stream)), (key & MASK32, key >> 32))
    return u52(w[0], w[1])


def u64_to_double(c):
    """uint64 array -> float64, round to nearest even: what oc_u64_to_double does (tests/test_smooth_host.py checks the two agree)."""
    return np.asarray(c, dtype=np.uint64).astype(np.float64)


def transition_logdensity(xn, mu, LSinv, cS):
    """h (B, N) of next states xn (B, nx) against means mu (N, nx): the chain of propagate_particles, every fma exactly rounded."""
    B, nx = xn.shape
    quad = np.zeros((B, mu.shape[0]))
    for k in range(nx):
        w = np.zeros_like(quad)
        for l in range(k + 1):
            w = fn.fma(LSinv[k, l], xn[:, None, l] - mu[None, :, l], w)
        quad = fn.fma(w, w, quad)
    return fn.fma(-0.5, quad, cS)


def means(cm1, N, key, A, S, x):
    """mu (T - 1, N, nx): mu[t, i] = eval_mean(x[t, i], u_{t+1}), the oracle's transition mean."""
    LS, LSinv, cS = cm1.chol_parts_dev(S)
    T, nx = cm1.T, cm1.nx
    out = np.empty((max(T - 1, 0), N, nx))
    for t in range(T - 1):
        pad = np.concatenate([x[t], x[t][-1:]], axis=0)
        out[t] = cm1.step(t + 1, key, pad, None, A, LS, LSinv, cS, np.zeros(nx), debug=True)[3]["aux"][:N]
    return out


def run(cm1, N, key, A, S, flt, lik, y, B, b0=0, mu=None):
    """One pgas_smooth call for one draw: cm1 the CanonModel with N + 1 particles, flt the dict of filter_numpy.run for the same key, A
    and S, y (T, ny) -> dict of idx (B, T) int32, xs (B, T, nx), sum, sumsq (T, nx + ny), u (B, T), S (B, T), v_last (the v of row 0)."""
    assert 1 <= B <= CHUNK
    T, nx = cm1.T, cm1.nx
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    ny = y.shape[1]
    _, LSinv, cS = cm1.chol_parts_dev(S)
    x, anc = flt["x"], flt["anc"]
    mu = means(cm1, N, key, A, S, x) if mu is None else mu
    u64 = canon.lib().oc_u64_to_double
    out = dict(idx=np.empty((B, T), np.int32), xs=np.empty((B, T, nx)), sum=np.empty((T, nx + ny)), sumsq=np.empty((T, nx + ny)),
               u=np.empty((B, T)), S=np.empty((B, T)))
    for t in range(T - 1, -1, -1):
        l = np.zeros(N) if np.isnan(y[t]).any() else flt["l"][t]
        if t == T - 1:
            v = np.broadcast_to(l, (B, N))
        else:
            v = l[None, :] + transition_logdensity(out["xs"][:, t + 1], mu[t], LSinv, cS)
        same = t == T - 1
        part = None
        for b in range(B):
            g = b0 + b
            if part is None or not same:
                segm, segs, c = canon.segment_partials(v[b])
                part = (float(u64(int(segs[0]))) * FIX_INV, u64_to_double(c) * FIX_INV)
            Ssum, cdf = part
            uu = uniform(key, t, g)
            out["u"][b, t], out["S"][b, t] = uu, Ssum
            if 0.0 < Ssum < np.inf:
                j = min(int(np.count_nonzero(cdf < uu * Ssum)), N - 1)
            else:
                j = g % N if t == T - 1 else int(anc[t, out["idx"][b, t + 1]])
            out["idx"][b, t] = j
        out["xs"][:, t] = x[t][out["idx"][:, t]]
        xs_t = out["xs"][:, t]
        ch = np.concatenate([xs_t, fn.predicted_obs(xs_t, lik.H)], axis=1)
        out["sum"][t], out["sumsq"][t] = rs.moments(ch.T)
        if t == 0:
            out["v_last"] = np.array(v)
    return out


def run_chunks(cm1, N, key, A, S, flt, lik, y, n_traj):
    """n_traj trajectories as the Python layer issues them: calls of <= 256 at b0 = 0, 256, ...; idx and xs concatenated, the chunks'
    sums added elementwise in ascending chunk order starting from the first chunk's."""
    mu = means(cm1, N, key, A, S, flt["x"])
    parts = [run(cm1, N, key, A, S, flt, lik, y, min(CHUNK, n_traj - b0), b0, mu) for b0 in range(0, n_traj, CHUNK)]
    out = {f: np.concatenate([p[f] for p in parts], axis=0) for f in ("idx", "xs", "u", "S")}
    s1, s2 = parts[0]["sum"], parts[0]["sumsq"]
    for p in parts[1:]:
        s1, s2 = s1 + p["sum"], s2 + p["sumsq"]
    out["sum"], out["sumsq"] = s1, s2
    return out


# ---- plain float64 counterparts, for the host tests ---------------------------------------------------------------------------------
def float_logweights(cm1, N, A, S, flt, lik, y, t, xn):
    """Plain float64 backward log-weights (B, N) of row t given the next states xn (B, nx): the Gaussian log densities written with
    NumPy's linear algebra, the transition mean as A phi(x, u_{t+1}) from the oracle's basis functions."""
    T = cm1.T
    y = np.asarray(y, dtype=np.float64).reshape(T, -1)
    x = flt["x"][t]
    if np.isnan(y[t]).any():
        l = np.zeros(N)
    else:
        R = np.atleast_2d(lik.R)
        e = y[t][None, :] - x @ np.atleast_2d(lik.H).T
        l = -0.5 * (R.shape[0] * np.log(2 * np.pi) + np.linalg.slogdet(R)[1]) - 0.5 * np.einsum("ij,jk,ik->i", e, np.linalg.inv(R), e)
    if xn is None:
        return l[None, :]
    S = np.atleast_2d(S)
    m = cm1.basis_eval(x, t + 1) @ np.asarray(A, dtype=np.float64).reshape(cm1.nx, -1).T
    d = xn[:, None, :] - m[None, :, :]
    h = -0.5 * (S.shape[0] * np.log(2 * np.pi) + np.linalg.slogdet(S)[1]) - 0.5 * np.einsum("bij,jk,bik->bi", d, np.linalg.inv(S), d)
    return l[None, :] + h


def float_indices(cm1, N, A, S, flt, lik, y, res):
    """A plain float64 FFBSi on the same trace and uniforms, row by row given the restatement's next state: log-sum-exp weights, their
    cumulative sum, searchsorted -> idx (B, T)."""
    T = cm1.T
    B = res["idx"].shape[0]
    out = np.empty((B, T), np.int64)
    for t in range(T - 1, -1, -1):
        lw = float_logweights(cm1, N, A, S, flt, lik, y, t, None if t == T - 1 else res["xs"][:, t + 1])
        lw = np.broadcast_to(lw, (B, N))
        w = np.exp(lw - lw.max(axis=1, keepdims=True))
        cdf = np.cumsum(w / w.sum(axis=1, keepdims=True), axis=1)
        for b in range(B):
            out[b, t] = min(int(np.searchsorted(cdf[b], res["u"][b, t], side="left")), N - 1)
    return out


def smoother_marginals(cm1, N, A, S, flt, lik, y):
    """The O(N^2) float64 forward-filter / backward-smoother weights w_{t|T} (T, N) on the trace: conditionally on the trace, the
    marginal of j_t under backward simulation.  The filter resamples at every step, so its weights at row t are softmax(l(t))."""
    T = cm1.T
    W = np.empty((T, N))
    for t in range(T):
        l = float_logweights(cm1, N, A, S, flt, lik, y, t, None)[0]
        W[t] = np.exp(l - l.max())
        W[t] /= W[t].sum()
    out = np.empty((T, N))
    out[T - 1] = W[T - 1]
    for t in range(T - 2, -1, -1):
        lf = float_logweights(cm1, N, A, S, flt, lik, y, t, flt["x"][t + 1]) - float_logweights(cm1, N, A, S, flt, lik, y, t, None)   # (j, i): log f(x_{t+1,j} | x_{t,i})
        f = np.exp(lf - lf.max())
        num = W[t][None, :] * f                              # (j, i)
        out[t] = (out[t + 1][:, None] * num / num.sum(axis=1, keepdims=True)).sum(axis=0)
    return out
