"""NumPy restatement of what pgas_rollout_stats computes from a rollout's cloud (csrc/pgas_rollout_stats.hip.h):
the three-level summation order, the exactly rounded fma chains of the predicted observation and the log-likelihood, and the log
predictive density from the blocks' (max, sum exp).  Replicate p = 1024 b + 256 r + lane.

    1. lane-local     s = (((+0.0 + v[r = 0]) + v[r = 1]) + ...), ascending r
    2. 256 lanes      the balanced adjacent-pair tree v <- v[0::2] + v[1::2], eight times; lanes without a replicate hold +0.0
    3. blocks         ascending b from +0.0

A lane-local sum that starts at +0.0 is never -0.0, so padding the replicates >= P with +0.0 IS "over the replicates < P only", and the
order does not depend on how many register rows (NR) a kernel instantiation carries: rows it does not have would add +0.0."""
from fractions import Fraction

import numpy as np

BLOCK, LANES = 1024, 256


def _blocks(v):
    """(..., P) -> (..., B, 4, 256) padded with +0.0."""
    v = np.asarray(v, dtype=np.float64)
    P = v.shape[-1]
    B = (P + BLOCK - 1) // BLOCK
    pad = np.zeros(v.shape[:-1] + (B * BLOCK,))
    pad[..., :P] = v
    return pad.reshape(v.shape[:-1] + (B, BLOCK // LANES, LANES))


def block_sums(v, nr=None):
    """Levels 1 and 2: (..., P) -> (..., B).  nr: register rows the instantiation carries (1, 2 or 4; None: 4) -- P <= 256 nr when B == 1."""
    w = _blocks(v)
    rows = BLOCK // LANES if nr is None else int(nr)
    assert rows == BLOCK // LANES or (w.shape[-3] == 1 and np.asarray(v).shape[-1] <= rows * LANES)
    s = np.zeros(w.shape[:-2] + (LANES,))
    for r in range(rows):
        s = s + w[..., r, :]
    for _ in range(8):
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def reduce_sum(v, nr=None):
    """All three levels: (..., P) -> (...)."""
    b = block_sums(v, nr)
    s = np.zeros(b.shape[:-1])
    for i in range(b.shape[-1]):
        s = s + b[..., i]
    return s


def moments(v, nr=None):
    """(S1, S2) of a value channel (..., P): sum v and sum (v * v), the product rounded before it is added."""
    v = np.asarray(v, dtype=np.float64)
    return reduce_sum(v, nr), reduce_sum(v * v, nr)


def _fma1(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c   # not finite either way
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))   # one rounding: a correctly rounded fma of finite doubles
    except OverflowError:
        return float("inf") if (a > 0) == (b > 0) else float("-inf")


fma = np.frompyfunc(_fma1, 3, 1)


def _f(a):
    return np.asarray(a, dtype=np.float64)


def predicted_obs(x, H, LR=None, e=None):
    """yhat (..., ny) of states x (..., nx): acc = fma(H[j,k], x_k, acc) ascending k from +0.0, then acc = fma(LR[j,l], e_l, acc), l = 0 .. j."""
    H = np.atleast_2d(H)
    ny, nx = H.shape
    out = np.empty(x.shape[:-1] + (ny,))
    for j in range(ny):
        acc = np.zeros(x.shape[:-1])
        for k in range(nx):
            acc = _f(fma(H[j, k], x[..., k], acc))
        if LR is not None:
            for l in range(j + 1):
                acc = _f(fma(LR[j, l], e[..., l], acc))
        out[..., j] = acc
    return out


def loglik(x, y, H, LRinv, cR):
    """The device function loglik<NX> (csrc/pgas_kernels.hip.h) on states x (..., nx) and one observation row y (ny,), or rows
    broadcastable against x's leading axes (..., ny)."""
    H, LRinv = np.atleast_2d(H), np.atleast_2d(LRinv)
    ny, nx = H.shape
    y = np.asarray(y, dtype=np.float64)
    e = []
    for j in range(ny):
        ej = np.broadcast_to(y[..., j], x.shape[:-1]).copy()
        for k in range(nx):
            ej = _f(fma(-H[j, k], x[..., k], ej))
        e.append(ej)
    quad = np.zeros(x.shape[:-1])
    for j in range(ny):
        w = np.zeros(x.shape[:-1])
        for l in range(j + 1):
            w = _f(fma(LRinv[j, l], e[l], w))
        quad = _f(fma(w, w, quad))
    return _f(fma(-0.5, quad, cR))


def lpd(ll, y, det_exp, det_log):
    """Log predictive density (..., T) from the replicates' log-likelihoods ll (..., T, P) and the observations y (T, ny): per block
    m_b = max l (NaN takes no part; -inf without one), s_b = sum exp(l - m_b) in the order of levels 1-2 (a NaN l and a block with
    m_b = -inf add +0.0); M = max_b m_b, S = sum_b s_b exp(m_b - M) ascending b from +0.0 over the blocks with m_b > -inf;
    (M + log S) - log P, -inf when S == 0, NaN where y_t holds a NaN.  det_exp / det_log: the library's exp and log (oracle.canon)."""
    ll = np.asarray(ll, dtype=np.float64)
    P = ll.shape[-1]
    w = _blocks(np.where(np.isnan(ll), -np.inf, ll))
    valid = _blocks(np.ones(P)) > 0
    w = np.where(valid, w, -np.inf)
    isn = _blocks(np.isnan(ll).astype(np.float64)) > 0
    mb = w.max(axis=(-1, -2))                                      # (..., B)
    takes = valid & ~isn & (mb != -np.inf)[..., None, None]
    with np.errstate(invalid="ignore"):
        arg = np.where(takes, w - np.where(mb == -np.inf, 0.0, mb)[..., None, None], 0.0)   # -inf for l = -inf: exp gives 0
    term = np.where(takes, det_exp(arg).reshape(arg.shape), 0.0)
    flat = term.reshape(term.shape[:-3] + (term.shape[-3], BLOCK))
    sb = np.stack([block_sums(flat[..., b, :])[..., 0] for b in range(flat.shape[-2])], axis=-1)
    M = mb.max(axis=-1)
    S = np.zeros(M.shape)
    for b in range(mb.shape[-1]):
        m = mb[..., b]
        sc = det_exp(np.where(m == -np.inf, 0.0, m - np.where(M == -np.inf, 0.0, M))).reshape(m.shape)
        S = np.where(m != -np.inf, S + sb[..., b] * sc, S)
    logS = det_log(np.where(S > 0, S, 1.0)).reshape(S.shape)
    out = np.where(S == 0.0, -np.inf, (np.where(S == 0.0, 0.0, M) + logS) - float(det_log(np.array([float(P)]))[0]))
    ynan = np.isnan(np.asarray(y, dtype=np.float64).reshape(ll.shape[-2], -1)).any(axis=1)
    return np.where(ynan, np.nan, out)
