"""NumPy restatement of what pgas_m_rollout_stats computes from a grey-box rollout's clouds (csrc/pgas_marginal_rollout_stats.hip.h,
DESIGN.md section 14): the two-level summation order, the exactly rounded fma chain of the observation noise, k_expr mode 2's
log-density and the log predictive density from the blocks' (max, sum exp).  Replicate p = 64 b + lane, one replicate per lane.

    1. inside a block   the balanced adjacent-pair tree v <- v[0::2] + v[1::2], six times; lanes with p >= P hold +0.0
    2. across blocks    ascending b from +0.0

Adding +0.0 changes no value (only the sign of a -0.0), so padding the replicates >= P with +0.0 IS "over the replicates < P only"."""
import numpy as np

from rollout_stats_numpy import _fma1, fma  # noqa: F401  (the Fraction-backed fma of section 13's restatement)

BLOCK = 64


def _f(a):
    return np.asarray(a, dtype=np.float64)


def _blocks(v, fill=0.0):
    """(..., P) -> (..., B, 64) padded with `fill`."""
    v = _f(v)
    P = v.shape[-1]
    B = (P + BLOCK - 1) // BLOCK
    pad = np.full(v.shape[:-1] + (B * BLOCK,), fill)
    pad[..., :P] = v
    return pad.reshape(v.shape[:-1] + (B, BLOCK))


def block_sums(v):
    """Level 1: (..., P) -> (..., B)."""
    s = _blocks(v)
    for _ in range(6):
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def reduce_sum(v):
    """Both levels: (..., P) -> (...)."""
    b = block_sums(v)
    s = np.zeros(b.shape[:-1])
    for i in range(b.shape[-1]):
        s = s + b[..., i]
    return s


def moments(v):
    """(S1, S2) of a value channel (..., P): sum v and sum (v * v), the product rounded before it is added."""
    v = _f(v)
    return reduce_sum(v), reduce_sum(v * v)


def predicted_obs(g, LR=None, e=None):
    """yhat (..., ny) of noise-free outputs g (..., ny): acc = g_j, then acc = fma(LR[j,l], e_l, acc) for l = 0 .. j ascending."""
    g = _f(g)
    if LR is None:
        return g.copy()
    out = np.empty_like(g)
    for j in range(g.shape[-1]):
        acc = g[..., j]
        for l in range(j + 1):
            acc = _f(fma(LR[j, l], e[..., l], acc))
        out[..., j] = acc
    return out


def loglik(g, y, LRinv, cR):
    """k_expr mode 2 on outputs g (..., ny) and observation rows y broadcastable to g: e_j = sum_l (y_l - g_l) * LRinv[j,l] from 0.0 over
    ALL l ascending, q = sum_j e_j * e_j from 0.0, cR - 0.5 * q; every product and sum rounded on its own (plain float64 NumPy)."""
    g, LRinv = _f(g), np.atleast_2d(_f(LRinv))
    ny = g.shape[-1]
    y = np.broadcast_to(_f(y), g.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.zeros(g.shape[:-1])
        for j in range(ny):
            e = np.zeros(g.shape[:-1])
            for l in range(ny):
                e = e + (y[..., l] - g[..., l]) * LRinv[j, l]
            q = q + e * e
        return cR - 0.5 * q


def lpd(ll, y, det_exp, det_log):
    """Log predictive density (..., T) from the replicates' log-densities ll (..., T, P) and the observations y (T, ny): per block
    m_b = max l (NaN takes no part; -inf without one), s_b = sum exp(l - m_b) in the order of level 1 (a NaN l and a block with
    m_b = -inf add +0.0); M = max_b m_b, S = sum_b s_b exp(m_b - M) ascending b from +0.0 over the blocks with m_b > -inf;
    (M + log S) - log P, -inf when S == 0, NaN where y_t holds a NaN.  det_exp / det_log: the library's exp and log (oracle.canon)."""
    ll = _f(ll)
    P = ll.shape[-1]
    isn = np.isnan(ll)
    w = _blocks(np.where(isn, -np.inf, ll), fill=-np.inf)           # (..., B, 64)
    takes = _blocks((~isn).astype(np.float64)) > 0                  # live and not NaN
    mb = w.max(axis=-1)                                             # (..., B)
    takes = takes & (mb != -np.inf)[..., None]
    with np.errstate(invalid="ignore"):
        arg = np.where(takes, w - np.where(mb == -np.inf, 0.0, mb)[..., None], 0.0)   # -inf for l = -inf: exp gives 0
    term = np.where(takes, det_exp(arg).reshape(arg.shape), 0.0)
    sb = term
    for _ in range(6):
        sb = sb[..., 0::2] + sb[..., 1::2]
    sb = sb[..., 0]                                                 # (..., B)
    M = mb.max(axis=-1)
    S = np.zeros(M.shape)
    for b in range(mb.shape[-1]):
        m = mb[..., b]
        sc = det_exp(np.where(m == -np.inf, 0.0, m - np.where(M == -np.inf, 0.0, M))).reshape(m.shape)
        S = np.where(m != -np.inf, S + sb[..., b] * sc, S)
    logS = det_log(np.where(S > 0, S, 1.0)).reshape(S.shape)
    out = np.where(S == 0.0, -np.inf, (np.where(S == 0.0, 0.0, M) + logS) - float(det_log(np.array([float(P)]))[0]))
    ynan = np.isnan(_f(y).reshape(ll.shape[-2], -1)).any(axis=1)
    return np.where(ynan, np.nan, out)
