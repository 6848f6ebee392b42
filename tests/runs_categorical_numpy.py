"""NumPy restatement of pgas_m_runs_categorical (csrc/pgas_marginal_chains.hip.h: k_runs_categorical) in its DEFINED order (DESIGN.md
section 23), and the weight vectors / uniforms its tests share.  A plain module (no fixtures, no pytest hooks), used by
tests/test_marginal_chains_host.py (CPU) and tests/test_gpu_marginal_chains.py.

The order: e_i = pgas_exp(logw_i - max logw) (the library's exponential, here through the canonical C oracle); thread t of 256 sums its
four consecutive particles 4 t .. 4 t + 3 in ascending order (+0.0 behind the row's end); the 256 thread totals are scanned inclusively by
Kogge-Stone (distances 1, 2, ..., 128); c_4t+j = (scanned total of thread t - 1) + (thread t's running sum l_j), c_j = l_j for t = 0;
S = the last scanned total; idx = min(#{i < N : c_i < u S}, N - 1).  A row with a NaN, or whose maximum is not finite, gives N - 1."""
from __future__ import annotations

import numpy as np

import resample_cases as rc
from oracle import canon

THREADS, PER = 256, 4
MARGIN = 1e-9          # of the total mass: how far every test uniform stays from every step of the CDF


def cdf_row(lw):
    """(c (N,), S) of one row in the kernel's order, or None for a row the kernel refuses (NaN, or no finite maximum)."""
    lw = np.asarray(lw, dtype=np.float64).reshape(-1)
    N = lw.size
    assert 1 <= N <= THREADS * PER
    if np.isnan(lw).any() or not np.isfinite(lw.max()):
        return None
    e = np.zeros(THREADS * PER)
    e[:N] = canon.det_exp(lw - lw.max())
    e = e.reshape(THREADS, PER)
    l = np.empty_like(e)
    l[:, 0] = e[:, 0]
    for j in range(1, PER):
        l[:, j] = l[:, j - 1] + e[:, j]
    v = l[:, PER - 1].copy()
    d = 1
    while d < THREADS:
        nxt = v.copy()
        nxt[d:] = v[d:] + v[:-d]
        v, d = nxt, 2 * d
    c = l.copy()
    c[1:] = v[:-1, None] + l[1:]
    return c.reshape(-1)[:N], float(v[-1])


def categorical_row(lw, u):
    N = np.asarray(lw).size
    got = cdf_row(lw)
    if got is None:
        return N - 1
    c, S = got
    return min(int(np.count_nonzero(c < float(u) * S)), N - 1)


def runs_categorical(logw, u):
    """logw (R, N), u (R,) -> idx (R,) int32."""
    logw = np.asarray(logw, dtype=np.float64)
    return np.array([categorical_row(logw[r], u[r]) for r in range(logw.shape[0])], dtype=np.int32)


def plain_row(lw, u):
    """min(searchsorted(cumsum(softmax(lw)), u), N - 1) in plain float64 NumPy, and the normalised CDF it searched."""
    lw = np.asarray(lw, dtype=np.float64)
    w = np.exp(lw - lw.max())
    cdf = np.cumsum(w / w.sum())
    return min(int(np.searchsorted(cdf, u)), lw.size - 1), cdf


# ------------------------------------------------------------------------------------------ the shared cases
def weight_rows(N):
    """Named log-weight vectors of tests/resample_cases.py at size N that have a softmax: degenerate, multi-scale, single survivor,
    all-equal."""
    rows = [("mild", rc.mild(N)), ("flat", rc.flat(N)), ("one_hot_first", rc.one_hot(N, 0)), ("one_hot_middle", rc.one_hot(N, N // 2)),
            ("one_hot_last", rc.one_hot(N, N - 1)), ("far_pair", rc.far_pair(N, 1e5)), ("stairs", rc.stairs(N, 700)), ("huge_range", rc.huge_range(N))]
    if N >= 2:
        rows.append(("one_plus_tail", rc.one_plus_tail(N, N // 3, 0.99)))
    return rows


def refused_rows(N):
    """Rows without a softmax: the kernel's defined answer is N - 1."""
    rows = [("all_nan", rc.all_nan(N)), ("with_nan", rc.with_nan(N)), ("all_empty", rc.all_empty(N)), ("nan_and_empty", rc.nan_and_empty(N))]
    lw = rc.mild(N)
    lw[N // 2] = np.inf
    return rows + [("plus_inf", lw)]


def place_uniform(lw, u0):
    """A uniform near u0 that lies at least 2 MARGIN of the total mass away from every step of the row's float64 CDF: u0 itself, moved into
    the interior of the CDF interval it falls into -- or, when that interval is too narrow, the middle of the widest one below 1."""
    _, cdf = plain_row(lw, 0.5)
    edges = np.concatenate([[0.0], cdf])
    k = int(np.searchsorted(cdf, u0))
    lo, hi = (edges[k], edges[k + 1]) if k < cdf.size else (edges[-1], 1.0)
    if hi - lo < 6 * MARGIN:
        gaps = np.diff(edges)
        k = int(np.argmax(gaps))
        lo, hi = edges[k], edges[k + 1]
        u0 = 0.5 * (lo + hi)
    return float(min(max(u0, lo + 2 * MARGIN), hi - 2 * MARGIN))


def margin(lw, u):
    """Distance of u from the nearest step of the row's float64 CDF (total mass 1)."""
    _, cdf = plain_row(lw, u)
    return float(np.abs(cdf - u).min())


U_CANDIDATES = (0.003, 0.37, 0.61, 0.83, 0.9991)


def batch(N):
    """(names, logw (R, N), u (R,)): every weight row under every candidate uniform, then the refused rows."""
    names, lws, us = [], [], []
    for name, lw in weight_rows(N):
        for u0 in U_CANDIDATES:
            names.append(f"{name}@{N}/u={u0}")
            lws.append(lw)
            us.append(place_uniform(lw, u0))
    for name, lw in refused_rows(N):
        names.append(f"{name}@{N}")
        lws.append(lw)
        us.append(0.37)
    return names, np.stack(lws), np.array(us)
