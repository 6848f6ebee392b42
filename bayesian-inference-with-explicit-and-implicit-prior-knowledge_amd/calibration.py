"""Calibration of the posterior predictive: empirical CDF counts at given thresholds, pooled over the draws.

``Rollout.cdf`` (open loop) and ``HeldOutFilter.forecast_cdf`` (horizons 1 .. H), and their grey-box twins ``ModelRollout.cdf`` and
``ModelRollout.forecast_cdf``, count, inside their kernels, the replicates or particles
whose value channel is <= a threshold: ``count[..., c, j]`` int32 against ``thresholds (T, nx + ny, J)``.  The posterior predictive is the
mixture over the draws, so its CDF is the mean of the per-draw CDFs and the per-draw counts add up exactly (per-draw quantiles do not
combine).  With the observations as thresholds the pooled CDF is the probability integral transform (PIT) of the observations; interval
coverage follows from the PIT; with a grid of thresholds the pooled CDF is inverted to bands.  Everything here is plain torch on the
small tensors:

* ``CdfCounts(n, count, thresholds)``: what the two calls return.
* ``calibration_summary(cdf, levels=(0.5, 0.8, 0.9, 0.95), bins=10)``: pooled CDF, PIT, interval coverage, PIT histogram, KS distance.
* ``threshold_grid(mean, std, J, width=4.0)``: thresholds around a predictive mean.
* ``predictive_bands(cdf, levels)``: quantile estimates from the pooled CDF on a threshold grid.
"""
from __future__ import annotations

import numpy as np
import torch

MAX_THRESHOLDS = 16   # PGAS_CDF_MAX_J


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else tuple(np.shape(a))


def check_thresholds(T, nx, ny, thresholds, has_observations):
    """Validates `thresholds` from its shape alone (nothing is copied, no device is touched) -> (J, form): form "all" for (T, nx + ny, J),
    "obs" for (T, ny, J), (T, ny) or (T,) (the yhat channels only; J = 1 for the last two), "pit" for None (the context's observations)."""
    if thresholds is None:
        if not has_observations:
            raise ValueError("thresholds=None counts against the observations (the PIT): this context has none")
        return 1, "pit"
    s = _shape(thresholds)
    if s == (T,) and ny == 1 or s == (T, ny):
        return 1, "obs"
    if len(s) == 3 and s[0] == T and s[1] in (nx + ny, ny):
        J = int(s[2])
        if J < 1 or J > MAX_THRESHOLDS:
            raise ValueError(f"thresholds: J = {J} thresholds per channel, expected 1..{MAX_THRESHOLDS}")
        return J, "all" if s[1] == nx + ny else "obs"
    raise ValueError(f"thresholds: expected ({T}, {nx + ny}, J), ({T}, {ny}, J), ({T}, {ny}) or None, got {s}")


def device_thresholds(engine, thresholds, J, form, observations=None):
    """The (T, nx + ny, J) fp64 device tensor of a checked `thresholds`: the state channels of the "obs" and "pit" forms get NaN (they
    count 0).  `engine`: an Engine, or any object with T, nx, ny and an Engine behind ``ops.eng`` (a ModelRollout).  Enqueues work only."""
    T, nx, ny = engine.T, engine.nx, engine.ny
    if not hasattr(engine, "_dev"):
        engine = engine.ops.eng   # the utility context: it carries the device and the upload helper, not the model's dimensions
    if form == "all":
        return engine._dev(thresholds, shape=(T, nx + ny, J))
    th = engine._dev(observations if form == "pit" else thresholds, shape=(T, ny, J))
    full = torch.full((T, nx + ny, J), float("nan"), dtype=torch.float64, device=engine.device)
    full[:, nx:] = th
    return full


class CdfCounts:
    """What ``cdf`` / ``forecast_cdf`` return, device tensors: n replicates (particles) per draw; count (K, T, nx + ny, J) or
    (K, H, T, nx + ny, J) int32, the number of them with value channel c <= thresholds[t, c, j] (-1: a forecast entry without an origin
    row); thresholds (T, nx + ny, J) fp64 as the kernel read them (NaN: nothing is counted).  nx: the number of state channels (the
    predicted observations follow them); pit: the thresholds are the observations."""

    def __init__(self, n, count, thresholds, nx=None, pit=False):
        self.n, self.count, self.thresholds, self.nx, self.pit = int(n), count, thresholds, None if nx is None else int(nx), bool(pit)


def _ks(u):
    """sup |ECDF(u) - uniform| of a 1-D tensor without NaN; NaN when it is empty."""
    m = int(u.numel())
    if m == 0:
        return torch.tensor(float("nan"), dtype=torch.float64, device=u.device)
    s = torch.sort(u).values
    i = torch.arange(1, m + 1, dtype=torch.float64, device=u.device)
    return torch.maximum((i / m - s).max(), (s - (i - 1) / m).max())


def calibration_summary(cdf, levels=(0.5, 0.8, 0.9, 0.95), bins=10):
    """dict of F, the pooled predictive CDF at the thresholds, (T, C, J) or (H, T, C, J): the int64 sum of the counts over the draws, then
    one division by K n; NaN where a count is -1.  For J = 1 (thresholds = observations: the PIT) also, over the predicted-observation
    channels (all channels when cdf.nx is None): pit (T, ny) or (H, T, ny); coverage, a dict level -> the share of rows with
    (1 - level) / 2 < pit <= 1 - (1 - level) / 2 among the rows whose threshold (observation) is not NaN and whose count is defined;
    hist (bins,) the PIT histogram on [0, 1] in equal bins (the last one closed); ks = sup |ECDF(pit) - u|.  A forecast's coverage, hist
    and ks carry a leading horizon axis (H,)."""
    cnt = cdf.count
    K = int(cnt.shape[0])
    missing = (cnt < 0).any(dim=0)
    F = cnt.to(torch.int64).sum(dim=0).to(torch.float64) / float(K * cdf.n)
    F = torch.where(missing, torch.full_like(F, float("nan")), F)
    out = {"F": F}
    if int(cnt.shape[-1]) != 1:
        return out
    c0 = 0 if cdf.nx is None else cdf.nx
    pit = F[..., c0:, 0]
    th = torch.as_tensor(cdf.thresholds, dtype=torch.float64, device=F.device)[:, c0:, 0]
    ok = ~torch.isnan(pit) & ~torch.isnan(th).expand_as(pit)
    out["pit"] = pit
    horizons = pit.dim() == 3
    rows = [(pit[h], ok[h]) for h in range(pit.shape[0])] if horizons else [(pit, ok)]
    cov = {float(lv): [] for lv in levels}
    hist, ks = [], []
    for p, m in rows:
        u = p[m]
        for lv in cov:
            a = (1.0 - lv) / 2.0
            inside = ((u > a) & (u <= 1.0 - a)).to(torch.float64)
            cov[lv].append(inside.mean() if u.numel() else torch.tensor(float("nan"), dtype=torch.float64, device=F.device))
        hist.append(torch.histc(u, bins=int(bins), min=0.0, max=1.0))
        ks.append(_ks(u))
    pack = (lambda v: torch.stack(v)) if horizons else (lambda v: v[0])
    out["coverage"] = {lv: pack(v) for lv, v in cov.items()}
    out["hist"] = pack(hist)
    out["ks"] = pack(ks)
    return out


def threshold_grid(mean, std, J, width=4.0):
    """(T, C, J) = mean + std * linspace(-width, width, J) from a pooled predictive mean and standard deviation (T, C), e.g. the
    concatenated x / y ``*_mean_pooled`` and ``*_std_pooled`` of ``predictive_summary``."""
    mean = torch.as_tensor(mean, dtype=torch.float64)
    std = torch.as_tensor(std, dtype=torch.float64, device=mean.device)
    if mean.shape != std.shape:
        raise ValueError(f"mean and std: equal shapes expected, got {tuple(mean.shape)} and {tuple(std.shape)}")
    J = int(J)
    if J < 1 or J > MAX_THRESHOLDS:
        raise ValueError(f"J = {J} thresholds per channel, expected 1..{MAX_THRESHOLDS}")
    z = torch.linspace(-float(width), float(width), J, dtype=torch.float64, device=mean.device)
    return mean[..., None] + std[..., None] * z


def predictive_bands(cdf, levels):
    """Quantile estimates (..., C, len(levels)) of the pooled predictive at `levels` in (0, 1): inverse linear interpolation of the pooled
    F (calibration_summary) on the ascending thresholds, between the last threshold with F < level and the first with F >= level; NaN
    where the thresholds do not bracket the level (F[0] >= level or F[J - 1] < level) or a count is undefined.  The resolution is the
    grid's: between two thresholds the CDF is taken to be linear."""
    F = calibration_summary(cdf)["F"].contiguous()
    th = torch.as_tensor(cdf.thresholds, dtype=torch.float64, device=F.device).expand_as(F)
    J = int(F.shape[-1])
    q = torch.as_tensor(list(levels), dtype=torch.float64, device=F.device)
    bad = torch.isnan(F).any(dim=-1, keepdim=True) | torch.isnan(th).any(dim=-1, keepdim=True)
    Fs = torch.where(bad, torch.zeros_like(F), F)
    j = torch.searchsorted(Fs, q.expand(F.shape[:-1] + (q.numel(),)).contiguous())   # entries of F below the level
    inside = (j >= 1) & (j <= J - 1) & ~bad
    hi = j.clamp(1, max(J - 1, 1)) if J > 1 else torch.zeros_like(j)
    lo = (hi - 1).clamp(min=0)
    F_lo, F_hi = torch.gather(Fs, -1, lo), torch.gather(Fs, -1, hi)
    t_lo, t_hi = torch.gather(th, -1, lo), torch.gather(th, -1, hi)
    den = torch.where(inside, F_hi - F_lo, torch.ones_like(F_hi))
    val = t_lo + (q - F_lo) / den * (t_hi - t_lo)
    return torch.where(inside, val, torch.full_like(val, float("nan")))
