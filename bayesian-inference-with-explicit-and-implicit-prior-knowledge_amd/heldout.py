"""Held-out log-likelihood: a bootstrap particle filter per posterior draw, all draws in one launch.

``PGAS``, ``MultiChainPGAS`` and their chain logs return draws ``(A_k, S_k)`` of the basis-function model x_t ~ N(A phi(x_{t-1}, u_t), S),
y_t ~ N(H x_t, R).  ``Rollout`` simulates them open-loop; this module runs them closed-loop on a record: the one-step-ahead predictive
density p(y_t | y_{0:t-1}, A_k, S_k), its sum over t (the log marginal likelihood of the record under the draw) and the filtered state.

* ``HeldOutFilter(observations, inputs, basis_fcn, likelihood_fcn, n_x, n_particles, init_state_mean=None, init_state_cov=None)``: a
  context of its own over a held-out record; ``__call__(coeff_mat (K, nx, M), error_cov (K, nx, nx), keys, init_state=None, moments=True,
  traces=False) -> FilterResult``.
* ``condSequentialMonteCarlo.filter`` / ``condSequentialMonteCarloChains.filter``: the same call in-sample on a training context, with that
  context's number of particles; its parameters, traces and sweep state are left as they are.
* ``evidence_summary(result, y=None)``: the log posterior-predictive evidence, the prediction band, the filtered mean and the RMSE of the
  predicted observation.
* ``HeldOutFilter.forecast(coeff_mat, error_cov, keys, horizon, init_state=None, log_score=True) -> ForecastResult`` (DESIGN.md section
  17): the filter with its traces, then the h-step-ahead predictions p(y_tau | y_{0:tau-h}, A_k, S_k) for h = 1 .. horizon from every
  origin row of every draw in one more launch; ``condSequentialMonteCarlo.forecast`` / ``condSequentialMonteCarloChains.forecast`` in-sample.
* ``forecast_summary(result, y=None)``: per horizon the prediction band, the log score and the RMSE of the predicted observation.
* ``HeldOutFilter.forecast_cdf(coeff_mat, error_cov, keys, horizon, thresholds=None, observation_noise=True, init_state=None) -> CdfCounts``
  (DESIGN.md section 19): the same clouds counted against thresholds of the target row inside the kernel; ``calibration_summary`` pools
  the counts into the PIT and the interval coverage per horizon.
* ``HeldOutFilter.smooth(coeff_mat, error_cov, keys, n_trajectories, init_state=None, trajectories=False, indices=False) -> SmoothResult``
  (DESIGN.md section 21): the filter with its traces, then backward simulation (FFBSi) over them, the smoothing distribution
  p(x_{0:T-1} | y_{0:T-1}, A_k, S_k) as n_trajectories draws per parameter draw, their moments reduced inside the kernel;
  ``condSequentialMonteCarlo.smooth`` / ``condSequentialMonteCarloChains.smooth`` in-sample.  ``smoothing_summary(result, y=None)``: the
  pooled smoothed mean and standard deviation, the per-draw mean and the RMSE of the smoothed H x.

Step t reads input row t, as the sweep's propagation does (x_t = A phi(x_{t-1}, inputs[t]) + LS z_t): a caller that pairs x_{t-1} with
u_{t-1}, as the reference's validation loop does, passes the input sequence shifted by one row.  The filter resamples at every step and
propagates from the resampled state.  Draw k uses the Philox streams of key k, so its results do not depend on which other draws share the
launch.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import Engine
from .calibration import CdfCounts, check_thresholds, device_thresholds
from .chains import keys_tensor
from .descriptors import BasisMap, GaussianLikelihood

MAX_PARTICLES = 1024   # pgas_filter: one workgroup per draw


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else tuple(np.shape(a))


def check_keys(keys, K):
    """keys: K integers or a (K,) int64 tensor, from the shape alone"""
    if isinstance(keys, torch.Tensor) and (keys.dtype != torch.int64 or keys.dim() != 1):
        raise ValueError("keys: expected K integers or a (K,) int64 tensor of key bit patterns")
    nk = int(keys.shape[0]) if isinstance(keys, torch.Tensor) else len(keys)
    if nk != K:
        raise ValueError(f"keys: expected {K} keys, got {nk}")


def check_horizon(horizon, T):
    """horizon: an integer in 1..T -> int"""
    if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)):
        raise ValueError(f"horizon: expected an integer in 1..{T}, got {horizon!r}")
    if int(horizon) < 1 or int(horizon) > int(T):
        raise ValueError(f"horizon: expected 1..{T} (the record has {T} rows), got {horizon}")
    return int(horizon)


MAX_TRAJECTORIES = 65536   # per smooth call
SMOOTH_CHUNK = 256         # pgas_smooth: trajectories per launch


def check_n_trajectories(n_trajectories):
    """n_trajectories: an integer in 1..65536 -> int"""
    if isinstance(n_trajectories, bool) or not isinstance(n_trajectories, (int, np.integer)):
        raise ValueError(f"n_trajectories: expected an integer in 1..{MAX_TRAJECTORIES}, got {n_trajectories!r}")
    if int(n_trajectories) < 1 or int(n_trajectories) > MAX_TRAJECTORIES:
        raise ValueError(f"n_trajectories: expected 1..{MAX_TRAJECTORIES}, got {n_trajectories}")
    return int(n_trajectories)


def check_call(nx, M, N, has_init, coeff_mat, error_cov, keys, init_state=None):
    """Validates the arguments of a filter call from their shapes alone (nothing is copied, no device is touched) -> (K, x0_mode)."""
    if int(N) < 1 or int(N) > MAX_PARTICLES:
        raise ValueError(f"the filter runs 1..{MAX_PARTICLES} particles in one workgroup per draw, got {N}")
    s = _shape(coeff_mat)
    if len(s) != 3 or s[1:] != (nx, M):
        raise ValueError(f"coeff_mat: expected (K, {nx}, {M}), got {s}")
    K = int(s[0])
    if K < 1:
        raise ValueError("coeff_mat: K must be >= 1")
    if error_cov is None or _shape(error_cov) != (K, nx, nx):
        raise ValueError(f"error_cov: expected ({K}, {nx}, {nx}), got {None if error_cov is None else _shape(error_cov)}")
    if keys is None:
        raise ValueError("keys: a filter needs one key per draw")
    check_keys(keys, K)
    if init_state is None:
        if not has_init:
            raise ValueError("init_state=None draws x_0 ~ N(init_state_mean, init_state_cov): construct the HeldOutFilter with both")
        return K, 0
    si = _shape(init_state)
    if si == (nx,) or (nx == 1 and si == ()):
        return K, 1
    if si == (K, nx):
        return K, 2
    if si == (K, N, nx):
        return K, 3
    raise ValueError(f"init_state: expected ({nx},), ({K}, {nx}) or ({K}, {N}, {nx}), got {si}")


def check_forecast(nx, M, N, T, has_init, coeff_mat, error_cov, keys, horizon, init_state=None):
    """Validates the arguments of a forecast call from their shapes alone (nothing is copied, no device is touched): check_call's
    refusals, and a horizon that is not an integer in 1..T -> (K, x0_mode, H)."""
    K, mode = check_call(nx, M, N, has_init, coeff_mat, error_cov, keys, init_state)
    return K, mode, check_horizon(horizon, T)


class FilterResult:
    """What a filter call returns, device tensors: n particles per draw; loglik (K) = sum_t ell[:, t] over the rows without a NaN; ell
    (K, T) = log p(y_t | y_{0:t-1}); with moments ess (K, T), pred_sum / pred_sumsq (K, T, nx + ny) (sums over the unweighted predictive
    cloud of the state and the predicted observation H x and of their squares), filt_sum (K, T, nx) and wtot (K, T) (the filtered mean is
    filt_sum / wtot); with traces x (K, T, N, nx) and anc (K, T, N) int32.  What was not asked for is None."""

    FIELDS = ("loglik", "ell", "ess", "pred_sum", "pred_sumsq", "filt_sum", "wtot", "x", "anc")

    def __init__(self, n, nx, **kw):
        self.n, self.nx = int(n), int(nx)
        for f in self.FIELDS:
            setattr(self, f, kw.get(f))


def run(engine, has_init, coeff_mat, error_cov, keys, init_state=None, moments=True, traces=False):
    """The filter on `engine`'s context: validation, then one pgas_filter.  Enqueues work only."""
    nx, N = engine.nx, engine.N
    K, mode = check_call(nx, engine.M, N, has_init, coeff_mat, error_cov, keys, init_state)
    seeds = keys_tensor(keys, engine.device)
    x0 = None if mode == 0 else engine._dev(init_state, shape={1: (nx,), 2: (K, nx), 3: (K, N, nx)}[mode])
    out = engine.filter(coeff_mat, error_cov, seeds, x0, mode, bool(moments), bool(traces))
    return FilterResult(N, nx, **out)


class ForecastResult:
    """What a forecast call returns, device tensors: filter, the FilterResult of the filter call (moments and traces); horizon H; sum /
    sumsq (K, H, T, nx + ny), the sums over the n particles of the h-step-ahead cloud of the state and the predicted observation H x and
    of their squares at [k, h - 1, target row tau]; lpd (K, H, T) = log p(y_tau | y_{0:tau-h}, A_k, S_k), or None without log_score.
    Entries with tau < h - 1 (no origin row) are NaN."""

    def __init__(self, filter, horizon, sum, sumsq, lpd=None):   # noqa: A002
        self.filter, self.horizon, self.sum, self.sumsq, self.lpd = filter, int(horizon), sum, sumsq, lpd
        self.n, self.nx = filter.n, filter.nx


def run_forecast(engine, has_init, coeff_mat, error_cov, keys, horizon, init_state=None, log_score=True):
    """The forecast on `engine`'s context: validation, one pgas_filter with moments and traces, one pgas_forecast.  Enqueues work only."""
    K, _, H = check_forecast(engine.nx, engine.M, engine.N, engine.T, has_init, coeff_mat, error_cov, keys, horizon, init_state)
    flt = run(engine, has_init, coeff_mat, error_cov, keys, init_state, moments=True, traces=True)
    s1, s2, lpd = engine.forecast(coeff_mat, error_cov, keys_tensor(keys, engine.device), flt.x, H, bool(log_score))
    return ForecastResult(flt, H, s1, s2, lpd)


def check_smooth(nx, M, N, has_init, coeff_mat, error_cov, keys, n_trajectories, init_state=None):
    """Validates the arguments of a smooth call from their shapes alone (nothing is copied, no device is touched): check_call's refusals,
    and an n_trajectories that is not an integer in 1..65536 -> (K, x0_mode, n_trajectories)."""
    K, mode = check_call(nx, M, N, has_init, coeff_mat, error_cov, keys, init_state)
    return K, mode, check_n_trajectories(n_trajectories)


class SmoothResult:
    """What a smooth call returns, device tensors: filter, the FilterResult of the filter call (moments and traces); n_trajectories B;
    sum / sumsq (K, T, nx + ny), the sums over the B backward-simulation trajectories of the smoothed state and of H x and of their
    squares; with trajectories xs (K, B, T, nx); with indices idx (K, B, T) int32, the particle of the trace each state is.  What was
    not asked for is None."""

    def __init__(self, filter, n_trajectories, sum, sumsq, xs=None, idx=None):   # noqa: A002
        self.filter, self.n_trajectories, self.sum, self.sumsq, self.xs, self.idx = filter, int(n_trajectories), sum, sumsq, xs, idx
        self.n, self.nx = filter.n, filter.nx


def run_smooth(engine, has_init, coeff_mat, error_cov, keys, n_trajectories, init_state=None, trajectories=False, indices=False):
    """The smoother on `engine`'s context: validation, one pgas_filter with moments and traces, one pgas_smooth per 256 trajectories; the
    chunks' sums are added elementwise in ascending chunk order, starting from the first chunk's.  Enqueues work only."""
    K, _, B = check_smooth(engine.nx, engine.M, engine.N, has_init, coeff_mat, error_cov, keys, n_trajectories, init_state)
    flt = run(engine, has_init, coeff_mat, error_cov, keys, init_state, moments=True, traces=True)
    seeds = keys_tensor(keys, engine.device)
    s1 = s2 = None
    xs, idx = [], []
    for b0 in range(0, B, SMOOTH_CHUNK):
        a1, a2, x, j = engine.smooth(coeff_mat, error_cov, seeds, flt.x, flt.anc, min(SMOOTH_CHUNK, B - b0), b0, True, bool(trajectories), bool(indices))
        s1, s2 = (a1, a2) if s1 is None else (s1 + a1, s2 + a2)
        xs.append(x)
        idx.append(j)
    cat = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)   # noqa: E731
    return SmoothResult(flt, B, s1, s2, cat(xs) if trajectories else None, cat(idx) if indices else None)


def check_forecast_cdf(nx, ny, M, N, T, has_init, coeff_mat, error_cov, keys, horizon, thresholds=None, init_state=None):
    """check_forecast's refusals, then the thresholds (a filter context always has observations) -> (K, x0_mode, H, J, form)."""
    K, mode, H = check_forecast(nx, M, N, T, has_init, coeff_mat, error_cov, keys, horizon, init_state)
    J, form = check_thresholds(T, nx, ny, thresholds, True)
    return K, mode, H, J, form


def run_forecast_cdf(engine, has_init, observations, coeff_mat, error_cov, keys, horizon, thresholds=None, observation_noise=True, init_state=None):
    """``forecast_cdf`` on `engine`'s context: validation, one pgas_filter with traces, one pgas_forecast_cdf.  Enqueues work only."""
    K, _, H, J, form = check_forecast_cdf(engine.nx, engine.ny, engine.M, engine.N, engine.T, has_init, coeff_mat, error_cov, keys, horizon, thresholds,
                                          init_state)
    th = device_thresholds(engine, thresholds, J, form, observations)
    flt = run(engine, has_init, coeff_mat, error_cov, keys, init_state, moments=False, traces=True)
    count = engine.forecast_cdf(coeff_mat, error_cov, keys_tensor(keys, engine.device), flt.x, H, th, bool(observation_noise))
    return CdfCounts(engine.N, count, th, nx=engine.nx, pit=form == "pit")


class HeldOutFilter:
    def __init__(self, observations, inputs, basis_fcn, likelihood_fcn, n_x, n_particles, init_state_mean=None, init_state_cov=None, device=None):
        """A context over a held-out record: observations (T,) or (T, ny) scored under likelihood_fcn (a GaussianLikelihood), inputs (T,),
        (T, nu) or (T, 0), n_particles <= 1024.  The device context is created by the first call."""
        if not isinstance(basis_fcn, BasisMap):
            raise TypeError("basis_fcn must be a pgas_amd.BasisMap descriptor, e.g. basis.on(sel=[0, 1])")
        if not isinstance(likelihood_fcn, GaussianLikelihood):
            raise TypeError("likelihood_fcn must be a pgas_amd.GaussianLikelihood descriptor")
        self.n_x = int(n_x)
        if self.n_x < 1:
            raise ValueError("n_x must be >= 1")
        if likelihood_fcn.nx != self.n_x:
            raise ValueError(f"likelihood_fcn: H has {likelihood_fcn.nx} columns, n_x = {self.n_x}")
        self.n_particles = int(n_particles)
        if self.n_particles < 1 or self.n_particles > MAX_PARTICLES:
            raise ValueError(f"n_particles: expected 1..{MAX_PARTICLES}, got {n_particles}")
        so = _shape(observations)
        if len(so) < 1 or so[0] < 1:
            raise ValueError("observations: expected T >= 1 rows")
        self.T = int(so[0])
        if so != (self.T, likelihood_fcn.ny) and not (likelihood_fcn.ny == 1 and so == (self.T,)):
            raise ValueError(f"observations: expected ({self.T},) or ({self.T}, {likelihood_fcn.ny}), got {so}")
        self.observations = np.asarray(observations, dtype=np.float64).reshape(self.T, likelihood_fcn.ny)
        self.inputs = np.asarray(inputs, dtype=np.float64)
        if self.inputs.ndim < 1 or self.inputs.shape[0] != self.T:
            raise ValueError(f"inputs: expected {self.T} rows ((T,), (T, nu) or (T, 0)), one per observation row")
        self.basis_fcn, self.likelihood_fcn = basis_fcn, likelihood_fcn
        if (init_state_mean is None) != (init_state_cov is None):
            raise ValueError("init_state_mean and init_state_cov go together")
        self.has_init = init_state_mean is not None
        self.init_state_mean = np.asarray(init_state_mean, dtype=np.float64).reshape(-1) if self.has_init else np.zeros(self.n_x)
        self.init_state_cov = np.atleast_2d(np.asarray(init_state_cov, dtype=np.float64)) if self.has_init else np.eye(self.n_x)
        if self.init_state_mean.shape != (self.n_x,) or self.init_state_cov.shape != (self.n_x, self.n_x):
            raise ValueError(f"init_state_mean / init_state_cov: expected ({self.n_x},) and ({self.n_x}, {self.n_x})")
        self._device = device
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            self._engine = Engine(self.n_particles, self.observations, self.inputs, self.init_state_mean, self.init_state_cov, self.likelihood_fcn,
                                  self.basis_fcn, device=self._device)
        return self._engine

    def __call__(self, coeff_mat, error_cov, keys, init_state=None, moments=True, traces=False):
        """coeff_mat (K, nx, M); error_cov (K, nx, nx); keys: K integers or a (K,) int64 device tensor; init_state (nx), (K, nx),
        (K, N, nx) or None (x_0 ~ N(init_state_mean, init_state_cov) from the draw's key) -> FilterResult.  ValueError before any launch
        for arguments that do not fit."""
        check_call(self.n_x, self.basis_fcn.basis.M, self.n_particles, self.has_init, coeff_mat, error_cov, keys, init_state)
        return run(self.engine, self.has_init, coeff_mat, error_cov, keys, init_state, moments, traces)

    def forecast(self, coeff_mat, error_cov, keys, horizon, init_state=None, log_score=True):
        """The call above with moments and traces, then the h-step-ahead predictions for h = 1 .. horizon <= T from every origin row of
        every draw in one more launch -> ForecastResult.  ValueError before any launch for arguments that do not fit."""
        check_forecast(self.n_x, self.basis_fcn.basis.M, self.n_particles, self.T, self.has_init, coeff_mat, error_cov, keys, horizon, init_state)
        return run_forecast(self.engine, self.has_init, coeff_mat, error_cov, keys, horizon, init_state, log_score)

    def forecast_cdf(self, coeff_mat, error_cov, keys, horizon, thresholds=None, observation_noise=True, init_state=None):
        """The filter with its traces, then the h-step-ahead clouds of ``forecast`` counted against the thresholds of the target row in one
        more launch -> CdfCounts(n, count (K, H, T, nx + ny, J) int32, thresholds (T, nx + ny, J)); -1 where the target row is < h - 1.
        thresholds as ``Rollout.cdf`` (None: the record's observations, the PIT); observation_noise adds LR e to the predicted
        observation, which a PIT of the observations needs.  K = 64, H = 16, T = 2000, J = 16 is 393 MB of counts (J = 1: 25 MB).
        ValueError before any launch."""
        check_forecast_cdf(self.n_x, self.likelihood_fcn.ny, self.basis_fcn.basis.M, self.n_particles, self.T, self.has_init, coeff_mat, error_cov, keys,
                           horizon, thresholds, init_state)
        return run_forecast_cdf(self.engine, self.has_init, self.observations, coeff_mat, error_cov, keys, horizon, thresholds, observation_noise, init_state)

    def smooth(self, coeff_mat, error_cov, keys, n_trajectories, init_state=None, trajectories=False, indices=False):
        """The filter with moments and traces, then n_trajectories <= 65536 backward-simulation draws of the state sequence given the
        whole record, per draw, one more launch per 256 trajectories -> SmoothResult.  Trajectory g of draw k depends
        on (key k, g) alone.  ValueError before any launch for arguments that do not fit."""
        check_smooth(self.n_x, self.basis_fcn.basis.M, self.n_particles, self.has_init, coeff_mat, error_cov, keys, n_trajectories, init_state)
        return run_smooth(self.engine, self.has_init, coeff_mat, error_cov, keys, n_trajectories, init_state, trajectories, indices)


def _t(a, like):
    return torch.as_tensor(np.asarray(a, dtype=np.float64) if not isinstance(a, torch.Tensor) else a, dtype=torch.float64, device=like.device)


def evidence_summary(result, y=None):
    """Plain torch on the small tensors of a FilterResult: dict of log_evidence = logsumexp_k loglik[k] - log K (the log
    posterior-predictive evidence of the record); with the moments x_pred_mean, x_pred_std (T, nx) and y_pred_mean, y_pred_std (T, ny),
    the one-step-ahead prediction over draws and particles (divisor K n, variance clamped at 0), and x_filt_mean (K, T, nx) = filt_sum /
    wtot (NaN where no particle had weight) with x_filt_mean_pooled (T, nx), its mean over the draws; with y (T,) or (T, ny) also rmse =
    sqrt(mean((y_pred_mean - y)^2)) over the entries of y that are not NaN."""
    ll = torch.as_tensor(result.loglik, dtype=torch.float64)
    K = int(ll.shape[0])
    out = {"log_evidence": torch.logsumexp(ll, dim=0) - float(np.log(K))}
    if result.pred_sum is None:
        if y is not None:
            raise ValueError("y: the RMSE of the predicted observation needs the moments (moments=True)")
        return out
    nx, kn = int(result.nx), float(K * result.n)
    mean = result.pred_sum.sum(dim=0) / kn
    std = torch.sqrt(torch.clamp(result.pred_sumsq.sum(dim=0) / kn - mean * mean, min=0.0))
    out.update(x_pred_mean=mean[:, :nx], x_pred_std=std[:, :nx], y_pred_mean=mean[:, nx:], y_pred_std=std[:, nx:])
    filt = result.filt_sum / result.wtot[..., None]
    out.update(x_filt_mean=filt, x_filt_mean_pooled=filt.mean(dim=0))
    if y is not None:
        pred = out["y_pred_mean"]
        yy = _t(y, pred)
        if yy.numel() != pred.numel() or yy.shape[0] != pred.shape[0]:
            raise ValueError(f"y: expected {tuple(pred.shape)}, got {tuple(yy.shape)}")
        yy = yy.reshape(pred.shape)
        ok = ~torch.isnan(yy)
        out["rmse"] = torch.sqrt(torch.mean((pred - yy)[ok] ** 2))
    return out


def smoothing_summary(result, y=None):
    """Plain torch on the small tensors of a SmoothResult: dict of x_smooth_mean, x_smooth_std (T, nx) and y_smooth_mean, y_smooth_std
    (T, ny), the smoothed state and H x pooled over draws and trajectories (divisor K n_trajectories, variance clamped at 0), and
    x_smooth_mean_draw (K, T, nx), the smoothed mean per draw; with y (T,) or (T, ny) also rmse = sqrt(mean((y_smooth_mean - y)^2)) over
    the entries of y that are not NaN."""
    K = int(result.sum.shape[0])
    nx, B = int(result.nx), float(result.n_trajectories)
    mean = result.sum.sum(dim=0) / (K * B)
    std = torch.sqrt(torch.clamp(result.sumsq.sum(dim=0) / (K * B) - mean * mean, min=0.0))
    out = dict(x_smooth_mean=mean[:, :nx], x_smooth_std=std[:, :nx], y_smooth_mean=mean[:, nx:], y_smooth_std=std[:, nx:],
               x_smooth_mean_draw=result.sum[..., :nx] / B)
    if y is not None:
        pred = out["y_smooth_mean"]
        yy = _t(y, pred)
        if yy.numel() != pred.numel() or yy.shape[0] != pred.shape[0]:
            raise ValueError(f"y: expected {tuple(pred.shape)}, got {tuple(yy.shape)}")
        yy = yy.reshape(pred.shape)
        ok = ~torch.isnan(yy)
        out["rmse"] = torch.sqrt(torch.mean((pred - yy)[ok] ** 2))
    return out


def forecast_summary(result, y=None):
    """Plain torch on the small tensors of a ForecastResult, per horizon h = 1 .. H (index h - 1): dict of x_pred_mean, x_pred_std
    (H, T, nx) and y_pred_mean, y_pred_std (H, T, ny), the h-step-ahead prediction of row tau pooled over draws and particles (divisor
    K n, variance clamped at 0; NaN where tau < h - 1); with the log score log_score (H) = the mean over the defined rows tau >= h - 1
    whose lpd is not NaN of logsumexp_k lpd[k, h - 1, tau] - log K (NaN for a horizon without such a row); with y (T,) or (T, ny) also
    rmse (H) = sqrt(mean((y_pred_mean - y)^2)) over the defined entries whose y is not NaN."""
    K, H, T = (int(v) for v in result.sum.shape[:3])
    nx, kn = int(result.nx), float(K * result.n)
    mean = result.sum.sum(dim=0) / kn
    std = torch.sqrt(torch.clamp(result.sumsq.sum(dim=0) / kn - mean * mean, min=0.0))
    out = dict(x_pred_mean=mean[..., :nx], x_pred_std=std[..., :nx], y_pred_mean=mean[..., nx:], y_pred_std=std[..., nx:])
    tau = torch.arange(T, device=mean.device)
    defined = tau[None, :] >= torch.arange(H, device=mean.device)[:, None]   # (H, T): an origin row exists
    if result.lpd is not None:
        pooled = torch.logsumexp(result.lpd, dim=0) - float(np.log(K))       # NaN where a draw's lpd is (a NaN observation row)
        ok = defined & ~torch.isnan(pooled)
        cnt = ok.sum(dim=1)
        tot = torch.where(ok, pooled, torch.zeros_like(pooled)).sum(dim=1)
        out["log_score"] = torch.where(cnt > 0, tot / cnt.clamp(min=1), torch.full_like(tot, float("nan")))
    if y is not None:
        pred = out["y_pred_mean"]
        yy = _t(y, pred)
        if yy.numel() != pred[0].numel() or yy.shape[0] != T:
            raise ValueError(f"y: expected {tuple(pred.shape[1:])}, got {tuple(yy.shape)}")
        yy = yy.reshape(pred.shape[1:])
        ok = defined[:, :, None] & ~torch.isnan(yy)[None]
        cnt = ok.sum(dim=(1, 2))
        sq = torch.where(ok, (pred - yy[None]) ** 2, torch.zeros_like(pred)).sum(dim=(1, 2))
        out["rmse"] = torch.where(cnt > 0, torch.sqrt(sq / cnt.clamp(min=1)), torch.full_like(sq, float("nan")))
    return out
