"""Open-loop simulation of the learned transition model under many posterior draws in one launch.

``PGAS``, ``MultiChainPGAS`` and their chain logs return draws ``(A_k, S_k)`` of the basis-function model
x_t ~ N(A phi(x_{t-1}, u_t), S).  The reference simulates one parameter matrix forward on validation inputs
(EMPS_Validation_Simulation, src/EMPS.py:129-151); here every kept draw is rolled forward, with or without process noise:

* ``Rollout(inputs, basis_fcn, n_x, init_state_mean=None, init_state_cov=None)``: a context of its own over a validation input
  sequence; ``__call__(coeff_mat (K, nx, M), error_cov=None, keys=None, replicates=1, init_state=None) -> (K, T, P, nx)``.
* ``condSequentialMonteCarlo.rollout`` / ``condSequentialMonteCarloChains.rollout``: the same call on a training context.
* ``rollout_summary(sim, H=None, y=None)``: predictive mean and standard deviation per time step, and the validation RMSE.
* ``Rollout.predict(...)`` (and ``.predict`` of the two training contexts): the same rollout reduced over its replicates inside the
  kernel -- per draw and step the sums and sums of squares of the state and of the predicted observation H x (+ measurement noise), and
  the log predictive density of the observations; the (K, T, P, nx) cloud is never stored.  ``predictive_summary(stats, y=None)`` turns
  them into the predictive band, the validation RMSE and the log score.
* ``Rollout.cdf(...)`` (and ``.cdf`` of the two training contexts): the same rollout counted against thresholds inside the kernel --
  per draw, step, channel and threshold the number of replicates at or below it; ``calibration_summary`` pools
  the counts over the draws into the predictive CDF, the PIT of the observations and interval coverage.

Step t reads input row t, as the sweep's propagation does (x_t = A phi(x_{t-1}, inputs[t]) + LS z_t): a caller that pairs x_{t-1} with
u_{t-1}, as the reference's validation loop does, passes the input sequence shifted by one row.  Replicate p of draw k uses the Philox
counters of particle p of a sweep with key k, so a rollout does not depend on how its replicates are split over launches.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import Engine
from .calibration import CdfCounts, check_thresholds, device_thresholds
from .chains import keys_tensor
from .descriptors import BasisMap, GaussianLikelihood

MAX_REPLICATES_PER_LAUNCH = 1024   # pgas_rollout: P <= 1024; more replicates run in chunks through p0
MAX_REPLICATES_PREDICT = 1 << 20   # pgas_rollout_stats: one call, a block of 1024 replicates per workgroup


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else tuple(np.shape(a))


def check_call(nx, M, has_init, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None, *, predict=False, observation_noise=False,
               log_score=None, has_observations=False):
    """Validates the arguments of a rollout from their shapes alone (nothing is copied, no device is touched) -> (K, P, x0_mode).
    predict=True: the call is ``predict`` (replicates <= 2^20 in one call; observation_noise needs the draws' keys; log_score=True needs
    observations)."""
    s = _shape(coeff_mat)
    if len(s) != 3 or s[1:] != (nx, M):
        raise ValueError(f"coeff_mat: expected (K, {nx}, {M}), got {s}")
    K = int(s[0])
    if K < 1:
        raise ValueError("coeff_mat: K must be >= 1")
    P = int(replicates)
    if P < 1:
        raise ValueError(f"replicates must be >= 1, got {replicates}")
    if predict:
        if P > MAX_REPLICATES_PREDICT:
            raise ValueError(f"replicates must be <= {MAX_REPLICATES_PREDICT} in one predict call, got {replicates}")
        if observation_noise and (error_cov is None or keys is None):
            raise ValueError("observation_noise needs keys (and error_cov): the measurement noise is drawn from the draw's key")
        if log_score and not has_observations:
            raise ValueError("log_score=True needs observations: construct the Rollout with likelihood_fcn and observations")
    if error_cov is not None:
        if _shape(error_cov) != (K, nx, nx):
            raise ValueError(f"error_cov: expected ({K}, {nx}, {nx}), got {_shape(error_cov)}")
        if keys is None:
            raise ValueError("a rollout with process noise (error_cov) needs keys, one per draw")
        nk = _shape(keys) if isinstance(keys, torch.Tensor) else (len(keys),)
        if isinstance(keys, torch.Tensor) and (keys.dtype != torch.int64 or keys.dim() != 1):
            raise ValueError("keys: expected K integers or a (K,) int64 tensor of key bit patterns")
        if nk != (K,):
            raise ValueError(f"keys: expected {K} keys, got {nk[0] if nk else 0}")
    if init_state is None:
        if error_cov is None:
            raise ValueError("a noise-free rollout needs init_state (a drawn x_0 comes from the draw's key)")
        if not has_init:
            raise ValueError("init_state=None draws x_0 ~ N(init_state_mean, init_state_cov): construct the Rollout with both")
        mode = 0
    else:
        si = _shape(init_state)
        if si == (nx,) or (nx == 1 and si == ()):
            mode = 1
        elif si == (K, nx):
            mode = 2
        elif si == (K, P, nx):
            mode = 3
        else:
            raise ValueError(f"init_state: expected ({nx},), ({K}, {nx}) or ({K}, {P}, {nx}), got {si}")
    if error_cov is None and P > 1 and mode != 3:
        raise ValueError("a noise-free rollout of replicates > 1 needs a per-replicate init_state (K, P, nx): its replicates would be copies")
    return K, P, mode


def run(engine, has_init, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None):
    """The rollout on `engine`'s context: validation, then one pgas_rollout per chunk of 1024 replicates.  Enqueues work only."""
    nx = engine.nx
    K, P, mode = check_call(nx, engine.M, has_init, coeff_mat, error_cov, keys, replicates, init_state)
    noisy = error_cov is not None
    seeds = keys_tensor(keys, engine.device) if noisy else None
    A = engine._dev(coeff_mat, shape=(K, nx, engine.M))
    S = engine._dev(error_cov, shape=(K, nx, nx)) if noisy else None
    x0 = None if mode == 0 else engine._dev(init_state, shape={1: (nx,), 2: (K, nx), 3: (K, P, nx)}[mode])
    if P <= MAX_REPLICATES_PER_LAUNCH:
        return engine.rollout(A, S, seeds, P, 0, x0, mode)
    out = torch.empty((K, engine.T, P, nx), dtype=torch.float64, device=engine.device)
    for p0 in range(0, P, MAX_REPLICATES_PER_LAUNCH):   # particle counters are global: the chunks are the replicates of one rollout
        n = min(MAX_REPLICATES_PER_LAUNCH, P - p0)
        xc = x0[:, p0:p0 + n].contiguous() if mode == 3 else x0
        out[:, :, p0:p0 + n] = engine.rollout(A, S, seeds, n, p0, xc, mode)
    return out


class PredictiveStats:
    """What ``predict`` returns, device tensors: n replicates per draw; x_sum, x_sumsq (K, T, nx) and y_sum, y_sumsq (K, T, ny), the sums
    over the replicates of the state, the predicted observation and their squares; lpd (K, T) = log (1/n) sum_p p(y_t | x_t^p), or None."""

    def __init__(self, n, x_sum, x_sumsq, y_sum, y_sumsq, lpd):
        self.n, self.x_sum, self.x_sumsq, self.y_sum, self.y_sumsq, self.lpd = int(n), x_sum, x_sumsq, y_sum, y_sumsq, lpd


def run_predict(engine, has_init, has_observations, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None, observation_noise=False,
                log_score=None):
    """``predict`` on `engine`'s context: validation, then one pgas_rollout_stats.  Enqueues work only."""
    nx = engine.nx
    K, P, mode = check_call(nx, engine.M, has_init, coeff_mat, error_cov, keys, replicates, init_state, predict=True, observation_noise=observation_noise,
                            log_score=log_score, has_observations=has_observations)
    score = has_observations if log_score is None else bool(log_score)
    noisy = error_cov is not None
    seeds = keys_tensor(keys, engine.device) if noisy else None
    A = engine._dev(coeff_mat, shape=(K, nx, engine.M))
    S = engine._dev(error_cov, shape=(K, nx, nx)) if noisy else None
    x0 = None if mode == 0 else engine._dev(init_state, shape={1: (nx,), 2: (K, nx), 3: (K, P, nx)}[mode])
    s1, s2, lpd = engine.rollout_stats(A, S, seeds, P, 0, x0, mode, bool(observation_noise), score)
    return PredictiveStats(P, s1[..., :nx], s2[..., :nx], s1[..., nx:], s2[..., nx:], lpd)


def check_cdf(nx, ny, M, T, has_init, has_observations, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None, thresholds=None,
              observation_noise=False):
    """Validates the arguments of ``cdf`` from their shapes alone (no device is touched): ``predict``'s refusals through check_call, then
    the thresholds -> (K, P, x0_mode, J, form)."""
    K, P, mode = check_call(nx, M, has_init, coeff_mat, error_cov, keys, replicates, init_state, predict=True, observation_noise=observation_noise)
    J, form = check_thresholds(T, nx, ny, thresholds, has_observations)
    return K, P, mode, J, form


def run_cdf(engine, has_init, observations, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None, thresholds=None, observation_noise=False):
    """``cdf`` on `engine`'s context: validation, then one pgas_rollout_cdf.  observations: the (T, ny) array ``thresholds=None`` counts
    against, or None.  Enqueues work only."""
    nx = engine.nx
    K, P, mode, J, form = check_cdf(nx, engine.ny, engine.M, engine.T, has_init, observations is not None, coeff_mat, error_cov, keys, replicates, init_state,
                                    thresholds, observation_noise)
    noisy = error_cov is not None
    seeds = keys_tensor(keys, engine.device) if noisy else None
    A = engine._dev(coeff_mat, shape=(K, nx, engine.M))
    S = engine._dev(error_cov, shape=(K, nx, nx)) if noisy else None
    x0 = None if mode == 0 else engine._dev(init_state, shape={1: (nx,), 2: (K, nx), 3: (K, P, nx)}[mode])
    th = device_thresholds(engine, thresholds, J, form, observations)
    count = engine.rollout_cdf(A, S, seeds, P, 0, x0, mode, bool(observation_noise), th)
    return CdfCounts(P, count, th, nx=nx, pit=form == "pit")


class Rollout:
    def __init__(self, inputs, basis_fcn, n_x, init_state_mean=None, init_state_cov=None, device=None, likelihood_fcn=None, observations=None):
        """A context over the validation inputs (T = number of input rows).  Without likelihood_fcn / observations the observations are
        zeros and the likelihood a unit Gaussian on the first state: a rollout reads neither.  ``predict`` forms the predicted observation
        and its measurement noise from likelihood_fcn (a GaussianLikelihood) and scores `observations` (T,) or (T, ny) under it.  The device
        context is created by the first call."""
        if not isinstance(basis_fcn, BasisMap):
            raise TypeError("basis_fcn must be a pgas_amd.BasisMap descriptor, e.g. basis.on(sel=[0, 1])")
        self.n_x = int(n_x)
        if self.n_x < 1:
            raise ValueError("n_x must be >= 1")
        self.inputs = np.asarray(inputs, dtype=np.float64)
        if self.inputs.ndim < 1 or self.inputs.shape[0] < 1:
            raise ValueError("inputs: expected T >= 1 rows ((T,), (T, nu) or (T, 0))")
        self.T = int(self.inputs.shape[0])
        self.basis_fcn = basis_fcn
        if (init_state_mean is None) != (init_state_cov is None):
            raise ValueError("init_state_mean and init_state_cov go together")
        self.has_init = init_state_mean is not None
        self.init_state_mean = np.asarray(init_state_mean, dtype=np.float64).reshape(-1) if self.has_init else np.zeros(self.n_x)
        self.init_state_cov = np.atleast_2d(np.asarray(init_state_cov, dtype=np.float64)) if self.has_init else np.eye(self.n_x)
        if self.init_state_mean.shape != (self.n_x,) or self.init_state_cov.shape != (self.n_x, self.n_x):
            raise ValueError(f"init_state_mean / init_state_cov: expected ({self.n_x},) and ({self.n_x}, {self.n_x})")
        if likelihood_fcn is not None and not isinstance(likelihood_fcn, GaussianLikelihood):
            raise TypeError("likelihood_fcn must be a pgas_amd.GaussianLikelihood descriptor")
        if likelihood_fcn is not None and likelihood_fcn.nx != self.n_x:
            raise ValueError(f"likelihood_fcn: H has {likelihood_fcn.nx} columns, n_x = {self.n_x}")
        if observations is not None and likelihood_fcn is None:
            raise ValueError("observations need the likelihood_fcn they are scored under")
        self.likelihood_fcn = likelihood_fcn
        self.has_observations = observations is not None
        self.observations = None
        if self.has_observations:
            so = _shape(observations)
            if so != (self.T, likelihood_fcn.ny) and not (likelihood_fcn.ny == 1 and so == (self.T,)):
                raise ValueError(f"observations: expected ({self.T},) or ({self.T}, {likelihood_fcn.ny}), got {so}")
            self.observations = np.asarray(observations, dtype=np.float64).reshape(self.T, likelihood_fcn.ny)
        self._device = device
        self._engine = None

    def _engine_args(self):
        """(N, observations, inputs, init_state_mean, init_state_cov, likelihood, basis_map) of the context's Engine."""
        lik = GaussianLikelihood(np.eye(1, self.n_x), np.eye(1)) if self.likelihood_fcn is None else self.likelihood_fcn
        y = self.observations if self.has_observations else np.zeros((self.T, lik.ny))
        return 1, y, self.inputs, self.init_state_mean, self.init_state_cov, lik, self.basis_fcn

    @property
    def engine(self):
        if self._engine is None:
            self._engine = Engine(*self._engine_args(), device=self._device)
        return self._engine

    def __call__(self, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None):
        """coeff_mat (K, nx, M); error_cov (K, nx, nx) or None (noise-free: replicates == 1 or a per-replicate init_state); keys: K integers
        or a (K,) int64 device tensor; init_state (nx), (K, nx), (K, P, nx) or None (x_0 ~ N(init_state_mean, init_state_cov) from the
        draw's key) -> fp64 device tensor (K, T, P, nx).  ValueError before any launch for arguments that do not fit."""
        check_call(self.n_x, self.basis_fcn.basis.M, self.has_init, coeff_mat, error_cov, keys, replicates, init_state)
        return run(self.engine, self.has_init, coeff_mat, error_cov, keys, replicates, init_state)

    def predict(self, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None, observation_noise=False, log_score=None):
        """The rollout of ``__call__`` (same arguments; replicates <= 2^20, one call) reduced over its replicates inside the kernel ->
        PredictiveStats(n, x_sum, x_sumsq, y_sum, y_sumsq, lpd).  The predicted observation is H x, with observation_noise H x + LR e (e from
        the draw's key, needs keys); log_score (default: observations were given) adds lpd (K, T), the log predictive density of the
        observation rows.  Replicate p carries the state ``__call__`` returns for it.  ValueError before any launch."""
        kw = dict(predict=True, observation_noise=observation_noise, log_score=log_score, has_observations=self.has_observations)
        check_call(self.n_x, self.basis_fcn.basis.M, self.has_init, coeff_mat, error_cov, keys, replicates, init_state, **kw)
        return run_predict(self.engine, self.has_init, self.has_observations, coeff_mat, error_cov, keys, replicates, init_state, observation_noise, log_score)

    def cdf(self, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None, thresholds=None, observation_noise=False):
        """The rollout of ``predict`` (same arguments) counted against thresholds inside the kernel -> CdfCounts(n, count (K, T, nx + ny, J)
        int32, thresholds (T, nx + ny, J)): count[k, t, c, j] replicates have value channel c (the state, then the predicted observation
        H x, with observation_noise H x + LR e) <= thresholds[t, c, j].  thresholds: (T, nx + ny, J) for all channels; (T, ny, J) for the
        predicted observations only (the state channels get NaN thresholds and count 0); (T,) or (T, ny): J = 1; None: the context's
        observations (the PIT; ValueError without observations).  J <= 16.  ValueError before any launch."""
        ny = 1 if self.likelihood_fcn is None else self.likelihood_fcn.ny
        check_cdf(self.n_x, ny, self.basis_fcn.basis.M, self.T, self.has_init, self.has_observations, coeff_mat, error_cov, keys, replicates, init_state,
                  thresholds, observation_noise)
        return run_cdf(self.engine, self.has_init, self.observations, coeff_mat, error_cov, keys, replicates, init_state, thresholds, observation_noise)


def rollout_summary(sim, H=None, y=None):
    """Plain torch on a rollout (K, T, P, nx): dict(mean (T, nx), std (T, nx)) over draws and replicates (std: the spread of the K P
    simulated states about their mean, divisor K P); with y (T,) or (T, ny) also rmse = sqrt(mean((mean H^T - y)^2)) -- with H picking
    the measured component, what the reference's EMPS_Validation_Simulation returns (src/EMPS.py:149-151).  H defaults to the identity."""
    sim = torch.as_tensor(sim, dtype=torch.float64)
    if sim.dim() != 4:
        raise ValueError(f"sim: expected (K, T, P, nx), got {tuple(sim.shape)}")
    T, nx = sim.shape[1], sim.shape[3]
    flat = sim.permute(1, 0, 2, 3).reshape(T, -1, nx)
    out = dict(mean=flat.mean(dim=1), std=flat.std(dim=1, correction=0))
    if y is not None:
        Hm = torch.eye(nx, dtype=torch.float64, device=sim.device) if H is None else \
            torch.as_tensor(np.atleast_2d(np.asarray(H, dtype=np.float64)) if not isinstance(H, torch.Tensor) else H, dtype=torch.float64, device=sim.device)
        yy = torch.as_tensor(np.asarray(y, dtype=np.float64) if not isinstance(y, torch.Tensor) else y, dtype=torch.float64, device=sim.device).reshape(T, -1)
        pred = out["mean"] @ Hm.reshape(-1, nx).T
        if pred.shape != yy.shape:
            raise ValueError(f"y: expected ({T}, {pred.shape[1]}), got {tuple(yy.shape)}")
        out["rmse"] = torch.sqrt(torch.mean((pred - yy) ** 2))
    return out


def predictive_summary(stats, y=None):
    """Plain torch on the small tensors of ``predict``: dict of per-draw x_mean, x_std (K, T, nx) and y_mean, y_std (K, T, ny) (divisor n,
    variance clamped at 0); pooled over the K draws x_mean_pooled, x_std_pooled (T, nx), y_mean_pooled, y_std_pooled (T, ny) (divisor K n);
    with y (T,) or (T, ny) rmse = sqrt(mean((y_mean_pooled - y)^2)); with stats.lpd elpd_t (T,) = logsumexp_k lpd[k, t] - log K and elpd,
    its sum over t."""
    K, n = int(stats.x_sum.shape[0]), float(stats.n)
    out = {}
    for name, s1, s2 in (("x", stats.x_sum, stats.x_sumsq), ("y", stats.y_sum, stats.y_sumsq)):
        mean = s1 / n
        out[name + "_mean"] = mean
        out[name + "_std"] = torch.sqrt(torch.clamp(s2 / n - mean * mean, min=0.0))
        pm = s1.sum(dim=0) / (K * n)
        out[name + "_mean_pooled"] = pm
        out[name + "_std_pooled"] = torch.sqrt(torch.clamp(s2.sum(dim=0) / (K * n) - pm * pm, min=0.0))
    if y is not None:
        pred = out["y_mean_pooled"]
        yy = torch.as_tensor(np.asarray(y, dtype=np.float64) if not isinstance(y, torch.Tensor) else y, dtype=torch.float64, device=pred.device)
        yy = yy.reshape(pred.shape[0], -1)
        if pred.shape != yy.shape:
            raise ValueError(f"y: expected {tuple(pred.shape)}, got {tuple(yy.shape)}")
        out["rmse"] = torch.sqrt(torch.mean((pred - yy) ** 2))
    if stats.lpd is not None:
        out["elpd_t"] = torch.logsumexp(stats.lpd, dim=0) - float(np.log(K))
        out["elpd"] = out["elpd_t"].sum()
    return out
