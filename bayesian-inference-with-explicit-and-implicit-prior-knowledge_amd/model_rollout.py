"""Open-loop simulation of a grey-box model under many coefficient draws in one launch.

Algorithm1 / Algorithm2 learn latent functions xi_i = A_i phi_i(.) that enter a known model (f_x, an RK4 step of the physics) as interface
variables.  The reference validates what it learned by simulating that model open-loop on validation inputs for ONE coefficient matrix
(EMPS_Validation_Simulation, src/EMPS.py:129-151: ``F = GP_Mean @ basis_fcn(X[i-1]); X[i] = f_x(X[i-1], Tau[i-1], F)``).  Here the time
loop runs inside one kernel (k_model_rollout) for K coefficient sets and P replicates each:

* ``ModelRollout(inputs, SSM, basis_fcn, init_state_mean=None, init_state_cov=None)`` over a ``SymbolicStateSpaceModel``;
  ``__call__(coeffs, keys=None, replicates=1, init_state=None, row_cov=None, process_noise=True, outputs=False) -> (K, T, P, nx)``
  [and ``(K, T, P, ny)``].
* ``ModelRollout(..., observations=...)`` and ``predict(coeffs, ...) -> PredictiveStats``: the same rollout reduced over its replicates
  inside the kernel (k_model_rollout_stats) -- per draw and step the sums and sums of squares of the state and of the predicted
  observation g(x, u, xi) (+ observation noise), and the log predictive density of the observation rows; neither cloud is stored.
  ``pgas_amd.predictive_summary`` turns the result into the predictive band, the validation RMSE and the log score.
* ``filter(coeffs, keys, particles, ...) -> ModelFilterResult``: the model closed-loop on the observation rows -- a bootstrap particle
  filter per draw, all draws in one launch (k_model_filter): the one-step-ahead predictive density, its sum (the log
  marginal likelihood of the record per draw) and the filtered state.  ``pgas_amd.evidence_summary`` works on the result.
* ``forecast(coeffs, keys, particles, horizon, ...) -> ModelForecastResult``: that filter with its traces, then from every row of the
  trace of every draw an open-loop rollout of horizon - 1 steps, all of them in one more launch (k_model_forecast):
  the h-step-ahead predictive moments and log score for h = 1 .. horizon.  ``pgas_amd.forecast_summary`` works on the result.
* ``smooth(coeffs, keys, particles, n_trajectories, ...) -> ModelSmoothResult``: that filter with its traces, then backward simulation
  (FFBSi) over them, up to 256 trajectories of every draw per launch (k_model_smooth): the smoothed state, the
  smoothed predicted observation and the smoothed INTERFACE variable xi_t given the whole record.  ``pgas_amd.smoothing_summary`` and
  ``pgas_amd.interface_summary`` work on the result.
* ``cdf(coeffs, ..., thresholds=None) -> CdfCounts`` and ``forecast_cdf(coeffs, keys, particles, horizon, thresholds=None) -> CdfCounts``:
  the open-loop rollout of ``predict`` and the h-step-ahead clouds of ``forecast`` counted against thresholds inside the kernels
  (k_model_rollout_cdf, k_model_forecast_cdf) -- with the observations as thresholds the PIT of the grey-box
  model.  ``pgas_amd.calibration_summary`` / ``predictive_bands`` work on the result.
* ``mniw_posterior_means(GP_prior, T0, T1)``: the per-iteration posterior means of a statistics trace -- the K "draws" the reference
  averages over.

Time convention: step t -> t+1 reads input row t (x_{t+1} = f(x_t, u_t, xi(x_t, u_t)), y_t = g(x_t, u_t, xi(x_t, u_t))): Algorithm1's
convention and the reference validation loop's, so a validation input sequence is passed as it is.  This is NOT the convention of
``pgas_amd.Rollout``, whose step t reads input row t for the step INTO x_t and whose callers shift the sequence by one row.
Replicate p of draw k uses the Philox counters of particle p under key k: the process noise of step t -> t+1 is row p of
``normal(key_k, STREAM_STATE, t + 1)``, exactly what ``Algorithm1._draw_states`` adds at time t + 1, so a rollout does not depend on how
its replicates are split over launches.  There is no torch fallback for a fused time loop: a model or feature the tracer does not
understand raises TypeError at construction.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import exprs
from .Algorithm1 import _small_cholesky
from .BayesianInferrence import prior_mniw_mean
from .descriptors import BasisMap
from .calibration import CdfCounts, check_thresholds, device_thresholds
from .heldout import SMOOTH_CHUNK, FilterResult, ForecastResult, SmoothResult, check_horizon, check_keys, check_n_trajectories
from .rollout import PredictiveStats

MAX_IV = 4            # PG_EX_MAXIV: latent functions per model
MAX_COMPONENTS = 8    # components of one interface variable
MAX_DRAWS_PER_LAUNCH = 65535
STREAM_ROLLOUT_INTVAR = 192   # PGAS_STREAM_M_ROLLOUT_INTVAR (include/pgas_marginal.h)
STREAM_ROLLOUT_OBS = 200      # PGAS_STREAM_M_ROLLOUT_OBS: the observation noise of predict
MAX_REPLICATES_PREDICT = 1 << 20   # PGAS_M_ROLLOUT_STATS_MAX_P
MAX_PARTICLES_FILTER = 1024        # k_model_filter: one workgroup per draw, 4 particle rows of 256
LDS_PER_WORKGROUP = 160 * 1024     # gfx950
# k_model_filter's static LDS: SmallSmem (2 x 1024 u64 numerators, 2 x 1024 CDF entries, 1024 log-likelihoods, 2 x 4 maxima, 2 x 4 wave
# totals, 4 counts = 41104 B) and the reduction slots (4 waves x (2 x 16 predictive + 8 filtered + 1) doubles = 1312 B)
FILTER_STATIC_LDS = 41104 + 1312
# k_model_forecast's static LDS: two sets of reduction slots (2 x 4 waves x (2 x 16 moments + maximum + exp sum) doubles); its dynamic LDS
# is the filter's, so what the filter holds the forecast holds
FORECAST_STATIC_LDS = 2176
# k_model_smooth<4>'s static LDS: 1024 log-weights, 256 x 8 trajectory states, 256 indices, 4 waves x 2 x 32 moment slots; its dynamic
# LDS is the filter's and its static LDS is smaller, so what the filter holds the smoother holds
SMOOTH_STATIC_LDS = 8192 + 16384 + 1024 + 2048
STREAM_SMOOTH = 201           # PGAS_STREAM_M_SMOOTH: the backward draw's uniforms
MAX_INTERFACE_SMOOTH = 16     # PGAS_M_SMOOTH_MAX_XI: interface components an interface output of smooth can have
CDF_SLOTS = 64   # PG_CDF_SLOTS: (nx + ny) J value-channel x threshold slots, one per lane of a wave


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else tuple(np.shape(a))


def mniw_posterior_means(GP_prior, T0, T1):
    """Posterior means (K, n, M) of the MNIW prior `GP_prior` = (eta0 (M, n), eta1 (M, M), ...) updated with each of the K statistics
    (T0 (K, M, n), T1 (K, M, M)) of an Algorithm1 / Algorithm2 statistics trace: ``prior_mniw_mean(eta0 + T0[k], eta1 + T1[k])`` draw by
    draw.  Host NumPy (K small solves); device tensors are copied to the host."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)  # noqa: E731
    e1 = np.asarray(GP_prior[1], dtype=np.float64)
    M = e1.shape[0]
    e0 = np.asarray(GP_prior[0], dtype=np.float64).reshape(M, -1)
    T0, T1 = host(T0), host(T1)
    if T0.ndim < 2 or T0.shape[1] != M or T1.shape != (T0.shape[0], M, M):
        raise ValueError(f"T0 / T1: expected (K, {M}, n) and (K, {M}, {M}), got {T0.shape} and {T1.shape}")
    T0 = T0.reshape(T0.shape[0], M, -1)
    if T0.shape[2] != e0.shape[1]:
        raise ValueError(f"T0: {T0.shape[2]} components, the prior has {e0.shape[1]}")
    return np.stack([prior_mniw_mean(e0 + T0[k], e1 + T1[k]) for k in range(T0.shape[0])])


def _trace(fn, nx, nu, widths, what):
    """exprs.trace; anything the symbolic namespace lacks (an attribute, an operator) is a TypeError too: there is no fallback to run."""
    try:
        return exprs.trace(fn, nx, nu, widths)
    except (AttributeError, NotImplementedError, IndexError) as e:
        raise TypeError(f"symbolic trace of the {what}: {type(e).__name__}: {e}") from e


class _Latent:
    """One latent function's basis argument: a BasisMap pick of concat(state, input), or a traced feature program under a BasisMap."""

    def __init__(self, bf, nx, nu):
        b = getattr(bf, "b", bf)   # experiments._BatchedBasis wraps its descriptor
        self.prog = None
        if isinstance(b, BasisMap):
            self.map = b
            if np.any(b.sel < 0) or np.any(b.sel >= nx + nu):
                raise ValueError(f"basis_fcn: sel {b.sel.tolist()} outside the {nx} state and {nu} input components")
        elif hasattr(b, "feature") and isinstance(getattr(b, "map", None), BasisMap):
            self.map = b.map
            fn = b.feature   # feature(xp) -> callable(state, input) -> (N, D')
            self.prog = _trace(lambda st, u: fn(exprs.SymNamespace(st.tr))(st, u), nx, nu, (), "basis feature")
            if np.any(self.map.sel < 0) or np.any(self.map.sel >= len(self.prog.out_regs)):
                raise TypeError("basis_fcn: the feature has fewer components than its BasisMap selects")
        else:
            raise TypeError("basis_fcn entries must be BasisMap descriptors (basis.on(sel, div)) or objects with `feature(xp)` and a BasisMap `map`: "
                            "a plain callable cannot run inside the kernel")
        if self.map.basis.D > 4:
            raise TypeError(f"basis_fcn: {self.map.basis.D} basis dimensions, the kernel takes 4")
        self.M, self.D = int(self.map.basis.M), int(self.map.basis.D)


def _bits(v):
    return struct.pack("<d", float(v))


def _assemble(progs, nx, nu, widths):
    """ONE register numbering for several traced programs: inputs [0, n_in) (the feature programs see only state and input), one pool of
    constants behind them, temporaries behind the pool.  Returns (codes, out_regs, consts, n_in, n_reg)."""
    n_in = nx + nu + sum(widths)
    pool, where = [], {}
    for p in progs:
        for c in p.consts:
            if _bits(c) not in where:
                where[_bits(c)] = len(pool)
                pool.append(float(c))
    first_tmp = n_in + len(pool)
    codes, outs, n_reg = [], [], first_tmp
    for p in progs:
        nc = len(p.consts)

        def reg(r, p=p, nc=nc):
            r = int(r)
            if r < p.n_in:
                return r
            if r < p.n_in + nc:
                return n_in + where[_bits(p.consts[r - p.n_in])]
            return first_tmp + r - (p.n_in + nc)

        code = np.array([[op, reg(d), reg(a), reg(b)] for op, d, a, b in p.code], dtype=np.int32).reshape(-1, 4)
        codes.append(np.ascontiguousarray(code))
        outs.append([reg(r) for r in p.out_regs])
        n_reg = max(n_reg, first_tmp + p.n_reg - (p.n_in + nc))
    return codes, outs, np.asarray(pool, dtype=np.float64), n_in, n_reg


class ModelFilterResult(FilterResult):
    """FilterResult of ``ModelRollout.filter`` (pred_sum / pred_sumsq hold the state and g(x, u, xi)); with traces also lw (K, T, N), the
    particles' log-likelihoods, and yhat (K, T, N, ny) = g."""

    FIELDS = FilterResult.FIELDS + ("lw", "yhat")


class ModelForecastResult(ForecastResult):
    """ForecastResult of ``ModelRollout.forecast`` (sum / sumsq hold the state and g(x, u, xi); filter is a ModelFilterResult); with
    clouds also cloud_x (K, H, T, N, nx) and cloud_y (K, H, T, N, ny), the h-step-ahead particles themselves at [k, h - 1, tau] (NaN where
    tau < h - 1), otherwise None."""

    def __init__(self, filter, horizon, sum, sumsq, lpd=None, cloud_x=None, cloud_y=None):   # noqa: A002
        super().__init__(filter, horizon, sum, sumsq, lpd)
        self.cloud_x, self.cloud_y = cloud_x, cloud_y


class ModelSmoothResult(SmoothResult):
    """SmoothResult of ``ModelRollout.smooth`` (sum / sumsq hold the smoothed state and g(x, u, xi) of the chosen particle; filter is a
    ModelFilterResult); with interface also xi_sum / xi_sumsq (K, T, n_xi), the sums over the trajectories of the smoothed interface
    variables (n_xi = sum n_i components, in the order of the latent functions) and of their squares, and with interface and
    trajectories xis (K, B, T, n_xi); otherwise None."""

    def __init__(self, filter, n_trajectories, sum, sumsq, xs=None, idx=None, xi_sum=None, xi_sumsq=None, xis=None):   # noqa: A002
        super().__init__(filter, n_trajectories, sum, sumsq, xs, idx)
        self.xi_sum, self.xi_sumsq, self.xis = xi_sum, xi_sumsq, xis
        self.fmean = self.xi = None   # the kernel's per-particle traces (ModelRollout._smooth_from(traces=True))


def interface_summary(result):
    """Plain torch on the small tensors of a ModelSmoothResult: dict of xi_smooth_mean, xi_smooth_std (T, n_xi), the smoothed interface
    variables pooled over draws and trajectories (divisor K n_trajectories, variance clamped at 0), and xi_smooth_mean_draw,
    xi_smooth_std_draw (K, T, n_xi), the same per draw."""
    if getattr(result, "xi_sum", None) is None:
        raise ValueError("interface_summary needs the interface moments: ModelRollout.smooth(..., interface=True)")
    K, B = int(result.xi_sum.shape[0]), float(result.n_trajectories)
    mean = result.xi_sum.sum(dim=0) / (K * B)
    std = torch.sqrt(torch.clamp(result.xi_sumsq.sum(dim=0) / (K * B) - mean * mean, min=0.0))
    mean_k = result.xi_sum / B
    std_k = torch.sqrt(torch.clamp(result.xi_sumsq / B - mean_k * mean_k, min=0.0))
    return dict(xi_smooth_mean=mean, xi_smooth_std=std, xi_smooth_mean_draw=mean_k, xi_smooth_std_draw=std_k)


class ModelRollout:
    def __init__(self, inputs, SSM, basis_fcn, init_state_mean=None, init_state_cov=None, device=None, int_var_widths=None, ops=None, observations=None):
        """inputs (T,), (T, nu) or (T, 0): the validation input sequence (T rows -> T simulated states, row 0 being x_0).  SSM: a
        SymbolicStateSpaceModel (its factory is traced here).  basis_fcn: one entry per latent function -- a BasisMap, or an object with
        `feature(xp)` and a BasisMap `map` (experiments._SlipAngleBasis).  int_var_widths: components n_i of every interface variable
        (default 1 each).  ops: MarginalOps to run on (default: a utility context of `device`, created by the first call).  observations
        (T,) (ny == 1) or (T, ny): the rows ``predict`` scores under the SSM's output noise.
        Nothing here touches a device."""
        model = getattr(SSM, "_model", None)
        if model is None or not hasattr(SSM, "process_noise"):
            raise TypeError("SSM must be a pgas_amd.SymbolicStateSpaceModel: the kernel runs the model as a traced program and has no torch fallback")
        self.SSM = SSM
        self.nx = int(SSM.process_noise.shape[0])
        self.inputs = np.asarray(inputs, dtype=np.float64)
        if self.inputs.ndim < 1 or self.inputs.ndim > 2 or self.inputs.shape[0] < 1:
            raise ValueError("inputs: expected T >= 1 rows ((T,), (T, nu) or (T, 0))")
        self.T = int(self.inputs.shape[0])
        self.inputs = np.ascontiguousarray(self.inputs.reshape(self.T, -1))
        self.nu = int(self.inputs.shape[1])
        basis_fcn = list(basis_fcn)
        self.L = len(basis_fcn)
        if not 1 <= self.L <= MAX_IV:
            raise ValueError(f"basis_fcn: {self.L} latent functions, expected 1 to {MAX_IV}")
        self.widths = tuple(int(w) for w in (int_var_widths if int_var_widths is not None else [1] * self.L))
        if len(self.widths) != self.L or any(not 1 <= w <= MAX_COMPONENTS for w in self.widths):
            raise ValueError(f"int_var_widths: expected {self.L} widths in 1..{MAX_COMPONENTS}")
        if (init_state_mean is None) != (init_state_cov is None):
            raise ValueError("init_state_mean and init_state_cov go together")
        self.has_init = init_state_mean is not None
        if self.has_init:
            m0 = np.asarray(init_state_mean, dtype=np.float64).reshape(-1)
            P0 = np.atleast_2d(np.asarray(init_state_cov, dtype=np.float64))
            if m0.shape != (self.nx,) or P0.shape != (self.nx, self.nx):
                raise ValueError(f"init_state_mean / init_state_cov: expected ({self.nx},) and ({self.nx}, {self.nx})")
            self._m0L0 = np.concatenate([m0, np.linalg.cholesky(P0).reshape(-1)])
        # ---- trace (TypeError for what the tracer does not understand), then one register numbering for all programs
        self.latents = [_Latent(bf, self.nx, self.nu) for bf in basis_fcn]

        def traced(which):
            return _trace(lambda st, u, *iv: model(exprs.SymNamespace(st.tr))[which](st, u, *iv), self.nx, self.nu, self.widths,
                          "output model" if which else "transition model")

        pf, pg = traced(0), traced(1)
        if len(pf.out_regs) != self.nx:
            raise TypeError(f"the transition model returns {len(pf.out_regs)} components, the state has {self.nx}")
        self.ny = len(pg.out_regs)
        if self.nx > 8 or self.ny > 8:
            raise TypeError("the kernel takes at most 8 state and 8 output components")
        feats = [h.prog for h in self.latents if h.prog is not None]
        codes, outs, self._consts, self.n_in, self.n_reg = _assemble([pf, pg] + feats, self.nx, self.nu, self.widths)
        if self.n_reg > exprs.MAX_REG:
            raise TypeError(f"the model's programs need {self.n_reg} registers together, the kernel has {exprs.MAX_REG}")
        self._fcode, self._gcode, self._fout, self._gout = codes[0], codes[1], outs[0], outs[1]
        k = 2
        for h in self.latents:
            if h.prog is not None:
                h.code, h.sel = codes[k], [outs[k][j] for j in h.map.sel]
                k += 1
            else:
                h.code, h.sel = None, [int(j) for j in h.map.sel]
        self.has_observations = observations is not None
        self.observations = None
        if self.has_observations:
            so = _shape(observations)
            if so != (self.T, self.ny) and not (self.ny == 1 and so == (self.T,)):
                raise ValueError(f"observations: expected ({self.T},) or ({self.T}, {self.ny}), got {so}")
            self.observations = np.ascontiguousarray(np.asarray(observations, dtype=np.float64).reshape(self.T, self.ny))
        self.is_deterministic = bool(SSM.is_deterministic)
        self._Qc = None if self.is_deterministic else np.ascontiguousarray(SSM._Q_chol, dtype=np.float64)
        self._device, self._ops, self._dev_cache, self._keep = device, ops, None, None

    def lds_bytes(self, predict=False):
        """LDS a workgroup of the kernel asks for: register file and normals (512 B per row), then the draw's coefficient rows.
        predict=True: k_model_rollout_stats, whose normals rows also hold the ny normals of the observation noise."""
        rows = max([self.nx] + list(self.widths) + ([self.ny] if predict else []))
        return (self.n_reg + rows) * 512 + 8 * sum(w * h.M for w, h in zip(self.widths, self.latents))

    def filter_lds_bytes(self, particles):
        """Dynamic LDS of k_model_filter: one register file per 64 particles, whose park rows also hold a gathered (x, xi) pair, then
        the draw's coefficient rows."""
        return -(-int(particles) // 64) * self._filter_file_bytes() + 8 * sum(w * h.M for w, h in zip(self.widths, self.latents))

    def _filter_file_bytes(self):
        return (self.n_reg + max([self.nx + sum(self.widths), self.ny] + list(self.widths))) * 512

    def max_particles(self):
        """The largest ``particles`` of ``filter``: 64 per register file that fits LDS_PER_WORKGROUP beside FILTER_STATIC_LDS and the
        coefficient rows, at most 1024.  Host arithmetic."""
        room = LDS_PER_WORKGROUP - FILTER_STATIC_LDS - 8 * sum(w * h.M for w, h in zip(self.widths, self.latents))
        return max(0, min(MAX_PARTICLES_FILTER, 64 * (room // self._filter_file_bytes())))

    # ------------------------------------------------------------------------------------------------------------------ validation
    def check_call(self, coeffs, keys=None, replicates=1, init_state=None, row_cov=None, process_noise=True, outputs=False, p0=0, *, predict=False,
                   observation_noise=False, log_score=None):
        """Validates a call from shapes alone (nothing is copied, no device is touched) -> (K, P, x0_mode, noisy_state, noisy_iv).
        predict=True: the call is ``predict`` (replicates <= 2^20; observation_noise needs the draws' keys and counts as noise;
        log_score=True needs observations; both need an output noise of the output model's ny components)."""
        if not isinstance(coeffs, (list, tuple)) or len(coeffs) != self.L:
            raise ValueError(f"coeffs: expected a list of {self.L} arrays (K, n_i, M_i)")
        K = None
        for i, (a, w, h) in enumerate(zip(coeffs, self.widths, self.latents)):
            s = _shape(a)
            if len(s) != 3 or s[1:] != (w, h.M):
                raise ValueError(f"coeffs[{i}]: expected (K, {w}, {h.M}), got {s}")
            if K is not None and s[0] != K:
                raise ValueError(f"coeffs[{i}]: {s[0]} draws, coeffs[0] has {K}")
            K = int(s[0])
        if K < 1:
            raise ValueError("coeffs: K must be >= 1")
        P = int(replicates)
        if P < 1:
            raise ValueError(f"replicates must be >= 1, got {replicates}")
        if int(p0) < 0:
            raise ValueError(f"p0 must be >= 0, got {p0}")
        noisy_obs = bool(predict) and bool(observation_noise)
        if predict:
            if self.ny < 1:
                raise ValueError("predict needs an output model with ny >= 1")
            if P > MAX_REPLICATES_PREDICT:
                raise ValueError(f"replicates must be <= {MAX_REPLICATES_PREDICT} in one predict call, got {replicates}")
            if log_score and not self.has_observations:
                raise ValueError("log_score=True needs observations: construct the ModelRollout with observations")
            if noisy_obs and keys is None:
                raise ValueError("observation_noise needs keys: the measurement noise is drawn from the draw's key")
            scored = self.has_observations if log_score is None else bool(log_score)
            if (noisy_obs or scored) and _shape(self.SSM.output_noise) != (self.ny, self.ny):
                raise ValueError(f"SSM.output_noise is {_shape(self.SSM.output_noise)}, the output model has {self.ny} components")
        noisy_iv = row_cov is not None
        if noisy_iv:
            if not isinstance(row_cov, (list, tuple)) or len(row_cov) != self.L:
                raise ValueError(f"row_cov: expected a list of {self.L} arrays (K, n_i, n_i)")
            for i, (r, w) in enumerate(zip(row_cov, self.widths)):
                if _shape(r) != (K, w, w):
                    raise ValueError(f"row_cov[{i}]: expected ({K}, {w}, {w}), got {_shape(r)}")
        noisy_state = bool(process_noise) and not self.is_deterministic
        drawn = init_state is None
        if keys is None:
            if noisy_state or noisy_iv:
                raise ValueError("a rollout with noise (process_noise of a stochastic model, row_cov) needs keys, one per draw; "
                                 "pass process_noise=False for the noise-free simulation")
            if drawn:
                raise ValueError("init_state=None draws x_0 from the draw's key: pass keys or an init_state")
        else:
            check_keys(keys, K)
        if drawn:
            if not self.has_init:
                raise ValueError("init_state=None draws x_0 ~ N(init_state_mean, init_state_cov): construct the ModelRollout with both")
            mode = 0
        else:
            si = _shape(init_state)
            if si == (self.nx,) or (self.nx == 1 and si == ()):
                mode = 1
            elif si == (K, self.nx):
                mode = 2
            elif si == (K, P, self.nx):
                mode = 3
            else:
                raise ValueError(f"init_state: expected ({self.nx},), ({K}, {self.nx}) or ({K}, {P}, {self.nx}), got {si}")
        if not (noisy_state or noisy_iv or noisy_obs or drawn) and P > 1 and mode != 3:
            raise ValueError("a noise-free rollout of replicates > 1 needs a per-replicate init_state (K, P, nx): its replicates would be copies")
        return K, P, mode, noisy_state, noisy_iv

    # ------------------------------------------------------------------------------------------------------------------ device side
    @property
    def ops(self):
        if self._ops is None:
            from ._lib import MarginalOps

            self._ops = MarginalOps(1, self._device)
        return self._ops

    def _static(self):
        """What does not change between calls, uploaded once: program words, constants, index tables, inputs, noise factors."""
        if self._dev_cache is None:
            dev = self.ops.device
            up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
            self._dev_cache = dict(
                consts=up(self._consts, torch.float64), fcode=up(self._fcode, torch.int32), gcode=up(self._gcode, torch.int32),
                u=up(self.inputs, torch.float64), y=None if self.observations is None else up(self.observations, torch.float64), Qc=None if self._Qc is None else up(self._Qc, torch.float64),
                m0L0=up(self._m0L0, torch.float64) if self.has_init else None,
                idx=[up(h.map.basis.indices, torch.int32) for h in self.latents],
                feat=[None if h.code is None else up(h.code, torch.int32) for h in self.latents])
        return self._dev_cache

    def _desc(self, K, P, p0, mode, coeffs, rows, seeds, x0, noisy_state, out_x, out_y):
        """The pgas_m_rollout descriptor of one launch; the tensors it points to are the caller's to keep alive."""
        from ._lib import RolloutDesc

        st = self._static()
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        d = RolloutDesc()
        d.K, d.T, d.P, d.L, d.nx, d.nu, d.ny = K, self.T, P, self.L, self.nx, self.nu, self.ny
        d.n_in, d.nconst, d.nreg, d.x0_mode, d.p0 = self.n_in, len(self._consts), self.n_reg, mode, p0
        d.f_ninstr, d.g_ninstr = self._fcode.shape[0], self._gcode.shape[0]
        for j, r in enumerate(self._fout):
            d.f_out[j] = r
        for j, r in enumerate(self._gout):
            d.g_out[j] = r
        d.consts_dev, d.fcode_dev, d.fcode_host = ptr(st["consts"]) if len(self._consts) else None, ptr(st["fcode"]), self._fcode.ctypes.data
        if out_y is not None or out_x is None:   # out_x None: predict, which always runs the output program
            d.gcode_dev, d.gcode_host, d.out_y_dev = ptr(st["gcode"]), self._gcode.ctypes.data, ptr(out_y)
        d.inputs_dev = ptr(st["u"]) if self.nu else None
        d.seeds_dev = ptr(seeds)
        d.Qc_dev = ptr(st["Qc"]) if noisy_state else None
        d.x0_dev, d.m0L0_dev, d.out_x_dev = ptr(x0), ptr(st["m0L0"]) if mode == 0 else None, ptr(out_x)
        for i, h in enumerate(self.latents):
            m, b = d.lat[i], h.map.basis
            m.M, m.D, m.n, m.feat = h.M, h.D, self.widths[i], 0 if h.code is None else 1
            for k in range(h.D):
                m.sel[k], m.div[k], m.center[k], m.L[k], m.size[k] = h.sel[k], float(h.map.div[k]), float(b.center[k]), float(b.L[k]), float(b.size[k])
            m.idx_dev, m.A_dev, m.Lrow_dev = st["idx"][i].data_ptr(), coeffs[i].data_ptr(), None if rows is None else rows[i].data_ptr()
            if h.code is not None:
                m.fcode_dev, m.fcode_host, m.f_ninstr = st["feat"][i].data_ptr(), h.code.ctypes.data, h.code.shape[0]
        return d

    def _chunks(self, K, P, p0, mode, A, rows, seeds, x0, noisy_state, out_x=None, out_y=None):
        """(k0, n, descriptor) of the launches of one call: draws k0 .. k0 + n - 1 each, the grid holds 65535 draws."""
        for k0 in range(0, K, MAX_DRAWS_PER_LAUNCH):
            n = min(MAX_DRAWS_PER_LAUNCH, K - k0)
            cut = lambda t: None if t is None else t[k0:k0 + n]  # noqa: E731, B023
            yield k0, n, self._desc(n, P, p0, mode, [cut(a) for a in A], None if rows is None else [cut(r) for r in rows], cut(seeds),
                                    cut(x0) if mode in (2, 3) else x0, noisy_state, cut(out_x), cut(out_y))

    def _fill_obs(self, desc, LR=False, LRinv=False, cR=False):
        """The constants of the output noise N(0, SSM.output_noise) a descriptor asks for: chol, its inverse (ny x ny, row-major), cR."""
        ny = self.ny
        flat = lambda m: [float(m[j, l]) for j in range(ny) for l in range(ny)]  # noqa: E731
        if LR:
            desc.LR[:ny * ny] = flat(np.linalg.cholesky(self.SSM.output_noise))
        if LRinv:
            desc.LRinv[:ny * ny] = flat(self.SSM._LRinv)
        if cR:
            desc.cR = float(self.SSM._cR)

    def __call__(self, coeffs, keys=None, replicates=1, init_state=None, row_cov=None, process_noise=True, outputs=False, p0=0):
        """coeffs: list of L arrays / tensors (K, n_i, M_i); keys: K integers or a (K,) int64 device tensor; init_state (nx), (K, nx),
        (K, P, nx) or None (x_0 = init_state_mean + chol(init_state_cov) z from the draw's key, as Algorithm1 draws it); row_cov: list of
        (K, n_i, n_i) covariances of a Gaussian noise on the interface variables (factored here: NumPy for host arrays, elementwise on the
        device for device tensors, without a host check); process_noise: add chol(Q) z to every step (ignored by a deterministic model); outputs: also return
        y_t = output_model(x_t, u_t, xi_t); p0: the replicates are p0 .. p0 + replicates - 1 of a larger rollout (their Philox particle counters
        start at p0), so that the chunks of one rollout computed in several calls are bit-identical to the one call.  Returns out_x (K, T, P, nx) fp64 on the device, or (out_x, out_y (K, T, P, ny)).
        Every ValueError is raised before a device is touched; the call itself only enqueues work."""
        K, P, mode, noisy_state, noisy_iv = self.check_call(coeffs, keys, replicates, init_state, row_cov, process_noise, outputs, p0)
        dev = self.ops.eng.device
        A, rows, seeds, x0 = self._operands(K, P, mode, coeffs, keys, init_state, row_cov if noisy_iv else None)
        out_x = torch.empty((K, self.T, P, self.nx), dtype=torch.float64, device=dev)
        out_y = torch.empty((K, self.T, P, self.ny), dtype=torch.float64, device=dev) if outputs else None
        for _, _, d in self._chunks(K, P, int(p0), mode, A, rows, seeds, x0, noisy_state, out_x, out_y):
            self.ops.model_rollout(d)
        self._keep = (A, rows, seeds, x0)   # until the kernel has run
        return (out_x, out_y) if outputs else out_x

    def _operands(self, K, P, mode, coeffs, keys, init_state, row_cov):
        """The per-call operands on the device -> (A, rows, seeds, x0); the caller keeps them alive until the kernel has run."""
        from .chains import keys_tensor

        eng = self.ops.eng
        A = [eng._dev(a, shape=(K, w, h.M)) for a, w, h in zip(coeffs, self.widths, self.latents)]
        rows = None
        if row_cov is not None:
            rows = []
            for r, w in zip(row_cov, self.widths):
                if isinstance(r, torch.Tensor) and r.is_cuda:
                    rows.append(_small_cholesky(r.to(torch.float64).contiguous()))   # elementwise: no library workspace, no host check
                else:
                    rows.append(eng._dev(np.linalg.cholesky(np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r, dtype=np.float64)), shape=(K, w, w)))
        seeds = None if keys is None else keys_tensor(keys, eng.device)
        x0 = None if mode == 0 else eng._dev(init_state, shape={1: (self.nx,), 2: (K, self.nx), 3: (K, P, self.nx)}[mode])
        return A, rows, seeds, x0

    def predict(self, coeffs, keys=None, replicates=1, init_state=None, row_cov=None, process_noise=True, observation_noise=False, log_score=None, p0=0):
        """The rollout of ``__call__`` (same arguments; replicates <= 2^20) reduced over its replicates inside the kernel ->
        PredictiveStats(n, x_sum, x_sumsq (K, T, nx), y_sum, y_sumsq (K, T, ny), lpd (K, T) or None).  The predicted observation is
        g(x_t, u_t, xi_t), with observation_noise g + chol(SSM.output_noise) e (e from the draw's key on STREAM_ROLLOUT_OBS: needs keys);
        log_score (default: observations were given) adds the log predictive density of the observation rows under SSM.output_noise.
        Replicate p carries exactly the x_t and y_t ``__call__(outputs=True)`` returns for it; the summation order is defined (DESIGN.md
        section 14).  Every ValueError is raised before a device is touched; the call itself only enqueues work."""
        K, P, mode, noisy_state, noisy_iv = self.check_call(coeffs, keys, replicates, init_state, row_cov, process_noise, True, p0, predict=True,
                                                            observation_noise=observation_noise, log_score=log_score)
        from ._lib import RolloutStatsDesc

        score = self.has_observations if log_score is None else bool(log_score)
        noisy_obs = bool(observation_noise)
        dev = self.ops.eng.device
        A, rows, seeds, x0 = self._operands(K, P, mode, coeffs, keys, init_state, row_cov if noisy_iv else None)
        nv, B, C = self.nx + self.ny, (P + 63) // 64, 2 * (self.nx + self.ny) + 2
        s1 = torch.empty((K, self.T, nv), dtype=torch.float64, device=dev)
        s2 = torch.empty((K, self.T, nv), dtype=torch.float64, device=dev)
        lpd = torch.empty((K, self.T), dtype=torch.float64, device=dev) if score else None
        part = torch.empty((min(K, MAX_DRAWS_PER_LAUNCH), B, self.T, C), dtype=torch.float64, device=dev)   # the launches of one stream share it
        st = RolloutStatsDesc()
        st.y_dev = self._static()["y"].data_ptr() if score else None
        st.part_dev, st.part_bytes, st.noise = part.data_ptr(), part.numel() * 8, int(noisy_obs)
        if noisy_obs or score:
            self._fill_obs(st, LR=True, LRinv=True, cR=True)
        for k0, n, d in self._chunks(K, P, int(p0), mode, A, rows, seeds, x0, noisy_state):
            st.sum_dev, st.sumsq_dev, st.lpd_dev = s1[k0:k0 + n].data_ptr(), s2[k0:k0 + n].data_ptr(), lpd[k0:k0 + n].data_ptr() if score else None
            self.ops.model_rollout_stats(d, st)
        self._keep = (A, rows, seeds, x0, part)   # until the kernels have run
        return PredictiveStats(P, s1[..., :self.nx], s2[..., :self.nx], s1[..., self.nx:], s2[..., self.nx:], lpd)

    # ------------------------------------------------------------------------------------------------------------------ calibration
    def max_thresholds(self):
        """J_max of ``cdf`` / ``forecast_cdf``: min(16, 64 // (nx + ny)) thresholds per channel (one wave lane per slot)."""
        from .calibration import MAX_THRESHOLDS

        return min(MAX_THRESHOLDS, CDF_SLOTS // max(self.nx + self.ny, 1))

    def _check_slots(self, thresholds):
        J, form = check_thresholds(self.T, self.nx, self.ny, thresholds, self.has_observations)
        if J > self.max_thresholds():
            raise ValueError(f"thresholds: J = {J} thresholds on {self.nx + self.ny} channels need {(self.nx + self.ny) * J} slots, the kernel has "
                             f"{CDF_SLOTS}: J_max = {self.max_thresholds()}")
        return J, form

    def check_cdf(self, coeffs, keys=None, replicates=1, init_state=None, row_cov=None, process_noise=True, thresholds=None, observation_noise=False,
                  p0=0):
        """Validates a ``cdf`` call from shapes alone (no device is touched): ``predict``'s refusals, then the thresholds and the slot
        limit J <= 64 // (nx + ny) -> (K, P, x0_mode, noisy_state, noisy_iv, J, form)."""
        out = self.check_call(coeffs, keys, replicates, init_state, row_cov, process_noise, True, p0, predict=True,
                              observation_noise=observation_noise, log_score=False)
        return out + self._check_slots(thresholds)

    def cdf(self, coeffs, keys=None, replicates=1, init_state=None, row_cov=None, process_noise=True, thresholds=None, observation_noise=False, p0=0):
        """The rollout of ``predict`` (same arguments) counted against thresholds inside the kernel (k_model_rollout_cdf, DESIGN.md
        section 20) -> CdfCounts(n = P, count (K, T, nx + ny, J) int32, thresholds (T, nx + ny, J), nx, pit): count[k, t, c, j] replicates
        have value channel c (the state, then the predicted observation g, with observation_noise g + chol(SSM.output_noise) e -- the e
        of ``predict``) <= thresholds[t, c, j].  thresholds: (T, nx + ny, J) for all channels; (T, ny, J) for the predicted observations
        only (the state channels get NaN thresholds and count 0); (T,) or (T, ny): J = 1; None: the object's observations (the PIT;
        ValueError without them).  J <= min(16, 64 // (nx + ny)).  The counts of calls with p0 = 0, P1, P1 + P2, ... add up exactly to
        the one call's.  Every ValueError is raised before a device is touched; the call itself only enqueues work."""
        K, P, mode, noisy_state, noisy_iv, J, form = self.check_cdf(coeffs, keys, replicates, init_state, row_cov, process_noise, thresholds,
                                                                    observation_noise, p0)
        from ._lib import ModelRolloutCdfDesc

        dev = self.ops.eng.device
        A, rows, seeds, x0 = self._operands(K, P, mode, coeffs, keys, init_state, row_cov if noisy_iv else None)
        th = device_thresholds(self, thresholds, J, form, self._static()["y"] if form == "pit" else None)   # the PIT reads the uploaded rows
        count = torch.empty((K, self.T, self.nx + self.ny, J), dtype=torch.int32, device=dev)
        cd = ModelRolloutCdfDesc()
        cd.thr_dev, cd.J, cd.noise = th.data_ptr(), J, int(bool(observation_noise))
        if observation_noise:
            self._fill_obs(cd, LR=True)
        for k0, n, d in self._chunks(K, P, int(p0), mode, A, rows, seeds, x0, noisy_state):
            cd.count_dev = count[k0:k0 + n].data_ptr()
            self.ops.model_rollout_cdf(d, cd)
        self._keep = (A, rows, seeds, x0, th)   # until the kernels have run
        return CdfCounts(P, count, th, nx=self.nx, pit=form == "pit")

    def check_forecast_cdf(self, coeffs, keys, particles, horizon, thresholds=None, observation_noise=True, init_state=None, row_cov=None,
                           process_noise=True):
        """Validates a ``forecast_cdf`` call from shapes alone (no device is touched): check_forecast's refusals, then the thresholds and
        the slot limit -> (K, N, x0_mode, noisy_state, noisy_iv, H, J, form)."""
        out = self.check_forecast(coeffs, keys, particles, horizon, init_state, row_cov, process_noise)
        return out + self._check_slots(thresholds)

    def forecast_cdf(self, coeffs, keys, particles, horizon, thresholds=None, observation_noise=True, init_state=None, row_cov=None, process_noise=True):
        """``filter(moments=False, traces=True)``, then the h-step-ahead clouds of ``forecast`` counted against the thresholds of the
        target row in one more launch per chunk of 65535 draws (k_model_forecast_cdf) -> CdfCounts(n = N, count
        (K, H, T, nx + ny, J) int32, thresholds (T, nx + ny, J), nx, pit); -1 where the target row is < h - 1.  thresholds as ``cdf``
        (None: the observations, the PIT); observation_noise adds chol(SSM.output_noise) e to the predicted observation g, which a PIT of
        the observations needs (e on STREAM_ROLLOUT_OBS at the target row with the Philox particle index h << 32 | i).  K = 64, H = 16,
        T = 2000, J = 16 on three channels is 393 MB of counts (J = 1: 25 MB).  Every ValueError is raised before a device is touched;
        the call itself only enqueues work."""
        K, N, mode, noisy_state, noisy_iv, H, J, form = self.check_forecast_cdf(coeffs, keys, particles, horizon, thresholds, observation_noise,
                                                                                init_state, row_cov, process_noise)
        from ._lib import ModelForecastCdfDesc

        flt = self.filter(coeffs, keys, N, init_state, row_cov, process_noise, moments=False, traces=True)
        A, rows, seeds, x0 = self._keep   # the filter call's operands: the same draws, the same seeds
        dev = self.ops.eng.device
        th = device_thresholds(self, thresholds, J, form, self._static()["y"] if form == "pit" else None)   # the PIT reads the uploaded rows
        count = torch.empty((K, H, self.T, self.nx + self.ny, J), dtype=torch.int32, device=dev)
        fc = ModelForecastCdfDesc()
        fc.thr_dev, fc.H, fc.J, fc.noise = th.data_ptr(), H, J, int(bool(observation_noise))
        if observation_noise:
            self._fill_obs(fc, LR=True)
        for k0, n, d in self._chunks(K, N, 0, mode, A, rows, seeds, x0, noisy_state):
            fc.x_dev, fc.count_dev = flt.x[k0:k0 + n].data_ptr(), count[k0:k0 + n].data_ptr()
            self.ops.model_forecast_cdf(d, fc)
        self._keep = (A, rows, seeds, x0, th, flt)   # until the kernels have run
        return CdfCounts(N, count, th, nx=self.nx, pit=form == "pit")

    # ------------------------------------------------------------------------------------------------------------------ closed loop
    def check_filter(self, coeffs, keys, particles, init_state=None, row_cov=None, process_noise=True):
        """Validates a ``filter`` call from shapes alone (no device is touched) -> (K, N, x0_mode, noisy_state, noisy_iv)."""
        if not self.has_observations:
            raise ValueError("filter needs observations: construct the ModelRollout with observations")
        N = int(particles)
        if N < 1 or N > self.max_particles():
            raise ValueError(f"particles: expected 1..{self.max_particles()} (one workgroup per draw; {self._filter_file_bytes()} B of LDS per 64 particles), "
                             f"got {particles}")
        if keys is None:
            raise ValueError("keys: a filter needs one key per draw")
        return self.check_call(coeffs, keys, N, init_state, row_cov, process_noise, True, 0, predict=True, log_score=True)

    def filter(self, coeffs, keys, particles, init_state=None, row_cov=None, process_noise=True, moments=True, traces=False):
        """A bootstrap particle filter of `particles` <= max_particles() particles per draw on the observation rows, resampling at every
        step; coeffs, keys, init_state ((nx), (K, nx), (K, N, nx) or None: drawn), row_cov and process_noise as
        ``__call__``.  -> ModelFilterResult: loglik (K), ell (K, T); with moments ess, pred_sum / pred_sumsq (K, T, nx + ny) over the
        unweighted cloud of x_t and g(x_t, u_t, xi_t), filt_sum (K, T, nx), wtot (K, T); with traces x (K, T, N, nx), anc (K, T, N) int32,
        lw (K, T, N), yhat (K, T, N, ny).  Slot i uses the Philox counters of particle i under key k; the interface variables of step t
        travel with the resampled particle.  Every ValueError is raised before a device is touched; the call itself only enqueues work."""
        K, N, mode, noisy_state, noisy_iv = self.check_filter(coeffs, keys, particles, init_state, row_cov, process_noise)
        from ._lib import ModelFilterDesc

        dev = self.ops.eng.device
        A, rows, seeds, x0 = self._operands(K, N, mode, coeffs, keys, init_state, row_cov if noisy_iv else None)
        T, nx, ny = self.T, self.nx, self.ny
        new = lambda *shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        out = dict(loglik=new(K), ell=new(K, T))
        if moments:
            out.update(ess=new(K, T), pred_sum=new(K, T, nx + ny), pred_sumsq=new(K, T, nx + ny), filt_sum=new(K, T, nx), wtot=new(K, T))
        if traces:
            out.update(x=new(K, T, N, nx), anc=new(K, T, N, dt=torch.int32), lw=new(K, T, N), yhat=new(K, T, N, ny))
        fl = ModelFilterDesc()
        fl.y_dev = self._static()["y"].data_ptr()
        self._fill_obs(fl, LRinv=True, cR=True)
        for k0, n, d in self._chunks(K, N, 0, mode, A, rows, seeds, x0, noisy_state):
            for f in ModelFilterResult.FIELDS:
                setattr(fl, f + "_dev", out[f][k0:k0 + n].data_ptr() if f in out else None)
            self.ops.model_filter(d, fl)
        self._keep = (A, rows, seeds, x0)   # until the kernels have run
        return ModelFilterResult(N, nx, **out)

    # ------------------------------------------------------------------------------------------------------------------ h steps ahead
    def check_forecast(self, coeffs, keys, particles, horizon, init_state=None, row_cov=None, process_noise=True):
        """Validates a ``forecast`` call from shapes alone (no device is touched): check_filter's refusals, and a horizon that is not an
        integer in 1..T -> (K, N, x0_mode, noisy_state, noisy_iv, H)."""
        out = self.check_filter(coeffs, keys, particles, init_state, row_cov, process_noise)
        return out + (check_horizon(horizon, self.T),)

    def forecast(self, coeffs, keys, particles, horizon, init_state=None, row_cov=None, process_noise=True, log_score=True, clouds=False):
        """``filter(moments=True, traces=True)``, then the h-step-ahead predictions for h = 1 .. horizon <= T from every origin row of
        every draw in one more launch per chunk of 65535 draws (k_model_forecast) -> ModelForecastResult: sum / sumsq
        (K, H, T, nx + ny) over the cloud of x_tau and g(x_tau, u_tau, xi_tau) propagated open-loop from the filter's row tau - h + 1, lpd
        (K, H, T) = log p(y_tau | y_{0:tau-h}, A_k) with log_score, cloud_x (K, H, T, N, nx) / cloud_y (K, H, T, N, ny) with clouds
        (K H T N (nx + ny) doubles: small problems only).  Entries with tau < h - 1 are NaN.  The propagation noise of lead l = h - 1 uses
        the Philox particle index l << 32 | i, so horizon 1 is the filter's own cloud and no entry depends on `horizon`.  Every ValueError
        is raised before a device is touched; the call itself only enqueues work."""
        K, N, mode, noisy_state, noisy_iv, H = self.check_forecast(coeffs, keys, particles, horizon, init_state, row_cov, process_noise)
        flt = self.filter(coeffs, keys, N, init_state, row_cov, process_noise, moments=True, traces=True)
        return self._forecast_from(flt, K, N, mode, noisy_state, H, log_score, clouds)

    def _forecast_from(self, flt, K, N, mode, noisy_state, H, log_score, clouds):
        """The pgas_m_forecast launches of ``forecast`` from the result `flt` of the filter call that ran LAST on this object (its
        operands are still held)."""
        from ._lib import ModelForecastDesc

        A, rows, seeds, x0 = self._keep   # the filter call's operands: the same draws, the same seeds
        dev = self.ops.eng.device
        T, nx, ny = self.T, self.nx, self.ny
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
        s1, s2 = new(K, H, T, nx + ny), new(K, H, T, nx + ny)
        lpd = new(K, H, T) if log_score else None
        cx, cy = (new(K, H, T, N, nx), new(K, H, T, N, ny)) if clouds else (None, None)
        fc = ModelForecastDesc()
        fc.H = H
        fc.y_dev = self._static()["y"].data_ptr() if log_score else None
        self._fill_obs(fc, LRinv=True, cR=True)
        for k0, n, d in self._chunks(K, N, 0, mode, A, rows, seeds, x0, noisy_state):
            fc.x_dev, fc.sum_dev, fc.sumsq_dev = flt.x[k0:k0 + n].data_ptr(), s1[k0:k0 + n].data_ptr(), s2[k0:k0 + n].data_ptr()
            fc.lpd_dev = lpd[k0:k0 + n].data_ptr() if log_score else None
            fc.cloud_x_dev, fc.cloud_y_dev = (cx[k0:k0 + n].data_ptr(), cy[k0:k0 + n].data_ptr()) if clouds else (None, None)
            self.ops.model_forecast(d, fc)
        return ModelForecastResult(flt, H, s1, s2, lpd, cx, cy)

    # ------------------------------------------------------------------------------------------------------------------ smoothing
    def check_smooth(self, coeffs, keys, particles, n_trajectories, init_state=None, row_cov=None, interface=True):
        """Validates a ``smooth`` call from shapes alone (no device is touched): a deterministic model, check_filter's refusals, an
        n_trajectories that is not an integer in 1..65536, and an interface output of more than 16 components
        -> (K, N, x0_mode, noisy_state, noisy_iv, n_trajectories)."""
        if self.is_deterministic:
            raise ValueError("backward simulation needs process noise: the transition of a deterministic model (process_noise == 0) has no density")
        out = self.check_filter(coeffs, keys, particles, init_state, row_cov, True)
        B = check_n_trajectories(n_trajectories)
        if interface and sum(self.widths) > MAX_INTERFACE_SMOOTH:
            raise ValueError(f"interface: {sum(self.widths)} interface components, the smoother's interface outputs take {MAX_INTERFACE_SMOOTH}; "
                             "pass interface=False")
        return out + (B,)

    def transition_constants(self):
        """(LQinv, cQ) of the transition density N(.; f, Q): the inverse of chol(Q), row-major nx x nx, and
        cQ = -nx/2 log 2pi - sum log diag chol(Q), as ``SymbolicStateSpaceModel.transition_logpdf`` forms them.  Host arithmetic."""
        import math

        Lq = self._Qc
        return np.linalg.inv(Lq), -0.5 * Lq.shape[0] * math.log(2 * math.pi) - float(np.sum(np.log(np.diag(Lq))))

    def _smooth_desc(self):
        """A ModelSmoothDesc with the constants of the transition density and the observation rows."""
        from ._lib import ModelSmoothDesc

        LQinv, cQ = self.transition_constants()
        sm = ModelSmoothDesc()
        sm.cQ = cQ
        for j in range(self.nx):
            for l in range(self.nx):
                sm.LQinv[j * self.nx + l] = float(LQinv[j, l])
        sm.y_dev = self._static()["y"].data_ptr()
        return sm

    def smooth(self, coeffs, keys, particles, n_trajectories, init_state=None, row_cov=None, trajectories=False, indices=False, interface=True):
        """``filter(moments=True, traces=True)``, then n_trajectories <= 65536 backward-simulation draws of (x_t, xi_t), t = 0 .. T - 1,
        given the whole record, per draw, one more launch per 256 trajectories and 65535 draws (k_model_smooth)
        -> ModelSmoothResult: sum / sumsq (K, T, nx + ny) over the trajectories of the smoothed state and of g of the chosen particle;
        with interface xi_sum / xi_sumsq (K, T, n_xi) of the smoothed interface variables; with trajectories xs (K, B, T, nx) (and xis
        (K, B, T, n_xi) with interface); with indices idx (K, B, T) int32.  The sums of the chunks of 256 are added elementwise in
        ascending chunk order, starting from the first chunk's.  Trajectory g of draw k depends on (key k, g) alone.  A deterministic
        model has no backward density and is refused.  Every ValueError is raised before a device is touched; the call itself only
        enqueues work."""
        K, N, mode, noisy_state, _, B = self.check_smooth(coeffs, keys, particles, n_trajectories, init_state, row_cov, interface)
        flt = self.filter(coeffs, keys, N, init_state, row_cov, True, moments=True, traces=True)
        return self._smooth_from(flt, K, N, mode, noisy_state, B, trajectories, indices, interface)

    def _smooth_from(self, flt, K, N, mode, noisy_state, B, trajectories=False, indices=False, interface=True, traces=False):
        """The pgas_m_smooth launches of ``smooth`` from the result `flt` of the filter call that ran LAST on this object (its operands
        are still held).  traces: the result also carries fmean (K, T, N, nx) = f(x_t^i, u_t, xi_t^i) (row T - 1 NaN) and xi
        (K, T, N, n_xi), what the kernel evaluated per particle -- the tests stand on them."""
        A, rows, seeds, x0 = self._keep[:4]   # the filter call's operands: the same draws, the same seeds
        dev = self.ops.eng.device
        T, nx, ny, nxi = self.T, self.nx, self.ny, sum(self.widths)
        new = lambda *shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        sm = self._smooth_desc()
        s1 = s2 = x1 = x2 = fm = xt = None
        if traces:
            fm, xt = new(K, T, N, nx), new(K, T, N, nxi)
            fm[:, T - 1] = float("nan")   # the kernel writes rows 0 .. T - 2
        xs, xis, idx = [], [], []
        ptr = lambda t, k0, n: None if t is None else t[k0:k0 + n].data_ptr()  # noqa: E731
        for b0 in range(0, B, SMOOTH_CHUNK):
            nb = min(SMOOTH_CHUNK, B - b0)
            a1, a2 = new(K, T, nx + ny), new(K, T, nx + ny)
            c1, c2 = (new(K, T, nxi), new(K, T, nxi)) if interface else (None, None)
            xb = new(K, nb, T, nx) if trajectories else None
            xib = new(K, nb, T, nxi) if trajectories and interface else None
            jb = new(K, nb, T, dt=torch.int32) if indices else None
            sm.b0, sm.B = b0, nb
            for k0, n, d in self._chunks(K, N, 0, mode, A, rows, seeds, x0, noisy_state):
                sm.x_dev, sm.anc_dev, sm.lw_dev, sm.yhat_dev = ptr(flt.x, k0, n), ptr(flt.anc, k0, n), ptr(flt.lw, k0, n), ptr(flt.yhat, k0, n)
                sm.sum_dev, sm.sumsq_dev, sm.xi_sum_dev, sm.xi_sumsq_dev = ptr(a1, k0, n), ptr(a2, k0, n), ptr(c1, k0, n), ptr(c2, k0, n)
                sm.xs_dev, sm.xis_dev, sm.idx_dev = ptr(xb, k0, n), ptr(xib, k0, n), ptr(jb, k0, n)
                sm.fmean_dev, sm.xi_dev = (ptr(fm, k0, n), ptr(xt, k0, n)) if b0 == 0 else (None, None)
                self.ops.model_smooth(d, sm)
            s1, s2 = (a1, a2) if s1 is None else (s1 + a1, s2 + a2)
            if interface:
                x1, x2 = (c1, c2) if x1 is None else (x1 + c1, x2 + c2)
            xs.append(xb)
            xis.append(xib)
            idx.append(jb)
        cat = lambda parts: None if parts[0] is None else parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)   # noqa: E731
        self._keep = (A, rows, seeds, x0, flt)   # until the kernels have run
        out = ModelSmoothResult(flt, B, s1, s2, cat(xs), cat(idx), x1, x2, cat(xis))
        out.fmean, out.xi = fm, xt
        return out
