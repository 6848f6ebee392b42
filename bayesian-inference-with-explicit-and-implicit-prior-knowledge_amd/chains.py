"""C independent PGAS chains of one model on one GPU, every step batched over the chains.

* ``condSequentialMonteCarloChains(C, N_samples, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn, basis_fcn)``:
  ``__call__(keys, ref_state, coeff_mat, error_cov)`` runs C conditional-SMC sweeps (src/PGAS.py:176-228) in one launch, one workgroup
  per chain; chain c computes exactly what ``condSequentialMonteCarlo`` computes with keys[c], ref_state[c], coeff_mat[c], error_cov[c].
* ``MultiChainPGAS(C, N_samples, N_iterations, ..., GP_prior, basis_fcn)``: C Gibbs chains (src/PGAS.py:345-397).  Chain c's root key
  is ``random.split(key, C)[c]`` (or ``keys[c]``); from there it follows ``PGAS.__call__`` step for step.  A Gibbs iteration of all
  chains is a fixed number of launches whatever C is, with no host synchronisation and no per-chain Python loop.
* ``split_rhat(x)``: split-R-hat over a (C, K, ...) array, the convergence check of several chains.

N <= 1024 particles per chain (the one-workgroup sweep); the corrected mode and keep_logw_trace have no batched form.
Keys on the device are int64 tensors holding the u64 bit patterns of ``pgas_amd.random`` keys.
"""
from __future__ import annotations

import numpy as np
import torch

from . import random as prng
from .PGAS import condSequentialMonteCarlo

_U64 = 0xFFFFFFFFFFFFFFFF


def root_keys(key, C, keys=None):
    """Root key of every chain: ``keys`` if given (C of them), else ``random.split(key, C)``."""
    if keys is not None:
        out = [prng.as_key(k) for k in keys]
        if len(out) != int(C):
            raise ValueError(f"keys: {len(out)} keys for {int(C)} chains")
        return out
    return prng.split(key, int(C))


def keys_tensor(keys, device):
    """C integer keys, or a (C,) int64 tensor of u64 bit patterns -> (C,) int64 tensor on `device`."""
    if isinstance(keys, torch.Tensor):
        if keys.dtype != torch.int64 or keys.dim() != 1:
            raise ValueError("keys: expected C integers or a (C,) int64 tensor of key bit patterns")
        return keys.to(device).contiguous()
    k = np.array([prng.as_key(v) & _U64 for v in keys], dtype=np.uint64)
    return torch.as_tensor(k.view(np.int64), device=device)


def keys_list(t):
    """(C,) int64 tensor of u64 bit patterns -> C Python integer keys (copies to the host)."""
    return [int(v) for v in t.detach().cpu().numpy().view(np.uint64)]


def split_rhat(x):
    """Split-R-hat (Gelman et al., Bayesian Data Analysis, 3rd ed., section 11.4) of draws x (C chains, K draws, ...): every chain is cut
    into halves of n = K // 2 draws (an odd K drops the middle draw) and the 2C half-chains are compared,
    R = sqrt(((n - 1) / n W + B / n) / W) with W the mean within-half variance and B = n times the variance of the half means.
    Returns a tensor of the trailing shape; values near 1 say the chains agree."""
    x = torch.as_tensor(x, dtype=torch.float64)
    K = x.shape[1]
    n = K // 2
    if n < 2:
        raise ValueError("split_rhat: needs at least 4 draws per chain")
    h = torch.cat([x[:, :n], x[:, K - n:]], dim=0)   # (2C, n, ...)
    W = h.var(dim=1, correction=1).mean(dim=0)
    B = n * h.mean(dim=1).var(dim=0, correction=1)
    return torch.sqrt(((n - 1) / n * W + B / n) / W)


class condSequentialMonteCarloChains:
    def __init__(self, C, N_samples, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn, basis_fcn, device=None,
                 keep_logw_trace=False, resample_before_propagate=False):
        """One model context for C chains.  ``single`` is the same context's single-chain condSequentialMonteCarlo.  keep_logw_trace and
        resample_before_propagate have no batched form: a context built with them serves ``single`` and refuses batched sweeps."""
        self.C = int(C)
        if self.C < 1:
            raise ValueError("C must be >= 1")
        self.single = condSequentialMonteCarlo(N_samples, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn, basis_fcn,
                                               device=device, keep_logw_trace=keep_logw_trace,
                                               resample_before_propagate=resample_before_propagate)
        self.engine = self.single.engine
        self.device = self.engine.device
        self.N_samples = self.single.N_samples

    def _batch(self, a, shape, what):
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: expected shape {shape}, got {tuple(t.shape)}")
        return t.to(device=self.device, dtype=torch.float64).contiguous()

    def _refs(self, ref_state):
        """(T, nx) shared by every chain, or (C, T, nx) -> (C, T, nx) on the device ((T,) / (C, T) accepted for nx = 1)."""
        C, T, nx = self.C, self.engine.T, self.engine.nx
        ref = ref_state if isinstance(ref_state, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(ref_state, dtype=np.float64))
        ref = ref.to(device=self.device, dtype=torch.float64)
        s = tuple(ref.shape)
        if s == (T, nx) or (nx == 1 and s == (T,)):
            return ref.reshape(1, T, nx).expand(C, T, nx).contiguous()
        if s == (C, T, nx) or (nx == 1 and s == (C, T)):
            return ref.reshape(C, T, nx).contiguous()
        raise ValueError(f"ref_state: expected ({T}, {nx}) or ({C}, {T}, {nx}), got {s}")

    def set_params(self, coeff_mat, error_cov):
        eng = self.engine
        eng.chains_set_params(self._batch(coeff_mat, (self.C, eng.nx, eng.M), "coeff_mat"),
                              self._batch(error_cov, (self.C, eng.nx, eng.nx), "error_cov"))

    def __call__(self, keys, ref_state, coeff_mat, error_cov):
        """keys: C integer keys or a (C,) int64 device tensor; ref_state (T, nx) or (C, T, nx); coeff_mat (C, nx, M); error_cov (C, nx, nx)
        -> trajectories (C, T, nx).  Enqueues work only."""
        seeds = keys_tensor(keys, self.device)
        if tuple(seeds.shape) != (self.C,):
            raise ValueError(f"keys: expected {self.C} keys, got {tuple(seeds.shape)[0]}")
        ref = self._refs(ref_state)
        self.set_params(coeff_mat, error_cov)
        return self.engine.chains_sweep(seeds, ref)

    def traces(self):
        """(state traces (C, T, N, nx), ancestor traces (C, T-1, N), last log-weights (C, N)) of the last sweep (library-owned views)."""
        return self.engine.chains_traces(self.C)

    def final_index(self):
        return self.engine.chains_final_index(self.C)

    def rollout(self, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None):
        """In-sample open-loop simulation under K parameter draws (K need not be C) on this context's inputs: ``single.rollout``.  The
        chains' parameters and traces are left as they are."""
        return self.single.rollout(coeff_mat, error_cov, keys, replicates, init_state)

    def predict(self, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None, observation_noise=False, log_score=None):
        """In-sample predictive moments and log score under K parameter draws on this context's observations: ``single.predict``.  The
        chains' parameters and traces are left as they are."""
        return self.single.predict(coeff_mat, error_cov, keys, replicates, init_state, observation_noise, log_score)

    def filter(self, coeff_mat, error_cov, keys, init_state=None, moments=True, traces=False):
        """In-sample bootstrap particle filter per parameter draw (K need not be C) on this context's observations: ``single.filter``.
        The chains' parameters and traces are left as they are."""
        return self.single.filter(coeff_mat, error_cov, keys, init_state, moments, traces)

    def forecast(self, coeff_mat, error_cov, keys, horizon, init_state=None, log_score=True):
        """In-sample h-step-ahead predictions per parameter draw (K need not be C) on this context's record: ``single.forecast``.  The
        chains' parameters and traces are left as they are."""
        return self.single.forecast(coeff_mat, error_cov, keys, horizon, init_state, log_score)

    def smooth(self, coeff_mat, error_cov, keys, n_trajectories, init_state=None, trajectories=False, indices=False):
        """In-sample backward-simulation smoother per parameter draw (K need not be C) on this context's record: ``single.smooth``.  The
        chains' parameters and traces are left as they are."""
        return self.single.smooth(coeff_mat, error_cov, keys, n_trajectories, init_state, trajectories, indices)

    def cdf(self, coeff_mat, error_cov=None, keys=None, replicates=1, init_state=None, thresholds=None, observation_noise=False):
        """In-sample predictive CDF counts under K parameter draws on this context's observations: ``single.cdf``.  The chains' parameters
        and traces are left as they are."""
        return self.single.cdf(coeff_mat, error_cov, keys, replicates, init_state, thresholds, observation_noise)

    def forecast_cdf(self, coeff_mat, error_cov, keys, horizon, thresholds=None, observation_noise=True, init_state=None):
        """In-sample CDF counts of the h-step-ahead clouds per parameter draw (K need not be C) on this context's record:
        ``single.forecast_cdf``.  The chains' parameters and traces are left as they are."""
        return self.single.forecast_cdf(coeff_mat, error_cov, keys, horizon, thresholds, observation_noise, init_state)


class MultiChainPGAS:
    def __init__(self, C, N_samples, N_iterations, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn, GP_prior,
                 basis_fcn, device=None, keep_chain_log=True):
        """keep_chain_log: keep every chain's root key, the per-iteration key blocks and (A_k, S_k) in ``chain_log`` (replaying a chain)."""
        cSMC = condSequentialMonteCarloChains(C, N_samples, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn, basis_fcn,
                                              device=device)
        self._setup(C, N_iterations, cSMC, likelihood_fcn, GP_prior, keep_chain_log)

    def _setup(self, C, N_iterations, cSMC, likelihood_fcn, GP_prior, keep_chain_log):
        """The state of the Gibbs driver over a batched sweep object ``cSMC`` (its engine, its ``single`` context and ``_refs``)."""
        self.C = int(C)
        self.N_iterations = int(N_iterations)
        self.cSMC = cSMC
        eng = self.cSMC.engine
        self.N_steps = eng.T
        dev = eng.device
        f = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
        self.GP_prior = (f(GP_prior[0]), f(GP_prior[1]), f(np.atleast_2d(GP_prior[2])), float(GP_prior[3]))
        self.df = self.GP_prior[3] + (self.N_steps - 1)
        self._eye = (torch.eye(eng.M, dtype=torch.float64, device=dev), torch.eye(eng.nx, dtype=torch.float64, device=dev))
        lik = likelihood_fcn
        self._lik = (torch.as_tensor(self.cSMC.single.observations.reshape(self.N_steps, -1), device=dev), f(lik.H), f(lik.LRinv), float(lik.cR))
        self.keep_chain_log = bool(keep_chain_log)
        self.chain_log = None

    # ---- src/PGAS.py:288-343 for every chain ------------------------------------------------------------
    def param_draws(self, keys6):
        """The random numbers sample_params consumes, per chain from rows 3..5 (key_A, key_chi, key_norm) of a key block (6, C)."""
        return self.cSMC.engine.chains_param_draws(keys6, self.df)

    def suffstats(self, state_trajectories):
        """(T0 (C, M, nx), T1 (C, M, M), T2 (C, nx, nx), T3) of every chain's trajectory in one batched SYRK on the engine."""
        return self.cSMC.engine.chains_suffstats(state_trajectories)

    def sample_params(self, keys6, state_trajectories, draws=None):
        """(A (C, nx, M), S (C, nx, nx)): PGAS.sample_params of every chain at once -- statistics in one batched SYRK on the engine, the MNIW
        algebra in batched torch.linalg calls (a fixed number whatever C is), the draws from the chains' parameter keys."""
        eng = self.cSMC.engine
        C, nx, M = self.C, eng.nx, eng.M
        T0, T1, T2, T3 = self.suffstats(state_trajectories)                             # :294-303
        P0, P1, P2, P3 = self.GP_prior
        e0, e1, e2 = P0 + T0, P1 + T1, P2 + T2
        Lc = torch.linalg.cholesky_ex(e1, check_errors=False)[0]                        # BI:35-45
        sol = torch.cholesky_solve(torch.cat([e0, self._eye[0].expand(C, M, M)], dim=2), Lc)
        mean, col_cov = sol[:, :, :nx].transpose(1, 2).contiguous(), sol[:, :, nx:]
        row_scale = e2 - mean @ e0
        if draws is None:
            draws = self.param_draws(keys6)
        eye = self._eye[1].expand(C, nx, nx)
        L = torch.linalg.solve_triangular(torch.linalg.cholesky_ex(row_scale, check_errors=False)[0], eye, upper=False)      # :317-319
        Tm = torch.tril(draws["normals_T"], diagonal=-1) + torch.diag_embed(torch.sqrt(draws["chi2"]))                       # :327-329
        S_chol = torch.linalg.solve_triangular((L @ Tm).transpose(1, 2).contiguous(), eye, upper=True)                     # :332-334
        S = S_chol @ S_chol.transpose(1, 2)                                                                                 # :335
        V_chol = torch.linalg.cholesky_ex(col_cov, check_errors=False)[0]                                                  # :339
        A = mean + S_chol @ draws["normals_A"] @ V_chol                                                                     # :341
        self.last_df = P3 + T3
        return A, S

    def step(self, keys, state_trajectories, coeff_mat, error_cov):
        """One Gibbs iteration of every chain (src/PGAS.py:365-378): keys (C,) device tensor, trajectories (C, T, nx), (A, S) of the chains
        -> (next keys, new trajectories, A, S, the iteration's key block (6, C)).  Enqueues work only."""
        k6 = self.cSMC.engine.chains_keys(keys, first=False)                           # :365, :377
        traj = self.cSMC(k6[1], state_trajectories, coeff_mat, error_cov)              # :366-371
        A, S = self.sample_params(k6, traj)                                            # :378
        return k6[0], traj, A, S, k6

    def __call__(self, key, init_ref_state, keys=None, progress=None):
        """-> state_trace (C, T, K, nx), log_likelihood (C, T, K); chain c is PGAS.__call__ from root key keys[c] (default split(key, C)[c])."""
        eng = self.cSMC.engine
        dev = eng.device
        C, K, T, nx = self.C, self.N_iterations, self.N_steps, eng.nx
        roots = root_keys(key, C, keys)
        trace = torch.zeros((K, C, T, nx), dtype=torch.float64, device=dev)             # :266-273
        trace[0] = self.cSMC._refs(init_ref_state)
        k6 = eng.chains_keys(keys_tensor(roots, dev), first=True)                      # :356
        A, S = self.sample_params(k6, trace[0])                                        # :358
        kd = k6[0]
        self.chain_log = dict(root_keys=roots, keys=[k6], params=[(A, S)]) if self.keep_chain_log else None
        for k in range(1, K):                                                           # :361
            kd, trace[k], A, S, k6 = self.step(kd, trace[k - 1], A, S)
            if self.chain_log is not None:
                self.chain_log["keys"].append(k6)
                self.chain_log["params"].append((A, S))
            if progress is not None:
                progress(k)
        state_trace = trace.permute(1, 2, 0, 3).contiguous()                            # :380 -> (C, T, K, nx)
        y, H, LRinv, cR = self._lik                                                     # :383-392
        e = y[None, :, None, :] - state_trace @ H.T
        w = e @ LRinv.T
        log_likelihood = cR - 0.5 * (w * w).sum(-1)
        self.coeff_mat, self.error_cov = A, S
        return state_trace, log_likelihood
