"""R independent runs of the online marginalised filter (Algorithm1, reference src/Algorithm1.py) on one model and one data set,
every step batched over the runs.

``MultiRunAlgorithm1(R, N_samples, ...)`` takes Algorithm1's constructor arguments behind the number of runs.  Run r uses root key
``keys[r]`` (default ``random.split(key, R)[r]``) and computes what ``Algorithm1(N_samples, ...)(keys[r])`` computes; a filter step of all
runs is the launches of one.  The per-particle kernels run over the R N particles of all runs with GLOBAL ancestor indices (r N + a); the
three things that are per run -- the Philox streams, systematic resampling, the weighted statistics reduction -- are the batched entry
points pgas_m_runs_* (include/pgas_marginal.h).

N_samples <= 1024 per run (the one-workgroup resampler).  Observations and inputs are shared by the runs.
"""
from __future__ import annotations

import torch

from .Algorithm1 import STREAM_RESAMPLE, Algorithm1
from .chains import keys_tensor, root_keys


class RunsRand:
    """Random numbers of R runs: DeviceRand's interface over the flattened particle axis, run r's Philox streams keyed by keys[r]."""

    def __init__(self, ops, keys):
        self.ops, self.keys = ops, keys   # keys: (R,) int64 device tensor of u64 bit patterns

    def normal(self, stream, t, ncol):
        return self.ops.runs_normal(self.keys, stream, t, ncol)

    def uniform_dev(self, stream, t):
        """(R,) device tensor: one uniform per run."""
        return self.ops.runs_uniform(self.keys, stream, t)

    uniform = uniform_dev   # the runs' uniforms never visit the host

    def student_t(self, stream, t, nu):
        return self.ops.runs_student_t(self.keys, stream, t, nu)

    def student_t_df(self, stream, t, anc, src, nu0, nu_scale):
        return self.ops.runs_student_t_df(self.keys, stream, t, anc, src, nu0, nu_scale)


class MultiRunAlgorithm1(Algorithm1):
    def __init__(self, R, N_samples, observations, inputs, SSM, forgetting_factor, init_state_mean, init_state_cov, init_int_var_mean,
                 init_int_var_cov, GP_prior, basis_fcn, device=None):
        self.R, self.N_run = int(R), int(N_samples)
        if self.R < 1:
            raise ValueError("R must be >= 1")
        if self.N_run < 1:
            raise ValueError("N_samples must be >= 1")
        if self.N_run > 1024:
            raise ValueError(f"N_samples = {self.N_run}: the batched resampler serves at most 1024 particles per run -- run Algorithm1 once per key instead")
        # Algorithm1 over the flattened particle axis: self.N_samples = R N, self.ops = MarginalOps(R N), traces time-major (T, R N, ...)
        super().__init__(self.R * self.N_run, observations, inputs, SSM, forgetting_factor, init_state_mean, init_state_cov, init_int_var_mean,
                         init_int_var_cov, GP_prior, basis_fcn, device=device)

    _weight_count = property(lambda self: self.N_run)   # the initial weights are 1 / N of the particle's own run

    # ---------------------------------------------------------------------------------------------------------------- helpers
    def _rand(self, key):
        """A provider as it is; (R,) keys (integers or an int64 device tensor of bit patterns) -> the runs' device streams."""
        if hasattr(key, "student_t"):
            return key
        keys = keys_tensor(key, self.device)
        if tuple(keys.shape) != (self.R,):
            raise ValueError(f"keys: expected {self.R} keys, got {tuple(keys.shape)[0]}")
        return RunsRand(self.ops, keys)

    def _weighted(self, stats, w):
        """sum_n w_n T_n per run: (R, M[, n]), (R, M, M), (R[, n, n]), (R,)."""
        return self.ops.runs_weighted_stats(self.R, w, stats)

    def _init_trace_vars(self):
        state_trace, int_var_trace, _, lw_trace, anc_trace = super()._init_trace_vars()
        T, R, dev = self.observations.shape[0], self.R, self.device
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
        return (state_trace, int_var_trace, [[z(T, R, M, nv), z(T, R, M, M), z(T, R, nv, nv), z(T, R)] for M, nv in zip(self.dim_basis, self.nvar)],
                lw_trace, anc_trace)

    def _softmax(self, lw):
        """softmax over every run's own particles, flattened again."""
        return torch.softmax(lw.view(self.R, self.N_run), dim=1).reshape(-1)

    # ------------------------------------------------------------------------------------------------------ :297-397
    def _step(self, key, time, log_weights, state, int_var, suff_stats):
        """Algorithm1.step over the R N particles; returns its tuple with the GLOBAL ancestors and, behind it, the local ones (R N,)."""
        rand, time, lam = self._rand(key), int(time), self.forgetting_factor
        suff_stats = self._dev_shapes(suff_stats)
        aux_state, aux_int_var, factors = self._generate_auxiliary_states(state, time, int_var, suff_stats, scale=lam)   # :323-325
        ll_aux = self.SSM.log_likelihood(self._obs(time), aux_state, self._inp(time), *aux_int_var)    # :328-341
        u = rand.uniform_dev(STREAM_RESAMPLE, time)
        a_loc, a = self.ops.runs_systematic(self.R, u, (ll_aux + log_weights).contiguous())   # :342-347, every run in its own workgroup
        a_loc, a = a_loc.reshape(-1), a.reshape(-1)
        new_state = self._draw_states(rand, time, state, int_var, a)                       # :350-353
        new_int_var, new_basis = self._draw_int_vars(rand, time, new_state, suff_stats, a, factors, scale=lam)   # :358-367
        new_stats = tuple(self.ops.stats_gather_update(lam, a, suff_stats[i], new_basis[i], new_int_var[i].reshape(-1) if self.nvar[i] == 1 else new_int_var[i])
                          for i in range(self.N_int))                                      # :370-377
        new_lw = self.SSM.log_likelihood(self._obs(time), new_state, self._inp(time), *new_int_var) - ll_aux[a.long()]   # :380-390
        return new_lw, new_state, new_int_var, new_stats, a, a_loc

    def step(self, key, time, log_weights, state, int_var, suff_stats):
        """Algorithm1.step over the flattened particle axis (run r at [r N, (r + 1) N)): `key` holds the R root keys; the returned ancestor
        indices are global (r N + the run's own index)."""
        return self._step(key, time, log_weights, state, int_var, suff_stats)[:5]

    # ------------------------------------------------------------------------------------------------------ :399-492
    def _loop_body(self, rand, time, traces, suff_stats):
        state_trace, int_var_trace, sst, lw_trace, anc_trace = traces
        if self._tidx is None:
            prev = lambda a: a[time - 1]                                                   # noqa: E731
            put = lambda a, v, back=0: a.__setitem__(time - back, v.reshape(a.shape[1:]))   # noqa: E731
        else:   # graph mode: rows addressed through the device-resident time index
            prev = lambda a: a.index_select(0, self._tidx[1]).squeeze(0)                   # noqa: E731
            put = lambda a, v, back=0: a.index_copy_(0, self._tidx[back], v.reshape((1,) + a.shape[1:]).to(a.dtype))   # noqa: E731
        lw, x, iv, suff_stats, _, a_loc = self._step(rand, time, prev(lw_trace), prev(state_trace), [prev(int_var_trace[i]) for i in range(self.N_int)],
                                                     suff_stats)
        put(state_trace, x)
        put(lw_trace, lw)
        put(anc_trace, a_loc, 1)   # the trace keeps every run's own indices
        w = self._softmax(lw)
        for i in range(self.N_int):
            put(int_var_trace[i], iv[i])
            for j, v in enumerate(self._weighted(suff_stats[i], w)):
                put(sst[i][j], v)                                                          # :445-457
        return suff_stats

    def __call__(self, key, keys=None, use_graph=None):
        """-> Algorithm1.__call__'s 8-tuple with a leading run axis on every array: state_trace (R, T, N, n_x), int_var_trace[i] (R, T, N, n),
        suff_stats_trace[i][j] (R, T, ...), weights_trace (R, T, N), ancestor_trace (R, T-1, N) (every run's own indices), suff_stats[i][j]
        (R, N, ...), obs_trace (R, T, N, n_y), log_likelihood (R, T, N).  Run r is Algorithm1(N_samples, ...)(keys[r]), keys default
        random.split(key, R).  use_graph as in Algorithm1; default: when R N <= 4096 -- Algorithm1's bound on the whole particle axis: the carried
        statistics are copied once per step, and from R N = 12 800 on (M = 41) the eager loop is the faster one."""
        R, N = self.R, self.N_run
        rand = self._rand(root_keys(key, R, keys))
        state_trace, int_var_trace, sst, lw_trace, anc_trace, suff_stats = self._init_algorithm(rand)
        T = self.observations.shape[0]
        traces = (state_trace, int_var_trace, sst, lw_trace, anc_trace)
        if use_graph is None:
            use_graph = R * N <= 4096
        if use_graph and T > 1:
            suff_stats = self._graphed_loop(rand, traces, suff_stats, T)
        else:
            for time in range(1, T):
                suff_stats = self._loop_body(rand, time, traces, suff_stats)
        self.ops.check()
        weights_trace = torch.softmax(lw_trace.view(T, R, N), dim=2)                       # :460
        obs_trace = torch.stack([self.SSM.output_mdl(state_trace[t], self.inputs[t], *[v[t] for v in int_var_trace]).reshape(R * N, -1)
                                 for t in range(T)])                                       # :463-468
        loglik = torch.stack([self.SSM.log_likelihood(self.observations[t], state_trace[t], self.inputs[t], *[v[t] for v in int_var_trace])
                              for t in range(T)])                                          # :471-481

        def runs_first(a):   # (T, R N, ...) -> (R, T, N, ...)
            return a.view((a.shape[0], R, N) + tuple(a.shape[2:])).transpose(0, 1).contiguous()

        stats = tuple(tuple(s.reshape((R, N) + tuple(s.shape[1:])) for s in per) for per in self._ref_shapes(suff_stats))
        return (runs_first(state_trace), [runs_first(v) for v in int_var_trace], [[s.transpose(0, 1).contiguous() for s in per] for per in sst],
                weights_trace.transpose(0, 1).contiguous(), runs_first(anc_trace), stats, runs_first(obs_trace), runs_first(loglik))
