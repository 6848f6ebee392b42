"""C independent chains of the marginalised Particle Gibbs sampler (Algorithm2 over the conditional filter Algorithm3, reference
src/Algorithm2.py, src/Algorithm3.py) on one model and one data set, every filter step batched over the chains.

``MultiChainAlgorithm3(C, N_samples, ...)`` and ``MultiChainAlgorithm2(C, N_samples, N_iterations, ...)`` take Algorithm3's / Algorithm2's
constructor arguments behind the number of chains.  Chain c uses root key ``keys[c]`` (default ``random.split(key, C)[c]``) and computes
what the single-chain class computes with that key and that chain's reference trajectory; a filter step of all chains is the launches of
one.  The particle axis is C N long with chain c at [c N, (c + 1) N): the per-particle kernels serve it with GLOBAL ancestor indices
(c N + a), as in pgas_amd/runs.py, whose random numbers (RunsRand) and resampler (runs_systematic) are reused.  Per chain, and therefore
batched entry points of their own (include/pgas_marginal.h): the reference statistics added in the second MNIW solve and in the base
measures (pgas_m_runs_mniw_solve_n, pgas_m_runs_lbm_diff), the categorical draws of the reference particle's ancestor and of the final
index (pgas_m_runs_categorical), and the trajectories (pgas_m_runs_backtrace).  No step contains a host round trip or a loop over chains.

N_samples <= 1024 per chain (the one-workgroup resampler and categorical draw).  Observations and inputs are shared by the chains.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import random as prng
from .Algorithm1 import STREAM_ANCESTOR, STREAM_FINAL, STREAM_RESAMPLE, _small_cholesky, _t
from .Algorithm3 import Algorithm3
from .chains import keys_tensor, root_keys
from .runs import RunsRand

MAX_PARTICLES = 1024


# ---------------------------------------------------------------------------------------------------------------- host-side checks
def check_sizes(C, N_samples):
    """(C, N) as integers, or ValueError -- before any device object exists."""
    C, N = int(C), int(N_samples)
    if C < 1:
        raise ValueError("C must be >= 1")
    if N < 1:
        raise ValueError("N_samples must be >= 1")
    if N > MAX_PARTICLES:
        raise ValueError(f"N_samples = {N}: the batched resampler and categorical draw serve at most {MAX_PARTICLES} particles per chain -- "
                         "run Algorithm2 once per key instead")
    return C, N


def check_keys(keys, C):
    """ValueError unless `keys` holds C keys (integers, or a (C,) int64 tensor of bit patterns).  Host only."""
    if isinstance(keys, torch.Tensor):
        n = keys.shape[0] if keys.dim() == 1 and keys.dtype == torch.int64 else -1
    else:
        keys = list(keys)
        n = len(keys)
    if n != int(C):
        raise ValueError(f"keys: expected {int(C)} keys (integers or a ({int(C)},) int64 tensor of key bit patterns), got {n if n >= 0 else 'another tensor'}")
    return keys


def chain_reference(a, C, T, width, what, shared_ok=False):
    """A reference array as a host or device tensor of shape (C, T, width): accepts (C, T, width), for width 1 also (C, T), and with
    shared_ok the same without the chain axis (one reference for every chain).  ValueError otherwise; nothing is launched."""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
    s = tuple(t.shape)
    if s == (C, T, width) or (width == 1 and s == (C, T)):
        return t.reshape(C, T, width)
    if shared_ok and (s == (T, width) or (width == 1 and s == (T,))):
        return t.reshape(1, T, width).expand(C, T, width)
    want = f"({C}, {T}, {width})" + (f" or ({T}, {width})" if shared_ok else "")
    raise ValueError(f"{what}: expected shape {want}, got {s}")


def iteration_keys(roots, N_iterations):
    """The (K - 1, C) keys of the conditional filters, row k - 1 for Gibbs iteration k: chain c splits its key once per iteration exactly as
    Algorithm2 does (``key, key_step = split(key, 2)``, src/Algorithm2.py:121).  Host arithmetic (Philox on Python integers)."""
    K, C = int(N_iterations), len(roots)
    out = np.zeros((max(K - 1, 0), C), dtype=np.uint64)
    for c, key in enumerate(roots):
        key = prng.as_key(key)
        for k in range(1, K):
            key, key_step = prng.split(key, 2)
            out[k - 1, c] = key_step
    return out


# ---------------------------------------------------------------------------------------------------------------- the conditional filter
class MultiChainAlgorithm3(Algorithm3):
    def __init__(self, C, N_samples, observations, inputs, SSM, init_state_mean, init_state_cov, init_int_var_mean, init_int_var_cov, GP_prior,
                 basis_fcn, device=None):
        self.C, self.N_run = check_sizes(C, N_samples)
        # Algorithm3 over the flattened particle axis: self.N_samples = C N, self.ops = MarginalOps(C N), traces time-major (T, C N, ...).
        # (_init_algorithm's weighted statistics trace then sums over all chains; the conditional filter never reads it.)
        super().__init__(self.C * self.N_run, observations, inputs, SSM, init_state_mean, init_state_cov, init_int_var_mean, init_int_var_cov,
                         GP_prior, basis_fcn, device=device)
        self._last_global = (torch.arange(self.C, dtype=torch.int32, device=self.device) * self.N_run + (self.N_run - 1)).contiguous()

    _weight_count = property(lambda self: self.N_run)   # the initial weights are 1 / N of the particle's own chain

    def _rand(self, key):
        """A provider as it is; C keys (integers or an int64 device tensor of bit patterns) -> the chains' device streams."""
        if hasattr(key, "student_t"):
            return key
        return RunsRand(self.ops, keys_tensor(check_keys(key, self.C), self.device))

    def _slot(self, a):
        """The reference slot (particle N - 1 of every chain) of a per-particle array (C N, ...) as a strided (C, ...) view."""
        return a.view((self.C, self.N_run) + tuple(a.shape[1:]))[:, -1]

    def _per_particle(self, r):
        """A per-chain array (C, ...) repeated over the chain's particles: (C N, ...)."""
        return r.repeat_interleave(self.N_run, dim=0)

    def _log_base_measure_runs(self, i, stats, ref, sol=None):
        """Algorithm3._log_base_measure's general form (n > 1, BI:111-124) with the reference statistics of the particle's own chain."""
        P0, P1, P2, P3 = self.GP_prior[i]
        T0, T1, T2, T3 = stats
        nv, M = self.nvar[i], P0.shape[0]
        R0, R1, r2, r3 = ref
        if sol is None:
            sol = self.ops.mniw_solve(P0, P1, T0, T1, R0=R0.contiguous(), R1=R1.contiguous(), want=("q", "logdet"), runs=self.C)
        nu = P3 + T3 + self._per_particle(r3)
        Lp = _small_cholesky(P2 + T2 + self._per_particle(r2) - sol["q"])
        logdet_psi = 2.0 * torch.log(torch.diagonal(Lp, dim1=1, dim2=2)).sum(dim=1)
        mgl = nv * (nv - 1) / 4.0 * math.log(math.pi) + sum(torch.lgamma(nu / 2 - j / 2.0) for j in range(nv))
        return (-0.5 * nv * M * math.log(2 * math.pi) + 0.5 * nv * sol["logdet"] - 0.5 * nu * nv * math.log(2.0) - mgl + logdet_psi * nu / 2)

    # ------------------------------------------------------------------------------------------------------ :43-197
    def _step(self, key, time, log_weights, state, int_var, suff_stats, ref_state, ref_int_var, ref_suff_stats):
        """Algorithm3.step over the C N particles.  ref_state (C, n_x), ref_int_var[i] (C,) or (C, n), ref_suff_stats[i] = (R0 (C, M[, n]),
        R1 (C, M, M), R2 (C[, n, n]), R3 (C,)).  Returns its tuple with the GLOBAL ancestors and, behind it, the chains' own (C N,)."""
        rand, time, C, N = self._rand(key), int(time), self.C, self.N_run
        suff_stats = self._dev_shapes(suff_stats)
        aux_state, aux_int_var, factors = self._generate_auxiliary_states(state, time, int_var, suff_stats)      # :66-68
        ll_aux = self.SSM.log_likelihood(self._obs(time), aux_state, self._inp(time), *aux_int_var)     # :71-84
        lw_aux = ll_aux + log_weights
        a_loc, a = self.ops.runs_systematic(C, rand.uniform_dev(STREAM_RESAMPLE, time), lw_aux.contiguous())   # :85-90, a workgroup per chain
        if self.SSM.is_deterministic:   # quirk Q15: the reference particle keeps its own ancestor
            a_loc[:, -1:].fill_(N - 1)
            a[:, -1].copy_(self._last_global)
        else:
            g = None
            for i in range(self.N_int):                                                    # :93-108  g_t - g_T
                if self.nvar[i] == 1:
                    P0, P1, P2, P3 = self.GP_prior[i]
                    T0, T1, T2, T3 = suff_stats[i]
                    R0, R1, r2, r3 = ref_suff_stats[i]
                    sol2 = self.ops.mniw_solve(P0, P1, T0, T1, R0=R0.contiguous(), R1=R1.contiguous(), want=("q", "logdet"), runs=C)
                    gi = self.ops.runs_lbm_diff(C, P0.numel(), T2, T3, factors[i], sol2, P2, P3, r2, r3)
                else:
                    gi = self._log_base_measure(i, suff_stats[i], sol=factors[i]) - self._log_base_measure_runs(i, suff_stats[i], ref_suff_stats[i])
                g = gi if g is None else g + gi
            if getattr(self, "_Qc", None) is None:
                Lq = np.linalg.cholesky(self.SSM.process_noise)
                self._Qc = (_t(np.linalg.inv(Lq), self.device).T.contiguous(), -0.5 * Lq.shape[0] * math.log(2 * math.pi) - float(np.sum(np.log(np.diag(Lq)))))
            target = self._per_particle(ref_state)                                         # (C N, n_x): every particle against its chain's reference
            h_x = self.SSM.transition_logpdf_rows(target, state, self._inp(time, 1), *int_var) if hasattr(self.SSM, "transition_logpdf_rows") else None
            if h_x is None:
                e = (target - aux_state) @ self._Qc[0]                                     # :109-116
                h_x = self._Qc[1] - 0.5 * (e * e).sum(dim=1)
            # :117-127 softmax, cumsum, searchsorted, clip and the write of the reference slot of both ancestor vectors, one launch
            self.ops.runs_categorical(C, lw_aux + g + h_x, rand.uniform_dev(STREAM_ANCESTOR, time), anc_local=a_loc, anc_global=a)
        a_loc, a = a_loc.reshape(-1), a.reshape(-1)
        new_state = self._draw_states(rand, time, state, int_var, a).contiguous()          # :130-133
        self._slot(new_state).copy_(ref_state)                                             # :134
        new_int_var, new_basis = self._draw_int_vars(rand, time, new_state, suff_stats, a, factors)              # :139-148
        new_int_var = tuple(v.contiguous() for v in new_int_var)
        for i in range(self.N_int):
            self._slot(new_int_var[i]).copy_(ref_int_var[i].reshape(C, self.nvar[i]))      # :149-152
        new_stats = tuple(self.ops.stats_gather_update(1.0, a, suff_stats[i], new_basis[i], new_int_var[i].reshape(-1) if self.nvar[i] == 1 else new_int_var[i])
                          for i in range(self.N_int))                                      # :155-162
        new_ref = []
        for i in range(self.N_int):                                                        # :165-176
            rb = self.basis_fcn[i](ref_state, self._inp(time))                             # (C, M)
            R0, R1, R2, R3 = ref_suff_stats[i]
            if self.nvar[i] > 1:
                xi = ref_int_var[i].reshape(C, self.nvar[i])
                new_ref.append((R0 - rb[:, :, None] * xi[:, None, :], R1 - rb[:, :, None] * rb[:, None, :], R2 - xi[:, :, None] * xi[:, None, :], R3 - 1.0))
                continue
            xi = ref_int_var[i].reshape(C)
            new_ref.append((R0 - rb * xi[:, None], R1 - rb[:, :, None] * rb[:, None, :], R2 - xi * xi, R3 - 1.0))
        new_lw = self.SSM.log_likelihood(self._obs(time), new_state, self._inp(time), *new_int_var) - ll_aux[a.long()]   # :179-189
        return new_lw, new_state, new_int_var, new_stats, a, tuple(new_ref), a_loc

    def step(self, key, time, log_weights, state, int_var, suff_stats, ref_state, ref_int_var, ref_suff_stats):
        """Algorithm3.step over the flattened particle axis (chain c at [c N, (c + 1) N)): `key` holds the C root keys, the reference
        arguments carry a leading chain axis on the device; the returned ancestor indices are global (c N + the chain's own index)."""
        return self._step(key, time, log_weights, state, int_var, suff_stats, ref_state, ref_int_var, ref_suff_stats)[:6]

    # ------------------------------------------------------------------------------------------------------ :199-303
    def _references(self, ref_state, ref_int_var, ref_suff_stats):
        """The call's reference arguments checked on the host and brought to the device time-major: ref_state (T, C, n_x), ref_int_var[i]
        (T, C) or (T, C, n), ref_suff_stats[i] = (R0 (C, M[, n]), R1 (C, M, M), R2 (C[, n, n]), R3 (C,))."""
        C, T, dev = self.C, self.observations.shape[0], self.device
        nx = self.init_state_mean.numel()
        if len(ref_int_var) != self.N_int or len(ref_suff_stats) != self.N_int:
            raise ValueError(f"ref_int_var / ref_suff_stats: expected one entry per interface variable ({self.N_int})")
        host = [chain_reference(ref_state, C, T, nx, "ref_state")]
        host += [chain_reference(v, C, T, nv, f"ref_int_var[{i}]") for i, (v, nv) in enumerate(zip(ref_int_var, self.nvar))]
        stats = []
        for i, (rs, M, nv) in enumerate(zip(ref_suff_stats, self.dim_basis, self.nvar)):
            if len(rs) != 4:
                raise ValueError(f"ref_suff_stats[{i}]: expected the four statistics (T0, T1, T2, T3)")
            shapes = ((C, M) if nv == 1 else (C, M, nv), (C, M, M), (C,) if nv == 1 else (C, nv, nv), (C,))
            row = []
            for j, (r, shp) in enumerate(zip(rs, shapes)):
                r = r if isinstance(r, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(r, dtype=np.float64))
                if r.numel() != math.prod(shp) or r.shape[0] != C:
                    raise ValueError(f"ref_suff_stats[{i}][{j}]: expected a leading chain axis and {shp} elements in all, got {tuple(r.shape)}")
                row.append((r, shp))
            stats.append(row)
        up = lambda t: t.to(device=dev, dtype=torch.float64)  # noqa: E731
        ref_state = up(host[0]).transpose(0, 1).contiguous()
        ref_int_var = [up(v).transpose(0, 1).contiguous().reshape((T, C) if nv == 1 else (T, C, nv)) for v, nv in zip(host[1:], self.nvar)]
        ref_ss = [tuple(up(r).reshape(shp).contiguous() for r, shp in row) for row in stats]
        return ref_state, ref_int_var, ref_ss

    def __call__(self, keys, ref_state, ref_int_var, ref_suff_stats, return_traces=False, use_graph=None):
        """keys: C integer keys or a (C,) int64 tensor; ref_state (C, T, n_x); ref_int_var[i] (C, T[, n]); ref_suff_stats[i][j] with a leading
        chain axis ((C, M[, n]), (C, M, M), (C[, n, n]), (C,); unit axes as Algorithm2 stores them are accepted)
        -> state_traj (C, T, n_x), int_var_traj [(C, T, n)]; chain c is Algorithm3(N_samples, ...)(keys[c], ref_state[c], ...).  With
        return_traces a dict behind them: state_trace (C, T, N, n_x), int_var_trace [(C, T, N, n)], ancestor_trace (C, T-1, N) (every chain's
        own indices), log_weights (C, N), idx (C,) int32 -- all on the device.  use_graph as in Algorithm3; default: when C N <= 4096."""
        C, N, dev = self.C, self.N_run, self.device
        if not hasattr(keys, "student_t"):
            keys = check_keys(keys, C)
        ref_state, ref_int_var, ref_ss = self._references(ref_state, ref_int_var, ref_suff_stats)   # refusals come before any launch
        rand = self._rand(keys)
        state_trace, int_var_trace, _, lw_trace, anc_trace, suff_stats = self._init_algorithm(rand)
        T = self.observations.shape[0]
        self._slot(state_trace[0]).copy_(ref_state[0])                                     # :221
        suff_stats = [list(s) for s in suff_stats]
        for i in range(self.N_int):
            nv = self.nvar[i]
            self._slot(int_var_trace[i][0]).copy_(ref_int_var[i][0].reshape(C, nv))        # :224
            ib = self.basis_fcn[i](ref_state[0], self.inputs[0])                           # :225  (C, M)
            xi = ref_int_var[i][0]
            ones = torch.ones(C, dtype=torch.float64, device=dev)
            if nv > 1:
                iT = (ib[:, :, None] * xi[:, None, :], ib[:, :, None] * ib[:, None, :], xi[:, :, None] * xi[:, None, :], ones)
            else:
                iT = (ib * xi[:, None], ib[:, :, None] * ib[:, None, :], xi * xi, ones)     # :226
            for j in range(4):
                suff_stats[i][j] = suff_stats[i][j].contiguous()
                self._slot(suff_stats[i][j]).copy_(iT[j])                                  # :228-231
            ref_ss[i] = tuple(ref_ss[i][j] - iT[j] for j in range(4))                      # :235-246
        suff_stats = tuple(tuple(s) for s in suff_stats)

        def body(time, carried):                                                           # one iteration of :251-290
            stats, rss = carried
            graphed = self._tidx is not None
            prev = (lambda a: a.index_select(0, self._tidx[1]).squeeze(0)) if graphed else (lambda a: a[time - 1])
            put = (lambda a, v, back=0: a.index_copy_(0, self._tidx[back], v.reshape((1,) + a.shape[1:]).to(a.dtype))) if graphed else \
                (lambda a, v, back=0: a.__setitem__(time - back, v.reshape(a.shape[1:])))
            lw, x, iv, stats, _, rss, a_loc = self._step(rand, time, prev(lw_trace), prev(state_trace), [prev(int_var_trace[i]) for i in range(self.N_int)],
                                                         stats, self._row(ref_state, time), [self._row(ref_int_var[i], time) for i in range(self.N_int)], rss)
            put(state_trace, x)
            put(lw_trace, lw)
            put(anc_trace, a_loc, 1)   # the trace keeps every chain's own indices
            for i in range(self.N_int):
                put(int_var_trace[i], iv[i])
            return stats, tuple(tuple(r) for r in rss)

        carried = (suff_stats, tuple(tuple(r) for r in ref_ss))
        if use_graph is None:
            use_graph = C * N <= 4096 and hasattr(rand, "uniform_dev")
        if use_graph and T > 1:
            carried = self._replay(T, carried, body)                                       # Algorithm1._replay: one captured step, replayed
        else:
            for time in range(1, T):
                carried = body(time, carried)
        self.ops.check()
        idx = self.ops.runs_categorical(C, lw_trace[-1], rand.uniform_dev(STREAM_FINAL, 0))   # :293-294, one draw per chain
        state_traj = self.ops.runs_backtrace(C, state_trace, anc_trace, idx)               # :295
        int_var_traj = tuple(self.ops.runs_backtrace(C, int_var_trace[i], anc_trace, idx) for i in range(self.N_int))   # :296-299
        if return_traces:
            def chains_first(a):   # (T', C N, ...) -> (C, T', N, ...)
                return a.view((a.shape[0], C, N) + tuple(a.shape[2:])).transpose(0, 1).contiguous()

            return state_traj, int_var_traj, dict(state_trace=chains_first(state_trace), int_var_trace=[chains_first(v) for v in int_var_trace],
                                                  ancestor_trace=chains_first(anc_trace), log_weights=lw_trace[-1].view(C, N).clone(), idx=idx)
        return state_traj, int_var_traj


# ---------------------------------------------------------------------------------------------------------------- Particle Gibbs
class MultiChainAlgorithm2:
    def __init__(self, C, N_samples, N_iterations, observations, inputs, SSM, init_state_mean, init_state_cov, init_int_var_mean,
                 init_int_var_cov, GP_prior, basis_fcn, device=None):
        self.C, _ = check_sizes(C, N_samples)
        self.N_iterations = int(N_iterations)
        self.N_steps = np.asarray(observations).shape[0]
        self.cSMC = MultiChainAlgorithm3(C, N_samples=N_samples, observations=observations, inputs=inputs, SSM=SSM, init_state_mean=init_state_mean,
                                         init_state_cov=init_state_cov, init_int_var_mean=init_int_var_mean, init_int_var_cov=init_int_var_cov,
                                         GP_prior=GP_prior, basis_fcn=basis_fcn, device=device)   # :28-39

    def _trajectory_stats(self, state_traj, int_var_traj):
        """Algorithm2._trajectory_stats for every chain at once: state_traj (C, T, n_x), int_var_traj[i] (C, T, n) -> per interface variable
        (T0 (C, M[, n]), T1 (C, M, M), T2 (C[, n, n]), T3 (C,)): the basis of the C T rows in one call, the sums over time as torch.bmm."""
        c, C, T = self.cSMC, self.C, self.N_steps
        out = []
        u = c.inputs.reshape(T, -1)
        for i in range(c.N_int):
            bf = c.basis_fcn[i]
            if hasattr(bf, "trajectory"):      # row (c, t) with inputs[t]
                basis = bf.trajectory(state_traj.reshape(C * T, -1), u.repeat(C, 1)).reshape(C, T, -1)
            else:                              # arbitrary user callables keep the reference's per-step call, all chains' rows of a step at once
                basis = torch.stack([bf(state_traj[:, t], c.inputs[t]).reshape(C, -1) for t in range(T)], dim=1)
            bt = basis.transpose(1, 2)
            T3 = torch.full((C,), float(T), dtype=torch.float64, device=c.device)
            xi = int_var_traj[i].reshape(C, T, c.nvar[i])
            if c.nvar[i] > 1:
                out.append((torch.bmm(bt, xi), torch.bmm(bt, basis), torch.bmm(xi.transpose(1, 2), xi), T3))
                continue
            out.append((torch.bmm(bt, xi).squeeze(-1), torch.bmm(bt, basis), (xi * xi).sum(dim=(1, 2)), T3))
        return out

    def __call__(self, key, init_ref_state, init_ref_int_var, keys=None, progress=None):
        """-> Algorithm2's 6-tuple with a leading chain axis: state_trace (C, T, K, n_x), int_var_trace [(C, T, K, n)], weights (C, T, K),
        suff_stats_trace [[(C, K, M, n), (C, K, M, M), (C, K, n, n), (C, K)]], obs_trace (C, T, K, n_y), log_likelihood (C, T, K).  Chain c is
        Algorithm2(N_samples, N_iterations, ...)(keys[c], init_ref_state[c], ...), keys default random.split(key, C); init_ref_state (T, n_x)
        shared by the chains or (C, T, n_x), init_ref_int_var[i] likewise."""
        c, C, K, T, dev = self.cSMC, self.C, self.N_iterations, self.N_steps, self.cSMC.device
        nx = c.init_state_mean.numel()
        roots = root_keys(key, C, keys)                                                    # ValueError on a wrong number of keys
        if len(init_ref_int_var) != c.N_int:
            raise ValueError(f"init_ref_int_var: expected one entry per interface variable ({c.N_int})")
        x0 = chain_reference(init_ref_state, C, T, nx, "init_ref_state", shared_ok=True)
        v0 = [chain_reference(v, C, T, nv, f"init_ref_int_var[{i}]", shared_ok=True) for i, (v, nv) in enumerate(zip(init_ref_int_var, c.nvar))]
        step_keys = keys_tensor(torch.as_tensor(iteration_keys(roots, K).view(np.int64)).reshape(-1), dev).reshape(max(K - 1, 0), C)   # one upload
        state_trace = torch.zeros((K, C, T, nx), dtype=torch.float64, device=dev)                                 # :46-54
        state_trace[0] = x0.to(device=dev, dtype=torch.float64)
        int_var_trace = [torch.zeros((K, C, T, nv), dtype=torch.float64, device=dev) for nv in c.nvar]            # :56-67
        for i in range(c.N_int):
            int_var_trace[i][0] = v0[i].to(device=dev, dtype=torch.float64)
        sst = [[torch.zeros((K, C, M, nv), dtype=torch.float64, device=dev), torch.zeros((K, C, M, M), dtype=torch.float64, device=dev),
                torch.zeros((K, C, nv, nv), dtype=torch.float64, device=dev), torch.zeros((K, C), dtype=torch.float64, device=dev)]
               for M, nv in zip(c.dim_basis, c.nvar)]   # :68-79
        ref_stats = self._trajectory_stats(state_trace[0], [v[0] for v in int_var_trace])                        # :81-93
        for i in range(c.N_int):
            for j in range(4):
                sst[i][j][0] = ref_stats[i][j].reshape(sst[i][j][0].shape)                                        # :94-99
        for k in range(1, K):                                                                                     # :117-160
            new_state, new_int_var = c(step_keys[k - 1], state_trace[k - 1], [v[k - 1] for v in int_var_trace],
                                       [[sst[i][j][k - 1] for j in range(4)] for i in range(c.N_int)])            # :122-134
            state_trace[k] = new_state                                                                            # :137
            stats = self._trajectory_stats(new_state, new_int_var)
            for i in range(c.N_int):
                int_var_trace[i][k] = new_int_var[i]                                                              # :139
                for j in range(4):
                    sst[i][j][k] = stats[i][j].reshape(sst[i][j][k].shape)                                        # :140-160
            if progress is not None:
                progress(k)
        state_trace = state_trace.permute(1, 2, 0, 3).contiguous()                                                # :161 -> (C, T, K, nx)
        int_var_trace = [v.permute(1, 2, 0, 3).contiguous() for v in int_var_trace]                               # :162-165
        flat = lambda a: a.reshape((C * K,) + tuple(a.shape[2:]))  # noqa: E731   # row t of every chain and iteration in one model call
        obs_trace = torch.stack([c.SSM.output_mdl(flat(state_trace[:, t]), c.inputs[t], *[flat(v[:, t]) for v in int_var_trace]).reshape(C, K, -1)
                                 for t in range(T)], dim=1)                                                       # :168-173
        loglik = torch.stack([c.SSM.log_likelihood(c.observations[t], flat(state_trace[:, t]), c.inputs[t], *[flat(v[:, t]) for v in int_var_trace]).reshape(C, K)
                              for t in range(T)], dim=1)                                                          # :176-185
        weights = torch.full((C, T, K), 1.0 / K, dtype=torch.float64, device=dev)                                 # :180
        return state_trace, int_var_trace, weights, [[s.transpose(0, 1).contiguous() for s in per] for per in sst], obs_trace, loglik
