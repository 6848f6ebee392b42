"""One model learned from several records (experiments) that share (A, S), every step batched over chains and records (DESIGN.md
section 24).

* ``condSequentialMonteCarloRecords(C, N_samples, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn, basis_fcn)``:
  ``observations`` / ``inputs`` are sequences of E arrays, record e of T_e rows.  ``__call__(keys, ref_state, coeff_mat, error_cov)``
  runs C x E conditional-SMC sweeps in one launch, one workgroup per (chain, record); nothing propagates across a seam, and sweep (c, e)
  is exactly what ``condSequentialMonteCarlo`` built on record e alone computes with seeds[c, e], record e's reference and chain c's
  (A, S).  Every result is laid out over the concatenation, Tsum = sum T_e rows with record e's at ``row0[e]``; ``record(e, a)`` cuts
  record e out of any (..., Tsum, ...) array.
* ``MultiRecordPGAS(C, N_samples, N_iterations, ..., GP_prior, basis_fcn)``: ``MultiChainPGAS`` step for step, with the sweeps per
  record, the statistics summed over the records (no pair across a seam) and df = P3 + sum (T_e - 1).

Seeds: chain c's step key k gives record 0 the seed k and record e >= 1 the seed ``random.split(k, E)[e]``, so one record is exactly
the chain layer.  N <= 1024 particles; the limits of ``condSequentialMonteCarloChains`` hold.  The validation calls (rollout, filter,
smooth, ...) are not offered on a record table: build an ordinary context on the record to validate on.
"""
from __future__ import annotations

import numpy as np
import torch

from . import random as prng
from .chains import MultiChainPGAS, keys_tensor
from .PGAS import condSequentialMonteCarlo


def record_table(observations, inputs):
    """Sequences of E observation / input arrays, record e of T_e >= 2 rows each -> (row0 (E + 1,) int64, observations (Tsum, ...),
    inputs (Tsum, ...)): the concatenations and the first row of every record.  ``inputs`` None: a model without inputs."""
    if isinstance(observations, np.ndarray) or not hasattr(observations, "__len__"):
        raise ValueError("observations: expected a sequence of E arrays, one per record")
    ys = [np.asarray(y, dtype=np.float64) for y in observations]
    E = len(ys)
    if E < 1:
        raise ValueError("observations: no record")
    if inputs is None:
        us = [np.zeros((y.shape[0], 0)) if y.ndim else y for y in ys]
    else:
        if isinstance(inputs, np.ndarray) or not hasattr(inputs, "__len__") or len(inputs) != E:
            raise ValueError(f"inputs: expected a sequence of {E} arrays, one per record")
        us = [np.asarray(u, dtype=np.float64) for u in inputs]
    for e, (y, u) in enumerate(zip(ys, us)):
        if y.ndim < 1 or y.shape[0] < 2:
            raise ValueError(f"record {e}: needs at least 2 rows of observations")
        if u.ndim < 1 or u.shape[0] != y.shape[0]:
            raise ValueError(f"record {e}: {y.shape[0]} rows of observations, but inputs of shape {u.shape}")
        if y.shape[1:] != ys[0].shape[1:] or u.shape[1:] != us[0].shape[1:]:
            raise ValueError(f"record {e}: row shapes {y.shape[1:]} / {u.shape[1:]} differ from record 0's {ys[0].shape[1:]} / {us[0].shape[1:]}")
    row0 = np.concatenate([[0], np.cumsum([y.shape[0] for y in ys])]).astype(np.int64)
    if row0[-1] > np.iinfo(np.int32).max:
        raise ValueError("the records have more rows than a 32-bit row number holds")
    return row0, np.concatenate(ys, axis=0), np.concatenate(us, axis=0)


def init_states(E, init_state_mean, init_state_cov):
    """Shared (nx,) / (nx, nx), or per record (E, nx) / (E, nx, nx) -> (mean (nx,), cov (nx, nx), per-record means or None, per-record
    covariances or None); the shared pair is what the context is created with (record 0's where they are per record)."""
    m = np.asarray(init_state_mean, dtype=np.float64)
    P = np.asarray(init_state_cov, dtype=np.float64)
    m_rec = P_rec = None
    if m.ndim == 2:
        if m.shape[0] != E:
            raise ValueError(f"init_state_mean: leading dimension {m.shape[0]} for {E} records")
        m_rec, m = m, m[0]
    m = m.reshape(-1)
    nx = m.shape[0]
    if P.ndim == 3:
        if P.shape != (E, nx, nx):
            raise ValueError(f"init_state_cov: expected ({E}, {nx}, {nx}), got {P.shape}")
        P_rec, P = P, P[0]
    P = np.atleast_2d(P)
    if P.shape != (nx, nx):
        raise ValueError(f"init_state_cov: expected ({nx}, {nx}), got {P.shape}")
    if m_rec is not None and m_rec.shape != (E, nx):
        raise ValueError(f"init_state_mean: expected ({E}, {nx}), got {m_rec.shape}")
    if (m_rec is None) != (P_rec is None):   # the table takes both or neither
        m_rec = np.repeat(m[None], E, axis=0) if m_rec is None else m_rec
        P_rec = np.repeat(P[None], E, axis=0) if P_rec is None else P_rec
    return m, P, m_rec, P_rec


def stack_refs(ref_state, row0, C, nx, device=None):
    """A list of E arrays (record e: (T_e, nx)) shared by all chains, a (Tsum, nx) array or a (C, Tsum, nx) array -> (C, Tsum, nx)
    float64 tensor ((T_e,) / (Tsum,) / (C, Tsum) accepted for nx = 1)."""
    E, Tsum = len(row0) - 1, int(row0[-1])
    if isinstance(ref_state, (list, tuple)) and len(ref_state) == E and all(np.ndim(r) >= 1 for r in ref_state):
        parts = []
        for e, r in enumerate(ref_state):
            r = r.detach().cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r, dtype=np.float64)
            Te = int(row0[e + 1] - row0[e])
            if r.shape not in ((Te, nx),) + (((Te,),) if nx == 1 else ()):
                raise ValueError(f"ref_state[{e}]: expected ({Te}, {nx}), got {r.shape}")
            parts.append(r.reshape(Te, nx))
        ref_state = np.concatenate(parts, axis=0)
    expected = f"ref_state: expected {E} per-record arrays, ({Tsum}, {nx}) or ({C}, {Tsum}, {nx})"
    try:
        ref = ref_state if isinstance(ref_state, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(ref_state, dtype=np.float64))
    except ValueError:   # a ragged list that is not one array per record
        raise ValueError(f"{expected}, got {len(ref_state)} arrays") from None
    ref = ref.to(device=device, dtype=torch.float64)
    s = tuple(ref.shape)
    if s == (Tsum, nx) or (nx == 1 and s == (Tsum,)):
        return ref.reshape(1, Tsum, nx).expand(C, Tsum, nx).contiguous()
    if s == (C, Tsum, nx) or (nx == 1 and s == (C, Tsum)):
        return ref.reshape(C, Tsum, nx).contiguous()
    raise ValueError(f"{expected}, got {s}")


def record_slice(row0, e, a, axis=None):
    """Record e's rows of an array / tensor with one axis of length Tsum (``axis``: which one, when several are that long)."""
    E, Tsum = len(row0) - 1, int(row0[-1])
    e = int(e)
    if not 0 <= e < E:
        raise IndexError(f"record {e} of {E}")
    if axis is None:
        hits = [i for i, n in enumerate(a.shape) if n == Tsum]
        if len(hits) != 1:
            raise ValueError(f"shape {tuple(a.shape)}: {len(hits)} axes of length Tsum = {Tsum}; say which with axis=")
        axis = hits[0]
    elif a.shape[axis] != Tsum:
        raise ValueError(f"axis {axis} of shape {tuple(a.shape)} is not Tsum = {Tsum} long")
    idx = [slice(None)] * a.ndim
    idx[axis] = slice(int(row0[e]), int(row0[e + 1]))
    return a[tuple(idx)]


def records_df(P3, row0):
    """Degrees of freedom of the MNIW posterior: the prior's plus one per transition, sum (T_e - 1)."""
    return float(P3) + float(int(row0[-1]) - (len(row0) - 1))


def host_seeds(step_keys, E):
    """The seed rule on the host: (C, E) Python integers, seeds[c][0] = step_keys[c], seeds[c][e] = random.split(step_keys[c], E)[e]."""
    out = []
    for k in step_keys:
        k = prng.as_key(k)
        out.append([k] + prng.split(k, int(E))[1:])
    return out


class condSequentialMonteCarloRecords:
    def __init__(self, C, N_samples, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn, basis_fcn, device=None):
        """One model context on the concatenation of the E records, with the record table set.  ``single`` is that context's
        condSequentialMonteCarlo: like every single-record call it treats the concatenation as ONE record of Tsum rows."""
        self.C = int(C)
        if self.C < 1:
            raise ValueError("C must be >= 1")
        self.row0, y, u = record_table(observations, inputs)
        self.E, self.Tsum = len(self.row0) - 1, int(self.row0[-1])
        m, P, m_rec, P_rec = init_states(self.E, init_state_mean, init_state_cov)
        self.single = condSequentialMonteCarlo(N_samples, y, u, m, P, likelihood_fcn, basis_fcn, device=device)
        self.engine = self.single.engine
        self.device = self.engine.device
        self.N_samples = self.single.N_samples
        self.engine.records_set(self.row0, m_rec, P_rec)

    def record(self, e, a, axis=None):
        """Record e's rows of any (..., Tsum, ...) result."""
        return record_slice(self.row0, e, a, axis)

    def _batch(self, a, shape, what):
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: expected shape {shape}, got {tuple(t.shape)}")
        return t.to(device=self.device, dtype=torch.float64).contiguous()

    def _refs(self, ref_state):
        return stack_refs(ref_state, self.row0, self.C, self.engine.nx, self.device)

    def seeds(self, keys):
        """C step keys (integers or a (C,) int64 device tensor) -> (C, E) seeds by the seed rule; a (C, E) int64 tensor is taken as is."""
        if isinstance(keys, torch.Tensor) and keys.dim() == 2:
            if keys.dtype != torch.int64 or tuple(keys.shape) != (self.C, self.E):
                raise ValueError(f"keys: expected {self.C} step keys or a ({self.C}, {self.E}) int64 tensor, got {tuple(keys.shape)} {keys.dtype}")
            return keys.to(self.device).contiguous()
        k = keys_tensor(keys, self.device)
        if tuple(k.shape) != (self.C,):
            raise ValueError(f"keys: expected {self.C} keys, got {tuple(k.shape)[0]}")
        return self.engine.records_seeds(k)

    def set_params(self, coeff_mat, error_cov):
        eng = self.engine
        eng.chains_set_params(self._batch(coeff_mat, (self.C, eng.nx, eng.M), "coeff_mat"),
                              self._batch(error_cov, (self.C, eng.nx, eng.nx), "error_cov"))

    def __call__(self, keys, ref_state, coeff_mat, error_cov):
        """keys: C step keys or a (C, E) int64 tensor of seeds; ref_state: E per-record arrays, (Tsum, nx) or (C, Tsum, nx); coeff_mat
        (C, nx, M); error_cov (C, nx, nx) -> trajectories (C, Tsum, nx).  Enqueues work only."""
        seeds = self.seeds(keys)
        ref = self._refs(ref_state)
        self.set_params(coeff_mat, error_cov)
        return self.engine.records_sweep(seeds, ref)

    def traces(self):
        """(state traces (C, Tsum, N, nx), ancestor traces (C, Tsum, N) -- record e's T_e - 1 rows start at row0[e], the last row of each
        record is unused --, last log-weights (C, E, N)) of the last sweep (library-owned views)."""
        return self.engine.records_traces(self.C)

    def final_index(self):
        """(C, E) final indices of the last sweep (synchronises)."""
        return self.engine.records_final_index(self.C)


class MultiRecordPGAS(MultiChainPGAS):
    def __init__(self, C, N_samples, N_iterations, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn, GP_prior,
                 basis_fcn, device=None, keep_chain_log=True):
        """C Gibbs chains on E records that share (A, S): MultiChainPGAS with the sweeps per record (seeds by the seed rule from the
        chain's step key), the statistics summed over the records and df = P3 + sum (T_e - 1).  ``__call__(key, init_ref_state,
        keys=None)`` -> state_trace (C, Tsum, K, nx), log_likelihood (C, Tsum, K); init_ref_state in any form ``stack_refs`` takes."""
        cSMC = condSequentialMonteCarloRecords(C, N_samples, observations, inputs, init_state_mean, init_state_cov, likelihood_fcn,
                                               basis_fcn, device=device)
        self.row0, self.E = cSMC.row0, cSMC.E
        self._setup(C, N_iterations, cSMC, likelihood_fcn, GP_prior, keep_chain_log)
        self.df = records_df(self.GP_prior[3], self.row0)

    def suffstats(self, state_trajectories):
        return self.cSMC.engine.records_suffstats(state_trajectories)

    def record(self, e, a, axis=None):
        return self.cSMC.record(e, a, axis)
