"""The ancestor chase (k_backtrace inside a sweep, k_backtrace_idx behind pgas_reconstruct_trajectory): one lane records the
ancestral indices, then all threads gather the state rows.  Every comparison is exact (torch.equal): the trajectory must be
the path through the traces that starts at the final index, chased here with plain torch indexing over the trace blocks
the way bench.py's verify_last_sweep does it.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from common import experiments, pgas_amd

pytestmark = pytest.mark.gpu

SEED = 12345678


def _bt_chunk():
    """PG_BT_CHUNK, read from the kernel source the library is built from: the indices the chase records in LDS per pass (a longer
    sweep takes several passes).  The cases "just above the bound" follow the constant when it changes."""
    src = os.path.join(os.path.dirname(pgas_amd._lib.__file__), "csrc", "pgas_kernels.hip.h")
    m = re.search(r"^#define PG_BT_CHUNK (\d+)", open(src).read(), re.M)
    assert m, "PG_BT_CHUNK not found in csrc/pgas_kernels.hip.h"
    return int(m.group(1))


BT_CHUNK = _bt_chunk()


_MAKE = {"smo": experiments.smo_pgas, "toy": experiments.toy}


@functools.lru_cache(maxsize=None)
def _params(name):
    """One (A, S) per model for every T: the parameters' shapes do not depend on T, and initial_params needs at least one transition."""
    return experiments.initial_params(_MAKE[name](T=8))


@functools.lru_cache(maxsize=None)
def _problem(name, T):
    pb = _MAKE[name](T=max(T, 2))
    if T == 1:   # the simulators need two time steps: cut the data to one (no resampling step at all)
        pb.observations, pb.inputs, pb.X_true = pb.observations[:1], pb.inputs[:1], pb.X_true[:1]
    return pb, _params(name)


def _sweep(name, N, T, opts=()):
    pb, (A, S) = _problem(name, T)
    csmc = pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov,
                                             pb.likelihood_fcn, pb.basis_fcn)
    for k, v in opts:
        csmc.engine.set_option(k, v)
    return pb, csmc, csmc(SEED, pb.X_true, A, S).reshape(T, pb.nx)   # squeezed like the reference's for nx = 1


def _chase(eng, T, nx):
    """The ancestral path of the final index through the trace blocks, by plain torch indexing."""
    px = eng.traces_blocks(eng.TRACE_X, (eng.N, nx), torch.float64)
    pa = eng.traces_blocks(eng.TRACE_ANC, (eng.N,), torch.int32)
    rx, ra = px[0].shape[0], pa[0].shape[0]
    b = torch.tensor([eng.last_final_index()], device=px[0].device, dtype=torch.int64)
    rows = [None] * T
    for t in range(T - 1, -1, -1):
        rows[t] = px[t // rx][t % rx].index_select(0, b)[0]
        if t:
            b = pa[(t - 1) // ra][(t - 1) % ra].index_select(0, b).to(torch.int64)
    return torch.stack(rows)


def _check(name, N, T, opts=()):
    pb, csmc, traj = _sweep(name, N, T, opts)
    assert traj.shape == (T, pb.nx)
    ref = _chase(csmc.engine, T, pb.nx)
    assert torch.equal(traj, ref), f"{int((traj != ref).any(dim=1).sum())} of {T} rows are not on the ancestral path"
    return csmc


# N: one lane, below one segment, just over one segment, not a power of two.  T: no hop, one hop, two, one more than the 256 threads
# of the gather (its loop wraps), several gather passes.  N <= 1024 takes the one-launch small sweep by default, which chases
# inside its own kernel: option 14 = 0 (PGAS_OPT_SMALL_SWEEP off) sends the same sizes through k_backtrace.
@pytest.mark.parametrize("T", [1, 2, 3, 257, 700])
@pytest.mark.parametrize("N", [1, 200, 1025, 3000])
@pytest.mark.parametrize("name", ["smo", "toy"])
def test_sweep_trajectory_is_the_ancestral_path(name, N, T):
    csmc = _check(name, N, T)
    assert csmc.engine.launch_info()["small"] == (N <= 1024)


@pytest.mark.parametrize("T", [1, 2, 3, 257, 700])
@pytest.mark.parametrize("N", [1, 200])
@pytest.mark.parametrize("name", ["smo", "toy"])
def test_sweep_trajectory_small_n_through_k_backtrace(name, N, T):
    csmc = _check(name, N, T, ((14, 0),))
    assert not csmc.engine.launch_info()["small"]


@pytest.mark.parametrize("name", ["smo", "toy"])
def test_sweep_longer_than_one_chase_pass(name):
    """T just above the LDS index list: the chase hands its index over from one pass to the next, and the second pass is one row."""
    csmc = _check(name, 64, BT_CHUNK + 1, ((14, 0),))
    assert not csmc.engine.launch_info()["small"]


def test_captured_sweep_replays_the_chase():
    """PGAS_OPT_GRAPH: k_backtrace is a node of the captured sweep; the replay with another seed must chase that sweep's traces."""
    pb, csmc, _ = _sweep("smo", 3000, 257, ((13, 1),))
    A, S = _problem("smo", 257)[1]
    for seed in (SEED, SEED + 1):
        traj = csmc(seed, pb.X_true, A, S).reshape(257, pb.nx)
        assert csmc.engine.launch_info()["graph"]
        assert torch.equal(traj, _chase(csmc.engine, 257, pb.nx))


@pytest.mark.parametrize("name", ["smo", "toy"])
def test_blocked_traces(name):
    """PGAS_OPT_TRACE_BLOCK_BYTES = 4 MiB at N = 3000, T = 700: the state rows and the ancestor rows fall into blocks of different
    lengths (different shifts in the chase's block table), at least three blocks each."""
    csmc = _check(name, 3000, 700, ((12, 1 << 22),))
    eng = csmc.engine
    (_, rpb_x, nblk_x, _), (_, rpb_a, nblk_a, _) = eng.trace_layout(eng.TRACE_X), eng.trace_layout(eng.TRACE_ANC)
    assert nblk_x >= 3 and nblk_a >= 3 and rpb_x != rpb_a


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["smo", "toy"])
def test_local_group_chase_across_ranks(name, world):
    """Several shards on one device: the chase follows global indices through every rank's row blocks; the trajectory is the
    unsharded context's."""
    from pgas_amd import sharded

    N, T = world * 3 * 1024, 70
    pb, csmc, traj = _sweep(name, N, T)
    assert torch.equal(traj, _chase(csmc.engine, T, pb.nx))
    A, S = _problem(name, T)[1]
    grp = sharded.make_local_group(world, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn,
                                   trace_block_bytes=1 << 18)
    eng0 = grp.shards[0].eng
    assert eng0.trace_layout(eng0.TRACE_X)[2] >= 3 and eng0.trace_layout(eng0.TRACE_ANC)[2] >= 3
    assert eng0.trace_layout(eng0.TRACE_X)[1] != eng0.trace_layout(eng0.TRACE_ANC)[1]
    trajs = sharded.sharded_sweep(grp, SEED, pb.X_true, A, S)
    for r, tr in enumerate(trajs):
        assert torch.equal(tr.reshape(traj.shape), traj), f"rank {r}"


def _numpy_chase(P, anc, idx):
    T = P.shape[0]
    out = np.empty((T,) + P.shape[2:], dtype=P.dtype)
    b = idx
    for t in range(T - 1, -1, -1):
        out[t] = P[t, b]
        if t:
            b = anc[t - 1, b]
    return out


@functools.lru_cache(maxsize=None)
def _random_traces(N, T, nx):
    rng = np.random.default_rng(7)
    return rng.standard_normal((T, N, nx)), rng.integers(0, N, (max(T - 1, 1), N)).astype(np.int32)   # ancestors deliberately unsorted


@pytest.mark.parametrize("N,T,nx", [(5000, 300, 2), (5000, 300, 1), (5000, 300, 3), (64, 2 * BT_CHUNK + 5, 2), (7, 1, 2)])
def test_reconstruct_trajectory_against_numpy(N, T, nx):
    P, anc = _random_traces(N, T, nx)
    Pd, Ad = torch.as_tensor(P, device="cuda"), torch.as_tensor(anc, device="cuda")
    for idx in (0, N - 1, N // 3):
        got = pgas_amd.reconstruct_trajectory(Pd, Ad, idx).reshape(T, nx)
        assert torch.equal(got.cpu(), torch.as_tensor(_numpy_chase(P, anc, idx)).reshape(T, nx)), f"final index {idx}"


def test_reconstruct_trajectory_unaligned_views():
    """nx = 2 rows are moved as one 16-byte access when particles and output are 16-byte aligned; a view that starts 8 bytes into
    an allocation must take the per-component path and give the same rows."""
    N, T = 5000, 300
    P, anc = _random_traces(N, T, 2)
    eng = pgas_amd._lib.Engine.utility(N)
    buf = torch.zeros(T * N * 2 + 1, dtype=torch.float64, device="cuda")
    Pv = buf[1:].view(T, N, 2)
    Pv.copy_(torch.as_tensor(P))
    assert Pv.data_ptr() % 16 == 8 and Pv.is_contiguous()
    got = eng.reconstruct_trajectory(Pv, torch.as_tensor(anc, device="cuda"), N // 3)
    assert torch.equal(got.cpu(), torch.as_tensor(_numpy_chase(P, anc, N // 3)))
