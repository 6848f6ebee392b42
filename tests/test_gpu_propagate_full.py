"""k_propagate's whole-segment instance (k_propagate<2, 2, 7, 4, W, 7, 4, true, 1>, csrc/pgas_kernels.hip.h: propagate_kernel's FULL): the
instance launch_propagate chooses for the SingleMassOscillator shape on one unsharded device when N is a multiple of 1024, the model has
ny = 1 and the trace rows are 16-byte aligned.  It leaves out the guards for ragged segments and ranks, takes ny at compile time and
handles the conditioned particle in the last workgroup only; the arithmetic is the general instance's, so it is bit-identical by
construction.  Here that is CHECKED, bit for bit: PGAS_OPT_STEP_GENERIC (option 16) = 0 against 1 on the same arguments and seed (the
option switches k_step's and k_propagate's instances together), and both against the canonical C oracle -- state trace, ancestor trace,
final log-weights, final index, trajectory.  Which instance ran is read from launch_info()["propagate_instance"].

Sizes and lengths are those of tests/test_gpu_step_full.py (one segment, two, odd counts, a full group of 64 segments and one past it;
T = 2, 3, 12), and the oracle's sweeps are the ones that module computes, shared through its cache.

Non-finite states.  The general and the whole-segment instance both keep the guarded sin/cos(pi r) of the basis (|r| >= 2^30, inf and
NaN arguments).  Two parameter sets drive states through it within T = 12, both found with the oracle on the CPU and asserted from
its trace before anything is compared:
    "overflow"   A = sign(A) 1.7e308: every second step all states are beyond 2^30 and half of them +-inf, finite again in between
    "nan"        A = sign(A) 1e307 with one infinite coefficient, S scaled by 1e19: step 1 beyond 2^30 / inf, step 2 a mixture of finite
                 states beyond 2^30 and NaN (inf * 0 behind the guard), NaN everywhere but the conditioned particle from step 3 on
The two instances are compared by bit pattern there (NaN payloads included), the oracle with NaN == NaN."""
import functools

import numpy as np
import pytest

from common import canon_model, experiments, pgas_amd
from test_gpu_step_full import SEED, _against_oracle, _oracle, _same

pytestmark = pytest.mark.gpu

OPT_SMALL_SWEEP, OPT_GRAPH, OPT_STEP_GENERIC = 14, 13, 16


def _new(pb, N, generic, graph=0):
    csmc = pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    csmc.engine.set_option(OPT_SMALL_SWEEP, 0)   # the general path at every size (N = 1024 would run the one-launch sweep)
    csmc.engine.set_option(OPT_STEP_GENERIC, generic)
    csmc.engine.set_option(OPT_GRAPH, graph)
    return csmc


def _run(csmc, T, seed, ref, A, S, instance):
    traj = csmc(seed, ref, A, S).cpu().numpy()
    info = csmc.engine.launch_info()
    assert info["chunk"] == 1 and info["groups"] == "k_groups" and info["propagate_instance"] == instance, info
    X, ANC, LW, _ = csmc.engine.traces()
    return X.cpu().numpy(), ANC[: T - 1].cpu().numpy(), LW.cpu().numpy(), csmc.engine.last_final_index(), traj


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x.reshape(y.shape), y), what


@pytest.mark.parametrize("T", [2, 3, 12])
@pytest.mark.parametrize("N", [1024, 2048, 3 * 1024, 5 * 1024, 64 * 1024, 65 * 1024])
def test_full_against_generic_and_oracle(N, T):
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    got = {g: _run(_new(pb, N, g), T, SEED, pb.X_true, A, S, "generic" if g else "full") for g in (0, 1)}
    _same(got[0], got[1], f"N={N} T={T}: the whole-segment against the general instance")
    for g in (0, 1):
        _against_oracle(got[g], _oracle(N, T), f"N={N} T={T}: option 16 = {g} against the oracle")


@pytest.mark.parametrize("N", [1024, 2048])   # the last workgroup is the only one / one of two
def test_conditioned_particle(N):
    T = 12
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    ref = pb.X_true + 0.125 * np.arange(1, T + 1)[:, None]   # not the trajectory the parameters were fitted to
    cm = canon_model(pb, N)
    LS, LSinv, cS = cm.chol_parts(S)
    trajo, Xo, ANCo, lwo = cm.sweep(SEED, ref, A, LS, LSinv, cS, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov))
    for g in (0, 1):
        got = _run(_new(pb, N, g), T, SEED, ref, A, S, "generic" if g else "full")
        for t in range(T):
            assert np.array_equal(got[0][t, N - 1], ref[t]), f"option 16 = {g}: x[{t}, N - 1] is not ref[{t}]"
        _against_oracle(got, (Xo, ANCo, lwo, cm.final_index(SEED, lwo), trajo), f"N={N}: option 16 = {g} against the oracle")


# ------------------------------------------------------------------------------------------ non-finite states
def _overflow_params(kind, A, S):
    sign = np.where(A >= 0, 1.0, -1.0)
    if kind == "overflow":
        return sign * 1.7e308, S
    A2 = sign * 1e307
    A2[0, 3] = np.inf
    return A2, S * 1e19


@functools.lru_cache(maxsize=None)
def _overflow_oracle(kind, N, T):
    pb = experiments.smo_pgas(T=T)
    A, S = _overflow_params(kind, *experiments.initial_params(pb))
    cm = canon_model(pb, N)
    LS, LSinv, cS = cm.chol_parts(S)
    trajo, Xo, ANCo, lwo = cm.sweep(SEED, pb.X_true, A, LS, LSinv, cS, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov))
    return Xo, ANCo, lwo, cm.final_index(SEED, lwo), trajo


@pytest.mark.parametrize("kind", ["overflow", "nan"])
def test_non_finite_states(kind):
    N, T = 2048, 12
    pb = experiments.smo_pgas(T=T)
    A, S = _overflow_params(kind, *experiments.initial_params(pb))
    ora = _overflow_oracle(kind, N, T)
    Xo = ora[0]
    big = [int((np.abs(Xo[t]) >= 2.0 ** 30).sum()) for t in range(T)]
    inf = [int(np.isinf(Xo[t]).sum()) for t in range(T)]
    nan = [int(np.isnan(Xo[t]).sum()) for t in range(T)]
    print(f"{kind}: per step, entries beyond 2^30 {big}, infinite {inf}, NaN {nan}")
    assert big[1] > inf[1] > 0, "step 1: finite states beyond 2^30 and infinite ones"
    if kind == "overflow":
        assert all(inf[t] > 0 for t in range(1, T, 2)) and all(big[t] == 0 for t in range(2, T, 2))
    else:
        assert nan[2] > 0 and big[2] > 0 and all(nan[t] == 2 * (N - 1) for t in range(3, T))
    got = {g: _run(_new(pb, N, g), T, SEED, pb.X_true, A, S, "generic" if g else "full") for g in (0, 1)}
    _same_bits(got[0], got[1], f"{kind}: the whole-segment against the general instance, by bit pattern")
    for g in (0, 1):
        _same(got[g], ora, f"{kind}: option 16 = {g} against the oracle")


# ------------------------------------------------------------------------------------------ where it must not apply
def test_ragged_size_takes_the_general_instance():
    N, T = 1025, 6
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    got = _run(_new(pb, N, 0), T, SEED, pb.X_true, A, S, "generic")
    _against_oracle(got, _oracle(N, T), f"N={N}: the general instance against the oracle")


def test_two_observations_take_the_general_instance():
    """Vehicle: ny = 2 (and a 3-D basis): whole segments, so k_step runs its whole-segment instance, k_propagate its general one."""
    N, T = 2048, 6
    pb = experiments.vehicle_pgas(T=T, M=27)
    assert np.asarray(pb.observations).reshape(T, -1).shape[1] == 2
    A, S = experiments.initial_params(pb)
    cm = canon_model(pb, N)
    LS, LSinv, cS = cm.chol_parts(S)
    trajo, Xo, ANCo, lwo = cm.sweep(SEED, pb.X_true, A, LS, LSinv, cS, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov))
    csmc = _new(pb, N, 0)
    got = _run(csmc, T, SEED, pb.X_true, A, S, "generic")
    assert csmc.engine.launch_info()["step_instance"] == "full"
    _against_oracle(got, (Xo, ANCo, lwo, cm.final_index(SEED, lwo), trajo), "Vehicle: the general instance against the oracle")


def test_emulated_shards_take_the_general_instance():
    from pgas_amd import sharded

    world, N, T = 2, 4096, 6
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    Xo, ANCo, lwo, _, trajo = _oracle(N, T)
    grp = sharded.make_local_group(world, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    trajs = sharded.sharded_sweep(grp, SEED, pb.X_true, A, S, propagate_chunk=1)
    Nl = N // world
    for r, (s, tr) in enumerate(zip(grp.shards, trajs)):
        info = s.eng.launch_info()
        assert info["propagate_instance"] == "generic" and info["step_instance"] == "generic", (r, info)
        assert np.array_equal(tr.cpu().numpy().reshape(np.shape(trajo)), trajo), f"trajectory on rank {r}"
        X, ANC, LW, _ = s.eng.traces()
        assert np.array_equal(X.cpu().numpy(), Xo[:, r * Nl:(r + 1) * Nl]), f"state trace of shard {r}"
        assert np.array_equal(ANC[: T - 1].cpu().numpy(), ANCo[:, r * Nl:(r + 1) * Nl]), f"ancestor trace of shard {r}"
        assert np.array_equal(LW.cpu().numpy(), lwo[r * Nl:(r + 1) * Nl]), f"log-weights of shard {r}"


def test_option_forces_the_general_instance():
    N, T = 2048, 3
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    csmc = _new(pb, N, 1)
    _run(csmc, T, SEED, pb.X_true, A, S, "generic")
    csmc.engine.set_option(OPT_STEP_GENERIC, 0)   # and back, on the same context
    got = _run(csmc, T, SEED, pb.X_true, A, S, "full")
    _against_oracle(got, _oracle(N, T), "option 16 back to 0 on the same context")


# ------------------------------------------------------------------------------------------ graph replay
def test_full_under_graph_replay():
    """Replays with changed seed and parameters equal the enqueued sweeps of the same instance; option 16 re-captures."""
    N, T = 2048, 6
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    replayed, enqueued = _new(pb, N, 0, graph=1), _new(pb, N, 0)
    cases = [(SEED, A, S), (SEED + 1, A * 0.97, S * 1.3), (SEED + 2, A * 1.01, S)]   # the first sweep captures, all three replay
    for i, (seed, a, s) in enumerate(cases):
        got = _run(replayed, T, seed, pb.X_true, a, s, "full")
        assert replayed.engine.launch_info()["graph"]
        _same(got, _run(enqueued, T, seed, pb.X_true, a, s, "full"), f"replay {i} against the enqueued sweep")
        if i == 0:
            _against_oracle(got, _oracle(N, T), "the first replay against the oracle")
    replayed.engine.set_option(OPT_STEP_GENERIC, 1)   # another instance: another graph
    seed, a, s = cases[1]
    got = _run(replayed, T, seed, pb.X_true, a, s, "generic")
    assert replayed.engine.launch_info()["graph"]
    _same(got, _run(enqueued, T, seed, pb.X_true, a, s, "full"), "the re-captured general instance against the enqueued sweep")
