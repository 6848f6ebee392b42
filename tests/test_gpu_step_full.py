"""k_step's whole-segment instance (k_step<PG_WM_GROUPS, false, FULL>, csrc/pgas_resample.hip.h): the instance launch_step chooses on one
unsharded device when N is a multiple of 1024, written without the guards for ragged segments and for ranks.  It is bit-identical to
the general instance by construction; here that is CHECKED, bit for bit: PGAS_OPT_STEP_GENERIC (option 16) = 0 against 1 on the same
arguments and seed, and both against the canonical C oracle -- trajectory, ancestor trace, state trace, final log-weights, final index.
Which instance ran is read from launch_info()["step_instance"].

Sizes: one segment, two, an odd number, exactly one group of 64 segments, one segment past a group boundary; 3 * 1024, 5 * 1024 and
65 * 1024 are not powers of two, so the division form of the slot thresholds runs under FULL as well as the multiplication form.
Lengths: T = 2 (the first launch only scans, the last neither searches with group records of its own nor scans), T = 3 (the middle
launch is the only one that searches and scans), T = 12.

Degenerate weights.  k_step takes its weights from the model (la_t + logw_{t-1}); a given log-weight vector cannot be handed to it, so
the named vectors of tests/resample_cases.py do not reach the sweep path as they are (they reach the same search code through
k_systematic, tests/test_gpu_resample_edges.py::test_direct_resampling).  What reaches k_step are whole sweeps whose MODEL makes the
weights degenerate -- the constructions of tests/test_gpu_resample_edges.py (_sweep_problem) -- and the branch census of
tests/resample_cases.py, computed from the oracle's own log-weights of every step, says which paths they entered:
    N = 4 * 1024, R = 1e-6 with outlier observations    scales flushed to zero at the group level (asserted from the segment records)
    N = 4 * 1024, NaN observations                       no positive weight (`!valid`): identity ancestors
    N = 128 * 1024, R = 1e-6                             ns > PG_NCAND: the per-slot bisection (four segments cannot hold nine sources)
    N = 2^21, T = 2, R = 1e-6, seed 1                    `!covered`: one workgroup's thresholds span more than the 1024 segments of a window
                                                         (and other workgroups take the 4 < ngw <= 16 window fill)
The uncovered window exists only above 2^20 particles (the window holds 1024 segments), so that case runs at the smallest power of two
above it; its cost is the serial oracle's one step at that size (about nine seconds on one host core, the GPU part is milliseconds).
Seeds 1..8 at 1280 * 1024 and 1536 * 1024 particles do not reach it (two weight carriers more than 2^20 indices apart are needed), seed
1 at 2^21 does: the seed was chosen on the CPU from the oracle's census, which the test asserts before it compares anything."""
import functools

import numpy as np
import pytest

from common import canon, canon_model, experiments, pgas_amd
import resample_cases as rc
from test_gpu_resample_edges import _sweep_problem

pytestmark = pytest.mark.gpu

SEED = 12345678
OPT_SMALL_SWEEP, OPT_GRAPH, OPT_STEP_GENERIC = 14, 13, 16
NAMES = ("state_trace", "ancestor_trace", "log_weights_trace[-1]", "final index", "trajectory")


def _same(a, b, what):
    for x, y, name in zip(a, b, NAMES):
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x.reshape(y.shape), y, equal_nan=y.dtype.kind == "f"), f"{what}: {name} differs in {int((x.reshape(y.shape) != y).sum())} of {y.size} entries"


def _new(pb, N, generic, graph=0):
    csmc = pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    csmc.engine.set_option(OPT_SMALL_SWEEP, 0)   # the general path at every size (N = 1024 would run the one-launch sweep)
    csmc.engine.set_option(OPT_STEP_GENERIC, generic)
    csmc.engine.set_option(OPT_GRAPH, graph)
    return csmc


def _run(csmc, T, seed, ref, A, S, instance):
    traj = csmc(seed, ref, A, S).cpu().numpy()
    info = csmc.engine.launch_info()
    assert info["groups"] == "k_groups" and info["step_instance"] == instance, info
    X, ANC, LW, _ = csmc.engine.traces()
    return X.cpu().numpy(), ANC[: T - 1].cpu().numpy(), LW.cpu().numpy(), csmc.engine.last_final_index(), traj


@functools.lru_cache(maxsize=None)
def _oracle(N, T):
    """The oracle's sweep of the plain SingleMassOscillator problem, computed once per shape: (X, ANC, logw_last, final index, trajectory)."""
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    cm = canon_model(pb, N)
    LS, LSinv, cS = cm.chol_parts(S)
    trajo, Xo, ANCo, lwo = cm.sweep(SEED, pb.X_true, A, LS, LSinv, cS, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov))
    return Xo, ANCo, lwo, cm.final_index(SEED, lwo), trajo


def _against_oracle(got, ora, what):
    X, ANC, LW, b, traj = got
    trajo = ora[4]
    _same(got, ora, what)
    for t in range(X.shape[0] - 1, -1, -1):   # the trajectory is the path from the final index through the trace
        assert np.array_equal(X[t, b], np.asarray(trajo[t]).reshape(-1)), f"{what}: trajectory row {t}"
        if t:
            b = ANC[t - 1, b]


SIZES = (1024, 2048, 3 * 1024, 64 * 1024, 65 * 1024)


@pytest.mark.parametrize("T", [2, 3, 12])
@pytest.mark.parametrize("N", SIZES + (5 * 1024,))
def test_full_against_generic_and_oracle(N, T):
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    got = {g: _run(_new(pb, N, g), T, SEED, pb.X_true, A, S, "generic" if g else "full") for g in (0, 1)}
    _same(got[0], got[1], f"N={N} T={T}: FULL against the general instance")
    for g in (0, 1):
        _against_oracle(got[g], _oracle(N, T), f"N={N} T={T}: option 16 = {g} against the oracle")


# ------------------------------------------------------------------------------------------ degenerate weights
@functools.lru_cache(maxsize=None)
def _oracle_steps(N, T, degenerate, nan_row):
    """The oracle's sweep of _sweep_problem step by step: (X, ANC, logw_last, trajectory) and, per step, the branch set of the census
    of the log-weights that step resamples and whether a segment's scale is flushed to zero inside its group."""
    pb, ref = _sweep_problem(T, degenerate, nan_row)
    A, S = experiments.initial_params(pb)
    cm = canon_model(pb, N)
    LS, LSinv, cS = cm.chol_parts(S)
    X = np.empty((T, N, pb.nx))
    ANC = np.empty((T - 1, N), np.int32)
    X[0] = cm.init_state(SEED, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), ref[0])
    lw, seen, flushed = None, [], []
    for t in range(1, T):
        lw, X[t], ANC[t - 1], dbg = cm.step(t, SEED, X[t - 1], lw, A, LS, LSinv, cS, ref[t], debug=True)
        seen.append(rc.branches(rc.census(dbg["lw1"], dbg["u"][0])))
        segk, segs, _ = canon.segment_partials(np.ascontiguousarray(dbg["lw1"], dtype=np.float64))
        fl = False
        for g0 in range(0, len(segk), rc.GRP):
            k = segk[g0:g0 + rc.GRP]
            live = k[np.isfinite(k) & (segs[g0:g0 + rc.GRP] > 0)]
            fl = fl or (live.size > 0 and float(live.max() - live.min()) > rc.FLUSH)
        flushed.append(fl)
    b_final = b = cm.final_index(SEED, lw)
    traj = np.empty((T, pb.nx))
    for t in range(T - 1, -1, -1):
        traj[t] = X[t, b]
        if t:
            b = ANC[t - 1, b]
    return (X, ANC, lw, b_final, traj), seen, flushed


@pytest.mark.parametrize("N,degenerate,nan_row,path", [(4 * 1024, True, None, "flushed"), (4 * 1024, False, 4, "!valid"), (128 * 1024, True, None, "ns>8")],
                         ids=["flushed_scales", "no_positive_weight", "per_slot_bisection"])
def test_full_degenerate_sweeps(N, degenerate, nan_row, path):
    T = 8
    pb, ref = _sweep_problem(T, degenerate, nan_row)
    A, S = experiments.initial_params(pb)
    ora, seen, flushed = _oracle_steps(N, T, degenerate, nan_row)
    print(f"census N={N}: {[sorted(s) for s in seen]}, flushed scale per step {flushed}")
    if path == "flushed":
        assert any(flushed), "no step with a segment scale flushed to zero"
    else:
        assert any(path in s for s in seen), (path, seen)
    got = {g: _run(_new(pb, N, g), T, SEED, ref, A, S, "generic" if g else "full") for g in (0, 1)}
    _same(got[0], got[1], f"{path}: FULL against the general instance")
    for g in (0, 1):
        _against_oracle(got[g], ora, f"{path}: option 16 = {g} against the oracle")
    if path == "!valid":
        assert np.array_equal(ora[1][nan_row - 1], np.arange(N)) and got[0][3] == N - 1


N_UNCOVERED, SEED_UNCOVERED = 1 << 21, 1


def test_full_uncovered_window():
    """`!covered` under FULL: step 1 of the degenerate three-step problem (its parameters, its first two rows: a sweep of T = 2, whose
    last launch searches step 1 and scans nothing).  A few particles carry the step, two of them more than 1024 segments apart."""
    N, seed = N_UNCOVERED, SEED_UNCOVERED
    pb, ref = _sweep_problem(3, True, None)
    A, S = experiments.initial_params(pb)   # of the three-step problem: the parameters depend on the data
    pb.observations, pb.inputs, pb.X_true, ref = pb.observations[:2].copy(), pb.inputs[:2].copy(), pb.X_true[:2].copy(), ref[:2].copy()
    T = pb.T
    assert T == 2
    cm = canon_model(pb, N)
    LS, LSinv, cS = cm.chol_parts(S)
    X = np.empty((T, N, pb.nx))
    X[0] = cm.init_state(seed, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), ref[0])
    lw, X[1], anc, dbg = cm.step(1, seed, X[0], None, A, LS, LSinv, cS, ref[1], debug=True)
    cen = rc.census(dbg["lw1"], dbg["u"][0])
    seen = rc.branches(cen)
    print(f"census N={N} seed={seed}: {sorted(seen)}, {int((~cen['covered']).sum())} uncovered workgroup(s), {len(np.unique(anc))} distinct ancestors")
    assert "!covered" in seen and "4<ngw<=16" in seen, seen
    b = cm.final_index(seed, lw)
    ora = (X, anc[None, :], lw, b, np.stack([X[0, anc[b]], X[1, b]]))
    got = {g: _run(_new(pb, N, g), T, seed, ref, A, S, "generic" if g else "full") for g in (0, 1)}
    _same(got[0], got[1], "!covered: FULL against the general instance")
    for g in (0, 1):
        _against_oracle(got[g], ora, f"!covered: option 16 = {g} against the oracle")


# ------------------------------------------------------------------------------------------ instance selection
@pytest.mark.parametrize("N", [1025, 65 * 1024 + 300])
def test_ragged_sizes_take_the_general_instance(N):
    T = 6
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    got = _run(_new(pb, N, 0), T, SEED, pb.X_true, A, S, "generic")
    _against_oracle(got, _oracle(N, T), f"N={N}: the general instance against the oracle")


def test_option_forces_the_general_instance():
    N, T = 2048, 3
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    csmc = _new(pb, N, 1)
    _run(csmc, T, SEED, pb.X_true, A, S, "generic")
    csmc.engine.set_option(OPT_STEP_GENERIC, 0)   # and back, on the same context
    got = _run(csmc, T, SEED, pb.X_true, A, S, "full")
    _against_oracle(got, _oracle(N, T), "option 16 back to 0 on the same context")


def test_full_under_graph_replay():
    N, T = 2048, 6
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    csmc = _new(pb, N, 0, graph=1)
    for rep in range(2):   # the first sweep captures, both replay
        got = _run(csmc, T, SEED, pb.X_true, A, S, "full")
        assert csmc.engine.launch_info()["graph"]
        _against_oracle(got, _oracle(N, T), f"graph replay {rep}")
