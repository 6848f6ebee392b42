"""PGAS_OPT_TAIL_GROUPS (option 9): the group scans of a step run inside k_step, by scanner waves that poll for the tagged granules
the segment workgroups hand over (csrc/pgas_resample.hip.h: scanner_groups, csrc/pgas_kernels.hip.h: segment_scan<HANDOFF>), instead
of a k_groups launch between two steps.  Everything is compared BIT FOR BIT: option 9 = 1 against option 9 = 0 on the same
arguments and seed, and both against the canonical C oracle -- state trace, ancestor trace, final log-weights, trajectory, final index.
After every case the engine's hand-off failure state must be clean (no scanner ran out of its bounded wait).

Shapes: the smallest at which the hand-off can go wrong -- two segments of which the second holds one particle (one group), a second
group that is one one-particle segment, a ragged last segment in the second group -- and the sweep lengths at which a launch only
scans (T = 2: the first launch scans, the last neither scans nor has group records to wait for) or the middle launch is the only one
that both searches and scans (T = 3).  More than 64 groups (N > 4 * 2^20) is not tested here: the top level is computed in k_step's
head, which does not depend on who wrote the group records."""
import numpy as np
import pytest

from common import canon_model, experiments, pgas_amd
from test_gpu_resample_edges import _csmc, _oracle_sweep, _sweep_problem

pytestmark = pytest.mark.gpu

SEED = 12345678
N_TWO_SEG = 1025                 # two segments, the second holds one particle; one group
N_GROUP_OF_ONE = 64 * 1024 + 1   # a second group of one one-particle segment
N_RAGGED = 65 * 1024 + 300       # ragged last segment in the second group


def _outputs(csmc, T):
    X, ANC, LW, _ = csmc.engine.traces()
    return X.cpu().numpy(), ANC[: T - 1].cpu().numpy(), LW.cpu().numpy(), csmc.engine.last_final_index()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("state_trace", "ancestor_trace", "log_weights_trace[-1]", "final index", "trajectory")):
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x.reshape(y.shape), y, equal_nan=y.dtype.kind == "f"), f"{what}: {name} differs in {int((x.reshape(y.shape) != y).sum())} of {y.size} entries"


def _new(pb, N, tail, graph=0):
    csmc = pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    csmc.engine.set_option(14, 0)   # PGAS_OPT_SMALL_SWEEP off: the general path at every size
    csmc.engine.set_option(9, tail)
    csmc.engine.set_option(13, graph)
    return csmc


def _run(csmc, T, seed, ref, A, S, tail):
    traj = csmc(seed, ref, A, S).cpu().numpy()
    info = csmc.engine.launch_info()
    assert info["groups"] == ("tail" if tail else "k_groups"), info
    assert not csmc.engine.scan_gave_up(), "a scanner wave gave up waiting for its segment partials"
    return _outputs(csmc, T) + (traj,)


@pytest.mark.parametrize("N,T", [(N_TWO_SEG, 12), (N_GROUP_OF_ONE, 12), (N_RAGGED, 12), (N_TWO_SEG, 2), (N_RAGGED, 2), (N_TWO_SEG, 3), (N_RAGGED, 3)])
def test_scanner_groups_against_k_groups_and_oracle(N, T):
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    cm = canon_model(pb, N)
    LS, LSinv, cS = cm.chol_parts(S)
    trajo, Xo, ANCo, lwo = cm.sweep(SEED, pb.X_true, A, LS, LSinv, cS, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov))
    got = {tail: _run(_new(pb, N, tail), T, SEED, pb.X_true, A, S, tail) for tail in (1, 0)}
    _same(got[1], got[0], f"N={N} T={T}: option 9 = 1 against 0")
    for tail in (1, 0):
        X, ANC, LW, b, traj = got[tail]
        _same((X, ANC, LW, b, traj), (Xo, ANCo, lwo, b, trajo), f"N={N} T={T}: option 9 = {tail} against the oracle")
        for t in range(T - 1, -1, -1):   # the trajectory is the path from the final index through the trace
            assert np.array_equal(X[t, b], trajo[t].reshape(-1))
            if t:
                b = ANC[t - 1, b]


@pytest.mark.parametrize("degenerate,nan_row", [(True, None), (False, 4)], ids=["flushed_scales", "no_positive_weight"])
def test_scanner_groups_degenerate_partials(degenerate, nan_row):
    """The partials as ordinary payload at their extremes, on the whole-sweep constructions of tests/test_gpu_resample_edges.py
    (_sweep_problem): degenerate = R of 1e-6 with outlier observations, so one or a few particles carry a step and the scales
    2^(kref - KG) of nearly every segment flush to zero at the group level; nan_row = NaN observations at steps 4 and T - 1, so in
    those steps (and the one after the first) EVERY segment hands over kref = -inf and total = 0."""
    N, T = N_RAGGED, 8
    pb, ref = _sweep_problem(T, degenerate, nan_row)
    A, S = experiments.initial_params(pb)
    trajo, Xo, ANCo, lwo, _, _ = _oracle_sweep(N, T, degenerate, nan_row)
    got = {}
    for tail in (1, 0):
        csmc = _csmc(pb, N)
        csmc.engine.set_option(9, tail)
        got[tail] = _run(csmc, T, SEED, ref, A, S, tail)
    _same(got[1], got[0], "option 9 = 1 against 0")
    X, ANC, LW, b, traj = got[1]
    _same((X, ANC, LW, b, traj), (Xo, ANCo, lwo, b, trajo), "option 9 = 1 against the oracle")
    if nan_row is not None:
        assert np.array_equal(ANCo[nan_row - 1], np.arange(N)) and b == N - 1
    else:
        assert min(len(np.unique(r)) for r in ANCo) < N // 100, "the sweep really was degenerate"


@pytest.mark.parametrize("graph", [0, 1], ids=["enqueued", "graph_replay"])
def test_scanner_groups_tags_do_not_go_stale(graph):
    """Three sweeps in a row on one context with different seeds, then the first seed again: each equals the sweep of a fresh
    context.  The granules of earlier launches and sweeps stay in the hand-off buffer, so a tag that repeated (or, under
    PGAS_OPT_GRAPH, one frozen into the captured launches instead of read from device memory) would let a scanner take stale partials."""
    N, T = N_RAGGED, 6
    pb = experiments.smo_pgas(T=T)
    A, S = experiments.initial_params(pb)
    seeds = [SEED, SEED + 1, SEED + 2, SEED]
    one = _new(pb, N, 1, graph)
    got = []
    for s in seeds:
        got.append(_run(one, T, s, pb.X_true, A, S, 1))
        assert one.engine.launch_info()["graph"] == bool(graph)
    fresh = {s: _run(_new(pb, N, 1, graph), T, s, pb.X_true, A, S, 1) for s in set(seeds)}
    for i, s in enumerate(seeds):
        _same(got[i], fresh[s], f"sweep {i} (seed {s}) on the reused context against a fresh one")
    _same(got[0], got[3], "first seed again")
    assert not np.array_equal(got[0][1], got[1][1]), "different seeds give different ancestors"
