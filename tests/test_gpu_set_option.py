"""The sweep engine's host layer as its callers see it (csrc/pgas_api.hip: pgas_set_option, pgas_sweep, pgas_step, pgas_get_launch_info),
on the SingleMassOscillator problem at N = 2048, T = 4.

Refusals: every option with a range refuses lo - 1 and hi + 1 with its code and its exact text and takes lo and hi; an unknown option,
PGAS_OPT_TRACE_BLOCK_BYTES once the traces exist and the corrected mode on a shard are refused with theirs.

Modes: which k_step instance a sweep runs follows the rules of include/pgas_hip.h from options 7, 9, 2 and 16 alone -- LOCAL where option 7
asks for it and option 2 does not forbid it, else the scanner waves of option 9, else k_groups launches; the whole-segment instance (FULL)
only on the k_groups path and without option 16 -- and all sixteen combinations, enqueued or replayed from the captured graph, give the
same sweep bit for bit.  So do the one-launch sweeps of N = 300 against the general path, and in the corrected mode pgas_step driven
T - 1 times against pgas_sweep."""
import itertools

import pytest
import torch

from common import experiments, pgas_amd
from pgas_amd._lib import PgasError

pytestmark = pytest.mark.gpu

SEED = 12345678
N, T = 2048, 4
E_ARG, E_STATE = -1, -3
OPT_CHUNK, OPT_FORCE_SLOW, OPT_LDS, OPT_CORRECTED, OPT_LOCAL, OPT_EVENT_STRIDE, OPT_TAIL, OPT_SYRK, OPT_MAX_LEAD = 1, 2, 4, 5, 7, 8, 9, 10, 11
OPT_BLOCK_BYTES, OPT_GRAPH, OPT_SMALL, OPT_MFMA, OPT_GENERIC = 12, 13, 14, 15, 16
INT_MAX = 2**31 - 1

# option, lo, hi (None: one-sided), text of the refusal
RANGES = [
    (OPT_CHUNK, 0, None, "pgas_set_option: chunk must be >= 0"),
    (OPT_MAX_LEAD, 0, None, "pgas_set_option: max lead must be >= 0"),
    (OPT_SYRK, 0, 32, "pgas_set_option: SYRK splits must be 0 (automatic) .. 32"),
    (OPT_EVENT_STRIDE, 1, None, "pgas_set_option: event stride must be >= 1"),
    (OPT_LDS, 0, 160 * 1024, "pgas_set_option: LDS bytes out of range"),
    (OPT_MFMA, 0, 1, "pgas_set_option: PGAS_OPT_MFMA_PROPAGATE takes 0 or 1"),
    (OPT_SMALL, 0, 2, "pgas_set_option: PGAS_OPT_SMALL_SWEEP takes 0, 1 or 2"),
    (OPT_BLOCK_BYTES, 0, None, "pgas_set_option: block bytes must be >= 0"),
]


@pytest.fixture(scope="module")
def problem():
    pb = experiments.smo_pgas(T=T)
    return (pb,) + tuple(experiments.initial_params(pb))


def _new(pb, n=N, **kw):
    return pgas_amd.condSequentialMonteCarlo(n, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn, **kw)


def _refused(call, what, code, text):
    with pytest.raises(PgasError) as e:
        call()
    assert str(e.value) == f"{what} failed ({code}): {text}"


def _sweep(csmc, pb, A, S):
    """One sweep: (trajectory, state trace, ancestor trace, final log-weights) as copies, and what it launched."""
    traj = csmc(SEED, pb.X_true, A, S).clone()
    X, ANC, LW, _ = csmc.engine.traces()
    out = (traj, X.clone(), ANC[: T - 1].clone(), LW.clone())
    torch.cuda.synchronize()
    return out, csmc.engine.launch_info()


def _same(a, b, what):
    for x, y, name in zip(a, b, ("trajectory", "state_trace", "ancestor_trace", "log_weights_trace[-1]")):
        assert torch.equal(x, y), f"{what}: {name} differs"


# ------------------------------------------------------------------------------------------ refusals
def test_ranges(problem):
    pb, A, S = problem
    eng = _new(pb).engine
    for opt, lo, hi, text in RANGES:
        _refused(lambda: eng.set_option(opt, lo - 1), "pgas_set_option", E_ARG, text)
        eng.set_option(opt, lo)
        if hi is None:
            _refused(lambda: eng.set_option(opt, -INT_MAX), "pgas_set_option", E_ARG, text)
            eng.set_option(opt, INT_MAX)
        else:
            _refused(lambda: eng.set_option(opt, hi + 1), "pgas_set_option", E_ARG, text)
            eng.set_option(opt, hi)
    _refused(lambda: eng.set_option(99, 0), "pgas_set_option", E_ARG, "pgas_set_option: unknown option 99")
    _refused(lambda: eng.set_option(0, 1), "pgas_set_option", E_ARG, "pgas_set_option: unknown option 0")


def test_block_bytes_after_a_sweep(problem):
    pb, A, S = problem
    csmc = _new(pb)
    csmc.engine.set_option(OPT_BLOCK_BYTES, 0)
    _sweep(csmc, pb, A, S)
    for v in (0, 1 << 20):
        _refused(lambda: csmc.engine.set_option(OPT_BLOCK_BYTES, v), "pgas_set_option", E_STATE, "pgas_set_option: the traces are already allocated")
    _refused(lambda: csmc.engine.set_option(OPT_BLOCK_BYTES, -1), "pgas_set_option", E_ARG, "pgas_set_option: block bytes must be >= 0")


def test_corrected_mode_on_a_shard(problem):
    pb, A, S = problem
    eng = _new(pb).engine
    eng.shard_setup(0, 1)
    _refused(lambda: eng.set_option(OPT_CORRECTED, 1), "pgas_set_option", E_STATE, "pgas_set_option: the corrected mode is not available on a sharded context")
    eng.set_option(OPT_CORRECTED, 0)   # switching it off is no request for it
    eng = _new(pb, resample_before_propagate=True).engine
    _refused(lambda: eng.shard_setup(0, 1), "pgas_shard_setup", E_STATE, "pgas_shard_setup: the corrected mode is not available on a sharded context")


# ------------------------------------------------------------------------------------------ modes
def _expected(local, tail, slow, generic):
    groups = "local" if local and not slow else ("tail" if tail else "k_groups")   # N = 2048: one device, two segments
    return groups, "full" if groups == "k_groups" and not generic else "generic"   # N % 1024 == 0


def test_sixteen_modes_one_sweep(problem):
    pb, A, S = problem
    csmc = _new(pb)
    eng = csmc.engine
    first = None
    for local, tail, slow, generic in itertools.product((0, 1), repeat=4):
        for opt, v in ((OPT_LOCAL, local), (OPT_TAIL, tail), (OPT_FORCE_SLOW, slow), (OPT_GENERIC, generic)):
            eng.set_option(opt, v)
        groups, instance = _expected(local, tail, slow, generic)
        for graph in (1, 1, 0):   # the second sweep replays the graph the first one captured
            eng.set_option(OPT_GRAPH, graph)
            got, info = _sweep(csmc, pb, A, S)
            what = f"options 7, 9, 2, 16 = {local}, {tail}, {slow}, {generic}, graph {graph}"
            assert (info["groups"], info["step_instance"], info["graph"], info["small"]) == (groups, instance, bool(graph), False), (what, info)
            assert not eng.scan_gave_up(), what
            first = first or got
            _same(got, first, what)


def test_small_sweeps(problem):
    pb, A, S = problem
    got = {}
    for small in (0, 1, 2):
        csmc = _new(pb, 300)
        csmc.engine.set_option(OPT_SMALL, small)
        got[small], info = _sweep(csmc, pb, A, S)
        assert info["small"] == (small != 0) and info["groups"] == ("small" if small else "k_groups") and not info["graph"], (small, info)
    for small in (1, 2):
        _same(got[small], got[0], f"PGAS_OPT_SMALL_SWEEP = {small} against 0")


def test_corrected_steps_against_the_sweep(problem):
    pb, A, S = problem
    csmc = _new(pb, resample_before_propagate=True)
    (traj, X, ANC, LW), info = _sweep(csmc, pb, A, S)
    assert not info["small"] and not info["graph"]
    x, lw = csmc.engine.init_state(SEED, pb.X_true[0]), None
    assert torch.equal(x, X[0])
    for t in range(1, T):
        lw, x, anc = csmc.step(SEED, t, lw, x, A, S, pb.X_true[t])
        assert torch.equal(x, X[t]) and torch.equal(anc, ANC[t - 1]), f"corrected step {t} against the sweep"
    assert torch.equal(lw, LW)
    assert (ANC.cpu() != torch.arange(N, dtype=torch.int32)).any()
