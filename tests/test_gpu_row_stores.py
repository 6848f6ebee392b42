"""The sweep's write-once rows (x_t, the la / h / ln hand-off rows, the ancestor trace, x_0) go through one store helper with a
per-site cache policy (csrc/pgas_kernels.hip.h: st_row / st_row16).  Whatever the policy and the width of a lane's store, the bytes
and their places are the same: every case checks the state trace, the ancestor trace, the final log-weights and the trajectory
bit for bit against the canonical oracle, at the shapes where a guard, a lane-pair packing or a 16-byte store can go wrong."""
import numpy as np
import pytest

from common import canon_model, experiments, pgas_amd

pytestmark = pytest.mark.gpu

SEED = 12345678


def _problem(name):
    return {"smo": lambda: experiments.smo_pgas(T=40), "toy": lambda: experiments.toy(T=40), "emps": lambda: experiments.emps_pgas(T=10),
            "veh": lambda: experiments.vehicle_pgas(T=12)}[name]()


_oracle_cache = {}


def _oracle(name, N):
    """(problem, A, S, oracle sweep) -- computed once per (problem, N) and shared."""
    if (name, N) not in _oracle_cache:
        pb = _problem(name)
        A, S = experiments.initial_params(pb)
        cm = canon_model(pb, N)
        LS, LSinv, cS = cm.chol_parts(S)
        ref = cm.sweep(SEED, pb.X_true, A, LS, LSinv, cS, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov))
        ref = tuple(np.asarray(r) for r in ref)
        for r in ref:
            r.setflags(write=False)
        _oracle_cache[(name, N)] = (pb, A, S, ref)
    return _oracle_cache[(name, N)]


def _eq(gpu, ref, what):
    g = gpu.cpu().numpy().reshape(np.shape(ref))
    assert np.array_equal(g, ref), f"{what}: {int((g != ref).sum())} of {g.size} entries differ, max |d| = {np.abs(g - ref).max():.3e}"


@pytest.mark.parametrize("name,N,opts", [
    ("smo", 1025, {}),             # a full segment and a one-particle last one: guarded stores, the conditioned particle alone in its workgroup, the ancestor row's ragged tail
    ("smo", 2051, {}),             # N no multiple of 4 or 2: the lane pairs at a segment's end, ancestor rows that do not start 16-byte aligned
    ("smo", 4096, {1: 7}),         # PGAS_OPT_PROPAGATE_CHUNK = 7: the chunked k_propagate
    ("smo", 5000, {3: 0}),         # PGAS_OPT_OVERLAP = 0: both pipelines on one stream
    ("smo", 5000, {12: 1 << 18}),  # PGAS_OPT_TRACE_BLOCK_BYTES: traces in row blocks
    ("toy", 1500, {}),             # n_x = 1: 8-byte state stores
    ("emps", 1025, {}),            # 3-D basis, coefficient tensor in LDS
    ("veh", 2048, {15: 1}),        # PGAS_OPT_MFMA_PROPAGATE: k_propagate_mx, one particle per pass
])
def test_row_stores_sweep_bit_exact(name, N, opts):
    pb, A, S, (trajo, Xo, ANCo, lwo) = _oracle(name, N)
    csmc = pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    eng = csmc.engine
    for k, v in opts.items():
        eng.set_option(k, v)
    traj = csmc(SEED, pb.X_true, A, S)
    X, ANC, LW, _ = eng.traces()
    _eq(X, Xo, "state_trace")
    _eq(ANC[: pb.T - 1], ANCo, "ancestor_trace")
    _eq(LW, lwo, "log_weights_trace[-1]")
    _eq(traj, trajo.reshape(traj.shape), "trajectory")
    info = eng.launch_info()
    assert not info["small"], "the multi-launch sweep (k_propagate / k_step) is what this test is about"
    assert info["mfma"] == (opts.get(15, 0) == 1), "which k_propagate ran"
    if 12 in opts:
        # the 16-byte stores address a row as (16-byte aligned base) + (multiple of 16): every row of every trace they may be used
        # on has to start on a 16-byte boundary, in every block (N = 5000: also each ancestor row, 20000 bytes)
        kinds = {"x": eng.TRACE_X, "la": eng.TRACE_LA, "h": eng.TRACE_H, "ln": eng.TRACE_LN, "anc": eng.TRACE_ANC}
        for what, kind in kinds.items():
            rows, rpb, nblk, row_bytes = eng.trace_layout(kind)
            assert nblk > 1, f"{what}: the trace should span several blocks in this case"
            assert row_bytes % 16 == 0, what
            for b in range(nblk):
                assert eng.trace_row(kind, b * rpb) % 16 == 0, f"{what}: block {b} does not start 16-byte aligned"
            for t in range(rows):
                assert eng.trace_row(kind, t) % 16 == 0, f"{what}: row {t} does not start 16-byte aligned"


def test_row_stores_sharded_sweep_bit_exact():
    """Two shards emulated on one device: each rank's k_step reads its peers' la / h rows, which k_propagate of the peer wrote."""
    from pgas_amd import sharded

    name, N, world = "smo", 4096, 2
    pb, A, S, (trajo, Xo, ANCo, lwo) = _oracle(name, N)
    grp = sharded.make_local_group(world, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn,
                                   trace_block_bytes=None)
    trajs = sharded.sharded_sweep(grp, SEED, pb.X_true, A, S, propagate_chunk=5)
    Nl = N // world
    for r, (s, tr) in enumerate(zip(grp.shards, trajs)):
        _eq(tr, trajo.reshape(tr.shape), f"trajectory on rank {r}")
        X, ANC, LW, _ = s.eng.traces()
        _eq(X, Xo[:, r * Nl:(r + 1) * Nl], f"state_trace shard {r}")
        _eq(ANC[: pb.T - 1], ANCo[:, r * Nl:(r + 1) * Nl], f"ancestor_trace shard {r}")
        _eq(LW, lwo[r * Nl:(r + 1) * Nl], f"log_weights shard {r}")
