"""One model learned from several records (pgas_amd.records, csrc/pgas_records.hip.h): every (chain, record) sweep against the
single-record engine built on that record alone and against the canonical C oracle, the seam-aware statistics against the NumPy sum of
per-record statistics, and whole Gibbs chains against a restatement from the oracle pieces.  Records are slices of one generated
problem, so the same rows serve as y, u and reference.  Every equality is bit for bit unless a tolerance is stated."""
import dataclasses

import numpy as np
import pytest
import torch

from common import canon_model, experiments, host_param_draws, numpy_csmc, pgas_amd, pgas_numpy
from pgas_amd import chains as ch
from pgas_amd import random as prng
from pgas_amd import records as rc
from pgas_amd._lib import PgasError

pytestmark = pytest.mark.gpu

LENGTHS = (2, 3, 17, 2, 9)   # cut from a T = 33 problem
NAMES = ("trajectory", "state trace", "ancestor trace", "final log-weights", "final index")


def _problem(name, T):
    return {"smo": lambda: experiments.smo_pgas(T=T), "toy": lambda: experiments.toy(T=T),
            "emps27": lambda: experiments.emps_pgas(T=T, M=27), "veh27": lambda: experiments.vehicle_pgas(T=T, M=27)}[name]()


def _cut(pb, lengths, m0s=None, P0s=None):
    """The records of `lengths` rows cut from pb in order, each a Problem of its own (record e's initial state: m0s[e], P0s[e])."""
    row0 = np.concatenate([[0], np.cumsum(lengths)])
    assert row0[-1] == pb.T
    return [dataclasses.replace(pb, observations=pb.observations[a:b], inputs=pb.inputs[a:b], X_true=pb.X_true[a:b],
                                init_state_mean=pb.init_state_mean if m0s is None else m0s[e],
                                init_state_cov=pb.init_state_cov if P0s is None else P0s[e])
            for e, (a, b) in enumerate(zip(row0[:-1], row0[1:]))]


def _chain_inputs(pb, C, seed=5):
    """C different (step key, reference (Tsum, nx), A, S): perturbations of the problem's truth and its posterior-mean parameters."""
    A, S = experiments.initial_params(pb)
    rng = np.random.default_rng(seed)
    keys = [prng.key(1000 + 7919 * c) for c in range(C)]
    refs = np.stack([pb.X_true + 0.01 * c * rng.standard_normal(pb.X_true.shape) for c in range(C)])
    As = np.stack([A * (1.0 + 0.02 * c) for c in range(C)])
    Ss = np.stack([S * (1.0 + 0.1 * c) for c in range(C)])
    return keys, refs, As, Ss


def _records(recs, C, N, m0=None, P0=None):
    r = recs[0]
    return rc.condSequentialMonteCarloRecords(C, N, [q.observations for q in recs], [q.inputs for q in recs],
                                              r.init_state_mean if m0 is None else m0, r.init_state_cov if P0 is None else P0,
                                              r.likelihood_fcn, r.basis_fcn)


def _single(pb, N):
    return pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn,
                                             pb.basis_fcn)


def _run(rs, keys, refs, As, Ss):
    """One batched sweep -> host copies of (traj, x, anc, logw_last, final index)."""
    traj = rs(keys, refs, As, Ss).cpu().numpy()
    X, ANC, LW = (t.cpu().numpy() for t in rs.traces())
    return traj, X, ANC, LW, rs.final_index()


def _cell(rs, out, c, e):
    """(chain c, record e) of a batched result, in the shapes of a single-record sweep of T_e rows."""
    traj, X, ANC, LW, fidx = out
    return rs.record(e, traj[c]), rs.record(e, X[c], axis=0), rs.record(e, ANC[c], axis=0)[:-1], LW[c, e], fidx[c, e]


def _check_against_single(recs, N, rs, out, seeds, refs, As, Ss, cells=None, singles=None):
    """(chain c, record e) of a batched sweep equals condSequentialMonteCarlo built on record e alone with seeds[c][e], the record's
    reference rows and chain c's (A, S) (error_cov on the device: the same factorisation)."""
    C, E = len(seeds), len(recs)
    singles = {} if singles is None else singles
    for c, e in [(c, e) for c in range(C) for e in range(E)] if cells is None else cells:
        pb = recs[e]
        if e not in singles:
            singles[e] = _single(pb, N)
        csmc = singles[e]
        dev = csmc.device
        t1 = csmc(seeds[c][e], torch.as_tensor(rs.record(e, refs[c]), device=dev), torch.as_tensor(As[c], device=dev), torch.as_tensor(Ss[c], device=dev))
        X1, A1, L1, _ = csmc.engine.traces()
        want = (t1.cpu().numpy().reshape(pb.T, pb.nx), X1.cpu().numpy(), A1.cpu().numpy()[: pb.T - 1], L1.cpu().numpy(), csmc.engine.last_final_index())
        for a, b, what in zip(_cell(rs, out, c, e), want, NAMES):
            assert np.array_equal(a, b), f"chain {c}, record {e}: {what}"


def _check_against_oracle(recs, N, rs, out, seeds, refs, As, Ss, cells):
    for c, e in cells:
        pb = recs[e]
        cm = canon_model(pb, N)
        LS, LSinv, cS = cm.chol_parts_dev(Ss[c])
        trajo, Xo, ANCo, lwo = cm.sweep(seeds[c][e], rs.record(e, refs[c]), As[c], LS, LSinv, cS, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov))
        got = _cell(rs, out, c, e)
        for a, b, what in zip(got[:4], (trajo.reshape(pb.T, pb.nx), Xo.reshape(got[1].shape), ANCo, lwo), NAMES):
            assert np.array_equal(a, b), f"chain {c}, record {e}: {what} vs the canonical sweep"


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name,N", [(m, n) for m in ("smo", "toy", "emps27", "veh27") for n in (1, 200, 257, 1024)])
def test_sweep_equals_single_record_sweeps_and_oracle(name, N, C):
    pb = _problem(name, sum(LENGTHS))
    recs = _cut(pb, LENGTHS)
    E = len(recs)
    keys, refs, As, Ss = _chain_inputs(pb, C)
    seeds = rc.host_seeds(keys, E)
    rs = _records(recs, C, N)
    assert list(rs.row0) == [0, 2, 5, 22, 24, 33]
    out = _run(rs, keys, refs, As, Ss)           # the seeds derived on the device from the C step keys
    assert out[0].shape == (C, pb.T, pb.nx) and out[1].shape == (C, pb.T, N, pb.nx) and out[2].shape == (C, pb.T, N)
    assert out[3].shape == (C, E, N) and out[4].shape == (C, E)
    _check_against_single(recs, N, rs, out, seeds, refs, As, Ss)
    _check_against_oracle(recs, N, rs, out, seeds, refs, As, Ss, sorted({(0, 0), (C - 1, E - 1)}))


def test_per_record_initial_states():
    """Every record with a mean and a (full) covariance of its own: x_0 of record e is drawn from them."""
    pb = _problem("smo", sum(LENGTHS))
    E, C, N = len(LENGTHS), 3, 200
    rng = np.random.default_rng(11)
    m0s = 0.05 * rng.standard_normal((E, pb.nx))
    B = rng.standard_normal((E, pb.nx, pb.nx))
    P0s = 1e-4 * (B @ B.transpose(0, 2, 1) + np.eye(pb.nx))
    recs = _cut(pb, LENGTHS, m0s, P0s)
    keys, refs, As, Ss = _chain_inputs(pb, C)
    seeds = rc.host_seeds(keys, E)
    rs = _records(recs, C, N, m0s, P0s)
    out = _run(rs, keys, refs, As, Ss)
    _check_against_single(recs, N, rs, out, seeds, refs, As, Ss)
    _check_against_oracle(recs, N, rs, out, seeds, refs, As, Ss, [(0, 0), (C - 1, E - 1)])
    shared = _run(_records(_cut(pb, LENGTHS), C, N), keys, refs, As, Ss)
    assert not np.array_equal(shared[1][:, rs.row0[:-1]], out[1][:, rs.row0[:-1]]), "the per-record initial states were not used"


def test_record_order_does_not_matter_and_more_workgroups_than_are_resident():
    """E = 40 records of 8 rows x C = 50 chains at N = 64: 2000 workgroups.  The same records in another order, with their seeds,
    give the same results in that order; a sample of (chain, record) equals the single-record sweep."""
    E, Te, C, N = 40, 8, 50, 64
    pb = _problem("smo", E * Te)
    recs = _cut(pb, (Te,) * E)
    keys, refs, As, Ss = _chain_inputs(pb, C)
    seeds = np.array(rc.host_seeds(keys, E), dtype=np.uint64)
    perm = np.random.default_rng(4).permutation(E)
    rows = np.concatenate([np.arange(e * Te, (e + 1) * Te) for e in perm])
    rs = _records(recs, C, N)
    dev = rs.device
    fwd = _run(rs, torch.as_tensor(seeds.view(np.int64), device=dev), refs, As, Ss)
    rp = _records([recs[e] for e in perm], C, N)
    per = _run(rp, torch.as_tensor(np.ascontiguousarray(seeds[:, perm]).view(np.int64), device=dev), refs[:, rows], As, Ss)
    for out, r in ((fwd, rs), (per, rp)):
        out[2][:, r.row0[1:] - 1] = 0   # the last ancestor row of every record is unused (and not written)
    for a, b, what in zip(fwd[:3], per[:3], NAMES):
        assert np.array_equal(a[:, rows], b), what
    for a, b, what in zip(fwd[3:], per[3:], NAMES[3:]):
        assert np.array_equal(a[:, perm], b), what
    cells = [(0, 0), (C - 1, E - 1), (17, 23), (49, 0), (0, 39), (31, 5)]
    _check_against_single(recs, N, rs, fwd, seeds.tolist(), refs, As, Ss, cells=cells)
    assert not np.array_equal(fwd[0][0, :Te], fwd[0][0, Te:2 * Te])


def test_one_record_matches_the_chain_layer():
    pb = _problem("emps27", 24)
    C, N = 3, 300
    keys, refs, As, Ss = _chain_inputs(pb, C)
    rs = _records([pb], C, N)
    got = _run(rs, keys, refs, As, Ss)
    chs = ch.condSequentialMonteCarloChains(C, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    traj = chs(keys, refs, As, Ss).cpu().numpy()
    X, ANC, LW = (t.cpu().numpy() for t in chs.traces())
    fidx = chs.final_index()
    for a, b, what in zip(got, (traj, X, ANC, LW[:, None], fidx[:, None]), NAMES):
        a = a[:, : pb.T - 1] if what == "ancestor trace" else a
        assert np.array_equal(a, b), what


def test_device_seeds_follow_the_seed_rule():
    """pgas_records_seeds against pgas_amd.random.split for 1000 random step keys and E = 5; column 0 is the step keys themselves."""
    E = 5
    pb = _problem("smo", 2 * E)
    eng = _records(_cut(pb, (2,) * E), 1, 16).engine
    rng = np.random.default_rng(3)
    host = [int(v) for v in rng.integers(0, 2**64 - 1, size=1000, dtype=np.uint64, endpoint=True)]
    got = eng.records_seeds(ch.keys_tensor(host, eng.device)).cpu().numpy().view(np.uint64)
    assert got.shape == (1000, E)
    assert got[:, 0].tolist() == host
    for c, k in enumerate(host):
        assert got[c, 1:].tolist() == prng.split(k, E)[1:], f"key {c}"


# ---------------------------------------------------------------------------------------------- statistics
STAT_LENGTHS = (2, 3, 17, 16, 15)
# The criterion of tests/test_gpu_suffstats.py for the single record: a Tsum-term fp64 dot product carries a rounding error of at most
# ~Tsum eps times the sum of the absolute products, whatever the summation order: 1e-15 per row and unit of scale.
RTOL = 1e-15


def _phi(nm, traj, u):
    return np.vstack([nm.basis(traj[t : t + 1], u[t]) for t in range(traj.shape[0] - 1)])   # traj[:-1] with inputs[:-1]


def _stats_numpy(recs, rs, traj):
    """float64 NumPy sum over the records of each record's own (T0, T1, T2, T3), and the scales the error bound is relative to."""
    tot, sc = None, None
    for e, pb in enumerate(recs):
        nm = numpy_csmc(pb, 4)
        tr = rs.record(e, traj)
        u = np.asarray(pb.inputs, dtype=np.float64).reshape(pb.T, -1)
        Phi = _phi(nm, tr, u)
        s = pgas_numpy.suff_stats(tr, Phi)
        Pa, Xp = np.abs(Phi), np.abs(tr[1:])
        a = (Pa.T @ Xp, Pa.T @ Pa, Xp.T @ Xp)
        tot = list(s) if tot is None else [x + y for x, y in zip(tot, s)]
        sc = list(a) if sc is None else [x + y for x, y in zip(sc, a)]
    return tot, [x.max() for x in sc]


@pytest.mark.parametrize("name", ["smo", "emps27"])
def test_statistics_are_the_sum_over_records_and_no_pair_crosses_a_seam(name):
    pb = _problem(name, sum(STAT_LENGTHS))
    recs = _cut(pb, STAT_LENGTHS)
    C = 2
    rs = _records(recs, C, 16)
    eng = rs.engine
    rng = np.random.default_rng(2)
    trajs = np.stack([pb.X_true * (1.0 + 0.05 * rng.standard_normal(pb.X_true.shape)) for _ in range(C)])
    T0, T1, T2, T3 = eng.records_suffstats(torch.as_tensor(trajs, device=eng.device))
    assert T3 == sum(n - 1 for n in STAT_LENGTHS)
    assert T0.shape == (C, eng.M, pb.nx) and T1.shape == (C, eng.M, eng.M) and T2.shape == (C, pb.nx, pb.nx)
    for c in range(C):
        want, scale = _stats_numpy(recs, rs, trajs[c])
        assert want[3] == T3
        for g, r, s, what in zip((T0[c], T1[c], T2[c]), want, scale, ("T0", "T1", "T2")):
            d = np.abs(g.cpu().numpy() - r).max()
            print(f"{name} chain {c} {what}: max |d| = {d:.3e}, bound {RTOL * s * pb.T:.3e}")
            assert d <= RTOL * s * pb.T, f"chain {c} {what}: max |d| = {d:.3e} (scale {s:.3e})"
    # inputs at every record's LAST row belong to no transition of that record: changing them changes nothing, bit for bit ...
    last = rs.row0[1:] - 1
    u2 = np.array(pb.inputs, dtype=np.float64)
    u2[last] = u2[last] * 1.5 + 0.25
    recs2 = _cut(dataclasses.replace(pb, inputs=u2), STAT_LENGTHS)
    eng2 = _records(recs2, C, 16).engine
    for a, b, what in zip((T0, T1, T2), eng2.records_suffstats(torch.as_tensor(trajs, device=eng.device))[:3], ("T0", "T1", "T2")):
        assert torch.equal(a, b), f"{what} depends on the inputs at a record's last row"
    # ... while a plain context over the concatenation pairs those rows with the next record's first state
    plain, plain2 = _single(pb, 16).engine.suffstats(trajs[0]), _single(dataclasses.replace(pb, inputs=u2), 16).engine.suffstats(trajs[0])
    assert not torch.equal(plain[0], T0[0]) and not torch.equal(plain[1], T1[0]) and not torch.equal(plain[2], T2[0])
    if max(pb.basis_fcn.sel) >= pb.nx:   # the basis reads the input (emps27; SingleMassOscillator's reads the state alone)
        assert not torch.equal(plain[0], plain2[0]) and not torch.equal(plain[1], plain2[1])
    else:
        assert name == "smo" and torch.equal(plain[1], plain2[1])


@pytest.mark.parametrize("name,T", [("smo", 53), ("emps27", 300)])
def test_statistics_of_one_record_equal_the_chain_statistics(name, T):
    pb = _problem(name, T)
    C = 3
    eng = _records([pb], C, 16).engine
    rng = np.random.default_rng(8)
    trajs = torch.as_tensor(np.stack([pb.X_true * (1.0 + 0.05 * rng.standard_normal(pb.X_true.shape)) for _ in range(C)]), device=eng.device)
    a, b = eng.records_suffstats(trajs), eng.chains_suffstats(trajs)
    assert a[3] == b[3] == T - 1
    for x, y, what in zip(a[:3], b[:3], ("T0", "T1", "T2")):
        assert torch.equal(x, y), what


# ---------------------------------------------------------------------------------------------- Gibbs
def test_gibbs_with_one_record_equals_multichain_gibbs():
    pb = _problem("smo", 25)
    C, N, K, root = 2, 200, 4, 20241004
    args = (pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.GP_prior, pb.basis_fcn)
    mr = pgas_amd.MultiRecordPGAS(C, N, K, [pb.observations], [pb.inputs], *args)
    mc = pgas_amd.MultiChainPGAS(C, N, K, pb.observations, pb.inputs, *args)
    tr, lr = mr(root, [pb.X_true])
    tc, lc = mc(root, pb.X_true)
    assert mr.df == mc.df
    assert torch.equal(tr, tc) and torch.equal(lr, lc)
    assert torch.equal(mr.coeff_mat, mc.coeff_mat) and torch.equal(mr.error_cov, mc.error_cov)
    for (A1, S1), (A2, S2) in zip(mr.chain_log["params"], mc.chain_log["params"]):
        assert torch.equal(A1, A2) and torch.equal(S1, S2)
    assert not torch.equal(tr[:, :, 0], tr[:, :, K - 1])


def test_gibbs_against_a_restatement_with_summed_statistics():
    """MultiRecordPGAS(E = 3, C = 2, K = 4, N = 64) against PGAS.__call__ restated here from the oracle pieces: per record the canonical
    sweep with the record's seed, the host parameter draws, and the NumPy MNIW algebra on the statistics summed over the records.  Sweep
    k runs with the device's (A, S) of iteration k - 1 (teacher forcing, as tests/test_gpu_chains.py): state traces bit for bit, A and S
    to the tolerance tests/test_gpu_gibbs.py holds the single-record chain to."""
    lengths = (9, 2, 13)
    pb = _problem("smo", sum(lengths))
    recs = _cut(pb, lengths)
    E, C, K, N, root = len(recs), 2, 4, 64, 777
    mr = pgas_amd.MultiRecordPGAS(C, N, K, [q.observations for q in recs], [q.inputs for q in recs], pb.init_state_mean, pb.init_state_cov,
                                  pb.likelihood_fcn, pb.GP_prior, pb.basis_fcn)
    trace, ll = mr(root, [q.X_true for q in recs])
    Tsum, M = pb.T, mr.cSMC.engine.M
    assert tuple(trace.shape) == (C, Tsum, K, pb.nx) and tuple(ll.shape) == (C, Tsum, K)
    trace, ll = trace.cpu().numpy(), ll.cpu().numpy()
    df = float(pb.GP_prior[3]) + sum(n - 1 for n in lengths)
    assert mr.df == df
    prior = tuple(np.asarray(g, dtype=np.float64) if np.ndim(g) else float(g) for g in pb.GP_prior)
    cms = [canon_model(q, N) for q in recs]
    ncs = [numpy_csmc(q, 4) for q in recs]
    L0 = np.linalg.cholesky(pb.init_state_cov)
    roots = prng.split(root, C)
    for c in range(C):
        key, kp = prng.split(roots[c], 2)                      # src/PGAS.py:356
        dev_params = [(A[c].cpu().numpy(), S[c].cpu().numpy()) for A, S in mr.chain_log["params"]]
        st = np.zeros((K, Tsum, pb.nx))
        st[0] = pb.X_true
        own = []
        for k in range(K):
            if k:
                key, ks = prng.split(key, 2)                   # :365
                key, kp = prng.split(key, 2)                   # :377
                A, S = dev_params[k - 1]
                seeds = rc.host_seeds([ks], E)[0]
                for e, (cm, q) in enumerate(zip(cms, recs)):   # :366-371, per record
                    LS, LSinv, cS = cm.chol_parts_dev(S)
                    tr = cm.sweep(seeds[e], mr.record(e, st[k - 1]), A, LS, LSinv, cS, pb.init_state_mean, L0)[0]
                    mr.record(e, st[k])[:] = tr.reshape(q.T, pb.nx)
            stats = None
            for e, (nc, q) in enumerate(zip(ncs, recs)):       # :294-303, summed over the records
                tr = mr.record(e, st[k])
                s = pgas_numpy.suff_stats(tr, _phi(nc, tr, np.asarray(q.inputs, dtype=np.float64).reshape(q.T, -1)))
                stats = list(s) if stats is None else [x + y for x, y in zip(stats, s)]
            assert stats[3] == df - float(pb.GP_prior[3])
            d = host_param_draws(kp, pb.nx, M, df)
            own.append(pgas_numpy.sample_params(prior, *stats, d["chi2"], d["normals_T"], d["normals_A"])[:2])   # :306-341
        assert np.array_equal(trace[c], np.swapaxes(st, 0, 1)), f"chain {c}: state_trace differs from the restated chain"
        y = np.asarray(pb.observations, dtype=np.float64).reshape(Tsum, -1)
        llo = np.stack([ncs[0].lik(y[t], trace[c][t], None) for t in range(Tsum)])
        np.testing.assert_allclose(ll[c], llo, rtol=1e-12, atol=1e-12)
        for k, ((A, S), (Ao, So)) in enumerate(zip(dev_params, own)):
            np.testing.assert_allclose(A, Ao, rtol=1e-9, atol=1e-9 * np.abs(Ao).max(), err_msg=f"chain {c}: coeff_mat of iteration {k}")
            np.testing.assert_allclose(S, So, rtol=1e-9, atol=1e-12, err_msg=f"chain {c}: error_cov of iteration {k}")
        assert not np.array_equal(st[0], st[K - 1]), f"chain {c} must move"
    assert not np.array_equal(trace[0], trace[1])


def test_gibbs_iterations_make_no_host_round_trip():
    lengths = (9, 2, 13)
    pb = _problem("smo", sum(lengths))
    recs = _cut(pb, lengths)
    C = 2
    mr = pgas_amd.MultiRecordPGAS(C, 64, 3, [q.observations for q in recs], [q.inputs for q in recs], pb.init_state_mean, pb.init_state_cov,
                                  pb.likelihood_fcn, pb.GP_prior, pb.basis_fcn)
    mr(7, pb.X_true)   # first call: allocations (those may synchronise)
    eng = mr.cSMC.engine
    kd = ch.keys_tensor(prng.split(11, C), eng.device)
    traj = mr.cSMC._refs(pb.X_true)
    A, S = mr.sample_params(eng.chains_keys(kd, first=True), traj)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            kd, traj, A, S, _ = mr.step(kd, traj, A, S)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(S).all()) and bool(torch.isfinite(traj).all())


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_are_clean_and_leave_the_context_usable():
    pb = _problem("smo", sum(LENGTHS))
    recs = _cut(pb, LENGTHS)
    C, N, E = 2, 200, len(LENGTHS)
    keys, refs, As, Ss = _chain_inputs(pb, C)
    seeds = rc.host_seeds(keys, E)
    A, S = experiments.initial_params(pb)
    # a plain context: a record sweep before any table is refused, and so is every bad table; then a good one works
    chs = ch.condSequentialMonteCarloChains(C, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    eng = chs.engine
    chs.set_params(As, Ss)
    sd = torch.zeros((C, 1), dtype=torch.int64, device=eng.device)
    with pytest.raises(PgasError, match="no record table"):
        eng.records_sweep(sd, torch.as_tensor(refs, device=eng.device))
    for row0, msg in [([0, 2, 3, 33], "record 1 has 1 row"), ([0, 5, 5, 33], "not strictly increasing"), ([0, 9, 4, 33], "not strictly increasing"),
                      ([0, 2, 32], "row0\\[E\\] = 32"), ([0, 2, 40], "row0\\[E\\] = 40"), ([1, 5, 33], "row0\\[0\\] = 1")]:
        with pytest.raises(PgasError, match=msg):
            eng.records_set(row0)
    with pytest.raises(PgasError, match="no record table"):
        eng.records_sweep(sd, torch.as_tensor(refs, device=eng.device))
    eng.records_set(np.concatenate([[0], np.cumsum(LENGTHS)]))
    sdev = torch.as_tensor(np.array(seeds, dtype=np.uint64).view(np.int64), device=eng.device)
    # parameters set for another C
    eng.chains_set_params(torch.as_tensor(As[:1], device=eng.device), torch.as_tensor(Ss[:1], device=eng.device))
    with pytest.raises(PgasError, match="parameters are set for 1 chains, not 2"):
        eng.records_sweep(sdev, torch.as_tensor(refs, device=eng.device))
    chs.set_params(As, Ss)
    traj = eng.records_sweep(sdev, torch.as_tensor(refs, device=eng.device)).cpu().numpy()
    rs = _records(recs, C, N)
    out = _run(rs, keys, refs, As, Ss)
    assert np.array_equal(traj, out[0])
    _check_against_single(recs, N, rs, out, seeds, refs, As, Ss, cells=[(1, 2)])
    # N = 1025: the table is refused, the context still runs a correct single-record sweep
    with pytest.raises(PgasError, match="N = 1025"):
        _records(recs, C, 1025)
    big = _single(pb, 1025)
    with pytest.raises(PgasError, match="N = 1025"):
        big.engine.records_set([0, 2, 33])
    cm = canon_model(pb, 1025)
    LS, LSinv, cS = cm.chol_parts_dev(S)
    want = cm.sweep(12345, pb.X_true, A, LS, LSinv, cS, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov))[0]
    got = big(12345, pb.X_true, A, torch.as_tensor(S, device=big.device)).cpu().numpy()
    assert np.array_equal(got.reshape(pb.T, pb.nx), want.reshape(pb.T, pb.nx))
