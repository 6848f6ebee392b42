"""C independent PGAS chains in batched launches (pgas_amd.chains, csrc/pgas_chains.hip.h): every chain against the single-chain engine
with the same key, reference, A and S, against the canonical C oracle, and whole Gibbs chains against the restated chain
(oracle/pgas_numpy.pgas_chain).  Every equality is bit for bit unless a tolerance is stated."""
import numpy as np
import pytest
import torch

from common import canon_model, experiments, host_param_draws, numpy_csmc, pgas_amd
from pgas_amd import chains as ch
from pgas_amd import random as prng
from pgas_amd._lib import PgasError

pytestmark = pytest.mark.gpu


def _problem(name):
    return {
        "smo": lambda: experiments.smo_pgas(T=24),
        "toy": lambda: experiments.toy(T=24),
        "emps27": lambda: experiments.emps_pgas(T=16, M=27),
        "veh27": lambda: experiments.vehicle_pgas(T=20, M=27),
        "emps": lambda: experiments.emps_pgas(T=6),     # M = 729
    }[name]()


def _chain_inputs(pb, C, seed=5):
    """C different (key, reference, A, S): perturbations of the problem's truth and its posterior-mean parameters."""
    A, S = experiments.initial_params(pb)
    rng = np.random.default_rng(seed)
    keys = [prng.key(1000 + 7919 * c) for c in range(C)]
    refs = np.stack([pb.X_true + 0.01 * c * rng.standard_normal(pb.X_true.shape) for c in range(C)])
    As = np.stack([A * (1.0 + 0.02 * c) for c in range(C)])
    Ss = np.stack([S * (1.0 + 0.1 * c) for c in range(C)])
    return keys, refs, As, Ss


def _chains(pb, C, N):
    return ch.condSequentialMonteCarloChains(C, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn,
                                             pb.basis_fcn)


def _single(pb, N, **kw):
    return pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn,
                                             pb.basis_fcn, **kw)


def _run(chs, keys, refs, As, Ss):
    """One batched sweep -> host copies of (traj, x, anc, logw_last, final index)."""
    traj = chs(keys, refs, As, Ss).cpu().numpy()
    X, ANC, LW = (t.cpu().numpy() for t in chs.traces())
    return traj, X, ANC, LW, chs.final_index()


def _check_against_single(pb, N, out, keys, refs, As, Ss, chains=None):
    """Chain c of a batched sweep equals a single-chain sweep (error_cov on the device: the same factorisation) with chain c's inputs."""
    traj, X, ANC, LW, fidx = out
    T, nx = pb.T, pb.nx
    csmc = _single(pb, N)
    dev = csmc.device
    for c in range(len(keys)) if chains is None else chains:
        t1 = csmc(keys[c], torch.as_tensor(refs[c], device=dev), torch.as_tensor(As[c], device=dev), torch.as_tensor(Ss[c], device=dev))
        X1, A1, L1, _ = csmc.engine.traces()
        assert np.array_equal(traj[c], t1.cpu().numpy().reshape(T, nx)), f"chain {c}: trajectory"
        assert np.array_equal(X[c], X1.cpu().numpy()), f"chain {c}: state trace"
        assert np.array_equal(ANC[c, : T - 1], A1.cpu().numpy()[: T - 1]), f"chain {c}: ancestor trace"
        assert np.array_equal(LW[c], L1.cpu().numpy()), f"chain {c}: final log-weights"
        assert fidx[c] == csmc.engine.last_final_index(), f"chain {c}: final index"


@pytest.mark.parametrize("C", [1, 7])
@pytest.mark.parametrize("name,N", [(m, n) for m in ("smo", "toy", "emps27", "veh27", "emps") for n in (1, 2, 200, 256, 257, 700, 1024)])
def test_chains_equal_single_chain_and_oracle(name, N, C):
    pb = _problem(name)
    keys, refs, As, Ss = _chain_inputs(pb, C)
    chs = _chains(pb, C, N)
    out = _run(chs, keys, refs, As, Ss)
    assert out[0].shape == (C, pb.T, pb.nx)
    _check_against_single(pb, N, out, keys, refs, As, Ss)
    traj, X, ANC, LW, fidx = out
    cm = canon_model(pb, N)
    L0 = np.linalg.cholesky(pb.init_state_cov)
    for c in sorted({0, C - 1}):
        LS, LSinv, cS = cm.chol_parts_dev(Ss[c])
        trajo, Xo, ANCo, lwo = cm.sweep(keys[c], refs[c], As[c], LS, LSinv, cS, pb.init_state_mean, L0)
        assert np.array_equal(traj[c], trajo.reshape(pb.T, pb.nx)), f"chain {c}: trajectory vs oracle"
        assert np.array_equal(X[c], Xo.reshape(X[c].shape)), f"chain {c}: state trace vs oracle"
        assert np.array_equal(ANC[c, : pb.T - 1], ANCo), f"chain {c}: ancestor trace vs oracle"
        assert np.array_equal(LW[c], lwo), f"chain {c}: final log-weights vs oracle"


@pytest.mark.parametrize("C,N,T", [(2000, 64, 16), (600, 1024, 8)])
def test_more_chains_than_the_gpu_holds_at_once(C, N, T):
    """2000 chains of 64 particles, 600 of 1024 (one wave per SIMD): more workgroups than are resident; every chain still equals its
    single-chain sweep."""
    pb = experiments.smo_pgas(T=T)
    keys, refs, As, Ss = _chain_inputs(pb, C)
    out = _run(_chains(pb, C, N), keys, refs, As, Ss)
    _check_against_single(pb, N, out, keys, refs, As, Ss)


def test_chains_are_independent_of_their_order_and_of_reference_sharing():
    pb = _problem("smo")
    C, N = 9, 200
    keys, refs, As, Ss = _chain_inputs(pb, C)
    chs = _chains(pb, C, N)
    fwd = _run(chs, keys, refs, As, Ss)
    rev = _run(chs, keys[::-1], refs[::-1], As[::-1], Ss[::-1])
    for a, b, what in zip(fwd, rev, ("trajectory", "state trace", "ancestor trace", "final log-weights", "final index")):
        assert np.array_equal(a[::-1], b), what
    shared = _run(chs, keys, pb.X_true, As, Ss)
    repeated = _run(chs, keys, np.repeat(pb.X_true[None], C, axis=0), As, Ss)
    for a, b, what in zip(shared, repeated, ("trajectory", "state trace", "ancestor trace", "final log-weights", "final index")):
        assert np.array_equal(a, b), what
    assert not np.array_equal(shared[0][0], shared[0][1]), "two chains with different keys drew the same trajectory"


def test_device_key_derivation_and_parameter_draws():
    """pgas_chains_keys against pgas_amd.random.split for 1000 random chain keys over 3 iterations (the order of PGAS.__call__), and the
    batched parameter draws against host_param_draws for every chain."""
    pb = experiments.smo_pgas(T=24)
    eng = _single(pb, 16).engine
    rng = np.random.default_rng(3)
    host = [int(v) for v in rng.integers(0, 2**64 - 1, size=1000, dtype=np.uint64, endpoint=True)]
    kd = ch.keys_tensor(host, eng.device)
    df = float(pb.GP_prior[3]) + (pb.T - 1)
    for it in range(3):
        k6 = eng.chains_keys(kd, first=it == 0)
        got = [ch.keys_list(k6[r]) for r in range(6)]
        want = [[] for _ in range(6)]
        for c, k in enumerate(host):
            ks = 0
            if it:
                k, ks = prng.split(k, 2)
            k, kp = prng.split(k, 2)
            kA, kS = prng.split(kp, 2)
            kchi, knorm = prng.split(kS, 2)
            for r, v in enumerate((k, ks, kp, kA, kchi, knorm)):
                want[r].append(v)
            host[c] = k
        assert got == want, f"iteration {it}: device keys differ from random.split"
        if it == 0:
            d = eng.chains_param_draws(k6, df)
            d = {n: v.cpu().numpy() for n, v in d.items()}
            for c in range(len(host)):
                h = host_param_draws(want[2][c], pb.nx, eng.M, df)
                assert all(np.array_equal(d[n][c], h[n]) for n in h), f"chain {c}: parameter draws"
        kd = k6[0]


@pytest.mark.parametrize("name,T", [("smo", 300), ("emps", 120)])
def test_batched_sufficient_statistics(name, T):
    pb = experiments.smo_pgas(T=T) if name == "smo" else experiments.emps_pgas(T=T)
    eng = _single(pb, 16).engine
    C = 5
    rng = np.random.default_rng(2)
    trajs = torch.as_tensor(np.stack([pb.X_true * (1.0 + 0.05 * rng.standard_normal(pb.X_true.shape)) for _ in range(C)]), device=eng.device)
    T0, T1, T2, T3 = eng.chains_suffstats(trajs)
    assert T0.shape == (C, eng.M, pb.nx) and T1.shape == (C, eng.M, eng.M) and T2.shape == (C, pb.nx, pb.nx) and T3 == T - 1
    for c in range(C):
        s = eng.suffstats(trajs[c])
        for got, want in zip((T0[c], T1[c], T2[c]), s[:3]):
            g, w = got.cpu().numpy(), want.cpu().numpy()
            np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12 * np.abs(w).max())


@pytest.mark.parametrize("name", ["toy", "smo"])
def test_multichain_gibbs_against_restated_chains(name):
    """MultiChainPGAS(C = 3, N = 700, K = 4): chain c replayed by oracle/pgas_numpy.pgas_chain with its own step keys (recomputed from its
    root key), host draws and the device's (A_k, S_k) of chain c as teacher forcing."""
    from oracle import pgas_numpy as o

    pb = experiments.toy(T=30) if name == "toy" else experiments.smo_pgas(T=25)
    C, N, K, root = 3, 700, 4, 20241004
    mc = pgas_amd.MultiChainPGAS(C, N, K, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.GP_prior,
                                 pb.basis_fcn)
    trace, ll = mc(root, pb.X_true)
    assert tuple(trace.shape) == (C, pb.T, K, pb.nx) and tuple(ll.shape) == (C, pb.T, K)
    trace, ll = trace.cpu().numpy(), ll.cpu().numpy()
    roots = prng.split(root, C)
    assert mc.chain_log["root_keys"] == roots
    M = mc.cSMC.engine.M
    df = float(pb.GP_prior[3]) + (pb.T - 1)
    cm = canon_model(pb, N)
    L0 = np.linalg.cholesky(pb.init_state_cov)

    def sweep(seed, ref, A, S):
        LS, LSinv, cS = cm.chol_parts_dev(S)
        return cm.sweep(seed, ref, A, LS, LSinv, cS, pb.init_state_mean, L0)[0]

    nc = numpy_csmc(pb, N)
    prior = tuple(np.asarray(g, dtype=np.float64) if np.ndim(g) else float(g) for g in pb.GP_prior)
    for c in range(C):
        key, key_para = prng.split(roots[c], 2)                  # src/PGAS.py:356, :365, :377
        para_keys, step_keys = [key_para], [None]
        for k in range(1, K):
            key, ks = prng.split(key, 2)
            key, kp = prng.split(key, 2)
            step_keys.append(ks)
            para_keys.append(kp)
        assert [ch.keys_list(k6[2])[c] for k6 in mc.chain_log["keys"]] == para_keys
        assert [ch.keys_list(k6[1])[c] for k6 in mc.chain_log["keys"]][1:] == step_keys[1:]
        draws = [host_param_draws(kp, pb.nx, M, df) for kp in para_keys]
        dev_params = [(A[c].cpu().numpy(), S[c].cpu().numpy()) for A, S in mc.chain_log["params"]]
        st, llo, own = o.pgas_chain(sweep, nc.basis, nc.lik, prior, pb.observations, pb.inputs, pb.X_true, K, step_keys, draws, params=dev_params)
        assert np.array_equal(trace[c], st), f"chain {c}: state_trace differs from the restated chain"
        np.testing.assert_allclose(ll[c], llo, rtol=1e-12, atol=1e-12)
        for k, ((A, S), (Ao, So)) in enumerate(zip(dev_params, own)):
            np.testing.assert_allclose(A, Ao, rtol=1e-9, atol=1e-9 * np.abs(Ao).max(), err_msg=f"chain {c}: coeff_mat of iteration {k}")
            np.testing.assert_allclose(S, So, rtol=1e-9, atol=1e-12, err_msg=f"chain {c}: error_cov of iteration {k}")
        assert not np.array_equal(st[:, 0], st[:, K - 1]), f"chain {c} must move"
    for a in range(C):
        for b in range(a + 1, C):
            assert not np.array_equal(trace[a], trace[b]), f"chains {a} and {b} are identical"


def test_batched_gibbs_iterations_make_no_host_round_trip():
    """Three batched Gibbs iterations (keys -> sweep -> statistics -> MNIW draw for every chain) with device synchronisation made an
    error: no .cpu() / .item() / blocking copy hides in the loop."""
    pb = experiments.toy(T=30)
    C = 4
    mc = pgas_amd.MultiChainPGAS(C, 500, 3, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.GP_prior,
                                 pb.basis_fcn)
    mc(7, pb.X_true)   # first call: allocations (those may synchronise)
    eng = mc.cSMC.engine
    kd = ch.keys_tensor(prng.split(11, C), eng.device)
    traj = torch.as_tensor(np.repeat(pb.X_true.reshape(1, pb.T, -1), C, axis=0), device=eng.device)
    A, S = mc.sample_params(eng.chains_keys(kd, first=True), traj)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            kd, traj, A, S, _ = mc.step(kd, traj, A, S)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(S).all()) and bool(torch.isfinite(traj).all())


def test_refusals_are_clean_and_leave_the_context_usable():
    pb = experiments.smo_pgas(T=16)
    C = 3
    keys, refs, As, Ss = _chain_inputs(pb, C)
    A, S = experiments.initial_params(pb)
    cm = canon_model(pb, 1025)
    L0 = np.linalg.cholesky(pb.init_state_cov)
    for N, kw, msg in [(1025, {}, "N = 1025"), (200, {"resample_before_propagate": True}, "corrected mode"),
                       (200, {"keep_logw_trace": True}, "keep_logw_trace")]:
        chs = ch.condSequentialMonteCarloChains(C, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn,
                                                pb.basis_fcn, **kw)
        with pytest.raises(PgasError, match=msg):
            chs(keys, refs, As, Ss)
        # the same context still runs a correct single-chain sweep
        traj = chs.single(12345, pb.X_true, A, torch.as_tensor(S, device=chs.device)).cpu().numpy().reshape(pb.T, pb.nx)
        if N == 1025:
            LS, LSinv, cS = cm.chol_parts_dev(S)
            want = cm.sweep(12345, pb.X_true, A, LS, LSinv, cS, pb.init_state_mean, L0)[0]
        else:
            want = _single(pb, N, **kw)(12345, pb.X_true, A, torch.as_tensor(S, device=chs.device)).cpu().numpy()
        assert np.array_equal(traj, want.reshape(pb.T, pb.nx)), f"single-chain sweep after refusing {kw or N}"
    # mismatched shapes, then the same context runs correct batched chains
    N = 200
    chs = _chains(pb, C, N)
    bad = [(keys[:2], refs, As, Ss), (keys, refs[:, :-1], As, Ss), (keys, refs, As[:, :, :-1], Ss), (keys, refs, As, Ss[:2]),
           (keys, refs, As[:2], Ss[:2])]
    for args in bad:
        with pytest.raises(ValueError):
            chs(*args)
    # more chains than the device can hold: PGAS_E_NOMEM with a message, nothing kept
    big = experiments.smo_pgas(T=2000)
    huge = ch.condSequentialMonteCarloChains(65535, 1024, big.observations, big.inputs, big.init_state_mean, big.init_state_cov,
                                             big.likelihood_fcn, big.basis_fcn, device=chs.device)
    Ab, Sb = experiments.initial_params(big)
    with pytest.raises(PgasError, match="do not fit"):
        huge.engine.chains_set_params(torch.as_tensor(np.repeat(Ab[None], 65535, axis=0), device=chs.device),
                                      torch.as_tensor(np.repeat(Sb[None], 65535, axis=0), device=chs.device))
    out = _run(chs, keys, refs, As, Ss)
    _check_against_single(pb, N, out, keys, refs, As, Ss)


def test_single_and_batched_statistics_share_one_pair_of_buffers():
    """pgas_suffstats and pgas_chains_suffstats run on ONE pair of grow-only buffers: a single-chain call, a batched call of 7 different
    trajectories (the buffers grow) and the single-chain call again, on one context.  At T = 40 the three row panels are one split each
    for one chain and for seven, so chain c of the batched result sums in the single call's order: every equality is bit for bit."""
    pb = experiments.smo_pgas(T=40)
    C = 7
    chs = _chains(pb, C, 16)
    eng = chs.single.engine
    rng = np.random.default_rng(8)
    trajs = torch.as_tensor(np.stack([pb.X_true * (1.0 + 0.05 * rng.standard_normal(pb.X_true.shape)) for _ in range(C)]), device=eng.device)
    first = eng.suffstats(trajs[0])
    batched = chs.engine.chains_suffstats(trajs)
    third = eng.suffstats(trajs[0])
    for a, b, what in zip(first[:3], third[:3], ("T0", "T1", "T2")):
        assert torch.equal(a, b), f"{what}: the single-chain statistics changed after a batched call"
    for c in range(C):
        for got, want, what in zip(batched[:3], eng.suffstats(trajs[c])[:3], ("T0", "T1", "T2")):
            assert torch.equal(got[c], want), f"chain {c}: {what}"
    assert not torch.equal(batched[1][0], batched[1][1]), "two different trajectories gave the same statistics"


def test_single_and_batched_sweeps_on_one_context():
    """The one-workgroup kernel serves both pgas_sweep (PGAS_OPT_SMALL_SWEEP = 2, the context's own buffers) and pgas_chains_sweep (the
    chains' buffers): a single sweep, a batched sweep of C = 3 and the single sweep again on one context.  N = 300: two particles per thread."""
    pb = _problem("smo")
    C, N = 3, 300
    keys, refs, As, Ss = _chain_inputs(pb, C)
    chs = _chains(pb, C, N)
    csmc, dev = chs.single, chs.device
    csmc.engine.set_option(14, 2)

    def single(c):
        traj = csmc(keys[c], torch.as_tensor(refs[c], device=dev), torch.as_tensor(As[c], device=dev), torch.as_tensor(Ss[c], device=dev))
        assert csmc.engine.launch_info()["small"], "which sweep ran"
        X, A, L, _ = csmc.engine.traces()
        return traj.cpu().numpy().reshape(pb.T, pb.nx), X.cpu().numpy(), A.cpu().numpy()[: pb.T - 1], L.cpu().numpy(), csmc.engine.last_final_index()

    names = ("trajectory", "state trace", "ancestor trace", "final log-weights", "final index")
    first = single(0)
    traj, X, ANC, LW, fidx = _run(chs, keys, refs, As, Ss)
    third = single(0)
    for a, b, what in zip(first, third, names):
        assert np.array_equal(a, b), f"{what}: the single sweep changed after a batched sweep"
    for c in range(C):
        for a, b, what in zip((traj[c], X[c], ANC[c, : pb.T - 1], LW[c], fidx[c]), third if c == 0 else single(c), names):
            assert np.array_equal(a, b), f"chain {c}: {what}"
