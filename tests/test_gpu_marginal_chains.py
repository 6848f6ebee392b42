"""GPU tests of C marginalised Particle-Gibbs chains in one batched pass (pgas_amd.MultiChainAlgorithm3 / MultiChainAlgorithm2, the entry
points pgas_m_runs_mniw_solve_n / _lbm_diff / _categorical / _backtrace).

Device primitives: bit for bit against the single-run entry points on every run's slice, the categorical draw bit for bit against its
NumPy restatement (tests/runs_categorical_numpy.py).  The chains: every chain against the single-chain class with that chain's key and
reference on the device (ancestors and indices equal, continuous outputs to 1e-12 relative -- the bound of tests/test_gpu_runs.py) and
against the NumPy restatement of the reference (oracle/marginal_numpy.py) at the tolerances of tests/test_gpu_marginal.py."""
import numpy as np
import pytest
import torch

import runs_categorical_numpy as rcn
from common import CanonRand, experiments, marginal_oracle, pgas_amd
from oracle import marginal_numpy as mo

pytestmark = pytest.mark.gpu
SEED = 12345678


def _ops(N):
    from pgas_amd._lib import MarginalOps

    return MarginalOps(N)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(np.shape(a))
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ------------------------------------------------------------------------------------------ 1. the solves and the base measures per run
def _solve_operands(R, N, M, nv, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    B = rnd(R * N, M, 3)
    T1 = (B @ B.transpose(1, 2)).to(dev).contiguous()
    T0 = (rnd(R * N, M, nv) if nv > 1 else rnd(R * N, M)).to(dev)
    P1 = torch.diag(torch.rand(M, generator=g, dtype=torch.float64) + 0.5).to(dev)
    P0 = (rnd(M, nv) if nv > 1 else rnd(M)).to(dev)
    phi = rnd(R * N, M).to(dev)
    Rb = rnd(R, M, 2) * 0.3
    R1 = (Rb @ Rb.transpose(1, 2)).to(dev).contiguous()
    R0 = (rnd(R, M, nv) if nv > 1 else rnd(R, M)).to(dev)
    loc = torch.randint(0, N, (R, N), generator=g)
    return P0, P1, T0, T1, R0, R1, phi, loc.to(dev).to(torch.int32)


@pytest.mark.parametrize("nv", [1, 2])
@pytest.mark.parametrize("M", [1, 41, 62, 63, 126])
def test_runs_mniw_solve_equals_the_single_run_solve_on_every_slice(M, nv):
    """Every output of pgas_m_runs_mniw_solve_n, the packed factor included, is the single-run call's on run r's slices with R0[r], R1[r]:
    the matrix-core kernel (M <= 62, n = 1), the column-by-column kernel (option 6 = 1) and the two-rows-per-lane kernel (M >= 63 or n > 1),
    with and without a (global) ancestor gather.  M + 1 + n <= 128 rows is the library's limit, so M = 126 with n = 2 is its clean refusal
    and the largest basis of two components, M = 125, stands in for it."""
    if M + 1 + nv > 128:
        from pgas_amd._lib import PgasError

        ops = _ops(10)
        P0, P1, T0, T1, R0, R1, phi, _ = _solve_operands(2, 5, M, nv, ops.device, 1)
        with pytest.raises(PgasError, match="outside"):
            ops.mniw_solve(P0, P1, T0, T1, R0=R0, R1=R1, phi=phi, runs=2)
        M = 128 - 1 - nv
    knobs = (0, 1) if (M <= 62 and nv == 1) else (0,)
    for R in (1, 3):
        for N in (5, 64):
            all_, one = _ops(R * N), _ops(N)
            dev = all_.device
            P0, P1, T0, T1, R0, R1, phi, loc = _solve_operands(R, N, M, nv, dev, 1000 * M + 10 * R + nv)
            glo = (loc + (torch.arange(R, device=dev, dtype=torch.int32) * N)[:, None]).reshape(-1).contiguous()
            for knob in knobs:
                try:
                    all_.eng.set_option(6, knob)
                    one.eng.set_option(6, knob)
                    for anc_g, anc_l, scale in ((None, None, 1.0), (glo, loc, 0.97)):
                        got = all_.mniw_solve(P0, P1, T0, T1, scale=scale, anc=anc_g, R0=R0, R1=R1, phi=phi, keep_factor=True, runs=R)
                        for r in range(R):
                            sl = slice(r * N, (r + 1) * N)
                            ref = one.mniw_solve(P0, P1, T0[sl].contiguous(), T1[sl].contiguous(), scale=scale, anc=None if anc_l is None else anc_l[r].contiguous(),
                                                 R0=R0[r].contiguous(), R1=R1[r].contiguous(), phi=phi[sl].contiguous(), keep_factor=True)
                            for k in ("m", "c", "q", "logdet", "L"):
                                assert torch.equal(got[k][sl], ref[k]), (k, R, N, r, knob, scale)
                            assert bool(torch.isfinite(ref["logdet"]).all())
                finally:
                    all_.eng.set_option(6, 0)
                    one.eng.set_option(6, 0)
            all_.check()
            one.check()


def test_runs_mniw_solve_refuses_operands_that_do_not_match():
    ops = _ops(10)
    dev = ops.device
    P0, P1, T0, T1, R0, R1, phi, _ = _solve_operands(2, 5, 4, 1, dev, 3)
    with pytest.raises(ValueError, match="runs"):
        ops.mniw_solve(P0, P1, T0, T1, R0=R0[0].contiguous(), R1=R1, runs=2)
    with pytest.raises(ValueError, match="runs"):
        ops.mniw_solve(P0, P1, T0, T1, R0=R0, R1=R1, runs=3)
    ops.mniw_solve(P0, P1, T0, T1, R0=R0, R1=R1, phi=phi, runs=2)
    ops.check()


@pytest.mark.parametrize("R,N", [(1, 5), (3, 64), (4, 257)])
def test_runs_lbm_diff_equals_the_single_run_call_on_every_slice(R, N):
    M = 41
    all_, one = _ops(R * N), _ops(N)
    dev = all_.device
    g = torch.Generator(device="cpu").manual_seed(R * N)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).to(dev)   # noqa: E731
    T2, T3 = rnd(R * N) + 3.0, rnd(R * N) * 9 + 1.0
    s1 = {"q": rnd(R * N), "logdet": rnd(R * N) * 5}
    s2 = {"q": rnd(R * N), "logdet": rnd(R * N) * 5}
    r2, r3 = rnd(R) + 0.5, rnd(R) * 6 + 1.0
    got = all_.runs_lbm_diff(R, M, T2, T3, s1, s2, 1.5, 3.0, r2, r3)
    for r in range(R):
        sl = slice(r * N, (r + 1) * N)
        ref = one.lbm_diff(M, T2[sl].contiguous(), T3[sl].contiguous(), {k: v[sl].contiguous() for k, v in s1.items()}, {k: v[sl].contiguous() for k, v in s2.items()},
                           1.5, 3.0, r2[r:r + 1], r3[r:r + 1])
        assert torch.equal(got[sl], ref) and bool(torch.isfinite(ref).all()), r


# ------------------------------------------------------------------------------------------ 2. the categorical draw
SENTINEL = -7


def _check_categorical(lw, u, names=None):
    """lw (R, N), u (R,) host arrays: the launch against the restatement, with and without the ancestor arrays."""
    R, N = lw.shape
    ops = _ops(N)
    dev = ops.device
    lwd, ud = torch.as_tensor(lw, device=dev), torch.as_tensor(u, device=dev)
    want = rcn.runs_categorical(lw, u)
    loc = torch.full((R, N), SENTINEL, dtype=torch.int32, device=dev)
    glo = torch.full((R, N), SENTINEL, dtype=torch.int32, device=dev)
    idx = ops.runs_categorical(R, lwd, ud, anc_local=loc, anc_global=glo)
    got = idx.cpu().numpy()
    bad = np.nonzero(got != want)[0].tolist()
    assert not bad, f"N = {N}: rows {[(names[r] if names else r, int(got[r]), int(want[r])) for r in bad[:8]]} differ from the restatement"
    assert idx.dtype == torch.int32 and ((got >= 0) & (got < N)).all()
    assert torch.equal(loc[:, -1], idx) and torch.equal(glo[:, -1], idx + torch.arange(R, device=dev, dtype=torch.int32) * N)
    assert bool((loc[:, :-1] == SENTINEL).all()) and bool((glo[:, :-1] == SENTINEL).all()), "a slot other than N - 1 was written"
    assert torch.equal(ops.runs_categorical(R, lwd, ud), idx), "the draw does not depend on the optional outputs"
    return got


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 200, 257, 1024])
def test_runs_categorical_equals_the_restatement(N):
    """Degenerate, multi-scale, single-survivor and all-equal weights under uniforms kept 1e-9 of the mass away from every CDF step, and the
    rows without a softmax (NaN, all -inf, +inf), which give N - 1."""
    names, lw, u = rcn.batch(N)
    got = _check_categorical(lw, u, names)
    for r, name in enumerate(names):
        if "/u=" in name:
            assert rcn.margin(lw[r], u[r]) >= rcn.MARGIN, name
            assert got[r] == rcn.plain_row(lw[r], u[r])[0], f"{name}: differs from plain float64 searchsorted(cumsum(softmax))"
        else:
            assert got[r] == N - 1, name


@pytest.mark.parametrize("R,N", [(1, 200), (3, 200), (300, 200), (300, 1024)])
def test_runs_categorical_with_any_number_of_runs(R, N):
    lw = np.stack([rcn.rc.mild(N, seed=r) for r in range(R)])
    u = np.array([rcn.place_uniform(lw[r], v) for r, v in enumerate(np.random.default_rng(R).uniform(0.0, 1.0, R))])
    got = _check_categorical(lw, u)
    assert R < 3 or len(set(got.tolist())) > 1


def test_runs_categorical_refuses_more_than_1024_particles():
    from pgas_amd._lib import PgasError

    ops = _ops(200)
    dev = ops.device
    with pytest.raises(PgasError, match="1025"):
        ops.runs_categorical(2, torch.zeros(2, 1025, dtype=torch.float64, device=dev), torch.full((2,), 0.5, dtype=torch.float64, device=dev))
    _check_categorical(np.stack([rcn.rc.mild(200, seed=r) for r in range(2)]), np.array([0.25, 0.75]))


# ------------------------------------------------------------------------------------------ 3. the trajectories
@pytest.mark.parametrize("T", [1, 2, 12])
def test_runs_backtrace_equals_reconstruct_trajectory_per_run(T):
    from pgas_amd._lib import Engine

    R, N = 3, 65
    ops, eng = _ops(R * N), Engine.utility(N)
    dev = ops.device
    g = torch.Generator(device="cpu").manual_seed(T)
    anc = torch.randint(0, N, (max(T - 1, 0), R, N), generator=g).to(torch.int32).to(dev)
    idx = torch.tensor([0, N - 1, N // 2], dtype=torch.int32, device=dev)
    for w in (1, 2, 3):
        x = torch.randn(T, R, N, w, generator=g, dtype=torch.float64).to(dev)
        got = ops.runs_backtrace(R, x.reshape(T, R * N, w), anc.reshape(max(T - 1, 0), R * N), idx)
        assert got.shape == (R, T, w)
        for r in range(R):
            ref = eng.reconstruct_trajectory(x[:, r].contiguous(), anc[:, r].contiguous(), int(idx[r]))
            assert torch.equal(got[r], ref), (T, w, r)
    flat = ops.runs_backtrace(R, x[..., 0].reshape(T, R * N), anc.reshape(max(T - 1, 0), R * N), idx)   # a trace without a component axis
    assert torch.equal(flat, ops.runs_backtrace(R, x[..., :1].reshape(T, R * N, 1), anc.reshape(max(T - 1, 0), R * N), idx))


# ------------------------------------------------------------------------------------------ 4. the conditional filter, chain by chain
def _problem(name, T=8):
    return {"smo": experiments.smo_marginal, "toy": experiments.toy_marginal, "vehicle": experiments.vehicle_marginal,
            "smo2": experiments.smo_two_component_marginal}[name.split("/")[0]](T=T)


def _args(pb, name):
    ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel) if name.endswith("/traced") else pb.ssm(pgas_amd.StateSpaceModel, torch)
    return dict(observations=pb.observations, inputs=pb.inputs, SSM=ssm, init_state_mean=pb.init_state_mean, init_state_cov=pb.init_state_cov,
                init_int_var_mean=pb.init_int_var_mean, init_int_var_cov=pb.init_int_var_cov, GP_prior=pb.GP_prior, basis_fcn=pb.basis_fcn())


def _references(pb, C, N):
    """Per-chain references: chain c starts from X_true shifted by c * 0.01; their statistics from the NumPy restatement.  -> (ref_x (C, T, n_x),
    ref_iv [(C, T, n)], stats per chain [[4 arrays] per interface variable], the same stacked over the chains)."""
    oracle = marginal_oracle(pb, N, "Algorithm3")
    ref_x = np.stack([np.asarray(pb.X_true, dtype=np.float64).reshape(pb.T, -1) + 0.01 * c for c in range(C)])
    ref_iv = [np.stack([np.asarray(v, dtype=np.float64).reshape(pb.T, -1)] * C) for v in pb.int_var_true]
    per_chain = [mo.trajectory_stats(oracle, ref_x[c], [v[c] for v in ref_iv]) for c in range(C)]
    stacked = [[np.stack([np.asarray(per_chain[c][i][j], dtype=np.float64) for c in range(C)]) for j in range(4)] for i in range(len(ref_iv))]
    return oracle, ref_x, ref_iv, per_chain, stacked


def _check_chains_against_single_chains(name, C, N, T=8, use_graph=None):
    pb = _problem(name, T)
    n_int = len(pb.init_int_var_mean)
    keys = pgas_amd.random.split(SEED + 3, C)
    oracle, ref_x, ref_iv, per_chain, stacked = _references(pb, C, N)
    traj, ivt, tr = pgas_amd.MultiChainAlgorithm3(C, N, **_args(pb, name))(keys, ref_x, ref_iv, stacked, return_traces=True, use_graph=use_graph)
    assert traj.shape == (C, T, ref_x.shape[2]) and tr["ancestor_trace"].shape == (C, T - 1, N) and tr["ancestor_trace"].dtype == torch.int32
    assert tr["idx"].shape == (C,) and tr["idx"].dtype == torch.int32 and tr["log_weights"].shape == (C, N)
    problems = []
    for c in range(C):
        st, si, sr = pgas_amd.Algorithm3(N, **_args(pb, name))(keys[c], ref_x[c], [v[c] for v in ref_iv], per_chain[c], return_traces=True, use_graph=use_graph)
        if not torch.equal(tr["ancestor_trace"][c], sr["ancestor_trace"]):
            problems.append(f"chain {c}: ancestor_trace differs")
        if int(tr["idx"][c]) != int(sr["idx"]):
            problems.append(f"chain {c}: idx {int(tr['idx'][c])} != {int(sr['idx'])}")
        pairs = [("state_trace", tr["state_trace"][c], sr["state_trace"]), ("log_weights", tr["log_weights"][c], sr["log_weights"]), ("state_traj", traj[c], st)]
        for i in range(n_int):
            pairs += [(f"int_var_trace[{i}]", tr["int_var_trace"][i][c], sr["int_var_trace"][i]), (f"int_var_traj[{i}]", ivt[i][c], si[i])]
        for what, a, b in pairs:
            assert a.numel() == b.numel(), (what, a.shape, b.shape)
            err = _rel(_np(b), _np(a).reshape(tuple(b.shape)))
            print(f"{name} C={C} N={N} chain {c} {what}: relative difference {err:.3e}, bit-equal {torch.equal(a.reshape(b.shape), b)}")
            if not err <= 1e-12:
                problems.append(f"chain {c}: {what} differs by {err:.3e} > 1e-12")
    assert not problems, problems
    for c in sorted({0, C - 1}):
        rt, ri, rr = oracle(CanonRand(keys[c], N), ref_x[c], [v[c] for v in ref_iv], per_chain[c])
        assert np.array_equal(_np(tr["ancestor_trace"][c]), rr["ancestor_trace"]) and int(tr["idx"][c]) == rr["idx"], f"chain {c}: indices differ from the restatement"
        checks = [("state_trace", tr["state_trace"][c], rr["state_trace"], 1e-8), ("log_weights", tr["log_weights"][c], rr["log_weights"], 1e-7),
                  ("state_traj", traj[c], rt, 1e-8)] + [(f"int_var_traj[{i}]", ivt[i][c], ri[i], 1e-8) for i in range(n_int)]
        for what, a, b, tol in checks:
            err = _rel(np.asarray(b), _np(a).reshape(np.shape(b)))
            assert err < tol, f"chain {c}: {what} differs from the restatement by {err:.3e}"


@pytest.mark.parametrize("name,C,N", [("smo", 3, 200), ("toy", 3, 200), ("vehicle", 3, 200), ("smo/traced", 3, 200), ("smo2", 3, 200), ("smo", 7, 257),
                                      ("smo", 2, 1024), ("smo", 1, 64)])
def test_every_chain_equals_the_single_chain_filter_and_the_restatement(name, C, N):
    """torch callables, a deterministic model (toy), two latent functions (vehicle), a traced model (the transition program against every
    chain's own reference) and an interface variable of two components (smo2: the general base measure with per-chain statistics)."""
    _check_chains_against_single_chains(name, C, N)


# ------------------------------------------------------------------------------------------ 5. Particle Gibbs, chain by chain
def _named2(out, n_int):
    st, iv, w, sst, obs, ll = out
    items = [("state_trace", st), ("weights", w), ("obs_trace", obs), ("log_likelihood", ll)]
    for i in range(n_int):
        items.append((f"int_var_trace[{i}]", iv[i]))
        items += [(f"suff_stats_trace[{i}][{j}]", sst[i][j]) for j in range(4)]
    return items


@pytest.mark.parametrize("per_chain_refs", [False, True])
@pytest.mark.parametrize("name", ["smo", "vehicle"])
def test_every_gibbs_chain_equals_algorithm2_and_the_restatement(name, per_chain_refs):
    from pgas_amd import random as prng

    pb = _problem(name, T=7)
    C, N, K, T = 3, 96, 4, 7
    n_int = len(pb.init_int_var_mean)
    keys = prng.split(SEED + 5, C)
    x0 = np.asarray(pb.X_true, dtype=np.float64).reshape(T, -1)
    iv0 = [np.asarray(v, dtype=np.float64).reshape(T, -1) for v in pb.int_var_true]
    xs = [x0 + 0.01 * c if per_chain_refs else x0 for c in range(C)]
    common = dict(N_samples=N, N_iterations=K, **{k: v for k, v in _args(pb, name).items() if k != "SSM"})
    alg = pgas_amd.MultiChainAlgorithm2(C, SSM=pb.ssm(pgas_amd.StateSpaceModel, torch), **common)
    got = alg(None, np.stack(xs) if per_chain_refs else x0, [np.stack([v] * C) for v in iv0] if per_chain_refs else iv0, keys=keys)
    assert got[0].shape == (C, T, K, x0.shape[1]) and got[2].shape == (C, T, K) and got[5].shape == (C, T, K)
    problems = []
    for c in range(C):
        one = pgas_amd.Algorithm2(SSM=pb.ssm(pgas_amd.StateSpaceModel, torch), **common)(keys[c], xs[c], iv0)

        def rands():
            key = prng.as_key(keys[c])
            while True:
                key, key_step = prng.split(key, 2)
                yield CanonRand(key_step, N)

        ref = mo.Algorithm2(SSM=pb.ssm(mo.StateSpaceModel, np), **common)(rands(), xs[c], iv0)
        for (what, a), (_, b), (_, r) in zip(_named2(got, n_int), _named2(one, n_int), _named2(ref, n_int)):
            a = a[c]
            assert a.shape == b.shape, (what, a.shape, b.shape)
            err = _rel(_np(b), _np(a))
            print(f"{name} chain {c} {what}: relative difference to Algorithm2 {err:.3e}, bit-equal {torch.equal(a, b)}")
            if not err <= 1e-12:
                problems.append(f"chain {c}: {what} differs from Algorithm2 by {err:.3e} > 1e-12")
            if what != "weights":
                err = _rel(np.asarray(r), _np(a).reshape(np.shape(r)))
                if not err < (1e-6 if what == "log_likelihood" else 1e-7):
                    problems.append(f"chain {c}: {what} differs from the restatement by {err:.3e}")
    assert not problems, problems
    rhat = pgas_amd.split_rhat(got[0].transpose(1, 2))   # (C, K, T, n_x): the documented way into the convergence check
    assert rhat.shape == (T, x0.shape[1])


# ------------------------------------------------------------------------------------------ 6. independence
def test_chains_are_independent_of_each_other():
    pb = _problem("smo", T=7)
    k = pgas_amd.random.split(SEED, 3)
    common = dict(N_samples=96, N_iterations=3, **_args(pb, "smo"))
    alg = pgas_amd.MultiChainAlgorithm2(4, **common)
    keys = [k[0], k[1], k[2], k[1]]

    def flat(out):
        return [a for _, a in _named2(out, 1)]

    fwd = flat(alg(None, pb.X_true, list(pb.int_var_true), keys=keys))
    rev = flat(alg(None, pb.X_true, list(pb.int_var_true), keys=keys[::-1]))
    for n, (a, b) in enumerate(zip(fwd, rev)):
        assert torch.equal(a, b.flip(0)), f"output {n}: reversing the keys does not reverse the chains"
        assert torch.equal(a[1], a[3]), f"output {n}: two chains with one key and one reference differ"
    assert not torch.equal(fwd[0][0][:, 1:], fwd[0][1][:, 1:]), "two chains with different keys agree"
    default = flat(alg(SEED, pb.X_true, list(pb.int_var_true)))
    split = flat(alg(None, pb.X_true, list(pb.int_var_true), keys=pgas_amd.random.split(SEED, 4)))
    assert all(torch.equal(a, b) for a, b in zip(default, split)), "the default keys are random.split(key, C)"


# ------------------------------------------------------------------------------------------ 7. graph replay
@pytest.mark.parametrize("name", ["smo", "vehicle"])
def test_chains_graph_replay_equals_eager_loop(name):
    pb = _problem(name, T=12)
    C, N = 3, 200
    keys = pgas_amd.random.split(SEED, C)
    _, ref_x, ref_iv, _, stacked = _references(pb, C, N)
    outs = []
    for mode in (False, True):
        traj, ivt, tr = pgas_amd.MultiChainAlgorithm3(C, N, **_args(pb, name))(keys, ref_x, ref_iv, stacked, return_traces=True, use_graph=mode)
        outs.append([traj, tr["state_trace"], tr["ancestor_trace"], tr["log_weights"], tr["idx"]] + list(ivt) + list(tr["int_var_trace"]))
    for n, (a, b) in enumerate(zip(*outs)):
        assert a.shape == b.shape and torch.equal(a, b), f"output {n} differs between the eager loop and the graph replay"


# ------------------------------------------------------------------------------------------ 8. no host round trip
def test_a_gibbs_iteration_of_all_chains_makes_no_host_round_trip():
    """One iteration (the conditional filter of every chain, launch by launch, then the trajectory statistics) with device synchronisation
    made an error (torch.cuda.set_sync_debug_mode): no .cpu() / .item() / blocking copy hides in it.  (The graph-replayed loop waits for
    its stream once, at its end, like Algorithm1's; the filter's final pgas_m_check reads the failure counter of the solves.)"""
    pb = _problem("smo", T=7)
    C, N = 3, 96
    alg = pgas_amd.MultiChainAlgorithm2(C, N, 3, **_args(pb, "smo"))
    c, dev = alg.cSMC, alg.cSMC.device
    _, ref_x, ref_iv, _, stacked = _references(pb, C, N)
    keys = pgas_amd.chains.keys_tensor(pgas_amd.random.split(SEED, C), dev)
    x = torch.as_tensor(ref_x, device=dev)
    iv = [torch.as_tensor(v, device=dev) for v in ref_iv]
    stats = [[torch.as_tensor(s, device=dev) for s in per] for per in stacked]
    warm = c(keys, x, iv, stats, use_graph=False)   # first call: allocations and uploads (those may synchronise)
    alg._trajectory_stats(warm[0], list(warm[1]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            x, iv = c(keys, x, iv, stats, use_graph=False)
            iv = list(iv)
            stats = alg._trajectory_stats(x, iv)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and all(bool(torch.isfinite(s).all()) for per in stats for s in per)


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refused_calls_leave_the_device_usable():
    pb = _problem("smo")
    C, N = 3, 200
    alg = pgas_amd.MultiChainAlgorithm3(C, N, **_args(pb, "smo"))
    _, ref_x, ref_iv, _, stacked = _references(pb, C, N)
    keys = pgas_amd.random.split(SEED, C)
    with pytest.raises(ValueError, match="keys"):
        alg(keys[:2], ref_x, ref_iv, stacked)
    with pytest.raises(ValueError, match="ref_state"):
        alg(keys, ref_x[:2], ref_iv, stacked)
    with pytest.raises(ValueError, match="ref_state"):
        alg(keys, ref_x[0], ref_iv, stacked)
    with pytest.raises(ValueError, match="ref_int_var"):
        alg(keys, ref_x, [v[:, :-1] for v in ref_iv], stacked)
    with pytest.raises(ValueError, match="ref_suff_stats"):
        alg(keys, ref_x, ref_iv, [[s[:2] for s in per] for per in stacked])
    with pytest.raises(ValueError, match="init_ref_state"):
        pgas_amd.MultiChainAlgorithm2(C, N, 3, **_args(pb, "smo"))(SEED, ref_x[:, :-1], list(pb.int_var_true))
    _check_chains_against_single_chains("smo", 2, 200)
