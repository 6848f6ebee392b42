"""Open-loop simulation under K parameter draws in one launch (pgas_amd.Rollout, csrc/pgas_rollout.hip.h) against the canonical C oracle.

The reference propagates particle i from its own previous state (quirk Q1), so particles 0 .. N - 2 of a conditional-SMC sweep are free
noisy rollouts of the model: CanonModel.sweep(key_k, ..., A_k, S_k)[1][:, :P] with N = P + 1 is the oracle of P noisy replicates, and
iterating step(debug=True)["aux"] is the oracle of the noise-free rollout.  Every equality is bit for bit (np.array_equal)."""
import functools

import numpy as np
import pytest
import torch

from common import canon_model, experiments, pgas_amd
from pgas_amd import chains as ch
from pgas_amd import random as prng
from pgas_amd._lib import PgasError

pytestmark = pytest.mark.gpu

MODELS = ("smo", "toy", "emps27", "veh27", "emps")


@functools.lru_cache(maxsize=None)
def _problem(name):
    return {
        "smo": lambda: experiments.smo_pgas(T=40),
        "toy": lambda: experiments.toy(T=40),
        "emps27": lambda: experiments.emps_pgas(T=16, M=27),
        "veh27": lambda: experiments.vehicle_pgas(T=30, M=27),
        "emps": lambda: experiments.emps_pgas(T=10),     # M = 729: a 23 KB coefficient tensor in LDS
    }[name]()


def _draws(pb, K):
    """K different (key, A, S): perturbations of the problem's posterior-mean parameters; S stays positive definite (scaled)."""
    A, S = experiments.initial_params(pb)
    keys = [prng.key(1000 + 7919 * k) for k in range(K)]
    As = np.stack([A * (1.0 + 0.02 * k) for k in range(K)])
    Ss = np.stack([S * (1.0 + 0.1 * k) for k in range(K)])
    return keys, As, Ss


@functools.lru_cache(maxsize=None)
def _rollout(name):
    pb = _problem(name)
    return pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)


def _np(t):
    return t.cpu().numpy()


# ---- 1. noisy rollout = the oracle's particle cloud -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 255, 256, 257, 512, 513, 1024])
@pytest.mark.parametrize("name", MODELS)
def test_noisy_rollout_equals_the_particle_cloud_of_the_oracle_sweep(name, P):
    pb = _problem(name)
    K = 3
    keys, As, Ss = _draws(pb, K)
    cm = canon_model(pb, P + 1)
    L0 = np.linalg.cholesky(pb.init_state_cov)
    want = np.stack([cm.sweep(keys[k], pb.X_true, As[k], *cm.chol_parts_dev(Ss[k]), pb.init_state_mean, L0)[1][:, :P] for k in range(K)])
    want = want.reshape(K, pb.T, P, pb.nx)
    sim = _rollout(name)
    drawn = _np(sim(As, Ss, keys, replicates=P))
    assert drawn.shape == (K, pb.T, P, pb.nx)
    given = _np(sim(As, Ss, keys, replicates=P, init_state=want[:, 0]))
    for t in range(pb.T):
        assert np.array_equal(drawn[:, t], want[:, t]), f"drawn x_0: step {t}"
        assert np.array_equal(given[:, t], want[:, t]), f"given x_0: step {t}"
    assert not np.array_equal(want[0], want[1])


# ---- 2. noise-free rollout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 257])
@pytest.mark.parametrize("name", MODELS)
def test_noise_free_rollout_equals_the_iterated_transition_mean(name, P):
    pb = _problem(name)
    K, T, nx = 2, pb.T, pb.nx
    keys, As, Ss = _draws(pb, K)
    cm = canon_model(pb, P)
    x0 = pb.X_true[0][None, :] + 1e-3 * (np.arange(P)[:, None] + 1.0) / P * np.array([1.0, -0.5])[None, :nx]
    want = np.empty((K, T, P, nx))
    for k in range(K):
        LS, LSinv, cS = cm.chol_parts_dev(Ss[k])
        x = x0
        want[k, 0] = x
        for t in range(1, T):
            x = cm.step(t, 7, x, None, As[k], LS, LSinv, cS, pb.X_true[t], debug=True)[3]["aux"].copy()
            want[k, t] = x
    sim = _rollout(name)
    got = _np(sim(As, replicates=P, init_state=np.repeat(x0[None], K, axis=0)))
    for t in range(T):
        assert np.array_equal(got[:, t], want[:, t]), f"step {t}"
    one = _np(sim(As, init_state=x0[0]))                         # shared (nx) initial state, replicates = 1
    assert one.shape == (K, T, 1, nx) and np.array_equal(one[:, :, 0], got[:, :, 0])
    per_draw = _np(sim(As, init_state=np.repeat(x0[:1], K, axis=0)))   # (K, nx)
    assert np.array_equal(per_draw, one)
    # the same two modes with P noisy replicates (P = 257: two register rows, the second ragged) are the per-replicate mode -- the one
    # test_noisy_rollout_equals_the_particle_cloud_of_the_oracle_sweep checks -- on the broadcast state; the draws' rows differ when P > 1
    per = x0[[0, P - 1]]
    for x0_mode, full in ((per[0], np.broadcast_to(per[0], (K, P, nx))), (per, np.broadcast_to(per[:, None, :], (K, P, nx)))):
        each = _np(sim(As, Ss, keys, replicates=P, init_state=np.ascontiguousarray(full)))
        assert np.array_equal(_np(sim(As, Ss, keys, replicates=P, init_state=x0_mode)), each), f"init_state {np.shape(x0_mode)}"
        assert P == 1 or not np.array_equal(each[:, 1, 0], each[:, 1, 1])


# ---- 3. against the existing device entry point ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smo", "emps27"])
def test_noise_free_rollout_equals_dependent_aux_states_launches(name):
    pb = _problem(name)
    P = 300
    A, S = experiments.initial_params(pb)
    csmc = pgas_amd.condSequentialMonteCarlo(P, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    eng = csmc.engine
    x0 = pb.X_true[0][None, :] + 1e-3 * np.arange(P)[:, None] / P * np.array([1.0, -0.5])[None, : pb.nx]
    got = _np(csmc.rollout(A[None], replicates=P, init_state=x0[None]))
    eng.set_params(A, torch.as_tensor(S, device=eng.device))
    x = torch.as_tensor(x0, device=eng.device)
    assert np.array_equal(got[0, 0], x0)
    for t in range(1, pb.T):
        x = eng.aux_states(x, t)
        assert np.array_equal(got[0, t], _np(x)), f"step {t}"


# ---- 4. independence and chunking -----------------------------------------------------------------------------------------------------
def test_draws_are_independent_of_their_order_and_equal_inputs_give_equal_slices():
    pb = _problem("smo")
    K, P = 5, 70
    keys, As, Ss = _draws(pb, K)
    sim = _rollout("smo")
    fwd = _np(sim(As, Ss, keys, replicates=P))
    rev = _np(sim(As[::-1].copy(), Ss[::-1].copy(), keys[::-1], replicates=P))
    assert np.array_equal(fwd[::-1], rev)
    idx = [0, 3, 0, 3, 1]
    dup = _np(sim(As[idx], Ss[idx], [keys[i] for i in idx], replicates=P))
    assert np.array_equal(dup[0], dup[2]) and np.array_equal(dup[1], dup[3]) and np.array_equal(dup[0], fwd[0]) and np.array_equal(dup[4], fwd[1])
    assert not np.array_equal(dup[0], dup[1])


def test_2500_replicates_equal_three_explicit_calls_through_p0():
    pb = experiments.smo_pgas(T=16)
    K = 2
    keys, As, Ss = _draws(pb, K)
    sim = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
    whole = _np(sim(As, Ss, keys, replicates=2500))
    assert whole.shape == (K, 16, 2500, 2)
    eng = sim.engine
    seeds = ch.keys_tensor(keys, eng.device)
    for p0, n in ((0, 1024), (1024, 1024), (2048, 452)):
        part = _np(eng.rollout(As, Ss, seeds, n, p0))
        assert np.array_equal(whole[:, :, p0:p0 + n], part), f"p0 = {p0}"
    # a given per-replicate x_0 is chunked with its replicates
    x0 = whole[:, 0].copy()
    assert np.array_equal(_np(sim(As, Ss, keys, replicates=2500, init_state=x0)), whole)


def test_more_draws_than_the_gpu_holds_at_once():
    K, P, T = 2000, 64, 16
    pb = experiments.smo_pgas(T=T)
    keys, As, Ss = _draws(pb, K)
    As = np.stack([As[0] * (1.0 + 1e-4 * k) for k in range(K)])
    Ss = np.stack([Ss[0] * (1.0 + 1e-3 * k) for k in range(K)])
    sim = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
    got = sim(As, Ss, keys, replicates=P)
    assert tuple(got.shape) == (K, T, P, 2)
    for k in (0, 1, 2, K - 3, K - 2, K - 1):
        one = sim(As[k:k + 1], Ss[k:k + 1], keys[k:k + 1], replicates=P)
        assert np.array_equal(_np(got[k]), _np(one[0])), f"draw {k}"


# ---- 5. a rollout leaves the context as it was ----------------------------------------------------------------------------------------
def test_rollout_leaves_single_chain_and_chains_state_as_it_was():
    pb = _problem("smo")
    Cn, N = 3, 200
    keys, As, Ss = _draws(pb, Cn)
    refs = np.stack([pb.X_true * (1.0 + 0.01 * c) for c in range(Cn)])
    chs = ch.condSequentialMonteCarloChains(Cn, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    eng, dev = chs.engine, chs.device
    Sd = torch.as_tensor(Ss[1], device=dev)

    def sweeps(set_params):
        if set_params:
            t1 = chs.single(4242, pb.X_true, As[1], Sd).clone()
            tc = chs(keys, refs, As, Ss).clone()
        else:   # the parameters packed before the rollout must still be there
            t1 = eng.sweep(prng.as_key(4242), torch.as_tensor(pb.X_true, device=dev)).clone()
            tc = eng.chains_sweep(ch.keys_tensor(keys, dev), torch.as_tensor(refs, device=dev)).clone()
        single = [t.clone() for t in eng.traces()[:3]]
        return [t1, tc] + single + [t.clone() for t in chs.traces()]

    before = sweeps(True)
    views = list(eng.traces()[:3]) + list(chs.traces())
    rk, rA, rS = _draws(pb, 4)
    sim = chs.rollout(rA * 1.3, rS * 2.0, [k + 5 for k in rk], replicates=100)
    assert tuple(sim.shape) == (4, pb.T, 100, pb.nx) and bool(torch.isfinite(sim).all())
    for a, b in zip(before[2:], views):
        assert torch.equal(a, b), "a rollout wrote into a trace buffer"
    for a, b in zip(before, sweeps(False)):
        assert torch.equal(a, b), "sweeps after a rollout (parameters not set again) differ"
    for a, b in zip(before, sweeps(True)):
        assert torch.equal(a, b)


# ---- 6. no host round trip ------------------------------------------------------------------------------------------------------------
def test_rollouts_make_no_host_round_trip():
    pb = experiments.smo_pgas(T=16)
    K = 4
    keys, As, Ss = _draws(pb, K)
    sim = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
    dev = sim.engine.device
    kd = ch.keys_tensor(keys, dev)
    Ad, Sd = torch.as_tensor(As, device=dev), torch.as_tensor(Ss, device=dev)
    x0 = torch.as_tensor(np.repeat(pb.X_true[:1], K, axis=0), device=dev)
    warm = [sim(Ad, Sd, kd, replicates=1500), sim(Ad, Sd, kd, replicates=3, init_state=x0), sim(Ad, init_state=x0)]   # allocations may synchronise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [sim(Ad, Sd, kd, replicates=1500), sim(Ad, Sd, kd, replicates=3, init_state=x0), sim(Ad, init_state=x0)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_clean_and_leave_the_context_usable():
    pb = experiments.smo_pgas(T=16)
    K = 2
    keys, As, Ss = _draws(pb, K)
    sim = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
    eng = sim.engine
    good = sim(As, Ss, keys, replicates=10).clone()
    Ad, Sd, kd = torch.as_tensor(As, device=eng.device), torch.as_tensor(Ss, device=eng.device), ch.keys_tensor(keys, eng.device)
    out = torch.empty((K, 16, 1025, 2), dtype=torch.float64, device=eng.device)
    PGAS_E_ARG = -1

    def call(Kc, P, seeds=kd, S=Sd, mode=0):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = eng.lib.pgas_rollout(eng._h, Kc, P, 0, p(seeds), Ad.data_ptr(), p(S), None, mode, out.data_ptr(), eng._stream())
        return rc, eng.lib.pgas_last_error(eng._h).decode()

    for args, msg in [((K, 1025), "P = 1025"), ((0, 10), "K = 0"), ((K, 0), "P = 0"), ((K, 10, None, None), "needs seeds"), ((K, 10, kd, None), "go together"),
                      ((K, 10, kd, Sd, 2), "without x0")]:
        rc, err = call(*args)
        assert rc == PGAS_E_ARG and msg in err, (args, rc, err)
        assert torch.equal(sim(As, Ss, keys, replicates=10), good), f"rollout after refusing {args}"
    with pytest.raises(PgasError, match="P = 1025"):
        eng.rollout(Ad, Sd, kd, 1025)
    # a context of more than one segment of particles has no one-workgroup variant
    big = pgas_amd.condSequentialMonteCarlo(5000, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    with pytest.raises(PgasError, match="no small variant"):
        big.rollout(As, Ss, keys, replicates=10)
    traj = big(77, pb.X_true, As[0], Sd[0])
    assert bool(torch.isfinite(traj).all())
