"""Predictive moments and log score reduced over the replicates inside the rollout kernel (pgas_amd.Rollout.predict, pgas_rollout_stats,
csrc/pgas_rollout_stats.hip.h) against the NumPy restatement of its defined order (tests/rollout_stats_numpy.py) applied to what
Rollout.__call__ itself returns -- which tests/test_gpu_rollout.py pins bit for bit to the canonical C oracle.  Comparisons are
np.array_equal unless stated.  Replicate p of a rollout does not depend on how many replicates the call has (its Philox particle counter
is p), so one materialised rollout of 2500 replicates per model is the cloud of every smaller P."""
import functools

import numpy as np
import pytest
import torch

import rollout_stats_numpy as rs
from common import canon, experiments, pgas_amd
from pgas_amd import chains as ch
from pgas_amd import random as prng
from pgas_amd._lib import PgasError
from test_gpu_rollout import MODELS, _draws, _np, _problem

pytestmark = pytest.mark.gpu

K = 3
PS = [1, 63, 64, 65, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2500]   # wave, register-row and block edges; B = 2 and a ragged B = 3
PS_EXACT = [1, 257, 1025]                                               # where every replicate's fma chain is restated with Fractions
PMAX = max(PS)
STREAM_OBS = 6


def _sim_for(pb, lik=None, obs=None):
    return pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov,
                            likelihood_fcn=pb.likelihood_fcn if lik is None else lik, observations=pb.observations if obs is None else obs)


@functools.lru_cache(maxsize=None)
def _sim(name):
    """A Rollout over the model's inputs with the model's likelihood and observations."""
    return _sim_for(_problem(name))


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(K, T, PMAX, nx): Rollout.__call__ with drawn x_0; computed once and never changed."""
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    c = _np(_sim(name)(As, Ss, keys, replicates=PMAX))
    c.setflags(write=False)
    return c


def _selector(H):
    H = np.atleast_2d(H)
    return bool(np.all((H == 0) | (H == 1)) and np.all(H.sum(axis=1) == 1))


def _want_moments(cloud, H):
    """Restated (sum, sumsq) (K, T, nx + ny) of a cloud (K, T, P, nx) under a 0/1 selector H (yhat = x @ H.T is exact)."""
    v = np.concatenate([cloud, cloud @ np.atleast_2d(H).T], axis=-1)   # (K, T, P, nx + ny)
    s1, s2 = rs.moments(np.moveaxis(v, 2, -1))
    return s1, s2


def _got(st):
    return np.concatenate([_np(st.x_sum), _np(st.y_sum)], axis=-1), np.concatenate([_np(st.x_sumsq), _np(st.y_sumsq)], axis=-1)


# ---- 1. moments = the restated reduction of Rollout.__call__'s own output -------------------------------------------------------------
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("name", MODELS)
def test_moments_equal_the_restated_reduction_of_the_materialised_rollout(name, P):
    pb = _problem(name)
    H = pb.likelihood_fcn.H
    assert _selector(H)
    keys, As, Ss = _draws(pb, K)
    sim = _sim(name)
    cloud = _cloud(name)[:, :, :P]
    want = _want_moments(cloud, H)
    drawn = sim.predict(As, Ss, keys, replicates=P)
    assert drawn.n == P and tuple(drawn.x_sum.shape) == (K, pb.T, pb.nx) and tuple(drawn.y_sumsq.shape) == (K, pb.T, H.shape[0])
    assert tuple(drawn.lpd.shape) == (K, pb.T)
    given = sim.predict(As, Ss, keys, replicates=P, init_state=cloud[:, 0].copy())
    for what, st in (("drawn x_0", drawn), ("given x_0", given)):
        got = _got(st)
        assert np.array_equal(got[0], want[0]), f"{what}: sums"
        assert np.array_equal(got[1], want[1]), f"{what}: sums of squares"
    # noise-free, a per-replicate x_0: against the noise-free Rollout.__call__
    x0 = cloud[:, 0].copy()
    free = _np(sim(As, replicates=P, init_state=x0))
    assert not np.array_equal(free, cloud) or pb.T == 1
    got = _got(sim.predict(As, replicates=P, init_state=x0))
    want = _want_moments(free, H)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "noise-free"


def test_shared_and_per_draw_initial_states():
    pb = _problem("smo")
    keys, As, Ss = _draws(pb, K)
    sim = _sim("smo")
    H = pb.likelihood_fcn.H
    for x0 in (pb.X_true[0].copy(), np.stack([pb.X_true[0] * (1.0 + 0.1 * k) for k in range(K)])):
        cloud = _np(sim(As, Ss, keys, replicates=300, init_state=x0))
        got = _got(sim.predict(As, Ss, keys, replicates=300, init_state=x0))
        want = _want_moments(cloud, H)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 2. measurement noise -------------------------------------------------------------------------------------------------------------
def _noise_lik(name):
    pb = _problem(name)
    H = pb.likelihood_fcn.H
    ny = H.shape[0]
    R = np.array([[0.04]]) if ny == 1 else np.array([[0.09, -0.021], [-0.021, 0.0049 + 0.16]])   # non-diagonal for ny = 2
    return pgas_amd.GaussianLikelihood(H, R)


@functools.lru_cache(maxsize=None)
def _noise_sim(name):
    return _sim_for(_problem(name), lik=_noise_lik(name))


def _obs_normals(keys, T, p0, P, ny):
    """e (K, T, P, ny) = oracle.canon.normals(seed_k, 6, t, p0, P, ny)."""
    return np.stack([np.stack([canon.normals(int(k), STREAM_OBS, t, p0, P, ny) for t in range(T)]) for k in keys])


def _want_noisy(cloud, lik, e):
    yh = rs.predicted_obs(cloud, lik.H, lik.LR, e)
    return rs.moments(np.moveaxis(np.concatenate([cloud, yh], axis=-1), 2, -1))


@pytest.mark.parametrize("P", PS_EXACT)
@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_measurement_noise_is_the_restated_fma_chain_on_the_obs_stream(name, P):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    lik, sim = _noise_lik(name), _noise_sim(name)
    assert lik.ny == 1 or lik.LR[1, 0] != 0.0
    cloud = _cloud(name)[:, :, :P]
    e = _obs_normals(keys, pb.T, 0, P, lik.ny)
    want = _want_noisy(cloud, lik, e)
    st = sim.predict(As, Ss, keys, replicates=P, observation_noise=True, log_score=False)
    assert st.lpd is None
    got = _got(st)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    clean = _got(sim.predict(As, Ss, keys, replicates=P, log_score=False))
    nx = pb.nx
    assert np.array_equal(clean[0][..., :nx], got[0][..., :nx]) and not np.array_equal(clean[0][..., nx:], got[0][..., nx:])


@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_p0_is_the_matching_slice_of_a_larger_rollout(name):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    lik, sim = _noise_lik(name), _noise_sim(name)
    p0, P = 300, 257
    cloud = _cloud(name)[:, :, p0:p0 + P]
    want = _want_noisy(cloud, lik, _obs_normals(keys, pb.T, p0, P, lik.ny))
    eng = sim.engine
    s1, s2, lpd = eng.rollout_stats(As, Ss, ch.keys_tensor(keys, eng.device), P, p0, None, 0, True, False)
    assert lpd is None
    assert np.array_equal(_np(s1), want[0]) and np.array_equal(_np(s2), want[1])


# ---- 3. log score ---------------------------------------------------------------------------------------------------------------------
def _want_lpd(cloud, lik, y):
    """cloud (K, T, P, nx), y (T, ny) -> (K, T)."""
    ll = rs.loglik(np.moveaxis(cloud, 2, 1), y[None, None], lik.H, lik.LRinv, lik.cR)   # x (K, P, T, nx), y rows along T
    return rs.lpd(np.moveaxis(ll, 1, -1), y, canon.det_exp, canon.det_log)


@pytest.mark.parametrize("P", PS_EXACT)
@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_log_score_equals_the_restated_definition(name, P):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    lik = pb.likelihood_fcn
    y = np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1)
    cloud = _cloud(name)[:, :, :P]
    want = _want_lpd(cloud, lik, y)
    assert np.isfinite(want).all()
    st = _sim(name).predict(As, Ss, keys, replicates=P)
    assert np.array_equal(_np(st.lpd), want)
    # lpd_dev = NULL: no log score, the moments unchanged
    off = _sim(name).predict(As, Ss, keys, replicates=P, log_score=False)
    assert off.lpd is None
    for a, b in zip(_got(st), _got(off)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_nan_and_far_observations(name):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    lik = pb.likelihood_fcn
    P = 257
    y = np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1).copy()
    sigma = np.sqrt(np.diag(lik.R))
    y[3, -1] = np.nan                       # one component of one row
    y[5] = y[5] + 1e4 * sigma               # 10^4 sigma away
    y[7, 0] = 1e200                         # the quadratic form overflows: every density is 0
    sim = _sim_for(pb, obs=y)
    base = _np(_sim(name).predict(As, Ss, keys, replicates=P).lpd)
    got = _np(sim.predict(As, Ss, keys, replicates=P).lpd)
    assert np.isnan(got[:, 3]).all()
    assert not np.isnan(got[:, 5]).any() and (np.isfinite(got[:, 5]) | (got[:, 5] == -np.inf)).all()
    assert (got[:, 7] == -np.inf).all()
    rest = [t for t in range(pb.T) if t not in (3, 5, 7)]
    assert np.array_equal(got[:, rest], base[:, rest]) and np.isfinite(base).all()
    want = _want_lpd(_cloud(name)[:, :, :P], lik, y)
    assert np.array_equal(got, want, equal_nan=True)


def test_non_selector_H_against_plain_numpy_on_the_cloud():
    pb = _problem("smo")
    keys, As, Ss = _draws(pb, K)
    H = np.array([[0.3, -1.7]])
    lik = pgas_amd.GaussianLikelihood(H, pb.likelihood_fcn.R)
    sim = _sim_for(pb, lik=lik)
    y = np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, 1)
    for P in (257, 1025):
        cloud = _cloud("smo")[:, :, :P]
        st = sim.predict(As, Ss, keys, replicates=P)
        yh = cloud @ H.T                                             # (K, T, P, 1)
        ll = lik.cR - 0.5 * ((y[None, :, None, :] - yh)[..., 0] / lik.LR[0, 0]) ** 2
        m = ll.max(axis=-1, keepdims=True)
        want_lpd = (m[..., 0] + np.log(np.exp(ll - m).sum(axis=-1))) - np.log(P)
        got_y, got_lpd = _np(st.y_sum)[..., 0], _np(st.lpd)
        want_y = yh[..., 0].sum(axis=-1)
        print(f"P = {P}: max rel. error y_sum {np.max(np.abs(got_y - want_y) / np.abs(want_y)):.3e}, lpd {np.max(np.abs(got_lpd - want_lpd) / np.abs(want_lpd)):.3e}")
        np.testing.assert_allclose(got_y, want_y, rtol=1e-13, atol=0)
        np.testing.assert_allclose(got_lpd, want_lpd, rtol=1e-13, atol=0)


# ---- 4. independence across draws -----------------------------------------------------------------------------------------------------
def _all(st):
    return [_np(t) for t in (st.x_sum, st.x_sumsq, st.y_sum, st.y_sumsq, st.lpd)]


def test_draws_are_independent_of_their_order_and_equal_inputs_give_equal_rows():
    pb = _problem("smo")
    Kd, P = 5, 1500
    keys, As, Ss = _draws(pb, Kd)
    sim = _sim("smo")
    fwd = _all(sim.predict(As, Ss, keys, replicates=P, observation_noise=True))
    rev = _all(sim.predict(As[::-1].copy(), Ss[::-1].copy(), keys[::-1], replicates=P, observation_noise=True))
    for a, b in zip(fwd, rev):
        assert np.array_equal(a[::-1], b)
    idx = [0, 3, 0, 3, 1]
    dup = _all(sim.predict(As[idx], Ss[idx], [keys[i] for i in idx], replicates=P, observation_noise=True))
    for a, d in zip(fwd, dup):
        assert np.array_equal(d[0], d[2]) and np.array_equal(d[1], d[3]) and np.array_equal(d[0], a[0]) and np.array_equal(d[4], a[1])
        assert not np.array_equal(d[0], d[1])


def test_more_draws_than_the_gpu_holds_at_once():
    Kd, P, T = 2000, 64, 8
    pb = experiments.smo_pgas(T=T)
    keys, As, Ss = _draws(pb, Kd)
    As = np.stack([As[0] * (1.0 + 1e-4 * k) for k in range(Kd)])
    Ss = np.stack([Ss[0] * (1.0 + 1e-3 * k) for k in range(Kd)])
    sim = _sim_for(pb)
    got = _all(sim.predict(As, Ss, keys, replicates=P))
    assert got[0].shape == (Kd, T, 2) and got[4].shape == (Kd, T)
    for k in (0, 1, 2, Kd - 3, Kd - 2, Kd - 1):
        one = _all(sim.predict(As[k:k + 1], Ss[k:k + 1], keys[k:k + 1], replicates=P))
        for a, b in zip(got, one):
            assert np.array_equal(a[k], b[0]), f"draw {k}"
    cloud = _np(sim(As[-2:], Ss[-2:], keys[-2:], replicates=P))
    want = _want_moments(cloud, pb.likelihood_fcn.H)
    assert np.array_equal(np.concatenate([got[0], got[2]], axis=-1)[-2:], want[0])


# ---- 5. no host round trip ------------------------------------------------------------------------------------------------------------
def test_predict_makes_no_host_round_trip():
    pb = experiments.smo_pgas(T=16)
    Kd = 4
    keys, As, Ss = _draws(pb, Kd)
    sim = _sim_for(pb)
    dev = sim.engine.device
    kd = ch.keys_tensor(keys, dev)
    Ad, Sd = torch.as_tensor(As, device=dev), torch.as_tensor(Ss, device=dev)
    x0 = torch.as_tensor(np.repeat(pb.X_true[:1], Kd, axis=0), device=dev)
    calls = [lambda: sim.predict(Ad, Sd, kd, replicates=1500, observation_noise=True), lambda: sim.predict(Ad, Sd, kd, replicates=3, init_state=x0),
             lambda: sim.predict(Ad, init_state=x0, log_score=False)]
    warm = [c() for c in calls]   # allocations may synchronise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        for u, v in zip((a.x_sum, a.x_sumsq, a.y_sum, a.y_sumsq), (b.x_sum, b.x_sumsq, b.y_sum, b.y_sumsq)):
            assert torch.equal(u, v) and bool(torch.isfinite(u).all())
        assert (a.lpd is None) == (b.lpd is None) and (a.lpd is None or torch.equal(a.lpd, b.lpd))


# ---- 6. predict leaves the context as it was ------------------------------------------------------------------------------------------
def test_predict_leaves_sweeps_and_the_plain_rollout_as_they_were():
    pb = _problem("smo")
    Cn, N = 3, 200
    keys, As, Ss = _draws(pb, Cn)
    refs = np.stack([pb.X_true * (1.0 + 0.01 * c) for c in range(Cn)])
    chs = ch.condSequentialMonteCarloChains(Cn, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    eng, dev = chs.engine, chs.device
    Sd = torch.as_tensor(Ss[1], device=dev)
    rk, rA, rS = _draws(pb, 4)

    def sweeps(set_params):
        if set_params:
            t1 = chs.single(4242, pb.X_true, As[1], Sd).clone()
            tc = chs(keys, refs, As, Ss).clone()
        else:   # the parameters packed before predict must still be there
            t1 = eng.sweep(prng.as_key(4242), torch.as_tensor(pb.X_true, device=dev)).clone()
            tc = eng.chains_sweep(ch.keys_tensor(keys, dev), torch.as_tensor(refs, device=dev)).clone()
        single = [t.clone() for t in eng.traces()[:3]]
        return [t1, tc] + single + [t.clone() for t in chs.traces()]

    plain = chs.rollout(rA, rS, rk, replicates=100).clone()
    before = sweeps(True)
    views = list(eng.traces()[:3]) + list(chs.traces())
    st = chs.predict(rA * 1.3, rS * 2.0, [k + 5 for k in rk], replicates=1300, observation_noise=True)
    assert tuple(st.x_sum.shape) == (4, pb.T, pb.nx) and bool(torch.isfinite(st.lpd).all())
    single_ctx = chs.single.predict(rA * 1.3, rS * 2.0, [k + 5 for k in rk], replicates=1300, observation_noise=True)
    assert torch.equal(single_ctx.y_sumsq, st.y_sumsq) and torch.equal(single_ctx.lpd, st.lpd)
    for a, b in zip(before[2:], views):
        assert torch.equal(a, b), "predict wrote into a trace buffer"
    for a, b in zip(before, sweeps(False)):
        assert torch.equal(a, b), "sweeps after predict (parameters not set again) differ"
    assert torch.equal(chs.rollout(rA, rS, rk, replicates=100), plain)
    # in-sample: the training context's own observations and likelihood
    want = _sim("smo").predict(rA, rS, rk, replicates=100)
    got = chs.predict(rA, rS, rk, replicates=100)
    assert torch.equal(got.lpd, want.lpd) and torch.equal(got.y_sum, want.y_sum)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_clean_and_leave_the_context_usable():
    pb = experiments.smo_pgas(T=16)
    Kd = 2
    keys, As, Ss = _draws(pb, Kd)
    sim = _sim_for(pb)
    eng = sim.engine
    good = _all(sim.predict(As, Ss, keys, replicates=10, observation_noise=True))
    Ad, Sd, kd = torch.as_tensor(As, device=eng.device), torch.as_tensor(Ss, device=eng.device), ch.keys_tensor(keys, eng.device)
    out = [torch.empty((Kd, 16, 3), dtype=torch.float64, device=eng.device) for _ in range(3)]
    x0 = torch.zeros(2, dtype=torch.float64, device=eng.device)
    LR = np.ascontiguousarray(eng.LR)
    PGAS_E_ARG = -1

    def call(Kc, P, seeds=kd, S=Sd, mode=0, xs=None, noise=False):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = eng.lib.pgas_rollout_stats(eng._h, Kc, P, 0, p(seeds), Ad.data_ptr(), p(S), p(xs), mode, LR.ctypes.data if noise else None,
                                        out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), eng._stream())
        return rc, eng.lib.pgas_last_error(eng._h).decode()

    for args, msg in [((Kd, 0), "P = 0"), ((Kd, (1 << 20) + 1), "P = 1048577"), ((0, 10), "K = 0"), ((Kd, 10, None, None), "needs seeds"),
                      ((Kd, 10, kd, None), "go together"), ((Kd, 10, kd, Sd, 2), "without x0"), ((Kd, 1, None, None, 1, x0, True), "measurement noise")]:
        rc, err = call(*args)
        assert rc == PGAS_E_ARG and msg in err, (args, rc, err)
        for a, b in zip(_all(sim.predict(As, Ss, keys, replicates=10, observation_noise=True)), good):
            assert np.array_equal(a, b), f"predict after refusing {args}"
    # the host layer refuses from shapes alone
    for kw, msg in [(dict(replicates=0), "replicates"), (dict(replicates=(1 << 20) + 1), "replicates"), (dict(keys=None), "needs keys")]:
        with pytest.raises(ValueError, match=msg):
            sim.predict(As, Ss, **{"keys": keys, "replicates": 10, **kw})
    with pytest.raises(ValueError, match="observation_noise needs keys"):
        sim.predict(As, init_state=np.zeros(2), observation_noise=True)
    bare = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
    with pytest.raises(ValueError, match="needs observations"):
        bare.predict(As, Ss, keys, replicates=10, log_score=True)
    st = bare.predict(As, Ss, keys, replicates=10)   # no observations: no log score by default; the unit likelihood observes x[0]
    assert st.lpd is None and torch.equal(st.y_sum[..., 0], st.x_sum[..., 0])
    # a context of more than one segment of particles has no one-workgroup variant
    big = pgas_amd.condSequentialMonteCarlo(5000, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    with pytest.raises(PgasError, match="no small variant"):
        big.predict(As, Ss, keys, replicates=10)
    traj = big(77, pb.X_true, As[0], Sd[0])
    assert bool(torch.isfinite(traj).all())
    for a, b in zip(_all(sim.predict(As, Ss, keys, replicates=10, observation_noise=True)), good):
        assert np.array_equal(a, b)
