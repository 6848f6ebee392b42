"""Predictive CDF counts inside the rollout kernel (pgas_amd.Rollout.cdf, pgas_rollout_cdf, csrc/pgas_rollout_cdf.hip.h, DESIGN.md section
19) against the NumPy restatement (tests/rollout_cdf_numpy.py) applied to what Rollout.__call__ itself returns -- which
tests/test_gpu_rollout.py pins bit for bit to the canonical C oracle.  Every comparison with the restatement is np.array_equal.  Replicate
p of a rollout does not depend on how many replicates the call has, so one materialised rollout of 2500 replicates per model (the one of
tests/test_gpu_rollout_stats.py) is the cloud of every smaller P, and its value channels are formed once.  Independent of the
restatement: with A = 0 the pooled counts are binomial with a known probability."""
import functools

import numpy as np
import pytest
import torch

import rollout_cdf_numpy as rc
from common import experiments, pgas_amd
from pgas_amd import chains as ch
from pgas_amd import random as prng
from pgas_amd._lib import PgasError
from test_gpu_rollout import _draws, _np, _problem
from test_gpu_rollout_stats import PMAX, PS, K, _cloud, _noise_lik, _noise_sim, _sim_for
from test_rollout_cdf_host import TAUS, binomial_z

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")


@functools.lru_cache(maxsize=None)
def _values(name, noise):
    """(K, T, PMAX, nx + ny): the value channels of the model's cloud under the noise likelihood, with or without measurement noise;
    computed once and never changed."""
    pb = _problem(name)
    keys, _, _ = _draws(pb, K)
    lik = _noise_lik(name)
    cloud = _cloud(name)
    e = rc.obs_normals(keys, pb.T, 0, PMAX, lik.ny) if noise else None
    v = rc.channels(cloud, lik.H, lik.LR if noise else None, e)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _thresholds(name, J):
    """threshold_grid of the noisy cloud's pooled moments: J = 16 spans +-2 sigma, J = 1 sits at -0.5 sigma, so counts are neither 0 nor P."""
    v = _values(name, True)
    flat = np.moveaxis(v, 1, 0).reshape(v.shape[1], -1, v.shape[-1])   # (T, K PMAX, nv)
    thr = pgas_amd.threshold_grid(torch.as_tensor(flat.mean(axis=1)), torch.as_tensor(flat.std(axis=1)), J, width=2.0 if J > 1 else 0.5).numpy()
    thr.setflags(write=False)
    return thr


# ---- 1. counts = the restated counts of Rollout.__call__'s own output -------------------------------------------------------------------
@pytest.mark.parametrize("name,P", [(n, P) for n in ("smo", "toy", "veh27") for P in PS] + [("emps", 257)])
def test_counts_equal_the_restated_counts_of_the_materialised_rollout(name, P):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    sim = _noise_sim(name)
    nv = pb.nx + _noise_lik(name).ny
    for J in (1, 16):
        thr = _thresholds(name, J)
        for noise in (False, True):
            want = rc.counts(_values(name, noise)[:, :, :P], thr)
            res = sim.cdf(As, Ss, keys, replicates=P, thresholds=thr, observation_noise=noise)
            got = _np(res.count)
            assert res.n == P and got.dtype == np.int32 and got.shape == (K, pb.T, nv, J)
            assert np.array_equal(_np(res.thresholds), thr)
            assert np.array_equal(got, want), f"J = {J}, noise = {noise}"
            if J == 16 and P >= 255:
                assert ((want > 0) & (want < P)).mean() > 0.5   # the grid sits inside the cloud
    clean, noisy = rc.counts(_values(name, False)[:, :, :P], thr), rc.counts(_values(name, True)[:, :, :P], thr)
    assert np.array_equal(clean[:, :, :pb.nx], noisy[:, :, :pb.nx]) and (P < 255 or not np.array_equal(clean, noisy))


def test_drawn_shared_per_draw_and_per_replicate_initial_states():
    pb = _problem("smo")
    keys, As, Ss = _draws(pb, K)
    sim, lik, thr = _noise_sim("smo"), _noise_lik("smo"), _thresholds("smo", 16)
    P = 300
    each = _cloud("smo")[:, 0, :P].copy()
    for x0 in (None, pb.X_true[0].copy(), np.stack([pb.X_true[0] * (1.0 + 0.1 * k) for k in range(K)]), each):
        cloud = _np(sim(As, Ss, keys, replicates=P, init_state=x0))
        want = rc.rollout_counts(cloud, lik, thr, keys)
        got = _np(sim.cdf(As, Ss, keys, replicates=P, init_state=x0, thresholds=thr, observation_noise=True).count)
        assert np.array_equal(got, want)
    # noise-free, a per-replicate x_0
    free = _np(sim(As, replicates=P, init_state=each))
    got = _np(sim.cdf(As, replicates=P, init_state=each, thresholds=thr).count)
    assert np.array_equal(got, rc.rollout_counts(free, lik, thr))


@pytest.mark.parametrize("P", [1, 300, 1500])
def test_a_record_of_one_row(P):
    pb = experiments.smo_pgas(T=1)
    keys, As, Ss = _draws(_problem("smo"), K)
    lik = _noise_lik("smo")
    sim = _sim_for(pb, lik=lik)
    cloud = _np(sim(As, Ss, keys, replicates=P))
    v = rc.channels(cloud, lik.H)
    thr = np.sort(np.concatenate([v[0, :, :3].transpose(0, 2, 1), v.mean(axis=(0, 2))[:, :, None]], axis=-1), axis=-1)[:, :, :min(4, P + 1)]
    got = _np(sim.cdf(As, Ss, keys, replicates=P, thresholds=thr).count)
    assert got.shape == (K, 1, 3, thr.shape[-1]) and np.array_equal(got, rc.counts(v, thr))


# ---- 2. special thresholds ----------------------------------------------------------------------------------------------------------------
def test_ties_nan_and_infinite_thresholds_and_monotone_counts():
    name, P = "veh27", 1300
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    sim = _noise_sim(name)
    v = _values(name, False)[:, :, :P]                       # noise-free channels: a threshold can equal a value
    nv = v.shape[-1]
    thr = np.empty((pb.T, nv, 6))
    thr[..., 0] = v[0, :, 5]                                  # the value of replicate 5 of draw 0: it counts itself
    thr[..., 1] = np.nextafter(v[0, :, 5], -INF)              # one ulp below: it does not
    thr[..., 2], thr[..., 3], thr[..., 4] = NAN, INF, -INF
    thr[..., 5] = v[1, :, 700]                                # a replicate of the second block
    got = _np(sim.cdf(As, Ss, keys, replicates=P, thresholds=thr).count)
    assert np.array_equal(got, rc.counts(v, thr))
    assert (got[0, ..., 0] - got[0, ..., 1] >= 1).all() and (got[1, ..., 5] >= 1).all()
    assert (got[..., 2] == 0).all() and (got[..., 3] == P).all() and (got[..., 4] == 0).all()
    up = np.sort(_thresholds(name, 16), axis=-1)
    mono = _np(sim.cdf(As, Ss, keys, replicates=P, thresholds=up, observation_noise=True).count)
    assert (np.diff(mono, axis=-1) >= 0).all() and mono.min() >= 0 and mono.max() <= P


@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_calls_with_p0_add_up_to_the_one_call(name):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    sim, thr = _noise_sim(name), _thresholds(name, 16)
    eng = sim.engine
    kd = ch.keys_tensor(keys, eng.device)
    whole = sim.cdf(As, Ss, keys, replicates=PMAX, thresholds=thr, observation_noise=True).count
    parts = [eng.rollout_cdf(As, Ss, kd, min(1024, PMAX - p0), p0, None, 0, True, thr) for p0 in (0, 1024, 2048)]
    assert torch.equal(parts[0] + parts[1] + parts[2], whole)
    for p0, part in zip((0, 1024, 2048), parts):
        assert np.array_equal(_np(part), rc.counts(_values(name, True)[:, :, p0:p0 + 1024], thr)), f"p0 = {p0}"


# ---- 3. batch behaviour -------------------------------------------------------------------------------------------------------------------
def test_more_draws_than_the_gpu_holds_at_once_chunks_and_reversed():
    Kd, P, T = 2000, 64, 8
    pb = experiments.toy(T=T)
    keys, As, Ss = _draws(pb, Kd)
    As = np.stack([As[0] * (1.0 + 1e-4 * k) for k in range(Kd)])
    Ss = np.stack([Ss[0] * (1.0 + 1e-3 * k) for k in range(Kd)])
    lik = _noise_lik("toy")
    sim = _sim_for(pb, lik=lik)
    cloud = _np(sim(As[-2:], Ss[-2:], keys[-2:], replicates=P))
    v = rc.channels(cloud, lik.H)
    flat = np.moveaxis(v, 1, 0).reshape(T, -1, v.shape[-1])
    thr = pgas_amd.threshold_grid(torch.as_tensor(flat.mean(axis=1)), torch.as_tensor(flat.std(axis=1)), 16, width=2.0).numpy()
    got = sim.cdf(As, Ss, keys, replicates=P, thresholds=thr, observation_noise=True).count
    assert tuple(got.shape) == (Kd, T, v.shape[-1], 16)
    for lo in range(0, Kd, 500):
        part = sim.cdf(As[lo:lo + 500], Ss[lo:lo + 500], keys[lo:lo + 500], replicates=P, thresholds=thr, observation_noise=True).count
        assert torch.equal(part, got[lo:lo + 500]), f"chunk at {lo}"
    rev = sim.cdf(As[::-1].copy(), Ss[::-1].copy(), keys[::-1], replicates=P, thresholds=thr, observation_noise=True).count
    assert torch.equal(rev.flip(0), got)
    assert np.array_equal(_np(got[-2:]), rc.rollout_counts(cloud, lik, thr, keys[-2:]))


def test_equal_draws_give_equal_rows_and_no_thresholds_means_the_observations():
    pb = _problem("smo")
    Kd, P = 5, 1500
    keys, As, Ss = _draws(pb, Kd)
    sim, thr = _noise_sim("smo"), _thresholds("smo", 16)
    fwd = _np(sim.cdf(As, Ss, keys, replicates=P, thresholds=thr, observation_noise=True).count)
    idx = [0, 3, 0, 3, 1]
    dup = _np(sim.cdf(As[idx], Ss[idx], [keys[i] for i in idx], replicates=P, thresholds=thr, observation_noise=True).count)
    assert np.array_equal(dup[0], dup[2]) and np.array_equal(dup[1], dup[3]) and np.array_equal(dup[0], fwd[0]) and np.array_equal(dup[4], fwd[1])
    assert not np.array_equal(dup[0], dup[1])
    # thresholds=None: the PIT counts of the context's observations on the yhat channels; the state channels count nothing
    y = np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1)
    pit = sim.cdf(As, Ss, keys, replicates=P, observation_noise=True)
    assert pit.pit and tuple(pit.count.shape) == (Kd, pb.T, pb.nx + 1, 1)
    for form in (y, y[:, 0], y[:, :, None]):
        given = sim.cdf(As, Ss, keys, replicates=P, thresholds=form, observation_noise=True)
        assert torch.equal(given.count, pit.count) and not given.pit
    assert bool((pit.count[:, :, :pb.nx] == 0).all()) and bool(torch.isnan(pit.thresholds[:, :pb.nx]).all())
    full = np.concatenate([np.full((pb.T, pb.nx, 1), NAN), y[:, :, None]], axis=1)
    assert np.array_equal(_np(pit.thresholds), full, equal_nan=True)
    assert torch.equal(sim.cdf(As, Ss, keys, replicates=P, thresholds=full, observation_noise=True).count, pit.count)
    s = pgas_amd.calibration_summary(pit)
    assert tuple(s["pit"].shape) == (pb.T, 1) and bool(((s["pit"] >= 0) & (s["pit"] <= 1)).all())
    assert torch.equal(s["pit"][:, 0], pit.count[:, :, pb.nx, 0].to(torch.int64).sum(dim=0).to(torch.float64) / float(Kd * P))


# ---- 4. side effects ----------------------------------------------------------------------------------------------------------------------
def test_cdf_makes_no_host_round_trip():
    pb = experiments.smo_pgas(T=16)
    Kd = 4
    keys, As, Ss = _draws(pb, Kd)
    sim = _sim_for(pb)
    dev = sim.engine.device
    kd = ch.keys_tensor(keys, dev)
    Ad, Sd = torch.as_tensor(As, device=dev), torch.as_tensor(Ss, device=dev)
    x0 = torch.as_tensor(np.repeat(pb.X_true[:1], Kd, axis=0), device=dev)
    thr = torch.linspace(-1.0, 1.0, 16, dtype=torch.float64, device=dev).expand(16, 3, 16).contiguous()
    thr_y = thr[:, 2:].contiguous()
    calls = [lambda: sim.cdf(Ad, Sd, kd, replicates=1500, thresholds=thr, observation_noise=True), lambda: sim.cdf(Ad, Sd, kd, replicates=3, init_state=x0, thresholds=thr_y),
             lambda: sim.cdf(Ad, init_state=x0, thresholds=thr)]
    warm = [c() for c in calls]   # allocations may synchronise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a.count, b.count) and bool((a.count >= 0).all()) and bool(a.count.sum() > 0)


def test_cdf_leaves_sweeps_and_the_plain_rollout_as_they_were():
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
        else:   # the parameters packed before cdf must still be there
            t1 = eng.sweep(prng.as_key(4242), torch.as_tensor(pb.X_true, device=dev)).clone()
            tc = eng.chains_sweep(ch.keys_tensor(keys, dev), torch.as_tensor(refs, device=dev)).clone()
        single = [t.clone() for t in eng.traces()[:3]]
        return [t1, tc] + single + [t.clone() for t in chs.traces()]

    plain = chs.rollout(rA, rS, rk, replicates=100).clone()
    before = sweeps(True)
    views = list(eng.traces()[:3]) + list(chs.traces())
    st = chs.cdf(rA * 1.3, rS * 2.0, [k + 5 for k in rk], replicates=1300, observation_noise=True)
    assert tuple(st.count.shape) == (4, pb.T, pb.nx + 1, 1) and bool((st.count[:, :, pb.nx:] >= 0).all())
    single_ctx = chs.single.cdf(rA * 1.3, rS * 2.0, [k + 5 for k in rk], replicates=1300, observation_noise=True)
    assert torch.equal(single_ctx.count, st.count)
    for a, b in zip(before[2:], views):
        assert torch.equal(a, b), "cdf wrote into a trace buffer"
    for a, b in zip(before, sweeps(False)):
        assert torch.equal(a, b), "sweeps after cdf (parameters not set again) differ"
    assert torch.equal(chs.rollout(rA, rS, rk, replicates=100), plain)
    # in-sample: the training context's own observations and likelihood
    want = _sim_for(pb).cdf(rA, rS, rk, replicates=100, observation_noise=True)
    got = chs.cdf(rA, rS, rk, replicates=100, observation_noise=True)
    assert torch.equal(got.count, want.count) and bool(got.count.sum() > 0)


def test_refusals_are_clean_and_leave_the_context_usable():
    pb = experiments.smo_pgas(T=16)
    Kd = 2
    keys, As, Ss = _draws(pb, Kd)
    sim = _sim_for(pb)
    eng = sim.engine
    thr = torch.linspace(-1.0, 1.0, 16, dtype=torch.float64, device=eng.device).expand(16, 3, 16).contiguous()
    good = sim.cdf(As, Ss, keys, replicates=10, thresholds=thr, observation_noise=True).count.clone()
    Ad, Sd, kd = torch.as_tensor(As, device=eng.device), torch.as_tensor(Ss, device=eng.device), ch.keys_tensor(keys, eng.device)
    out = torch.empty((Kd, 16, 3, 16), dtype=torch.int32, device=eng.device)
    x0 = torch.zeros(2, dtype=torch.float64, device=eng.device)
    LR = np.ascontiguousarray(eng.LR)
    PGAS_E_ARG = -1

    def call(Kc, P, seeds=kd, S=Sd, mode=0, xs=None, noise=False, th=thr, J=16, cnt=out):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc_ = eng.lib.pgas_rollout_cdf(eng._h, Kc, P, 0, p(seeds), Ad.data_ptr(), p(S), p(xs), mode, LR.ctypes.data if noise else None, p(th), J, p(cnt),
                                       eng._stream())
        return rc_, eng.lib.pgas_last_error(eng._h).decode()

    for args, kw, msg in [((Kd, 0), {}, "P = 0"), ((Kd, (1 << 20) + 1), {}, "P = 1048577"), ((0, 10), {}, "K = 0"), ((Kd, 10, None, None), {}, "needs seeds"),
                          ((Kd, 10, kd, None), {}, "go together"), ((Kd, 10, kd, Sd, 2), {}, "without x0"), ((Kd, 1, None, None, 1, x0, True), {}, "measurement noise"),
                          ((Kd, 10), dict(J=0), "J = 0"), ((Kd, 10), dict(J=17), "J = 17"), ((Kd, 10), dict(th=None), "NULL"), ((Kd, 10), dict(cnt=None), "NULL")]:
        rc_, err = call(*args, **kw)
        assert rc_ == PGAS_E_ARG and msg in err, (args, kw, rc_, err)
        assert torch.equal(sim.cdf(As, Ss, keys, replicates=10, thresholds=thr, observation_noise=True).count, good), f"cdf after refusing {args} {kw}"
    big = pgas_amd.condSequentialMonteCarlo(5000, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    with pytest.raises(PgasError, match="no small variant"):
        big.cdf(As, Ss, keys, replicates=10)
    traj = big(77, pb.X_true, As[0], Sd[0])
    assert bool(torch.isfinite(traj).all())
    assert torch.equal(sim.cdf(As, Ss, keys, replicates=10, thresholds=thr, observation_noise=True).count, good)


# ---- 5. independent of the restatement: a model whose predictive is known ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "smo", "veh27"])
def test_pooled_counts_of_a_model_with_A_zero_are_binomial(name):
    """A = 0: x_t = LS z_t for t >= 1, iid N(0, S), and yhat_t + noise ~ N(0, H S H^T + R).  The count pooled over draws, rows t >= 1 and
    replicates at the thresholds sigma_c * TAUS is Binomial(n, Phi(TAUS)): |z| <= 4, the bound of the project's other closed-form tests."""
    pb = _problem(name)
    Kd, P = 3, 4096
    keys, _, Ss = _draws(pb, Kd)
    S = Ss[0]
    lik = _noise_lik(name)
    Hm = np.atleast_2d(lik.H)
    sig = np.sqrt(np.concatenate([np.diag(S), np.diag(Hm @ S @ Hm.T + np.atleast_2d(lik.R))]))
    thr = np.broadcast_to(sig[:, None] * np.array(TAUS)[None, :], (pb.T, len(sig), len(TAUS))).copy()
    A0 = np.zeros((Kd, pb.nx, pb.basis_fcn.basis.M))
    res = _noise_sim(name).cdf(A0, np.stack([S] * Kd), keys, replicates=P, thresholds=thr, observation_noise=True)
    tot = _np(res.count).astype(np.int64)[:, 1:].sum(axis=(0, 1))   # (nv, 7)
    n = Kd * (pb.T - 1) * P
    for c in range(len(sig)):
        z = binomial_z(tot[c], n)
        print(f"{name}: channel {c}, n = {n}, z = {np.round(z, 3).tolist()}")
        assert (np.abs(z) <= 4.0).all()
