"""A bootstrap particle filter per parameter draw in one launch (pgas_amd.HeldOutFilter, pgas_filter, csrc/pgas_filter.hip.h) against the
NumPy restatement of its definition from the canonical oracle's primitives (tests/filter_numpy.py), which tests/test_filter_host.py
pins to a plain float filter.  Every comparison against the restatement is np.array_equal.  The last test is independent of the
restatement: a linear-Gaussian model whose evidence is known in closed form."""
import numpy as np
import pytest
import torch

import filter_numpy as fn
from common import canon_model, experiments, pgas_amd
from pgas_amd import chains as ch
from pgas_amd import random as prng
from pgas_amd._lib import PgasError
from test_gpu_rollout import MODELS, _draws, _np, _problem

pytestmark = pytest.mark.gpu

K = 3
NS = [1, 2, 255, 256, 257, 512, 513, 1024]   # every NR (1, 2, 4 register rows) and both sides of each row boundary
FIELDS = ("x", "anc", "ell", "ess", "pred_sum", "pred_sumsq", "filt_sum", "wtot")


def _y(pb):
    return np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1)


def _filter_for(pb, N, obs=None):
    return pgas_amd.HeldOutFilter(pb.observations if obs is None else obs, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, pb.nx, N,
                                  pb.init_state_mean, pb.init_state_cov)


def _restate(pb, N, keys, As, Ss, y=None, x0=None):
    """The restatement of every draw, stacked: dict of (K, ...) arrays."""
    y = _y(pb) if y is None else y
    pb = type(pb)(**{**pb.__dict__, "observations": y})
    cm1 = canon_model(pb, N + 1)
    L0 = np.linalg.cholesky(pb.init_state_cov)
    rs_ = [fn.run(cm1, N, keys[k], As[k], Ss[k], pb.init_state_mean, L0, pb.likelihood_fcn, y, None if x0 is None else x0[k]) for k in range(len(keys))]
    return {f: np.stack([np.asarray(r[f]) for r in rs_]) for f in FIELDS + ("loglik",)}


def _assert_equal(res, want, what, fields=FIELDS + ("loglik",)):
    for f in fields:
        got = _np(getattr(res, f))
        assert got.shape == want[f].shape, f"{what}: {f} shape {got.shape} != {want[f].shape}"
        assert np.array_equal(got, want[f], equal_nan=True), f"{what}: {f}"


# ---- 1. traces and reductions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", MODELS)
def test_filter_equals_the_restated_definition(name, N):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    want = _restate(pb, N, keys, As, Ss)
    flt = _filter_for(pb, N)
    drawn = flt(As, Ss, keys, traces=True)
    assert drawn.n == N and tuple(drawn.x.shape) == (K, pb.T, N, pb.nx) and drawn.anc.dtype == torch.int32
    _assert_equal(drawn, want, "drawn x_0")
    given = flt(As, Ss, keys, init_state=want["x"][:, 0].copy(), traces=True)
    _assert_equal(given, want, "given x_0 (K, N, nx)")
    assert not np.array_equal(want["ell"][0], want["ell"][1])
    assert np.isfinite(want["ell"]).all() and (want["ess"] > 0).all()
    if N >= 255:   # the gather of the resampled state is exercised: some step keeps fewer distinct ancestors than N
        distinct = np.array([[len(np.unique(a)) for a in want["anc"][k]] for k in range(K)])
        assert distinct.min() < N
        moved = (want["anc"] != np.arange(N)[None, None, :]).any()
        assert moved


def test_shared_and_per_draw_initial_states():
    pb = _problem("smo")
    keys, As, Ss = _draws(pb, K)
    one = pb.X_true[0] + np.array([0.01, -0.02])
    per = np.stack([one * (1.0 + 0.1 * k) for k in range(K)])
    for N in (70, 257):   # one particle per thread, and the instance with two register rows (the second one ragged)
        flt = _filter_for(pb, N)
        for x0, full in ((one, np.broadcast_to(one, (K, N, pb.nx))), (per, np.broadcast_to(per[:, None, :], (K, N, pb.nx)))):
            want = _restate(pb, N, keys, As, Ss, x0=full)
            _assert_equal(flt(As, Ss, keys, init_state=x0, traces=True), want, f"N = {N}, init_state {np.shape(x0)}")


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 300])
def test_a_record_of_one_row(N):
    pb = experiments.smo_pgas(T=1)
    keys, As, Ss = _draws(_problem("smo"), K)
    want = _restate(pb, N, keys, As, Ss)
    res = _filter_for(pb, N)(As, Ss, keys, traces=True)
    _assert_equal(res, want, "T = 1")
    assert np.array_equal(_np(res.loglik), _np(res.ell)[:, 0])


@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_nan_row_and_outlier_row(name):
    pb = _problem(name)
    N = 257
    keys, As, Ss = _draws(pb, K)
    y = _y(pb).copy()
    y[7, -1] = np.nan      # one component of one row: a pure prediction step
    y[12] = 1e200          # the quadratic form overflows: every l_i is -inf
    want = _restate(pb, N, keys, As, Ss, y=y)
    res = _filter_for(pb, N, obs=y)(As, Ss, keys, traces=True)
    ell, anc = _np(res.ell), _np(res.anc)
    ident = np.arange(N, dtype=np.int32)
    assert np.isnan(ell[:, 7]).all() and (anc[:, 7] == ident).all()
    assert (ell[:, 12] == -np.inf).all() and (anc[:, 12] == ident).all()
    assert (_np(res.ess)[:, [7, 12]] == 0.0).all() and (_np(res.wtot)[:, [7, 12]] == 0.0).all()
    rest = np.delete(np.arange(pb.T), [7, 12])
    assert np.isfinite(ell[:, rest]).all()
    assert (_np(res.loglik) == -np.inf).all()          # the -inf row is in the total, the NaN row is not
    _assert_equal(res, want, "NaN and outlier rows")    # the later steps included
    # without the outlier the total is finite and skips the NaN row
    y2 = y.copy()
    y2[12] = _y(pb)[12]
    r2 = _filter_for(pb, N, obs=y2)(As, Ss, keys)
    e2 = _np(r2.ell)
    tot = np.zeros(K)
    for t in range(pb.T):
        if t != 7:
            tot = tot + e2[:, t]
    assert np.isfinite(tot).all() and np.array_equal(_np(r2.loglik), tot)


# ---- 3. independence of the launch ----------------------------------------------------------------------------------------------------
def test_more_draws_than_the_gpu_holds_at_once_in_chunks_and_reversed():
    Kb, N, T = 2000, 64, 8
    pb = experiments.smo_pgas(T=T)
    keys, As, Ss = _draws(pb, Kb)
    As = np.stack([As[0] * (1.0 + 1e-4 * k) for k in range(Kb)])
    Ss = np.stack([Ss[0] * (1.0 + 1e-3 * k) for k in range(Kb)])
    flt = _filter_for(pb, N)
    whole = flt(As, Ss, keys, traces=True)
    got = {f: _np(getattr(whole, f)) for f in FIELDS + ("loglik",)}
    assert np.isfinite(got["loglik"]).all()
    for lo in range(0, Kb, 700):    # chunks of 700, 700, 600
        part = flt(As[lo:lo + 700], Ss[lo:lo + 700], keys[lo:lo + 700], traces=True)
        for f in got:
            assert np.array_equal(_np(getattr(part, f)), got[f][lo:lo + 700]), f"chunk at {lo}: {f}"
    rev = flt(As[::-1].copy(), Ss[::-1].copy(), keys[::-1], traces=True)
    for f in got:
        assert np.array_equal(_np(getattr(rev, f))[::-1], got[f]), f"reversed: {f}"
    want = _restate(pb, N, keys[-2:], As[-2:], Ss[-2:])
    for f in got:
        assert np.array_equal(got[f][-2:], want[f]), f"last draws: {f}"


def test_equal_draws_give_equal_outputs_and_nullable_outputs_change_nothing():
    pb = _problem("veh27")
    N = 300
    keys, As, Ss = _draws(pb, K)
    flt = _filter_for(pb, N)
    full = flt(As, Ss, keys, traces=True)
    idx = [0, 2, 0, 2, 1]
    dup = flt(As[idx], Ss[idx], [keys[i] for i in idx], traces=True)
    for f in FIELDS + ("loglik",):
        d, g = _np(getattr(dup, f)), _np(getattr(full, f))
        assert np.array_equal(d[0], d[2]) and np.array_equal(d[1], d[3]) and np.array_equal(d, g[idx]), f
    assert not np.array_equal(_np(dup.ell)[0], _np(dup.ell)[1])
    for moments, traces in ((False, False), (True, False), (False, True)):
        r = flt(As, Ss, keys, moments=moments, traces=traces)
        on = ("loglik", "ell") + (("ess", "pred_sum", "pred_sumsq", "filt_sum", "wtot") if moments else ()) + (("x", "anc") if traces else ())
        for f in FIELDS + ("loglik",):
            if f in on:
                assert np.array_equal(_np(getattr(r, f)), _np(getattr(full, f))), (moments, traces, f)
            else:
                assert getattr(r, f) is None, (moments, traces, f)


# ---- 4. other contexts and host synchronisation ---------------------------------------------------------------------------------------
def test_in_sample_filter_leaves_single_chain_and_chains_state_as_it_was():
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
        else:   # the parameters packed before the filter call must still be there
            t1 = eng.sweep(prng.as_key(4242), torch.as_tensor(pb.X_true, device=dev)).clone()
            tc = eng.chains_sweep(ch.keys_tensor(keys, dev), torch.as_tensor(refs, device=dev)).clone()
        single = [t.clone() for t in eng.traces()[:3]]
        return [t1, tc] + single + [t.clone() for t in chs.traces()]

    before = sweeps(True)
    views = list(eng.traces()[:3]) + list(chs.traces())
    fk, fA, fS = _draws(pb, 4)
    fkeys = [k + 5 for k in fk]
    res = chs.filter(fA * 1.01, fS * 2.0, fkeys, traces=True)
    one = chs.single.filter(fA * 1.01, fS * 2.0, fkeys, traces=True)
    want = _restate(pb, N, fkeys, fA * 1.01, fS * 2.0)
    _assert_equal(res, want, "chains context")
    _assert_equal(one, want, "single-chain context")
    for a, b in zip(before[2:], views):
        assert torch.equal(a, b), "a filter call wrote into a trace buffer"
    for a, b in zip(before, sweeps(False)):
        assert torch.equal(a, b), "sweeps after a filter call (parameters not set again) differ"
    for a, b in zip(before, sweeps(True)):
        assert torch.equal(a, b)


def test_filter_calls_make_no_host_round_trip():
    pb = experiments.smo_pgas(T=16)
    Kc, N = 4, 300
    keys, As, Ss = _draws(pb, Kc)
    flt = _filter_for(pb, N)
    dev = flt.engine.device
    kd = ch.keys_tensor(keys, dev)
    Ad, Sd = torch.as_tensor(As, device=dev), torch.as_tensor(Ss, device=dev)
    x0 = torch.as_tensor(np.repeat(pb.X_true[:1], Kc, axis=0), device=dev)
    calls = [lambda: flt(Ad, Sd, kd, traces=True), lambda: flt(Ad, Sd, kd, init_state=x0), lambda: flt(Ad, Sd, kd, moments=False)]
    warm = [c() for c in calls]   # allocations may synchronise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a.ell, b.ell) and torch.equal(a.loglik, b.loglik) and bool(torch.isfinite(a.loglik).all())


def test_refusals_are_clean_and_leave_the_context_usable():
    pb = experiments.smo_pgas(T=16)
    Kc, N, T = 2, 40, 16
    keys, As, Ss = _draws(pb, Kc)
    flt = _filter_for(pb, N)
    eng = flt.engine
    good = flt(As, Ss, keys).ell.clone()
    Ad, Sd, kd = torch.as_tensor(As, device=eng.device), torch.as_tensor(Ss, device=eng.device), ch.keys_tensor(keys, eng.device)
    f = lambda *s: torch.empty(s, dtype=torch.float64, device=eng.device)  # noqa: E731
    ell, ll, a, b = f(Kc, T), f(Kc), f(Kc, T, 3), f(Kc, T, 3)
    PGAS_E_ARG = -1

    def call(Kn=Kc, seeds=kd, S=Sd, mode=0, ps=None, pq=None, fs=None, wt=None):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = eng.lib.pgas_filter(eng._h, Kn, p(seeds), Ad.data_ptr(), p(S), None, mode, ell.data_ptr(), ll.data_ptr(), None, p(ps), p(pq), p(fs), p(wt),
                                 None, None, eng._stream())
        return rc, eng.lib.pgas_last_error(eng._h).decode()

    for kw, msg in [(dict(Kn=0), "K = 0"), (dict(seeds=None), "seeds and S"), (dict(S=None), "seeds and S"), (dict(mode=4), "x0_mode = 4"),
                    (dict(mode=-1), "x0_mode = -1"), (dict(mode=2), "without x0"), (dict(ps=a), "pred_sum and pred_sumsq"),
                    (dict(pq=a), "pred_sum and pred_sumsq"), (dict(fs=a), "filt_sum and wtot"), (dict(wt=ell), "filt_sum and wtot")]:
        rc, err = call(**kw)
        assert rc == PGAS_E_ARG and msg in err, (kw, rc, err)
        assert torch.equal(flt(As, Ss, keys).ell, good), f"filter after refusing {kw}"
    rc, _ = call(ps=a, pq=b)
    assert rc == 0
    with pytest.raises(PgasError, match="seeds and S"):
        eng.filter(Ad, None, kd)
    # a context of more than one segment of particles has no one-workgroup variant
    big = pgas_amd.condSequentialMonteCarlo(5000, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    with pytest.raises(PgasError, match="no one-workgroup variant"):
        big.engine.filter(Ad, Sd, kd)
    with pytest.raises(ValueError, match="particles"):
        big.filter(As, Ss, keys)
    traj = big(77, pb.X_true, As[0], Sd[0])
    assert bool(torch.isfinite(traj).all())


# ---- 5. analytic check, independent of the restatement --------------------------------------------------------------------------------
def _mvn_logpdf(e, C):
    C = np.atleast_2d(C)
    return float(-0.5 * (len(e) * np.log(2 * np.pi) + np.linalg.slogdet(C)[1] + e @ np.linalg.solve(C, e)))


@pytest.mark.parametrize("name", ["smo", "toy", "veh27"])
def test_evidence_of_a_linear_gaussian_model_is_the_closed_form(name):
    """With A = 0 the states are iid N(0, S) (x_0 ~ N(m0, P0)), so log p(y_{0:T-1}) = log N(y_0; H m0, H P0 H^T + R) + sum_{t >= 1} log
    N(y_t; 0, H S H^T + R).  S is scaled so that tr(H S H^T) = tr(R); y is drawn from that model.  The mean over 16 keys of the filter's
    loglik must lie within 4 standard errors (std_k / sqrt(16)) of the closed form."""
    pb = _problem(name)
    lik, T, nx = pb.likelihood_fcn, pb.T, pb.nx
    H, R = lik.H, lik.R
    _, S = experiments.initial_params(pb)
    S = S * (np.trace(R) / np.trace(H @ S @ H.T))
    assert np.isclose(np.trace(H @ S @ H.T), np.trace(R))
    rng = np.random.default_rng(20240607)
    m0, P0 = pb.init_state_mean, pb.init_state_cov
    xs = rng.standard_normal((T, nx)) @ np.linalg.cholesky(S).T
    xs[0] = m0 + np.linalg.cholesky(P0) @ rng.standard_normal(nx)
    y = xs @ H.T + rng.standard_normal((T, lik.ny)) @ lik.LR.T
    analytic = _mvn_logpdf(y[0] - H @ m0, H @ P0 @ H.T + R) + sum(_mvn_logpdf(y[t], H @ S @ H.T + R) for t in range(1, T))
    Kk = 16
    keys = [prng.key(1000 + 7919 * k) for k in range(Kk)]
    A = np.zeros((Kk, nx, pb.basis_fcn.basis.M))
    res = _filter_for(pb, 1024, obs=y)(A, np.repeat(S[None], Kk, axis=0), keys)
    ll = _np(res.loglik)
    assert np.isfinite(ll).all()
    mean, se = ll.mean(), ll.std() / np.sqrt(Kk)
    print(f"{name}: analytic {analytic:.6f}, mean loglik {mean:.6f}, std {ll.std():.6f}, z = {(mean - analytic) / se:.3f}")
    assert abs(mean - analytic) <= 4.0 * se
    summary = pgas_amd.evidence_summary(res, y=y)
    assert mean <= float(summary["log_evidence"]) + 1e-12 and float(summary["log_evidence"]) <= ll.max() + 1e-12   # a log-mean-exp
    assert bool(torch.isfinite(summary["rmse"]))
