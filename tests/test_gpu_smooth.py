"""Backward simulation over the held-out filter's trace, every draw and trajectory in one launch per 256 trajectories
(pgas_amd.HeldOutFilter.smooth, pgas_smooth, csrc/pgas_smooth.hip.h) against the NumPy restatement of its definition from the canonical
oracle's primitives (tests/smooth_numpy.py), which tests/test_smooth_host.py pins to a plain float64 FFBSi and to the exact smoother
marginals.  Every comparison against the restatement is np.array_equal."""
import functools

import numpy as np
import pytest
import torch

import filter_numpy as fn
import smooth_numpy as sn
from common import canon_model, experiments, pgas_amd
from pgas_amd import chains as ch
from pgas_amd import random as prng
from pgas_amd._lib import PgasError
from test_gpu_filter import _filter_for, _y
from test_gpu_rollout import _draws, _np, _problem
from test_smooth_host import check_marginals

pytestmark = pytest.mark.gpu

K = 3
FIELDS = ("idx", "xs", "sum", "sumsq")
# (N, B): both sides of a wave of particles (63, 64, 65), of a register row (256, 257), all three instances (R = 4, 8, 16 particles per
# lane), trajectory counts around the four waves' assignment (1, 3, 4, 5) and the ends of the 256-position tree (255, 256)
SIZES = [(1, 1), (2, 3), (63, 4), (64, 5), (65, 64), (200, 255), (256, 256), (257, 64), (1024, 5), (1, 256), (63, 255), (257, 256), (1024, 64)]
CASES = [("smo", n, b) for n, b in SIZES] + [(m, n, b) for m in ("toy", "emps27", "veh27") for n, b in ((65, 64), (257, 5), (1024, 3))] + [("emps", 200, 64)]


def _restate(pb, N, keys, As, Ss, n_traj, y=None):
    """The restatement of the filter and of n_traj trajectories of every draw: (dict of (K, ...) arrays, the filters' dicts)."""
    y = _y(pb) if y is None else y
    pb = type(pb)(**{**pb.__dict__, "observations": y})
    cm1 = canon_model(pb, N + 1)
    L0 = np.linalg.cholesky(pb.init_state_cov)
    flts = [fn.run(cm1, N, keys[k], As[k], Ss[k], pb.init_state_mean, L0, pb.likelihood_fcn, y) for k in range(len(keys))]
    rs_ = [sn.run_chunks(cm1, N, keys[k], As[k], Ss[k], flts[k], pb.likelihood_fcn, y, n_traj) for k in range(len(keys))]
    return {f: np.stack([r[f] for r in rs_]) for f in FIELDS + ("u", "S")}, flts


def _assert_equal(res, want, what, fields=FIELDS):
    for f in fields:
        got = _np(getattr(res, f))
        assert got.shape == want[f].shape and got.dtype == want[f].dtype, f"{what}: {f} {got.shape} {got.dtype} != {want[f].shape} {want[f].dtype}"
        assert np.array_equal(got, want[f]), f"{what}: {f}"


@functools.lru_cache(maxsize=None)
def _smo65():
    """SMO, N = 65, 300 trajectories of K draws: shared by the tests that need a reference of more than one chunk."""
    pb = _problem("smo")
    keys, As, Ss = _draws(pb, K)
    want, flts = _restate(pb, 65, keys, As, Ss, 300)
    return pb, keys, As, Ss, want, flts


# ---- 1. indices, trajectories and moments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,B", CASES)
def test_smooth_equals_the_restated_definition(name, N, B):
    pb = _problem(name)
    keys, As, Ss = _draws(pb, K)
    want, flts = _restate(pb, N, keys, As, Ss, B)
    res = _filter_for(pb, N).smooth(As, Ss, keys, B, trajectories=True, indices=True)
    assert res.n_trajectories == B and res.n == N and res.idx.dtype == torch.int32
    assert np.array_equal(_np(res.filter.x), np.stack([f["x"] for f in flts])) and np.array_equal(_np(res.filter.anc), np.stack([f["anc"] for f in flts]))
    _assert_equal(res, want, f"{name}, N = {N}, B = {B}")
    assert ((want["S"] > 0) & np.isfinite(want["S"])).all()
    if N >= 63 and B > 1:   # enough particles that neither two draws nor two trajectories coincide over the whole record
        assert not np.array_equal(want["idx"][0], want["idx"][1]) and not np.array_equal(want["idx"][0, 0], want["idx"][0, 1])


@pytest.mark.parametrize("T,N,B", [(1, 1, 1), (1, 300, 5), (2, 65, 5), (2, 513, 4)])
def test_records_of_one_and_two_rows(T, N, B):
    pb = experiments.smo_pgas(T=T)
    keys, As, Ss = _draws(_problem("smo"), K)
    want, _ = _restate(pb, N, keys, As, Ss, B)
    _assert_equal(_filter_for(pb, N).smooth(As, Ss, keys, B, trajectories=True, indices=True), want, f"T = {T}")


# ---- 2. a trajectory depends on (key, g) alone ----------------------------------------------------------------------------------------
def test_trajectory_g_is_the_same_alone_in_a_full_launch_and_in_a_chunked_call():
    pb, keys, As, Ss, want, _ = _smo65()
    flt = _filter_for(pb, 65)
    full = flt.smooth(As, Ss, keys, 300, trajectories=True, indices=True)
    _assert_equal(full, want, "300 trajectories")
    eng, f = flt.engine, full.filter
    kd = ch.keys_tensor(keys, eng.device)
    s1, s2, xs, idx = eng.smooth(As, Ss, kd, f.x, f.anc, 256, 0, True, True, True)
    assert torch.equal(idx, full.idx[:, :256]) and torch.equal(xs, full.xs[:, :256])
    t1, t2, _, _ = eng.smooth(As, Ss, kd, f.x, f.anc, 44, 256, True, False, False)
    assert torch.equal(s1 + t1, full.sum) and torch.equal(s2 + t2, full.sumsq)     # the chunks' sums, ascending from the first chunk's
    assert not torch.equal(s1, full.sum)
    for g in (0, 7, 255, 256, 299):
        _, _, x1, i1 = eng.smooth(As, Ss, kd, f.x, f.anc, 1, g, False, True, True)
        assert torch.equal(i1[:, 0], full.idx[:, g]) and torch.equal(x1[:, 0], full.xs[:, g]), f"trajectory {g} alone"


def test_more_draws_than_the_gpu_holds_at_once_in_chunks_and_reversed():
    Kb, N, T, B = 2000, 64, 8, 5
    pb = experiments.smo_pgas(T=T)
    keys, As, Ss = _draws(pb, Kb)
    As = np.stack([As[0] * (1.0 + 1e-4 * k) for k in range(Kb)])
    Ss = np.stack([Ss[0] * (1.0 + 1e-3 * k) for k in range(Kb)])
    flt = _filter_for(pb, N)
    whole = flt.smooth(As, Ss, keys, B, trajectories=True, indices=True)
    got = {f: _np(getattr(whole, f)) for f in FIELDS}
    for lo in range(0, Kb, 700):    # chunks of 700, 700, 600
        part = flt.smooth(As[lo:lo + 700], Ss[lo:lo + 700], keys[lo:lo + 700], B, trajectories=True, indices=True)
        for f in got:
            assert np.array_equal(_np(getattr(part, f)), got[f][lo:lo + 700]), f"chunk at {lo}: {f}"
    rev = flt.smooth(As[::-1].copy(), Ss[::-1].copy(), keys[::-1], B, trajectories=True, indices=True)
    for f in got:
        assert np.array_equal(_np(getattr(rev, f))[::-1], got[f]), f"reversed: {f}"
    want, _ = _restate(pb, N, keys[-2:], As[-2:], Ss[-2:], B)
    for f in got:
        assert np.array_equal(got[f][-2:], want[f]), f"last draws: {f}"
    dup_i = [0, 2, 0, 2, 1]
    dup = flt.smooth(As[dup_i], Ss[dup_i], [keys[i] for i in dup_i], B, trajectories=True, indices=True)
    for f in got:
        d = _np(getattr(dup, f))
        assert np.array_equal(d[0], d[2]) and np.array_equal(d[1], d[3]) and np.array_equal(d, got[f][dup_i]), f"equal draws: {f}"


# ---- 3. rows without weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "veh27"])
def test_nan_row_and_outlier_rows_fall_back_to_the_filter_genealogy(name):
    pb = _problem(name)
    N, B = 257, 16
    keys, As, Ss = _draws(pb, K)
    y = _y(pb).copy()
    y[7, -1] = np.nan        # the filter's weights are uniform: the transition density alone decides
    y[12] = 1e200            # every l_i is -inf: j_12 = anc[12, j_13], the identity on that row
    y[pb.T - 1] = 1e200      # ... and on the last row j = g mod N
    want, flts = _restate(pb, N, keys, As, Ss, B, y=y)
    res = _filter_for(pb, N, obs=y).smooth(As, Ss, keys, B, trajectories=True, indices=True)
    idx = _np(res.idx)
    assert (want["S"][:, :, [12, pb.T - 1]] == 0.0).all() and (np.delete(want["S"], [12, pb.T - 1], axis=2) > 0).all()
    assert np.array_equal(idx[:, :, pb.T - 1], np.broadcast_to(np.arange(B) % N, (K, B)))
    assert np.array_equal(idx[:, :, 12], idx[:, :, 13])
    assert all(len(np.unique(idx[k, :, 7])) > 1 for k in range(K))
    _assert_equal(res, want, "NaN and outlier rows")    # the earlier rows included


# ---- 4. independent of the restatement's arithmetic -----------------------------------------------------------------------------------
def test_chosen_index_brackets_the_uniform_in_plain_float64():
    """Row t of every trajectory of draw 0, with the next state taken from xs: the float64 CDF of softmax(l + h) at the chosen index
    brackets u.  Tolerance 1e-10: the fixed-point weights are quantised to 2^-51 of the largest (65 of them: 3e-14 of the total), the
    float64 log-densities carry a few 1e-16 relative on exponents below 40 (1e-14), and the sums of 65 terms as much again."""
    pb, keys, As, Ss, want, flts = _smo65()
    res = _filter_for(pb, 65).smooth(As, Ss, keys, 64, trajectories=True, indices=True)
    xs, idx = _np(res.xs)[0], _np(res.idx)[0]
    cm1 = canon_model(pb, 66)
    for t in (0, pb.T // 2, pb.T - 2, pb.T - 1):
        lw = sn.float_logweights(cm1, 65, As[0], Ss[0], flts[0], pb.likelihood_fcn, _y(pb), t, None if t == pb.T - 1 else xs[:, t + 1])
        lw = np.broadcast_to(lw, (64, 65))
        w = np.exp(lw - lw.max(axis=1, keepdims=True))
        cdf = np.cumsum(w / w.sum(axis=1, keepdims=True), axis=1)
        for b in range(64):
            u, j = sn.uniform(keys[0], t, b), int(idx[b, t])
            lo = cdf[b, j - 1] if j > 0 else 0.0
            assert lo - 1e-10 <= u <= cdf[b, j] + 1e-10, (t, b, j, lo, u, cdf[b, j])


@pytest.mark.parametrize("name", ["toy", "smo"])
def test_marginal_of_the_device_indices_is_the_exact_smoother_marginal(name):
    N, Tn, n = 8, 6, 4096
    pb = {"smo": experiments.smo_pgas, "toy": experiments.toy}[name](T=Tn)
    A, S = experiments.initial_params(pb)
    key = prng.key(1000)
    y = _y(pb)
    cm1 = canon_model(pb, N + 1)
    flt = fn.run(cm1, N, key, A, S, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), pb.likelihood_fcn, y)
    res = _filter_for(pb, N).smooth(A[None], S[None], [key], n, indices=True)
    assert np.array_equal(_np(res.filter.x)[0], flt["x"])
    w = sn.smoother_marginals(cm1, N, A, S, flt, pb.likelihood_fcn, y)
    check_marginals(_np(res.idx)[0].astype(np.int64), w, n)
    # the moments are the chunks' sums of the states the indices name
    xs = flt["x"][np.arange(Tn)[None, :], _np(res.idx)[0]]
    assert np.allclose(_np(res.sum)[0, :, :pb.nx], xs.sum(axis=0), rtol=1e-12, atol=1e-300)
    summary = pgas_amd.smoothing_summary(res, y=y)
    assert bool(torch.isfinite(summary["rmse"])) and tuple(summary["x_smooth_mean_draw"].shape) == (1, Tn, pb.nx)


# ---- 5. nullable outputs, other contexts, host synchronisation, refusals --------------------------------------------------------------
def test_nullable_outputs_change_nothing():
    pb, keys, As, Ss, want, _ = _smo65()
    flt = _filter_for(pb, 65)
    full = flt.smooth(As, Ss, keys, 300, trajectories=True, indices=True)
    for traj, ind in ((False, False), (True, False), (False, True)):
        r = flt.smooth(As, Ss, keys, 300, trajectories=traj, indices=ind)
        assert torch.equal(r.sum, full.sum) and torch.equal(r.sumsq, full.sumsq)
        assert (torch.equal(r.xs, full.xs) if traj else r.xs is None) and (torch.equal(r.idx, full.idx) if ind else r.idx is None)
    eng, f = flt.engine, full.filter
    kd = ch.keys_tensor(keys, eng.device)
    s1, s2, xs, idx = eng.smooth(As, Ss, kd, f.x, f.anc, 256, 0, False, False, True)
    assert s1 is None and s2 is None and xs is None and torch.equal(idx, full.idx[:, :256])
    s1, s2, xs, idx = eng.smooth(As, Ss, kd, f.x, f.anc, 256, 0, False, True, False)
    assert s1 is None and idx is None and torch.equal(xs, full.xs[:, :256])


def test_in_sample_smooth_leaves_single_chain_and_chains_state_as_it_was():
    pb = _problem("smo")
    Cn, N, B = 3, 200, 8
    keys, As, Ss = _draws(pb, Cn)
    refs = np.stack([pb.X_true * (1.0 + 0.01 * c) for c in range(Cn)])
    chs = ch.condSequentialMonteCarloChains(Cn, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    eng, dev = chs.engine, chs.device
    Sd = torch.as_tensor(Ss[1], device=dev)

    def sweeps(set_params):
        if set_params:
            t1 = chs.single(4242, pb.X_true, As[1], Sd).clone()
            tc = chs(keys, refs, As, Ss).clone()
        else:   # the parameters packed before the smooth call must still be there
            t1 = eng.sweep(prng.as_key(4242), torch.as_tensor(pb.X_true, device=dev)).clone()
            tc = eng.chains_sweep(ch.keys_tensor(keys, dev), torch.as_tensor(refs, device=dev)).clone()
        single = [t.clone() for t in eng.traces()[:3]]
        return [t1, tc] + single + [t.clone() for t in chs.traces()]

    before = sweeps(True)
    views = list(eng.traces()[:3]) + list(chs.traces())
    fk, fA, fS = _draws(pb, 2)
    fkeys = [k + 5 for k in fk]
    res = chs.smooth(fA * 1.01, fS * 2.0, fkeys, B, trajectories=True, indices=True)
    one = chs.single.smooth(fA * 1.01, fS * 2.0, fkeys, B, trajectories=True, indices=True)
    want, _ = _restate(pb, N, fkeys, fA * 1.01, fS * 2.0, B)
    _assert_equal(res, want, "chains context")
    _assert_equal(one, want, "single-chain context")
    for a, b in zip(before[2:], views):
        assert torch.equal(a, b), "a smooth call wrote into a trace buffer"
    for a, b in zip(before, sweeps(False)):
        assert torch.equal(a, b), "sweeps after a smooth call (parameters not set again) differ"
    for a, b in zip(before, sweeps(True)):
        assert torch.equal(a, b)


def test_smooth_calls_make_no_host_round_trip():
    pb = experiments.smo_pgas(T=16)
    Kc, N = 4, 300
    keys, As, Ss = _draws(pb, Kc)
    flt = _filter_for(pb, N)
    dev = flt.engine.device
    kd = ch.keys_tensor(keys, dev)
    Ad, Sd = torch.as_tensor(As, device=dev), torch.as_tensor(Ss, device=dev)
    x0 = torch.as_tensor(np.repeat(pb.X_true[:1], Kc, axis=0), device=dev)
    calls = [lambda: flt.smooth(Ad, Sd, kd, 300, trajectories=True, indices=True), lambda: flt.smooth(Ad, Sd, kd, 5, init_state=x0),
             lambda: flt.smooth(Ad, Sd, kd, 256, indices=True)]
    warm = [c() for c in calls]   # allocations may synchronise
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a.sum, b.sum) and torch.equal(a.sumsq, b.sumsq) and bool(torch.isfinite(a.sum).all())
    assert torch.equal(warm[0].idx, outs[0].idx) and torch.equal(warm[2].idx, outs[2].idx)


def test_refusals_are_clean_and_leave_the_context_usable():
    pb = experiments.smo_pgas(T=16)
    Kc, N, T, B = 2, 40, 16, 4
    keys, As, Ss = _draws(pb, Kc)
    flt = _filter_for(pb, N)
    eng = flt.engine
    good = flt.smooth(As, Ss, keys, B, indices=True)
    Ad, Sd, kd = torch.as_tensor(As, device=eng.device), torch.as_tensor(Ss, device=eng.device), ch.keys_tensor(keys, eng.device)
    xt, at = good.filter.x, good.filter.anc
    nv = pb.nx + 1
    s1, s2 = (torch.empty((Kc, T, nv), dtype=torch.float64, device=eng.device) for _ in range(2))
    idx = torch.empty((Kc, B, T), dtype=torch.int32, device=eng.device)
    PGAS_E_ARG = -1

    def call(Kn=Kc, Bn=B, b0=0, seeds=kd, S=Sd, x=xt, anc=at, ix=idx, xs=None, a=s1, b=s2):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = eng.lib.pgas_smooth(eng._h, Kn, Bn, b0, p(seeds), Ad.data_ptr(), p(S), p(x), p(anc), p(ix), p(xs), p(a), p(b), eng._stream())
        return rc, eng.lib.pgas_last_error(eng._h).decode()

    for kw, msg in [(dict(Kn=0), "K = 0"), (dict(Bn=0), "B = 0"), (dict(Bn=257), "B = 257"), (dict(b0=-1), "b0 = -1"), (dict(x=None), "NULL argument"),
                    (dict(anc=None), "NULL argument"), (dict(seeds=None), "seeds and S"), (dict(S=None), "seeds and S"), (dict(a=None), "sum and sumsq"),
                    (dict(b=None), "sum and sumsq"), (dict(ix=None, a=None, b=None), "every output is NULL")]:
        rc, err = call(**kw)
        assert rc == PGAS_E_ARG and msg in err, (kw, rc, err)
        again = flt.smooth(As, Ss, keys, B, indices=True)
        assert torch.equal(again.idx, good.idx) and torch.equal(again.sum, good.sum), f"smooth after refusing {kw}"
    rc, _ = call()
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(idx, good.idx) and torch.equal(s1, good.sum) and torch.equal(s2, good.sumsq)
    with pytest.raises(PgasError, match="seeds and S"):
        eng.smooth(Ad, None, kd, xt, at, B)
    # a context of more than one segment of particles has no one-workgroup variant
    big = pgas_amd.condSequentialMonteCarlo(5000, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    with pytest.raises(PgasError, match="no one-workgroup variant"):
        big.engine.smooth(Ad, Sd, kd, torch.zeros((Kc, T, 5000, pb.nx), dtype=torch.float64, device=eng.device),
                          torch.zeros((Kc, T, 5000), dtype=torch.int32, device=eng.device), B)
    with pytest.raises(ValueError, match="particles"):
        big.smooth(As, Ss, keys, B)
    traj = big(77, pb.X_true, As[0], Sd[0])
    assert bool(torch.isfinite(traj).all())
