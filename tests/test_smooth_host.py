"""Host side of the held-out smoother (pgas_amd/heldout.py), no GPU: the NumPy restatement of pgas_smooth's
definition (tests/smooth_numpy.py) against the oracle's uniform, a plain float64 FFBSi on the same trace and uniforms, and the exact
forward-filter / backward-smoother marginals; the argument checks of HeldOutFilter.smooth; smoothing_summary on hand-made numbers."""
import functools

import numpy as np
import pytest
import torch

import filter_numpy as fn
import smooth_numpy as sn
from common import canon, canon_model, experiments, pgas_amd
from pgas_amd import heldout
from pgas_amd import random as prng

T, B = 40, 64
NS = [1, 2, 65, 200]


@functools.lru_cache(maxsize=None)
def _problem(name, T=T):
    return {"smo": lambda: experiments.smo_pgas(T=T), "toy": lambda: experiments.toy(T=T)}[name]()


@functools.lru_cache(maxsize=None)
def _case(name, N, T=T, n_traj=B, seed=1000):
    """(pb, cm1, A, S, y, flt, res): the filter's restatement and n_traj backward trajectories over its trace, computed once."""
    pb = _problem(name, T)
    A, S = experiments.initial_params(pb)
    y = np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1)
    cm1 = canon_model(pb, N + 1)
    key = prng.key(seed)
    flt = fn.run(cm1, N, key, A, S, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), pb.likelihood_fcn, y)
    res = sn.run_chunks(cm1, N, key, A, S, flt, pb.likelihood_fcn, y, n_traj)
    return pb, cm1, A, S, y, flt, res


# ---- (a) the transcribed primitives -------------------------------------------------------------------------------------------------
def test_transcribed_uniform_equals_the_oracle_at_particle_zero():
    for seed in (0, 1, 1000, 2 ** 63 + 12345, 2 ** 64 - 1, prng.key(7)):
        for stream in (canon.STREAM_RESAMPLE, canon.STREAM_ANCESTOR, canon.STREAM_FINAL):
            for t in (0, 1, 39, 1999, 2 ** 31):
                assert sn.uniform(seed, t, 0, stream) == canon.uniform(seed, stream, t)
    us = np.array([sn.uniform(1000, t, g) for t in range(8) for g in (0, 1, 255, 256, 2 ** 32 + 5)])
    assert ((us > 0) & (us < 1)).all() and len(np.unique(us)) == us.size      # the trajectory number and the row both reach the counter


def test_numpy_conversion_of_the_cumsum_is_the_oracle_conversion():
    rng = np.random.default_rng(5)
    c = np.concatenate([rng.integers(0, 2 ** 62, 2000, dtype=np.uint64), np.array([0, 1, 2 ** 53 - 1, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 61 + 2 ** 8 + 1], np.uint64)])
    u64 = canon.lib().oc_u64_to_double
    assert np.array_equal(sn.u64_to_double(c), np.array([u64(int(v)) for v in c]))


# ---- (b), (c) the restatement is a backward simulation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", ["smo", "toy"])
def test_restatement_agrees_with_a_float_ffbsi_on_the_same_trace_and_uniforms(name, N):
    pb, cm1, A, S, y, flt, res = _case(name, N)
    assert res["idx"].shape == (B, pb.T) and (res["idx"] >= 0).all() and (res["idx"] < N).all()
    assert ((res["S"] > 0) & np.isfinite(res["S"])).all()                     # no fall-back row in these cases
    assert np.array_equal(res["xs"], np.stack([flt["x"][t][res["idx"][:, t]] for t in range(pb.T)], axis=1))
    want = sn.float_indices(cm1, N, A, S, flt, pb.likelihood_fcn, y, res)
    differ = int(np.count_nonzero(want != res["idx"]))
    print(f"{name}, N = {N}: {differ} of {want.size} indices differ from the float FFBSi")
    assert differ <= 0.005 * want.size
    assert np.abs(want - res["idx"]).max() <= 1                              # ... and then by one position: u S at a CDF boundary
    ch = np.concatenate([res["xs"], res["xs"] @ np.atleast_2d(pb.likelihood_fcn.H).T], axis=-1)
    assert np.allclose(res["sum"], ch.sum(axis=0), rtol=1e-12, atol=1e-300)
    assert np.allclose(res["sumsq"], (ch * ch).sum(axis=0), rtol=1e-12, atol=1e-300)
    if N == 200:   # (c) the backward weights are not trivial: most draws leave the filter's genealogy
        left = np.array([(res["idx"][:, t] != flt["anc"][t][res["idx"][:, t + 1]]).mean() for t in range(pb.T - 1)])
        print(f"{name}: mean share of j_t != anc[t, j_t+1] = {left.mean():.3f}")
        assert left.mean() > 0.5
        assert len({tuple(r) for r in res["idx"]}) == B                       # and the trajectories differ from each other


def check_marginals(idx, w, n):
    """(d): idx (n, T) drawn indices, w (T, N) the exact marginals.  Over the cells with n w >= 20 every count lies within 4.5 binomial
    standard deviations; those cells carry >= 90 % of each row's mass; there are at most 48 of them."""
    Tn, N = w.shape
    cells = 0
    for t in range(Tn):
        big = n * w[t] >= 20.0
        assert w[t][big].sum() >= 0.9, f"row {t}: the tested cells carry {w[t][big].sum():.3f} of the mass"
        cnt = np.bincount(idx[:, t], minlength=N)
        sd = np.sqrt(n * w[t] * (1.0 - w[t]))
        z = np.abs(cnt - n * w[t])[big] / np.maximum(sd[big], 1e-300)
        print(f"row {t}: cells {int(big.sum())}, worst z = {z.max():.2f}")
        assert (np.abs(cnt - n * w[t])[big] <= 4.5 * sd[big]).all(), f"row {t}: counts {cnt}, expected {n * w[t]}"
        cells += int(big.sum())
    assert cells <= 48


@pytest.mark.parametrize("name", ["toy", "smo"])
def test_marginal_of_the_drawn_indices_is_the_exact_smoother_marginal(name):
    N, Tn, n = 8, 6, 4096
    pb, cm1, A, S, y, flt, res = _case(name, N, T=Tn, n_traj=n)
    w = sn.smoother_marginals(cm1, N, A, S, flt, pb.likelihood_fcn, y)
    assert np.allclose(w.sum(axis=1), 1.0, atol=1e-12)
    assert res["idx"].shape == (n, Tn)
    check_marginals(res["idx"], w, n)


def test_restatement_fallback_rows():
    """A NaN observation row has uniform filter weights (the transition density alone decides); a row at 1e200 has no weight at all and
    follows the filter's genealogy, which is the identity there."""
    pb = _problem("toy")
    N = 65
    A, S = experiments.initial_params(pb)
    y = np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1).copy()
    y[5], y[9], y[pb.T - 1] = np.nan, 1e200, 1e200
    toy = experiments.toy(T=T)
    toy.observations = y
    cm1 = canon_model(toy, N + 1)
    key = prng.key(3)
    flt = fn.run(cm1, N, key, A, S, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), pb.likelihood_fcn, y)
    res = sn.run(cm1, N, key, A, S, flt, pb.likelihood_fcn, y, 16, b0=60)
    assert (res["S"][:, [9, pb.T - 1]] == 0.0).all() and (np.delete(res["S"], [9, pb.T - 1], axis=1) > 0).all()
    assert np.array_equal(res["idx"][:, pb.T - 1], (60 + np.arange(16)) % N)
    assert np.array_equal(res["idx"][:, 9], res["idx"][:, 10])                # anc[9] is the identity
    assert len(np.unique(res["idx"][:, 5])) > 1


# ---- (e) every argument error is a ValueError before a device is touched -------------------------------------------------------------
def test_smooth_refusals_touch_no_device():
    pb = _problem("smo")
    flt = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, pb.nx, 32, pb.init_state_mean, pb.init_state_cov)
    nx, M, K, N = pb.nx, pb.basis_fcn.basis.M, 3, 32
    A, S, keys = np.zeros((K, nx, M)), np.stack([np.eye(nx)] * K), [1, 2, 3]
    bad = [
        (dict(coeff_mat=np.zeros((nx, M))), "coeff_mat"),
        (dict(coeff_mat=np.zeros((K, nx, M + 1))), "coeff_mat"),
        (dict(coeff_mat=np.zeros((0, nx, M)), error_cov=np.zeros((0, nx, nx)), keys=[]), "K must be"),
        (dict(error_cov=None), "error_cov"),
        (dict(error_cov=np.zeros((K + 1, nx, nx))), "error_cov"),
        (dict(keys=None), "keys"),
        (dict(keys=[1, 2]), "keys"),
        (dict(keys=torch.zeros(K, dtype=torch.int32)), "keys"),
        (dict(init_state=np.zeros((K, N + 1, nx))), "init_state"),
        (dict(n_trajectories=0), "n_trajectories"),
        (dict(n_trajectories=-4), "n_trajectories"),
        (dict(n_trajectories=65537), "n_trajectories"),
        (dict(n_trajectories=2.0), "n_trajectories"),
        (dict(n_trajectories=True), "n_trajectories"),
        (dict(n_trajectories=None), "n_trajectories"),
        (dict(n_trajectories="8"), "n_trajectories"),
    ]
    for kw, match in bad:
        args = dict(coeff_mat=A, error_cov=S, keys=keys, n_trajectories=8)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            flt.smooth(**args)
    assert flt._engine is None
    bare = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, pb.nx, 32)
    with pytest.raises(ValueError, match="init_state=None"):
        bare.smooth(A, S, keys, 8)
    assert bare._engine is None
    assert heldout.check_smooth(nx, M, N, True, A, S, keys, 1) == (K, 0, 1)
    assert heldout.check_smooth(nx, M, N, False, A, S, keys, np.int64(65536), np.zeros((K, nx))) == (K, 2, 65536)
    with pytest.raises(ValueError, match="particles"):
        heldout.check_smooth(nx, M, 2048, True, A, S, keys, 8)


# ---- smoothing_summary on hand-made numbers -----------------------------------------------------------------------------------------
def test_smoothing_summary_by_hand():
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    # K = 2 draws, 2 trajectories, T = 2, nx = 1, ny = 1 (yhat = x): trajectories {1, 3}, {5, 7} at t = 0 and {0, 0}, {2, 2} at t = 1
    flt = heldout.FilterResult(4, 1)
    res = heldout.SmoothResult(flt, 2, t([[[4.0, 4.0], [0.0, 0.0]], [[12.0, 12.0], [4.0, 4.0]]]), t([[[10.0, 10.0], [0.0, 0.0]], [[74.0, 74.0], [8.0, 8.0]]]))
    assert res.xs is None and res.idx is None and res.n == 4 and res.nx == 1
    out = pgas_amd.smoothing_summary(res, y=np.array([5.0, np.nan]))
    assert np.array_equal(out["x_smooth_mean"].numpy(), [[4.0], [1.0]]) and np.array_equal(out["y_smooth_mean"].numpy(), [[4.0], [1.0]])
    assert np.allclose(out["x_smooth_std"].numpy(), [[np.sqrt(5.0)], [1.0]], rtol=1e-15)
    assert np.array_equal(out["x_smooth_mean_draw"].numpy(), [[[2.0], [0.0]], [[6.0], [2.0]]])
    assert float(out["rmse"]) == 1.0            # the NaN row of y takes no part
    assert "rmse" not in pgas_amd.smoothing_summary(res)
    with pytest.raises(ValueError):
        pgas_amd.smoothing_summary(res, y=np.zeros(3))
