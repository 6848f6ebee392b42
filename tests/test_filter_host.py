"""Host side of the held-out filter (pgas_amd/heldout.py), no GPU: the NumPy restatement of the definition
(tests/filter_numpy.py) against a plain float64 filter on the same particles, the argument checks of HeldOutFilter, and
evidence_summary on hand-made numbers."""
import functools

import numpy as np
import pytest
import torch

import filter_numpy as fn
from common import canon_model, experiments, pgas_amd
from pgas_amd import heldout
from pgas_amd import random as prng


@functools.lru_cache(maxsize=None)
def _problem(name):
    return {"smo": lambda: experiments.smo_pgas(T=40), "toy": lambda: experiments.toy(T=40)}[name]()


# ---- 0. the vectorised fma of the restatement is the exactly rounded one ---------------------------------------------------------------
def test_vectorised_fma_equals_the_rational_one():
    import rollout_stats_numpy as rs

    rng = np.random.default_rng(0)
    n = 4000
    a, b, c = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    ai, bi = rng.integers(1, 2 ** 27, n).astype(float), rng.integers(1, 2 ** 27, n).astype(float)
    ci = rng.integers(1, 2 ** 53, n).astype(float) * 2.0 ** rng.integers(-3, 3, n)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e200, -1e200, 1e-300, 5e-324, 1.0])
    A, B, C = (m.ravel() for m in np.meshgrid(sp, sp, sp))
    cases = [(a, b, c), (a, b, -(a * b)), (a, b, -(a * b) * (1 + 2.0 ** -30)), (a * 2.0 ** -53, b, np.round(c * 2 ** 20) / 2 ** 20),
             (a * 2.0 ** -54, b, np.ones(n)), (ai, bi, ci), (ai, bi * 2.0 ** -53, ci), (A, B, C)]   # cancellation, ties, special values
    for x, y, z in cases:
        got, want = fn.fma(x, y, z), np.asarray(rs.fma(x, y, z), dtype=np.float64)
        assert np.array_equal(got, want, equal_nan=True)
    pb = _problem("smo")
    lik = pb.likelihood_fcn
    xs = pb.X_true[:, None, :] + 0.05 * rng.standard_normal((pb.T, 50, pb.nx))
    for yrow in (np.array([0.3]), np.array([1e200]), np.array([np.nan])):
        assert np.array_equal(fn.loglik(xs, yrow, lik.H, lik.LRinv, lik.cR), rs.loglik(xs, yrow, lik.H, lik.LRinv, lik.cR), equal_nan=True)


# ---- 1. the restatement is a particle filter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 200, 257, 1024])
@pytest.mark.parametrize("name", ["smo", "toy"])
def test_restatement_agrees_with_a_float_filter_on_the_same_ancestors(name, N):
    pb = _problem(name)
    A, S = experiments.initial_params(pb)
    lik = pb.likelihood_fcn
    y = np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1)
    res = fn.run(canon_model(pb, N + 1), N, prng.key(1000), A, S, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), lik, y)
    ell, mean, ess = fn.float_filter(res, lik, y)
    assert np.isfinite(res["ell"]).all()
    assert np.abs(res["ell"] - ell).max() <= 1e-12                                   # fixed-point increment against logsumexp - log N
    got_mean = res["filt_sum"] / res["wtot"][:, None]
    assert np.all(np.abs(got_mean - mean) <= 1e-10 * np.abs(mean))
    assert np.all(np.abs(res["ess"] - ess) <= 1e-10 * ess)
    assert res["loglik"] == pytest.approx(ell.sum(), abs=1e-10)
    if N >= 200:   # the resampling is not trivial: some step keeps fewer distinct ancestors than N, none keeps one only
        distinct = np.array([len(np.unique(a)) for a in res["anc"]])
        assert distinct.min() < N and distinct.max() > 1
    # the predictive channels are the unweighted sums of the cloud
    v = np.concatenate([res["x"], res["x"] @ lik.H.T], axis=-1)
    assert np.allclose(res["pred_sum"], v.sum(axis=1), rtol=1e-12, atol=1e-300)
    assert np.allclose(res["pred_sumsq"], (v * v).sum(axis=1), rtol=1e-12, atol=1e-300)


def test_restatement_nan_row_and_outlier_row():
    pb = _problem("toy")
    N = 65
    A, S = experiments.initial_params(pb)
    lik = pb.likelihood_fcn
    y = np.asarray(pb.observations, dtype=np.float64).reshape(pb.T, -1).copy()
    y[5] = np.nan
    y[9] = 1e200
    toy = experiments.toy(T=40)
    toy.observations = y
    res = fn.run(canon_model(toy, N + 1), N, prng.key(3), A, S, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), lik, y)
    ident = np.arange(N)
    assert np.isnan(res["ell"][5]) and np.array_equal(res["anc"][5], ident) and res["ess"][5] == 0.0 and res["wtot"][5] == 0.0
    assert res["ell"][9] == -np.inf and np.array_equal(res["anc"][9], ident)
    assert res["loglik"] == -np.inf
    rest = np.delete(np.arange(pb.T), [5, 9])
    assert np.isfinite(res["ell"][rest]).all()


# ---- 2. every argument error is a ValueError before a device is touched --------------------------------------------------------------
def _filter(n_particles=32, **kw):
    pb = _problem("smo")
    args = dict(init_state_mean=pb.init_state_mean, init_state_cov=pb.init_state_cov)
    args.update(kw)
    return pb, pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, pb.nx, n_particles, **args)


def test_constructor_refusals():
    pb = _problem("smo")
    mk = lambda *a, **k: pgas_amd.HeldOutFilter(*a, **k)  # noqa: E731
    ok = (pb.observations, pb.inputs, pb.basis_fcn, pb.likelihood_fcn, pb.nx, 32)
    with pytest.raises(TypeError):
        mk(ok[0], ok[1], object(), *ok[3:])
    with pytest.raises(TypeError):
        mk(ok[0], ok[1], ok[2], lambda *a: 0.0, ok[4], ok[5])
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="n_particles"):
            mk(*ok[:5], bad)
    with pytest.raises(ValueError, match="n_x"):
        mk(*ok[:4], 0, 32)
    with pytest.raises(ValueError, match="likelihood_fcn"):
        mk(*ok[:4], 1, 32)
    with pytest.raises(ValueError, match="observations"):
        mk(np.zeros((pb.T, 3)), *ok[1:])
    with pytest.raises(ValueError, match="observations"):
        mk(np.zeros(0), *ok[1:])
    with pytest.raises(ValueError, match="inputs"):
        mk(ok[0], pb.inputs[:-1], *ok[2:])
    with pytest.raises(ValueError, match="go together"):
        mk(*ok, init_state_mean=pb.init_state_mean)
    with pytest.raises(ValueError, match="init_state_mean"):
        mk(*ok, init_state_mean=np.zeros(3), init_state_cov=np.eye(3))


def test_call_refusals_touch_no_device():
    pb, flt = _filter()
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
        (dict(keys=torch.zeros((K, 1), dtype=torch.int64)), "keys"),
        (dict(init_state=np.zeros((K, N + 1, nx))), "init_state"),
        (dict(init_state=np.zeros(nx + 1)), "init_state"),
    ]
    for kw, match in bad:
        args = dict(coeff_mat=A, error_cov=S, keys=keys)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            flt(**args)
    assert flt._engine is None
    _, bare = _filter(init_state_mean=None, init_state_cov=None)
    with pytest.raises(ValueError, match="init_state=None"):
        bare(A, S, keys)
    assert bare._engine is None
    assert heldout.check_call(nx, M, N, True, A, S, keys) == (K, 0)
    assert heldout.check_call(nx, M, N, False, A, S, keys, np.zeros(nx)) == (K, 1)
    assert heldout.check_call(nx, M, N, False, A, S, torch.zeros(K, dtype=torch.int64), np.zeros((K, nx))) == (K, 2)
    assert heldout.check_call(nx, M, N, False, A, S, keys, np.zeros((K, N, nx))) == (K, 3)
    with pytest.raises(ValueError, match="particles"):
        heldout.check_call(nx, M, 2048, True, A, S, keys)


# ---- 3. evidence_summary on hand-made numbers -----------------------------------------------------------------------------------------
def test_evidence_summary_by_hand():
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    # K = 2 draws, n = 2 particles, T = 2, nx = 1, ny = 1 (yhat = x): clouds {1, 3}, {5, 7} at t = 0 and {0, 0}, {2, 2} at t = 1
    res = heldout.FilterResult(
        2, 1, loglik=t([np.log(0.2), np.log(0.6)]), ell=t([[0.0, 0.0], [0.0, 0.0]]),
        pred_sum=t([[[4.0, 4.0], [0.0, 0.0]], [[12.0, 12.0], [4.0, 4.0]]]), pred_sumsq=t([[[10.0, 10.0], [0.0, 0.0]], [[74.0, 74.0], [8.0, 8.0]]]),
        filt_sum=t([[[1.5], [0.0]], [[3.0], [0.5]]]), wtot=t([[0.5, 0.25], [0.5, 0.25]]), ess=t([[2.0, 2.0], [2.0, 2.0]]))
    out = pgas_amd.evidence_summary(res, y=np.array([5.0, np.nan]))
    assert float(out["log_evidence"]) == pytest.approx(np.log(0.4), abs=1e-15)
    assert np.array_equal(out["x_pred_mean"].numpy(), [[4.0], [1.0]]) and np.array_equal(out["y_pred_mean"].numpy(), [[4.0], [1.0]])
    assert np.allclose(out["x_pred_std"].numpy(), [[np.sqrt(5.0)], [1.0]], rtol=1e-15)
    assert np.array_equal(out["x_filt_mean"].numpy(), [[[3.0], [0.0]], [[6.0], [2.0]]])
    assert np.array_equal(out["x_filt_mean_pooled"].numpy(), [[4.5], [1.0]])
    assert float(out["rmse"]) == 1.0            # the NaN row of y takes no part
    bare = heldout.FilterResult(2, 1, loglik=res.loglik, ell=res.ell)
    assert set(pgas_amd.evidence_summary(bare)) == {"log_evidence"}
    with pytest.raises(ValueError):
        pgas_amd.evidence_summary(bare, y=np.zeros(2))
    with pytest.raises(ValueError):
        pgas_amd.evidence_summary(res, y=np.zeros(3))
