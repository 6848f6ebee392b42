"""Host side of the in-kernel predictive moments and log score (pgas_amd.Rollout.predict, pgas_rollout_stats): the NumPy restatement of
the defined summation order (tests/rollout_stats_numpy.py), argument validation before any device is touched, predictive_summary on
CPU tensors, the C ABI binding, and that a Rollout built without the new arguments is the context it was.  No GPU."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import rollout_stats_numpy as rs
from common import ROOT, canon, experiments, pgas_amd
from pgas_amd import rollout as ro


@pytest.fixture(scope="module")
def sim():
    pb = experiments.smo_pgas(T=12)
    A, S = experiments.initial_params(pb)
    r = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov, likelihood_fcn=pb.likelihood_fcn, observations=pb.observations)
    return r, pb, np.repeat(A[None], 3, axis=0), np.repeat(S[None], 3, axis=0)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 63, 64, 255, 256, 257, 513, 1024, 1025, 2500])
def test_restated_order_agrees_with_np_sum(P):
    v = np.random.default_rng(P).standard_normal((3, 5, P)) * 10.0 ** np.random.default_rng(P + 1).integers(-3, 4, (3, 5, P))
    s1, s2 = rs.moments(v)
    scale1, scale2 = np.abs(v).sum(axis=-1), (v * v).sum(axis=-1)
    assert np.max(np.abs(s1 - v.sum(axis=-1)) / scale1) < 1e-12
    assert np.max(np.abs(s2 - scale2) / scale2) < 1e-12


def test_restated_order_is_the_literal_three_levels():
    P = 2500
    v = np.random.default_rng(7).standard_normal(P)
    pad = np.zeros(3 * 1024)
    pad[:P] = v
    total = 0.0
    for b in range(3):
        lanes = []
        for lane in range(256):
            s = 0.0
            for r in range(4):
                p = 1024 * b + 256 * r + lane
                if p < P:                    # over the replicates < P only
                    s = s + pad[p]
            lanes.append(s)
        while len(lanes) > 1:
            lanes = [lanes[i] + lanes[i + 1] for i in range(0, len(lanes), 2)]
        total = total + lanes[0]
    assert rs.reduce_sum(v) == total


@pytest.mark.parametrize("P", [1, 100, 256, 257, 512])
def test_restated_order_does_not_depend_on_the_register_rows(P):
    v = np.random.default_rng(P).standard_normal((4, P))
    v[0, 0] = -0.0
    full = rs.reduce_sum(v)
    for nr in (1, 2, 4):
        if P <= 256 * nr:
            got = rs.reduce_sum(v, nr)
            assert np.array_equal(got, full) and np.array_equal(np.signbit(got), np.signbit(full)), nr


def test_fraction_fma_is_correctly_rounded():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30           # a b = 1 - 2^-60: rounds to 1, so a b - 1 is 0 without the fusion
    assert rs._fma1(a, b, -1.0) == -(2.0 ** -60) and a * b - 1.0 == 0.0
    rng = np.random.default_rng(3)
    for x, y, z in rng.standard_normal((200, 3)):
        assert rs._fma1(x, y, z) == float(Fraction(x) * Fraction(y) + Fraction(z))
    assert math.isnan(rs._fma1(float("nan"), 1.0, 0.0)) and rs._fma1(1e200, 1e200, 0.0) == float("inf")


def test_restated_loglik_and_lpd_against_plain_numpy():
    rng = np.random.default_rng(11)
    lik = pgas_amd.GaussianLikelihood(np.array([[1.0, 0.0], [0.3, -1.7]]), np.array([[0.09, -0.02], [-0.02, 0.16]]))
    T, P = 4, 1500
    x = rng.standard_normal((T, P, 2))
    y = rng.standard_normal((T, 2))
    ll = rs.loglik(x, y[:, None, :], lik.H, lik.LRinv, lik.cR)
    want = np.array([[lik(y[t], x[t, p]) for p in range(P)] for t in range(T)])
    np.testing.assert_allclose(ll, want, rtol=1e-12)
    got = rs.lpd(ll, y, canon.det_exp, canon.det_log)
    m = want.max(axis=1)
    np.testing.assert_allclose(got, m + np.log(np.exp(want - m[:, None]).sum(axis=1)) - np.log(P), rtol=1e-12)
    # NaN takes no part in the max, a block without a finite l contributes nothing, a NaN observation row gives NaN
    ll2 = ll.copy()
    ll2[0, 5] = np.nan
    ll2[1, 1024:2048] = -np.inf
    ll2[2, :] = -np.inf
    y2 = y.copy()
    y2[3, 1] = np.nan
    got2 = rs.lpd(ll2, y2, canon.det_exp, canon.det_log)
    keep = np.ones(P, dtype=bool)
    keep[5] = False
    np.testing.assert_allclose(got2[0], m[0] + np.log(np.exp(want[0, keep] - m[0]).sum()) - np.log(P), rtol=1e-12)
    keep = np.ones(P, dtype=bool)
    keep[1024:2048] = False
    m1 = want[1, keep].max()
    np.testing.assert_allclose(got2[1], m1 + np.log(np.exp(want[1, keep] - m1).sum()) - np.log(P), rtol=1e-12)
    assert got2[2] == -np.inf and np.isnan(got2[3])


# ---- check_call ------------------------------------------------------------------------------------------------------------------------
def test_predict_refusals_are_value_errors_before_a_device_is_touched(sim):
    r, pb, As, Ss = sim
    keys = [1, 2, 3]
    x0 = np.zeros(2)
    bad = [
        ("coeff_mat", dict(coeff_mat=As[:, :, :-1], init_state=x0)),
        ("replicates", dict(coeff_mat=As, error_cov=Ss, keys=keys, replicates=0)),
        ("replicates must be <=", dict(coeff_mat=As, error_cov=Ss, keys=keys, replicates=(1 << 20) + 1)),
        ("needs keys", dict(coeff_mat=As, error_cov=Ss)),
        ("observation_noise needs keys", dict(coeff_mat=As, init_state=x0, observation_noise=True)),
        ("noise-free", dict(coeff_mat=As, init_state=x0, replicates=2)),
        ("init_state", dict(coeff_mat=As, error_cov=Ss, keys=keys, replicates=5, init_state=np.zeros((3, 4, 2)))),
    ]
    for msg, kw in bad:
        with pytest.raises(ValueError, match=msg):
            r.predict(**kw)
    assert r._engine is None, "a refused call created the device context"
    bare = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
    with pytest.raises(ValueError, match="needs observations"):
        bare.predict(As, Ss, keys, log_score=True)
    assert bare._engine is None
    with pytest.raises(ValueError, match="likelihood_fcn"):
        pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, observations=pb.observations)
    with pytest.raises(ValueError, match="observations"):
        pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, likelihood_fcn=pb.likelihood_fcn, observations=np.zeros(pb.T + 1))
    with pytest.raises(TypeError):
        pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, likelihood_fcn=lambda y, x, u: 0.0)


def test_check_call_extensions(sim):
    r, pb, As, Ss = sim
    M = As.shape[2]
    assert ro.check_call(2, M, True, As, Ss, [1, 2, 3], 1 << 20, predict=True) == (3, 1 << 20, 0)
    assert ro.check_call(2, M, True, As, Ss, [1, 2, 3], 7, predict=True, observation_noise=True, log_score=True, has_observations=True) == (3, 7, 0)
    assert ro.check_call(2, M, False, As, None, None, 5, np.zeros((3, 5, 2)), predict=True, log_score=False) == (3, 5, 3)
    # a materialised rollout keeps its own limits: replicates beyond 2^20 are chunked there
    assert ro.check_call(2, M, True, As, Ss, [1, 2, 3], (1 << 20) + 1) == (3, (1 << 20) + 1, 0)
    with pytest.raises(ValueError, match="needs observations"):
        ro.check_call(2, M, True, As, Ss, [1, 2, 3], 7, predict=True, log_score=True)
    for n in ("predictive_summary", "Rollout"):
        assert n in pgas_amd.__all__ and hasattr(pgas_amd, n)
    for cls in (pgas_amd.Rollout, pgas_amd.condSequentialMonteCarlo, pgas_amd.condSequentialMonteCarloChains):
        assert callable(getattr(cls, "predict"))


def test_rollout_without_the_new_arguments_builds_the_context_it_built_before():
    pb = experiments.smo_pgas(T=12)
    r = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
    N, y, u, m0, P0, lik, basis = r._engine_args()
    assert N == 1 and y.shape == (12, 1) and not y.any() and u is r.inputs and basis is pb.basis_fcn
    assert np.array_equal(m0, pb.init_state_mean) and np.array_equal(P0, pb.init_state_cov)
    assert isinstance(lik, pgas_amd.GaussianLikelihood) and np.array_equal(lik.H, np.eye(1, 2)) and np.array_equal(lik.R, np.eye(1))
    assert not r.has_observations and r.likelihood_fcn is None
    r2 = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov, None, pb.likelihood_fcn, pb.observations)
    a = r2._engine_args()
    assert a[5] is pb.likelihood_fcn and np.array_equal(a[1], np.asarray(pb.observations, dtype=np.float64).reshape(12, -1)) and r2.has_observations


# ---- predictive_summary -----------------------------------------------------------------------------------------------------------------
def test_predictive_summary_against_direct_numpy():
    rng = np.random.default_rng(5)
    K, T, P, nx, ny = 3, 6, 50, 2, 1
    x = rng.standard_normal((K, T, P, nx))
    yh = x[..., :1] * 2.0 + 0.1 * rng.standard_normal((K, T, P, ny))
    x[1, 2] = 0.5                                   # a constant channel: the clamped variance gives exactly 0, never NaN
    lpd = rng.standard_normal((K, T)) - 3.0
    lpd[:, 4] = -np.inf
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)   # noqa: E731
    st = ro.PredictiveStats(P, t(x.sum(axis=2)), t((x * x).sum(axis=2)), t(yh.sum(axis=2)), t((yh * yh).sum(axis=2)), t(lpd))
    y = rng.standard_normal((T, ny))
    s = pgas_amd.predictive_summary(st, y=y)
    np.testing.assert_allclose(s["x_mean"].numpy(), x.mean(axis=2), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(s["x_std"].numpy(), x.std(axis=2), rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(s["y_mean"].numpy(), yh.mean(axis=2), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(s["y_std"].numpy(), yh.std(axis=2), rtol=1e-9)
    assert not torch.isnan(s["x_std"]).any() and float(s["x_std"][1, 2].max()) < 1e-7
    pool = lambda a: np.moveaxis(a, 1, 0).reshape(T, K * P, -1)   # noqa: E731
    np.testing.assert_allclose(s["x_mean_pooled"].numpy(), pool(x).mean(axis=1), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(s["x_std_pooled"].numpy(), pool(x).std(axis=1), rtol=1e-9)
    np.testing.assert_allclose(s["y_std_pooled"].numpy(), pool(yh).std(axis=1), rtol=1e-9)
    np.testing.assert_allclose(float(s["rmse"]), np.sqrt(np.mean((pool(yh).mean(axis=1) - y) ** 2)), rtol=1e-12)
    m = lpd.max(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(m == -np.inf, -np.inf, m + np.log(np.exp(lpd - np.where(m == -np.inf, 0.0, m)).sum(axis=0))) - np.log(K)
    np.testing.assert_allclose(s["elpd_t"].numpy(), want, rtol=1e-12)
    assert float(s["elpd"]) == -np.inf
    s2 = pgas_amd.predictive_summary(ro.PredictiveStats(P, st.x_sum, st.x_sumsq, st.y_sum, st.y_sumsq, None))
    assert "rmse" not in s2 and "elpd" not in s2
    with pytest.raises(ValueError):
        pgas_amd.predictive_summary(st, y=np.zeros((T, 2)))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_rollout_stats_is_declared_and_bound_with_matching_argument_counts():
    from pgas_amd import _lib

    txt = open(os.path.join(ROOT, "include", "pgas_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+pgas_rollout_stats\s*\(([^)]*)\)\s*;", txt)
    assert m, "pgas_rollout_stats is not declared in include/pgas_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14
    assert "pgas_rollout_stats" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "pgas_rollout_stats")
    assert L.pgas_rollout_stats.restype is not None and len(L.pgas_rollout_stats.argtypes) == len(params)
    want = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for p, a in zip(params, L.pgas_rollout_stats.argtypes):
        if "*" in p:
            assert a is C.c_void_p, p
        else:
            assert a is want[p.split()[0]], p
    canon_h = open(os.path.join(ROOT, "include", "pgas_canon.h")).read()
    ids = re.findall(r"#define\s+PGAS_STREAM_(\w+)\s+(\d+)u", canon_h)
    assert ("OBS", "6") in ids and len({v for _, v in ids}) == len(ids), "stream ids must be distinct"
