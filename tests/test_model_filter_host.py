"""Host side of the grey-box held-out filter (pgas_amd.ModelRollout.filter, pgas_m_filter), no GPU: the NumPy
restatement (tests/model_filter_numpy.py) against a plain float64 filter on the same ancestors, every refusal of ``filter`` before a
device is touched, max_particles() against its formula, the C ABI binding -- and the two properties the GPU tests lean on: that the
resampling on the models' records is not the identity, and that the Kalman comparison has room at the sizes the GPU test uses."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import model_filter_cases as cases
import model_filter_numpy as mf
import model_rollout_numpy as mrn
import model_rollout_stats_numpy as ms
from common import ROOT, canon, experiments, pgas_amd
from pgas_amd import model_rollout as mr
from test_model_rollout_stats_host import _c_struct_layout

K, T = cases.K, cases.T


# ---- a plain NumPy filter of one draw on a model's record -------------------------------------------------------------------------------
def _numpy_filter(name, k, N, seed, key=None):
    """Draw k of the test coefficients, N particles, NumPy's own random numbers; key: resample with the canonical scan and search on that
    key (the restatement's ancestors) instead of NumPy's systematic resampling."""
    pb, _, R = cases.problem(name)
    lat, model = [mrn.Latent(b) for b in pb.basis], pb.model(np)
    A = [a[k] for a in cases.coeffs(pb)]
    rng = np.random.default_rng(seed)
    u = np.asarray(pb.inputs[:T], dtype=np.float64).reshape(T, -1)
    y = np.asarray(pb.observations[:T], dtype=np.float64).reshape(T, -1)
    nx = len(pb.init_state_mean)
    x0 = np.asarray(pb.init_state_mean) + rng.standard_normal((N, nx)) @ np.linalg.cholesky(pb.init_state_cov).T
    Qc = np.linalg.cholesky(pb.process_noise) if np.any(pb.process_noise) else None
    resample = loglik = None
    if key is not None:
        LR = np.linalg.cholesky(R)
        LRinv, cR = np.linalg.inv(LR), -0.5 * R.shape[0] * np.log(2 * np.pi) - np.sum(np.log(np.diag(LR)))
        loglik = lambda yh, yt: ms.loglik(yh, yt[None, :], LRinv, cR)  # noqa: E731  (the device's operations)

        def resample(t, l):
            segm, segs, c = canon.segment_partials(l)
            return canon.resample_range(segm, segs, c, N, canon.uniform(key, canon.STREAM_M_RESAMPLE, t), 0, N)
    return mf.bootstrap(lambda t, x: mrn.step(model, lat, A, x, u[t], rng.standard_normal((N, nx)) if Qc is not None else None, Qc)[2],
                        lambda t, x: mrn.step(model, lat, A, x, u[t])[1], x0, y, R, rng.random(T), resample, loglik), y


# ---- 1. the restatement is a particle filter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 200, 257, 1024])
@pytest.mark.parametrize("name", ["smo", "toy"])
def test_restatement_agrees_with_a_float_filter_on_the_same_ancestors(name, N):
    key = 1000 + N
    res, y = _numpy_filter(name, 0, N, seed=N, key=key)
    _, _, R = cases.problem(name)
    lw = res["lw"]
    assert np.abs(lw - mf.gauss_loglik(res["yhat"], y[:, None, :], R)).max() <= 1e-9 * np.abs(lw).max()   # mode 2's operations ARE the Gaussian log-density
    got = mf.run(key, lw, res["x"], res["yhat"], y)
    ell, mean, ess = mf.float_filter(lw, res["x"])
    assert np.isfinite(got["ell"]).all()
    assert np.abs(got["ell"] - ell).max() <= 1e-12                                     # fixed-point increment against logsumexp - log N
    got_mean = got["filt_sum"] / got["wtot"][:, None]
    assert np.all(np.abs(got_mean - mean) <= 1e-10 * np.abs(mean))
    assert np.all(np.abs(got["ess"] - ess) <= 1e-10 * ess)
    assert got["loglik"] == pytest.approx(ell.sum(), abs=1e-10)
    assert np.array_equal(got["anc"], res["anc"])                                      # the same ancestors
    v = np.concatenate([res["x"], res["yhat"]], axis=-1)
    assert np.allclose(got["pred_sum"], v.sum(axis=1), rtol=1e-12, atol=1e-300)
    assert np.allclose(got["pred_sumsq"], (v * v).sum(axis=1), rtol=1e-12, atol=1e-300)


def test_restatement_nan_row_and_outlier_row():
    res, y = _numpy_filter("toy", 0, 65, seed=3)
    y = y.copy()
    y[5], y[9] = np.nan, 1e200
    _, _, R = cases.problem("toy")
    LRinv, cR = np.linalg.inv(np.linalg.cholesky(R)), 0.0
    lw = ms.loglik(res["yhat"], y[:, None, :], LRinv, cR)
    got = mf.run(7, lw, res["x"], res["yhat"], y)
    ident = np.arange(65)
    assert np.isnan(got["ell"][5]) and np.array_equal(got["anc"][5], ident) and got["ess"][5] == 0.0 and got["wtot"][5] == 0.0
    assert got["ell"][9] == -np.inf and np.array_equal(got["anc"][9], ident)
    assert got["loglik"] == -np.inf
    assert np.isfinite(got["ell"][np.delete(np.arange(T), [5, 9])]).all()


# ---- 2. the GPU tests do not pass on identity ancestors ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _max_particles(name):
    return cases.rollout(name)[2].max_particles()


@pytest.mark.parametrize("name", list(cases.MODELS))
def test_resampling_is_not_trivial(name):
    """For every N >= 64 the GPU tests use on this model: some step of a plain NumPy filter on the model's record, under the output noise
    the GPU tests use, keeps at most 0.8 N distinct ancestors."""
    ns = [n for n in cases.NS if 64 <= n <= _max_particles(name)] + ([1024] if name == "toy" else [])
    assert ns
    for N in ns:
        res, _ = _numpy_filter(name, 0, N, seed=N)
        distinct = np.array([len(np.unique(a)) for a in res["anc"]])
        assert distinct.min() <= 0.8 * N, f"{name}, N = {N}: at least {distinct.min()} distinct ancestors at every step"
        assert distinct.max() > 1


# ---- 3. the Kalman test has room ---------------------------------------------------------------------------------------------------------
def test_the_kalman_comparison_has_room_at_the_sizes_the_gpu_test_uses():
    kal = cases.KAL
    y = cases.kalman_record()
    want = mf.kalman_loglik(kal["a"], kal["q"], kal["r"], kal["m0"], kal["p0"], y)
    ll = []
    for s in range(kal["seeds"]):
        rng = np.random.default_rng(100 + s)
        x0 = kal["m0"] + np.sqrt(kal["p0"]) * rng.standard_normal((kal["N"], 1))
        res = mf.bootstrap(lambda t, x: kal["a"] * x + np.sqrt(kal["q"]) * rng.standard_normal(x.shape), lambda t, x: x, x0, y.reshape(-1, 1),
                           np.array([[kal["r"]]]), rng.random(kal["T"]))
        ll.append(res["loglik"])
    ll = np.array(ll)
    se = ll.std(ddof=1) / np.sqrt(len(ll))
    assert abs(ll.mean() - want) <= 2 * se, f"mean {ll.mean():.4f}, Kalman {want:.4f}, standard error {se:.4f}"


# ---- 4. every refusal of filter is a ValueError before a device is touched ---------------------------------------------------------------
def test_every_filter_refusal_is_raised_without_a_device():
    pb, ssm, sim = cases.rollout("smo")
    A = cases.coeffs(pb)
    keys, x0, N = [1, 2, 3], np.zeros(2), 70
    assert sim.check_filter(A, keys, N) == (3, N, 0, True, False)
    assert sim.check_filter(A, keys, sim.max_particles(), x0) == (3, sim.max_particles(), 1, True, False)
    assert sim.check_filter(A, torch.zeros(3, dtype=torch.int64), N, np.zeros((3, N, 2)), process_noise=False) == (3, N, 3, False, False)
    assert sim.check_filter(A, keys, N, x0, row_cov=[np.stack([np.eye(1)] * 3)], process_noise=False) == (3, N, 1, False, True)
    assert sim.check_filter(A, keys, 1, x0, process_noise=False)[1] == 1             # one particle is no copy of anything
    bad = [
        (dict(particles=0), "particles"),
        (dict(particles=sim.max_particles() + 1), "particles"),
        (dict(particles=1025), "particles"),
        (dict(keys=None), "keys"),
        (dict(keys=[1, 2]), "expected 3 keys"),
        (dict(keys=torch.zeros(3, dtype=torch.int32)), "keys"),
        (dict(coeffs=A[0]), "list of 1"),
        (dict(coeffs=[A[0][:, :, :-1]]), r"coeffs\[0\]"),
        (dict(init_state=np.zeros((3, N + 1, 2))), "init_state"),
        (dict(init_state=np.zeros(3)), "init_state"),
        (dict(row_cov=[np.zeros((3, 2, 2))]), r"row_cov\[0\]"),
        (dict(init_state=x0, process_noise=False), "copies"),
        (dict(init_state=np.zeros((3, 2)), process_noise=False), "copies"),
    ]
    for kw, msg in bad:
        args = dict(coeffs=A, keys=keys, particles=N)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            sim.filter(**args)
    _, _, bare = cases.rollout("smo", has_obs=False)
    with pytest.raises(ValueError, match="needs observations"):
        bare.filter(A, keys, N)
    wide = pgas_amd.SymbolicStateSpaceModel(pb.process_noise, np.diag([1e-3, 1e-3]), pb.model)   # ny = 1 under a 2 x 2 output noise
    odd = pgas_amd.ModelRollout(pb.inputs[:T], wide, pb.basis, pb.init_state_mean, pb.init_state_cov, observations=pb.observations[:T])
    with pytest.raises(ValueError, match="output_noise"):
        odd.filter(A, keys, N)
    noinit = pgas_amd.ModelRollout(pb.inputs[:T], ssm, pb.basis, observations=pb.observations[:T])
    with pytest.raises(ValueError, match="construct the ModelRollout with both"):
        noinit.filter(A, keys, N)
    for s in (sim, bare, odd, noinit):
        assert s._ops is None and s._dev_cache is None, "a refused call created the device context"


# ---- 5. max_particles() ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.MODELS))
def test_max_particles_is_the_formula(name):
    _, _, sim = cases.rollout(name)
    nz = max(sim.nx, max(sim.widths), sim.ny, sim.nx + sum(sim.widths))
    file_bytes = (sim.n_reg + nz) * 512
    coef = 8 * sum(w * h.M for w, h in zip(sim.widths, sim.latents))
    assert mr.LDS_PER_WORKGROUP == 160 * 1024 and mr.FILTER_STATIC_LDS == 42416
    files = (mr.LDS_PER_WORKGROUP - mr.FILTER_STATIC_LDS - coef) // file_bytes
    want = min(1024, 64 * files)
    assert sim.max_particles() == want and want >= 200 and sim._ops is None
    assert sim.filter_lds_bytes(want) + mr.FILTER_STATIC_LDS <= mr.LDS_PER_WORKGROUP
    assert want == 1024 or sim.filter_lds_bytes(want + 1) + mr.FILTER_STATIC_LDS > mr.LDS_PER_WORKGROUP
    for N in (1, 64, 65, 200):
        assert sim.filter_lds_bytes(N) == -(-N // 64) * file_bytes + coef
    assert {"smo": 8192, "vehicle": 13824}.get(name, file_bytes) == file_bytes       # the 8 KB and 13 KB files of DESIGN.md section 16
    assert (name != "toy" or want == 1024) and (name != "vehicle" or want == 512)


# ---- 6. C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_filter_is_declared_and_bound_and_the_ctypes_struct_is_the_c_struct():
    from pgas_amd import _lib

    txt = open(os.path.join(ROOT, "include", "pgas_marginal.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+pgas_m_filter\s*\(([^)]*)\)\s*;", txt)
    assert m, "pgas_m_filter is not declared in include/pgas_marginal.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 4 and "pgas_m_rollout_desc" in params[1] and "pgas_m_filter_desc" in params[2]
    fields, size = _c_struct_layout(txt, "pgas_m_filter_desc")
    S = _lib.ModelFilterDesc
    assert C.sizeof(S) == size == 12 * 8 + 8 + 64 * 8
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == fields
    assert [n for n, _ in S._fields_][:12] == ["y_dev"] + [f + "_dev" for f in ("ell", "loglik", "ess", "pred_sum", "pred_sumsq", "filt_sum", "wtot", "x", "anc", "lw",
                                                                                 "yhat")]
    assert "pgas_m_filter" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "pgas_m_filter")
    assert L.pgas_m_filter.restype is C.c_int and len(L.pgas_m_filter.argtypes) == 4
    assert callable(_lib.MarginalOps.model_filter)
    R = pgas_amd.ModelFilterResult
    assert issubclass(R, pgas_amd.heldout.FilterResult) and R.FIELDS == pgas_amd.heldout.FilterResult.FIELDS + ("lw", "yhat")
    assert pgas_amd.heldout.FilterResult.FIELDS == ("loglik", "ell", "ess", "pred_sum", "pred_sumsq", "filt_sum", "wtot", "x", "anc")
    r = R(4, 1, loglik=torch.zeros(2, dtype=torch.float64), ell=torch.zeros((2, 3), dtype=torch.float64))
    assert r.lw is None and r.yhat is None and set(pgas_amd.evidence_summary(r)) == {"log_evidence"}
