"""Host side of the grey-box rollout's in-kernel predictive moments and log score (pgas_amd.ModelRollout.predict, pgas_m_rollout_stats,
DESIGN.md section 14): the NumPy restatement of the defined order (tests/model_rollout_stats_numpy.py), every refusal of ``predict``
before a device is touched, and the C ABI binding.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import model_rollout_stats_numpy as ms
from common import ROOT, canon, experiments, pgas_amd
from pgas_amd import model_rollout as mr


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _literal(v, padded):
    """Blocks of 64 in ascending order from +0.0; inside a block the adjacent-pair tree, written as loops.  padded: lanes >= P hold +0.0;
    otherwise a pair whose right partner has no replicate passes the left value on and a pair without replicates does not exist."""
    P = len(v)
    total = 0.0
    for b in range((P + 63) // 64):
        lanes = [float(v[64 * b + i]) if 64 * b + i < P else (0.0 if padded else None) for i in range(64)]
        while len(lanes) > 1:
            nxt = []
            for i in range(0, len(lanes), 2):
                a, c = lanes[i], lanes[i + 1]
                nxt.append(a + c if a is not None and c is not None else a if c is None else c)
            lanes = nxt
        total = total + lanes[0]
    return total


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 128, 129, 1000])
def test_the_tree_is_the_literal_nested_loop_and_padding_is_replicates_below_P_only(P):
    rng = np.random.default_rng(P)
    v = rng.standard_normal((2, P)) * 10.0 ** rng.integers(-3, 4, (2, P))
    got1, got2 = ms.moments(v)
    for r in range(2):
        assert got1[r] == _literal(v[r], padded=True) == _literal(v[r], padded=False)
        assert got2[r] == _literal(v[r] * v[r], padded=True) == _literal(v[r] * v[r], padded=False)
    assert np.max(np.abs(got1 - v.sum(axis=-1)) / np.abs(v).sum(axis=-1)) < 1e-13


def test_restated_log_density_is_mode_2_in_plain_numpy():
    rng = np.random.default_rng(2)
    R = np.array([[0.09, -0.021], [-0.021, 0.1649]])
    LR = np.linalg.cholesky(R)
    LRinv, cR = np.linalg.inv(LR), -np.log(2 * np.pi) - np.sum(np.log(np.diag(LR)))
    g, y = rng.standard_normal((5, 7, 2)), rng.standard_normal((5, 1, 2))
    got = ms.loglik(g, y, LRinv, cR)
    d = y - g
    want = -np.log(2 * np.pi) - 0.5 * np.log(np.linalg.det(R)) - 0.5 * np.einsum("...i,ij,...j->...", d, np.linalg.inv(R), d)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    e0 = (0.0 + d[..., 0] * LRinv[0, 0]) + d[..., 1] * LRinv[0, 1]          # ALL l, the zero above the diagonal included
    e1 = (0.0 + d[..., 0] * LRinv[1, 0]) + d[..., 1] * LRinv[1, 1]
    assert np.array_equal(got, cR - 0.5 * ((0.0 + e0 * e0) + e1 * e1))
    yh = ms.predicted_obs(g, LR, rng.standard_normal((5, 7, 2)))
    assert yh.shape == g.shape and not np.array_equal(yh, g) and np.array_equal(ms.predicted_obs(g), g)


def test_restated_lpd_on_hand_built_log_densities():
    de, dl = canon.det_exp, canon.det_log
    T, P = 6, 129                                                          # blocks of 64, 64 and 1
    y = np.zeros((T, 1))
    y[4, 0] = np.nan
    ll = np.full((T, P), -2.5)                                            # row 0: all equal -> that value
    ll[1, 64:128] = -np.inf                                               # row 1: one block without a finite l
    ll[2, 7] = np.nan                                                     # row 2: a NaN l takes no part
    ll[3] = -np.inf                                                       # row 3: nothing finite -> -inf
    ll[5, :] = np.linspace(-30.0, -1.0, P)                                # row 5: against plain NumPy
    got = ms.lpd(ll, y, de, dl)
    logP = float(dl(np.array([float(P)]))[0])
    assert got[0] == (-2.5 + float(dl(np.array([129.0]))[0])) - logP and abs(got[0] + 2.5) < 2e-15
    assert got[1] == (-2.5 + float(dl(np.array([65.0]))[0])) - logP
    assert got[2] == (-2.5 + float(dl(np.array([128.0]))[0])) - logP
    assert got[3] == -np.inf and np.isnan(got[4])
    m = ll[5].max()
    np.testing.assert_allclose(got[5], m + np.log(np.exp(ll[5] - m).sum()) - np.log(P), rtol=1e-13)
    assert np.isnan(ms.lpd(ll[3:4], np.full((1, 1), np.nan), de, dl)[0])   # the NaN of y_t wins over -inf


# ---- check_call -----------------------------------------------------------------------------------------------------------------------
def _coeffs(pb, K, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for g in pb.GP_prior:
        e0, e1 = np.asarray(g[0]), np.asarray(g[1])
        M = e1.shape[0]
        mean = pgas_amd.prior_mniw_mean(e0.reshape(M, -1), e1)
        out.append(mean[None] + 0.1 * rng.standard_normal((K,) + mean.shape) * np.diag(np.linalg.inv(e1)))
    return out


def _sim(pb, T=6, obs=True, init=True, **kw):
    ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
    return pgas_amd.ModelRollout(pb.inputs[:T], ssm, pb.basis, pb.init_state_mean if init else None, pb.init_state_cov if init else None,
                                 observations=pb.observations[:T] if obs else None, **kw)


def test_every_predict_refusal_is_raised_without_a_device():
    pb = experiments.smo_marginal(T=6)
    sim = _sim(pb)
    assert sim._ops is None
    K = 3
    A = _coeffs(pb, K)
    x0, keys = np.zeros(2), [1, 2, 3]
    assert sim.check_call(A, keys, 1 << 20, predict=True) == (3, 1 << 20, 0, True, False)
    assert sim.check_call(A, keys, 4, x0, process_noise=False, predict=True, observation_noise=True) == (3, 4, 1, False, False)
    assert sim.check_call(A, keys, (1 << 20) + 1) == (3, (1 << 20) + 1, 0, True, False)   # __call__ keeps its own limits
    bad = [
        (dict(coeffs=A[0]), "list of 1"),
        (dict(coeffs=A, keys=[1, 2]), "expected 3 keys"),
        (dict(coeffs=A, keys=keys, replicates=0), "replicates"),
        (dict(coeffs=A, keys=keys, replicates=(1 << 20) + 1), "replicates must be <="),
        (dict(coeffs=A, keys=keys, p0=-1), "p0"),
        (dict(coeffs=A, keys=None, init_state=x0), "needs keys"),
        (dict(coeffs=A, keys=None, init_state=x0, process_noise=False, observation_noise=True), "observation_noise needs keys"),
        (dict(coeffs=A, keys=None, process_noise=False), "draws x_0"),
        (dict(coeffs=A, keys=None, init_state=x0, process_noise=False, replicates=2), "copies"),
        (dict(coeffs=A, keys=keys, init_state=np.zeros((2, 2))), "init_state"),
        (dict(coeffs=A, keys=keys, row_cov=[np.zeros((K, 2, 2))]), r"row_cov\[0\]"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            sim.predict(**kw)
    # observation noise counts as noise: replicates of a noise-free state are no copies when their observations are noisy
    assert sim.check_call(A, keys, 5, x0, process_noise=False, predict=True, observation_noise=True)[1] == 5
    with pytest.raises(ValueError, match="copies"):
        sim.check_call(A, keys, 5, x0, process_noise=False, observation_noise=True)           # not predict: the flag means nothing
    bare = _sim(pb, obs=False)
    with pytest.raises(ValueError, match="needs observations"):
        bare.predict(A, keys, log_score=True)
    wide = pgas_amd.SymbolicStateSpaceModel(pb.process_noise, np.diag([1e-3, 1e-3]), pb.model)   # ny = 1 under a 2 x 2 output noise
    odd = pgas_amd.ModelRollout(pb.inputs[:6], wide, pb.basis, pb.init_state_mean, pb.init_state_cov)
    with pytest.raises(ValueError, match="output_noise"):
        odd.predict(A, keys, observation_noise=True)
    assert odd.check_call(A, keys, predict=True)[0] == 3                                        # moments alone need no output noise
    with pytest.raises(ValueError, match="construct the ModelRollout with both"):
        _sim(pb, init=False).predict(A, keys)
    for s in (sim, bare, odd):
        assert s._ops is None and s._dev_cache is None, "a refused call created the device context"


def test_observations_are_validated_at_construction_from_shapes_alone():
    pb = experiments.smo_marginal(T=6)
    sim = _sim(pb)
    assert sim.has_observations and sim.observations.shape == (6, 1) and sim._ops is None
    assert _sim(pb, obs=False).observations is None
    ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
    for obs in (np.zeros(7), np.zeros((6, 2)), np.zeros((1, 6))):
        with pytest.raises(ValueError, match="observations"):
            pgas_amd.ModelRollout(pb.inputs[:6], ssm, pb.basis, observations=obs)
    veh = experiments.vehicle_marginal(T=6)
    vs = veh.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
    with pytest.raises(ValueError, match="observations"):
        pgas_amd.ModelRollout(veh.inputs[:6], vs, veh.basis, observations=np.zeros(6))          # (T,) only when ny == 1
    v = pgas_amd.ModelRollout(veh.inputs[:6], vs, veh.basis, observations=np.zeros((6, 2)))
    assert v.ny == 2 and v.lds_bytes(predict=True) == v.lds_bytes() and v.lds_bytes(predict=True) <= 64 * 1024
    toy = experiments.toy_marginal(T=6)
    t = pgas_amd.ModelRollout(toy.inputs[:6], toy.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel), toy.basis, observations=toy.observations[:6])
    assert t.lds_bytes(predict=True) == t.lds_bytes()                                           # max(nx, n_i, ny) = 1
    assert callable(pgas_amd.ModelRollout.predict) and mr.PredictiveStats is pgas_amd.rollout.PredictiveStats


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
_SIZES = {"int32_t": 4, "uint32_t": 4, "int64_t": 8, "uint64_t": 8, "double": 8}


def _c_struct_layout(txt, name):
    """[(field, offset, size)] and the total size of `typedef struct name { ... } name;` with natural alignment (LP64)."""
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", txt, flags=re.S).group(1)
    off, fields, align_max = 0, [], 1
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        if "*" in decl:
            base, names = 8, [decl.rsplit("*", 1)[1]]
        else:
            ty, rest = decl.split(None, 1)
            base, names = _SIZES[ty], rest.split(",")
        for n in names:
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", n)
            size = base * int(m.group(2) or 1)
            off = (off + base - 1) // base * base
            fields.append((m.group(1), off, size))
            off += size
            align_max = max(align_max, base)
    return fields, (off + align_max - 1) // align_max * align_max


def test_rollout_stats_is_declared_and_bound_and_the_ctypes_struct_is_the_c_struct():
    from pgas_amd import _lib

    txt = open(os.path.join(ROOT, "include", "pgas_marginal.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+pgas_m_rollout_stats\s*\(([^)]*)\)\s*;", txt)
    assert m, "pgas_m_rollout_stats is not declared in include/pgas_marginal.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 4 and "pgas_m_rollout_desc" in params[1] and "pgas_m_rollout_stats_desc" in params[2]
    ids = dict(re.findall(r"#define\s+(PGAS_STREAM_M_ROLLOUT_\w+)\s+(\d+)u", txt))
    assert ids == {"PGAS_STREAM_M_ROLLOUT_INTVAR": "192", "PGAS_STREAM_M_ROLLOUT_OBS": "200"}
    assert mr.STREAM_ROLLOUT_OBS == 200 and mr.STREAM_ROLLOUT_OBS >= mr.STREAM_ROLLOUT_INTVAR + mr.MAX_IV
    assert re.search(r"#define\s+PGAS_M_ROLLOUT_STATS_MAX_P\s+\(1 << 20\)", txt) and mr.MAX_REPLICATES_PREDICT == 1 << 20
    fields, size = _c_struct_layout(txt, "pgas_m_rollout_stats_desc")
    S = _lib.RolloutStatsDesc
    assert C.sizeof(S) == size == 5 * 8 + 8 + 8 + 2 * 4 + 2 * 64 * 8
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == fields
    lat, _ = _c_struct_layout(txt, "pgas_m_rollout_latent")
    assert [(n, getattr(_lib.RolloutLatent, n).offset, getattr(_lib.RolloutLatent, n).size) for n, _ in _lib.RolloutLatent._fields_] == lat
    assert "pgas_m_rollout_stats" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "pgas_m_rollout_stats")
    assert L.pgas_m_rollout_stats.restype is C.c_int and len(L.pgas_m_rollout_stats.argtypes) == 4
    assert callable(_lib.MarginalOps.model_rollout_stats)
