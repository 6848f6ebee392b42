"""Host side of the batched open-loop simulation (pgas_amd/rollout.py, pgas_rollout): argument validation before any device is
touched, the public names, the C ABI binding, and rollout_summary on a hand-made tensor.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT, experiments, pgas_amd
from pgas_amd import rollout as ro


@pytest.fixture(scope="module")
def sim():
    """An unlaunched Rollout over the SMO inputs (nx = 2, M = 41) with init_state_mean / cov; K = 3 parameter draws."""
    pb = experiments.smo_pgas(T=12)
    A, S = experiments.initial_params(pb)
    r = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
    return r, pb, np.repeat(A[None], 3, axis=0), np.repeat(S[None], 3, axis=0)


def test_names_are_public():
    for n in ("Rollout", "rollout_summary"):
        assert n in pgas_amd.__all__ and hasattr(pgas_amd, n)
    assert callable(getattr(pgas_amd.condSequentialMonteCarlo, "rollout")) and callable(getattr(pgas_amd.condSequentialMonteCarloChains, "rollout"))


def test_every_refusal_is_a_value_error_before_a_device_is_touched(sim):
    r, pb, As, Ss = sim
    keys = [1, 2, 3]
    x0 = np.zeros(2)
    bad = [
        ("coeff_mat", dict(coeff_mat=As[:, :, :-1], init_state=x0)),
        ("coeff_mat", dict(coeff_mat=As[0], init_state=x0)),
        ("K must be", dict(coeff_mat=As[:0], init_state=x0)),
        ("replicates", dict(coeff_mat=As, init_state=x0, replicates=0)),
        ("error_cov", dict(coeff_mat=As, error_cov=Ss[:2], keys=keys)),
        ("error_cov", dict(coeff_mat=As, error_cov=Ss[:, :1], keys=keys)),
        ("needs keys", dict(coeff_mat=As, error_cov=Ss)),
        ("keys", dict(coeff_mat=As, error_cov=Ss, keys=keys[:2])),
        ("keys", dict(coeff_mat=As, error_cov=Ss, keys=torch.zeros(3, dtype=torch.int32))),
        ("keys", dict(coeff_mat=As, error_cov=Ss, keys=torch.zeros(4, dtype=torch.int64))),
        ("init_state", dict(coeff_mat=As, error_cov=Ss, keys=keys, init_state=np.zeros(3))),
        ("init_state", dict(coeff_mat=As, error_cov=Ss, keys=keys, replicates=5, init_state=np.zeros((3, 4, 2)))),
        ("noise-free", dict(coeff_mat=As)),                                            # drawn x_0 without keys / noise
        ("noise-free", dict(coeff_mat=As, init_state=x0, replicates=2)),               # copies
        ("noise-free", dict(coeff_mat=As, init_state=np.zeros((3, 2)), replicates=2)),
    ]
    for msg, kw in bad:
        with pytest.raises(ValueError, match=msg):
            r(**kw)
    assert r._engine is None, "a refused call created the device context"
    # drawn x_0 without init_state_mean / cov
    r2 = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx)
    with pytest.raises(ValueError, match="init_state_mean"):
        r2(As, Ss, keys)
    assert r2._engine is None
    with pytest.raises(ValueError):
        pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, init_state_mean=pb.init_state_mean)
    with pytest.raises(ValueError):
        pgas_amd.Rollout(pb.inputs, pb.basis_fcn, 1, pb.init_state_mean, pb.init_state_cov)
    with pytest.raises(TypeError):
        pgas_amd.Rollout(pb.inputs, lambda x, u: x, pb.nx)


def test_accepted_forms(sim):
    r, pb, As, Ss = sim
    M = As.shape[2]
    keys = torch.zeros(3, dtype=torch.int64)
    assert ro.check_call(2, M, True, As, Ss, keys, 7) == (3, 7, 0)
    assert ro.check_call(2, M, False, As, None, None, 1, np.zeros(2)) == (3, 1, 1)
    assert ro.check_call(2, M, False, As, None, None, 1, np.zeros((3, 2))) == (3, 1, 2)
    assert ro.check_call(2, M, False, As, None, None, 5, np.zeros((3, 5, 2))) == (3, 5, 3)
    assert ro.check_call(2, M, False, As, Ss, [1, 2, 3], 2500, np.zeros((3, 2))) == (3, 2500, 2)
    assert r.T == 12 and r.n_x == 2


def test_rollout_is_declared_and_bound_with_matching_argument_counts():
    from pgas_amd import _lib

    txt = open(os.path.join(ROOT, "include", "pgas_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+pgas_rollout\s*\(([^)]*)\)\s*;", txt)
    assert m, "pgas_rollout is not declared in include/pgas_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 11
    assert "pgas_rollout" in _lib.EXPORTS
    L = _lib.load()
    assert L.pgas_rollout.restype is not None and len(L.pgas_rollout.argtypes) == len(params)
    import ctypes as C

    want = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for p, a in zip(params, L.pgas_rollout.argtypes):
        if "*" in p:
            assert a is C.c_void_p, p
        else:
            assert a is want[p.split()[0]], p


def test_rollout_summary_on_a_hand_made_tensor():
    # (K, T, P, nx) = (2, 3, 2, 1): the four simulated states of time t are sim[:, t, :, 0]
    sim = torch.tensor([[[[1.0], [3.0]], [[0.0], [0.0]], [[2.0], [4.0]]],
                        [[[5.0], [7.0]], [[2.0], [-2.0]], [[6.0], [8.0]]]], dtype=torch.float64)
    assert tuple(sim.shape) == (2, 3, 2, 1)
    s = pgas_amd.rollout_summary(sim)
    assert set(s) == {"mean", "std"}
    # t = 0: {1, 3, 5, 7}: mean 4, variance (9 + 1 + 1 + 9) / 4 = 5; t = 1: {0, 0, 2, -2}: 0, 2; t = 2: {2, 4, 6, 8}: 5, 5
    np.testing.assert_allclose(s["mean"].numpy(), [[4.0], [0.0], [5.0]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(s["std"].numpy(), np.sqrt([[5.0], [2.0], [5.0]]), rtol=1e-15)
    # y = (3, 0, 7) against H mean = (8, 0, 10) with H = 2: errors (5, 0, 3), rmse = sqrt(34 / 3)
    s = pgas_amd.rollout_summary(sim, H=[[2.0]], y=[3.0, 0.0, 7.0])
    np.testing.assert_allclose(float(s["rmse"]), np.sqrt(34.0 / 3.0), rtol=1e-15)
    # H defaults to the identity: errors (1, 0, -2), rmse = sqrt(5 / 3)
    np.testing.assert_allclose(float(pgas_amd.rollout_summary(sim, y=[3.0, 0.0, 7.0])["rmse"]), np.sqrt(5.0 / 3.0), rtol=1e-15)
    with pytest.raises(ValueError):
        pgas_amd.rollout_summary(sim[0])
