"""CPU tests of the batched marginalised Particle-Gibbs chains (pgas_amd/marginal_chains.py): the NumPy
restatement of the categorical kernel against plain float64 NumPy, the key schedule of MultiChainAlgorithm2 against Algorithm2's loop, and
the refusals, which are raised before any device object exists."""
import numpy as np
import pytest

import runs_categorical_numpy as rcn
from common import pgas_amd
from pgas_amd import marginal_chains as mc
from pgas_amd import random as prng

SIZES = (1, 2, 63, 64, 65, 200, 257, 1024)


@pytest.mark.parametrize("N", SIZES)
def test_restatement_equals_plain_float64_categorical(N):
    """On the degenerate, multi-scale, single-survivor and all-equal weight vectors the kernel's defined order gives the index of
    min(searchsorted(cumsum(softmax)), N - 1) in plain float64 -- for uniforms that keep 1e-9 of the total mass between themselves and every
    step of the CDF (asserted here), far more than the orders differ by (a sum of at most 1024 terms: ~1e-13)."""
    names, lw, u = rcn.batch(N)
    got = rcn.runs_categorical(lw, u)
    n_plain = 0
    for r, name in enumerate(names):
        if "/u=" not in name:
            continue
        n_plain += 1
        assert rcn.margin(lw[r], u[r]) >= rcn.MARGIN, f"{name}: the uniform {u[r]!r} sits on a step of the CDF"
        want, _ = rcn.plain_row(lw[r], u[r])
        assert got[r] == want, f"{name}: restatement {got[r]}, plain float64 {want}"
        c, S = rcn.cdf_row(lw[r])
        assert abs(c[-1] / S - 1.0) < 1e-13, name
    assert n_plain == len(rcn.weight_rows(N)) * len(rcn.U_CANDIDATES)
    picks = {int(v) for v in got[:n_plain]}
    assert N == 1 or len(picks) > 1, "the cases draw more than one index"


@pytest.mark.parametrize("N", SIZES)
def test_rows_without_a_softmax_give_the_last_index(N):
    for name, lw in rcn.refused_rows(N):
        assert rcn.cdf_row(lw) is None, name
        for u in (0.0, 0.37, 0.999):
            assert rcn.categorical_row(lw, u) == N - 1, name


def test_uniform_at_the_ends():
    lw = rcn.rc.mild(200)
    assert rcn.categorical_row(lw, 0.0) == 0                       # no c_i is below 0
    assert rcn.categorical_row(lw, 1.0) == 199                     # c_N-1 = S is not below S: N - 1 entries are, and the clip keeps N - 1
    assert rcn.categorical_row(rcn.rc.one_hot(200, 199), 0.5) == 199
    assert rcn.categorical_row(rcn.rc.one_hot(200, 0), 0.5) == 0


# ------------------------------------------------------------------------------------------ key schedule
def _algorithm2_step_keys(root, K):
    """What Algorithm2.__call__ hands to its conditional filter in iterations 1 .. K - 1 (pgas_amd/Algorithm2.py, src/Algorithm2.py:121)."""
    key, out = prng.as_key(root), []
    for _ in range(1, K):
        key, key_step = prng.split(key, 2)
        out.append(key_step)
    return out


@pytest.mark.parametrize("C,K", [(1, 4), (3, 4), (7, 2), (2, 1)])
def test_iteration_keys_follow_algorithm2(C, K):
    roots = pgas_amd.chains.root_keys(12345678, C)
    assert roots == prng.split(12345678, C), "the default root keys are random.split(key, C)"
    got = mc.iteration_keys(roots, K)
    assert got.shape == (K - 1, C) and got.dtype == np.uint64
    for c in range(C):
        assert [int(v) for v in got[:, c]] == _algorithm2_step_keys(roots[c], K)
    given = [5, 2**64 - 1, 17][:C] + list(range(100, 100 + max(0, C - 3)))
    assert pgas_amd.chains.root_keys(None, C, given) == [prng.as_key(k) for k in given]
    assert [int(v) for v in mc.iteration_keys(given, 3)[:, -1]] == _algorithm2_step_keys(given[-1], 3)


# ------------------------------------------------------------------------------------------ refusals, without a device
def test_sizes_are_refused_before_anything_is_built():
    bad = dict(observations=None, inputs=None, SSM=None, init_state_mean=None, init_state_cov=None, init_int_var_mean=None, init_int_var_cov=None,
               GP_prior=None, basis_fcn=None)
    with pytest.raises(ValueError, match="1024"):
        pgas_amd.MultiChainAlgorithm3(2, 1025, **bad)
    with pytest.raises(ValueError, match="C must be"):
        pgas_amd.MultiChainAlgorithm3(0, 200, **bad)
    with pytest.raises(ValueError, match="N_samples must be"):
        pgas_amd.MultiChainAlgorithm3(2, 0, **bad)
    with pytest.raises(ValueError, match="1024"):
        pgas_amd.MultiChainAlgorithm2(2, 1025, 4, **bad)
    with pytest.raises(ValueError, match="C must be"):
        pgas_amd.MultiChainAlgorithm2(0, 200, 4, **bad)
    assert mc.check_sizes(7, 1024) == (7, 1024)


def test_keys_and_references_are_checked_on_the_host():
    import torch

    with pytest.raises(ValueError, match="keys"):
        mc.check_keys([1, 2], 3)
    with pytest.raises(ValueError, match="keys"):
        mc.check_keys([1, 2, 3, 4], 3)
    with pytest.raises(ValueError, match="keys"):
        mc.check_keys(torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="keys"):
        mc.check_keys(torch.zeros(3, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="keys"):
        pgas_amd.chains.root_keys(1, 3, [1, 2])
    assert mc.check_keys([1, 2, 3], 3) == [1, 2, 3]
    C, T, nx = 3, 8, 2
    ok = np.zeros((C, T, nx))
    assert tuple(mc.chain_reference(ok, C, T, nx, "ref_state").shape) == (C, T, nx)
    assert tuple(mc.chain_reference(np.zeros((C, T)), C, T, 1, "ref_int_var[0]").shape) == (C, T, 1)
    assert tuple(mc.chain_reference(np.zeros((T, nx)), C, T, nx, "init_ref_state", shared_ok=True).shape) == (C, T, nx)
    for shape in ((T, nx), (C, T + 1, nx), (C + 1, T, nx), (C, T, nx + 1), (C, T)):
        with pytest.raises(ValueError, match="ref_state"):
            mc.chain_reference(np.zeros(shape), C, T, nx, "ref_state")
    with pytest.raises(ValueError, match="init_ref_state"):
        mc.chain_reference(np.zeros((T + 1, nx)), C, T, nx, "init_ref_state", shared_ok=True)
