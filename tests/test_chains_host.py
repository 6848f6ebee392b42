"""Host-side pieces of the batched chains (pgas_amd.chains): split-R-hat against an independent NumPy restatement, the chains' root keys,
the u64 key bit patterns carried in int64 tensors.  No GPU needed."""
import numpy as np
import pytest

from common import pgas_amd  # noqa: F401


def _split_rhat_numpy(x):
    """Split-R-hat restated from its definition (Gelman et al., BDA3, section 11.4), loop by loop."""
    C, K = x.shape[:2]
    n = K // 2
    halves = [x[c, :n] for c in range(C)] + [x[c, K - n:] for c in range(C)]
    m = len(halves)
    means = np.array([h.mean(axis=0) for h in halves])
    within = np.array([((h - h.mean(axis=0)) ** 2).sum(axis=0) / (n - 1) for h in halves])
    grand = means.mean(axis=0)
    B = n / (m - 1) * ((means - grand) ** 2).sum(axis=0)
    W = within.mean(axis=0)
    return np.sqrt(((n - 1) / n * W + B / n) / W)


@pytest.mark.parametrize("C,K,tail", [(4, 1000, ()), (3, 501, (2,)), (8, 64, (2, 3))])
def test_split_rhat_matches_numpy_restatement(C, K, tail):
    from pgas_amd.chains import split_rhat

    rng = np.random.default_rng(7)
    x = rng.standard_normal((C, K) + tail) * np.arange(1, C + 1).reshape((C, 1) + (1,) * len(tail)) + 0.1 * rng.standard_normal((C, 1) + tail)
    got = split_rhat(x).numpy()
    want = _split_rhat_numpy(x)
    assert got.shape == tail
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_split_rhat_separates_agreeing_from_shifted_chains():
    from pgas_amd.chains import split_rhat

    rng = np.random.default_rng(11)
    same = rng.standard_normal((4, 4000, 3))
    r_same = split_rhat(same).numpy()
    assert np.all(np.abs(r_same - 1.0) < 0.01), r_same
    shifted = same + np.array([0.0, 0.0, 1.5, 3.0]).reshape(4, 1, 1)
    r_shift = split_rhat(shifted).numpy()
    assert np.all(r_shift > 1.3), r_shift
    np.testing.assert_allclose(r_shift, _split_rhat_numpy(shifted), rtol=1e-12, atol=0)
    # a chain that drifts is caught by the split even when every chain drifts alike
    drift = same + np.linspace(0.0, 4.0, 4000).reshape(1, 4000, 1)
    assert np.all(split_rhat(drift).numpy() > 1.3)
    with pytest.raises(ValueError):
        split_rhat(same[:, :3])


def test_chain_root_keys_are_the_split_of_the_key():
    from pgas_amd import random as prng
    from pgas_amd.chains import root_keys

    for key, C in [(20241004, 1), (7, 5), (2**64 - 1, 64)]:
        assert root_keys(key, C) == prng.split(key, C)
    assert root_keys(0, 3, keys=[5, 6, 2**63 + 1]) == [5, 6, 2**63 + 1]
    with pytest.raises(ValueError):
        root_keys(0, 3, keys=[1, 2])


def test_keys_survive_the_int64_carrier():
    from pgas_amd import random as prng
    from pgas_amd.chains import keys_list, keys_tensor

    keys = prng.split(123, 50) + [0, 2**63, 2**64 - 1]
    t = keys_tensor(keys, "cpu")
    assert t.dtype.is_floating_point is False and tuple(t.shape) == (len(keys),)
    assert keys_list(t) == keys
    assert keys_list(keys_tensor(t, "cpu")) == keys
