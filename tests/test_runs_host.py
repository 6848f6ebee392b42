"""Host-side checks of pgas_amd.MultiRunAlgorithm1 that need no GPU: what it refuses, it refuses before it touches the device."""
import pytest

from common import experiments, pgas_amd


def _args(pb):
    return dict(observations=pb.observations, inputs=pb.inputs, SSM=None, forgetting_factor=pb.forgetting_factor, init_state_mean=pb.init_state_mean,
                init_state_cov=pb.init_state_cov, init_int_var_mean=pb.init_int_var_mean, init_int_var_cov=pb.init_int_var_cov,
                GP_prior=pb.GP_prior, basis_fcn=pb.basis_fcn())


@pytest.mark.parametrize("R,N,what", [(0, 200, "R must be"), (-1, 200, "R must be"), (2, 1025, "run Algorithm1 once per key"), (2, 0, "N_samples must be")])
def test_bad_sizes_are_refused_before_the_device_is_touched(R, N, what):
    pb = experiments.smo_marginal(T=4)
    with pytest.raises(ValueError, match=what):
        pgas_amd.MultiRunAlgorithm1(R, N, **_args(pb))


def test_the_class_is_exported():
    assert "MultiRunAlgorithm1" in pgas_amd.__all__ and issubclass(pgas_amd.MultiRunAlgorithm1, pgas_amd.Algorithm1)
