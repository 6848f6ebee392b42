"""What tests/test_model_filter_host.py and tests/test_gpu_model_filter.py share: the five grey-box models of
tests/test_gpu_model_rollout_stats.py with the output noise the filter tests score them under, the particle counts, and the linear
model of the Kalman test.  No GPU, no device context."""
import numpy as np

from common import experiments, pgas_amd

K, T = 3, 12
KEYS = [0x1234567, 0x9E3779B97F4A7C15, 42]
MODELS = {
    "smo": (experiments.smo_marginal, None),
    "emps": (experiments.emps_marginal, None),
    "toy": (experiments.toy_marginal, None),
    "vehicle": (experiments.vehicle_marginal, None),
    "smo2": (experiments.smo_two_component_marginal, [2]),
}
NS = [1, 2, 63, 64, 65, 200, 256, 257, 512, 513]   # clipped per model by max_particles(); N = 1024 runs on the toy model
# The output noise the filter tests score a model under; None: the model's stock noise.  tests/test_model_filter_host.py
# (test_resampling_is_not_trivial) shows that on these 12 rows every model then has a step with at most 0.8 N distinct ancestors.  The
# toy model's stock variance of 4 keeps 59 of 64 at best, so it is shrunk to 1 (0.62 N or fewer at every N); smaller still would push
# |ell| into the thousands, where one ulp is no longer small against the restatement's absolute bound of 1e-12.
NOISE_R = {"smo": None, "emps": None, "toy": np.array([[1.0]]), "vehicle": None, "smo2": None}


def coeffs(pb, Kn=K, seed=5):
    """Kn coefficient sets per latent function: prior mean + 0.1 N(0, 1) sd (the draws of tests/test_gpu_model_rollout_stats.py)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in pb.GP_prior:
        e0, e1 = np.asarray(g[0]), np.asarray(g[1])
        M = e1.shape[0]
        mean = pgas_amd.prior_mniw_mean(e0.reshape(M, -1), e1)
        out.append(mean[None] + 0.1 * rng.standard_normal((Kn,) + mean.shape) * np.diag(np.linalg.inv(e1)))
    return out


def problem(name):
    make, widths = MODELS[name]
    pb = make(T=T)
    R = pb.output_noise if NOISE_R[name] is None else NOISE_R[name]
    return pb, widths, np.atleast_2d(np.asarray(R, dtype=np.float64))


def rollout(name, ops=None, observations=None, has_obs=True, **kw):
    """(pb, ssm, ModelRollout) of a model over its T rows under the filter tests' output noise; touches no device."""
    pb, widths, R = problem(name)
    ssm = pgas_amd.SymbolicStateSpaceModel(pb.process_noise, R, pb.model)
    y = np.asarray(pb.observations if observations is None else observations, dtype=np.float64).reshape(T, -1)
    sim = pgas_amd.ModelRollout(pb.inputs[:T], ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, int_var_widths=widths, ops=ops,
                                observations=y if has_obs else None, **kw)
    return pb, ssm, sim


# ---- the Kalman test's model: x' = a x + xi, y = x, with A = 0 (xi = 0) and Gaussian process and output noise ----------------------------
KAL = dict(a=0.9, q=0.25, r=0.5, m0=0.0, p0=1.0, T=20, N=512, seeds=16)


def kalman_model(xp):
    def f_x(state, input, *int_var):
        return KAL["a"] * state + int_var[0].reshape(-1, 1)

    def f_y(state, input, *int_var):
        return state[:, 0:1]

    return f_x, f_y


def kalman_record(seed=7):
    """y (T,) simulated from the linear model itself."""
    rng = np.random.default_rng(seed)
    x = KAL["m0"] + np.sqrt(KAL["p0"]) * rng.standard_normal()
    y = np.empty(KAL["T"])
    for t in range(KAL["T"]):
        y[t] = x + np.sqrt(KAL["r"]) * rng.standard_normal()
        x = KAL["a"] * x + np.sqrt(KAL["q"]) * rng.standard_normal()
    return y
