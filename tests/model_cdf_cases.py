"""What tests/test_model_rollout_cdf_host.py, tests/test_gpu_model_rollout_cdf.py and tests/test_gpu_model_forecast_cdf.py share beside
tests/model_filter_cases.py: two test-local traced models (defined the way model_filter_cases.kalman_model is) and the closed-form
binomial statistic.  No GPU, no device context.

    wide         linear, nx = 3, ny = 2, one latent function: 5 value channels, so J_max = 64 // 5 = 12 < 16
    memoryless   x' = xi + process noise q, y = x, nx = ny = 1; with A = 0 (xi = 0) x_t, t >= 1, is iid N(0, q) across rows, replicates,
                 leads and particles, whatever the ancestors are, and yhat + e is N(0, q + r)
"""
import math

import numpy as np

import model_filter_cases as cases
from common import experiments, pgas_amd

K, T, KEYS = cases.K, cases.T, cases.KEYS

# ---- wide -----------------------------------------------------------------------------------------------------------------------------
WIDE = dict(Q=np.diag([0.01, 0.02, 0.015]), R=np.array([[0.04, 0.01], [0.01, 0.09]]), m0=np.array([0.1, -0.2, 0.3]), P0=0.01 * np.eye(3))


def wide_model(xp):
    def f_x(state, input, *int_var):
        xi = int_var[0].reshape(-1)
        return xp.stack([0.8 * state[:, 0] + 0.1 * state[:, 1] + xi, 0.7 * state[:, 1] - 0.2 * state[:, 2], 0.5 * state[:, 2] + 0.3 * state[:, 0]], 1)

    def f_y(state, input, *int_var):
        return xp.stack([state[:, 0] + 0.5 * state[:, 2], state[:, 1] - state[:, 0]], 1)

    return f_x, f_y


def wide_rollout(ops=None, Tn=T):
    """(ssm, ModelRollout, coefficient draws [A (K, 1, M)], observations (Tn, 2)) of the wide model; touches no device."""
    toy = experiments.toy_marginal(T=Tn)
    ssm = pgas_amd.SymbolicStateSpaceModel(WIDE["Q"], WIDE["R"], wide_model)
    rng = np.random.default_rng(21)
    y = 0.3 * rng.standard_normal((Tn, 2))
    sim = pgas_amd.ModelRollout(np.zeros((Tn, 0)), ssm, toy.basis, WIDE["m0"], WIDE["P0"], ops=ops, observations=y)
    A = [0.05 * rng.standard_normal((K, 1, sim.latents[0].M))]
    return ssm, sim, A, y


# ---- memoryless -----------------------------------------------------------------------------------------------------------------------
MEM = dict(q=0.37, r=0.21, m0=0.0, p0=1.0)
TAUS = (-2.0, -1.0, -0.25, 0.0, 0.5, 1.5, 2.5)
CLOSED_P, CLOSED_N, CLOSED_H = 4096, 1024, 4


def memoryless_model(xp):
    def f_x(state, input, *int_var):
        return int_var[0].reshape(-1, 1)

    def f_y(state, input, *int_var):
        return state[:, 0:1]

    return f_x, f_y


def memoryless_rollout(ops=None, Tn=T):
    """(ssm, ModelRollout, [A = 0 (K, 1, M)], observations (Tn,)) of the memoryless model; touches no device."""
    toy = experiments.toy_marginal(T=Tn)
    ssm = pgas_amd.SymbolicStateSpaceModel(np.array([[MEM["q"]]]), np.array([[MEM["r"]]]), memoryless_model)
    y = np.sqrt(MEM["q"] + MEM["r"]) * np.random.default_rng(22).standard_normal(Tn)
    sim = pgas_amd.ModelRollout(np.zeros((Tn, 0)), ssm, toy.basis, np.array([MEM["m0"]]), np.array([[MEM["p0"]]]), ops=ops, observations=y)
    return ssm, sim, [np.zeros((K, 1, sim.latents[0].M))], y


def closed_thresholds(Tn=T):
    """(Tn, 2, 7): sigma * TAUS with sigma = sqrt(q) for the state and sqrt(q + r) for the noisy predicted observation."""
    sig = np.array([math.sqrt(MEM["q"]), math.sqrt(MEM["q"] + MEM["r"])])
    return np.ascontiguousarray(np.broadcast_to(sig[:, None] * np.array(TAUS)[None, :], (Tn, 2, len(TAUS))))


def binomial_z(count, n):
    """count (..., len(TAUS)) pooled over n values of N(0, sigma^2) at sigma * TAUS -> z = (count - n Phi) / sqrt(n Phi (1 - Phi))."""
    Phi = np.array([0.5 * math.erfc(-t / math.sqrt(2.0)) for t in TAUS])
    return (np.asarray(count, dtype=np.float64) - n * Phi) / np.sqrt(n * Phi * (1.0 - Phi))


def pool_rollout(count):
    """count (K, T, 2, 7) -> (pooled (2, 7) over draws and rows t >= 1, the number of rows pooled K (T - 1))."""
    count = np.asarray(count)
    return count[:, 1:].astype(np.int64).sum(axis=(0, 1)), count.shape[0] * (count.shape[1] - 1)


def pool_forecast(count):
    """count (K, H, T, 2, 7) -> (pooled (2, 7) over draws, every h and rows tau >= max(h - 1, 1), the number of (draw, h, row) pooled)."""
    count = np.asarray(count)
    tot, rows = np.zeros(count.shape[-2:], dtype=np.int64), 0
    for h in range(1, count.shape[1] + 1):
        part = count[:, h - 1, max(h - 1, 1):]
        assert (part >= 0).all()
        tot += part.astype(np.int64).sum(axis=(0, 1))
        rows += part.shape[0] * part.shape[1]
    return tot, rows
