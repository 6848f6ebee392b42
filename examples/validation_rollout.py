#!/usr/bin/env python3
"""The EMPS validation of examples/EMPS_Simulation.py::validation_rmse (PGAS branch; the reference's EMPS_Validation_Simulation,
src/EMPS.py:129-151) through pgas_amd.Rollout: the plain-PGAS baseline is learned on the synthetic EMPS data, then EVERY kept draw
(A_k, S_k) of the chain is simulated open-loop over a synthetic pulse input in one launch, next to the single simulation of the
posterior-mean parameter matrix the reference runs.  Prints both validation RMSEs and the width of the predictive band, and the band and
log score of the predicted OBSERVATIONS through Rollout.predict, which reduces over the replicates inside the kernel.

The grey-box half of the same validation (X_Alg2 there: the RK4 model with the learned friction curve as its interface variable) goes
through pgas_amd.ModelRollout: Algorithm1 + Algorithm2 are run on the same data, and the model is simulated under the averaged posterior
mean the reference uses AND under the posterior mean of every Algorithm2 iteration, in one launch; the host loop's RMSE
(EMPS_Simulation.py::validation_rmse) is printed beside it.  ModelRollout.predict then gives the grey-box model's RMSE, band width and
log predictive density of the same validation positions beside the black-box ones, again without a cloud.

    python examples/validation_rollout.py [--pgas-iterations K] [--iterations K2] [--particles N] [--steps T] [--validation-steps V]
                                          [--burn-in B] [--replicates P]

The reference's loop pairs x_{i-1} with the input of step i - 1 (src/EMPS.py:147).  The PGAS engine's step t reads input row t, so the
input sequence is handed to Rollout shifted by one row; ModelRollout follows the reference's (and Algorithm1's) convention and takes
the sequence as it is.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def validation_data(steps):
    """The pulse input and linear-friction truth of EMPS_Simulation.py::validation_rmse."""
    dt, Mass = 0.01, 95.11
    tt = np.arange(steps) * dt
    tau = 45.0 * np.sign(np.sin(2 * np.pi * tt / 1.5))

    def truth(s, u):
        return np.array([s[1], (u - 203.5 * s[1] - 20.39 * np.sign(s[1]) + 3.16) / Mass])

    X = np.zeros((steps, 2))
    for i in range(1, steps):
        s, u = X[i - 1], tau[i - 1]
        k1 = truth(s, u); k2 = truth(s + dt * k1 / 2, u); k3 = truth(s + dt * k2 / 2, u); k4 = truth(s + dt * k3, u)
        X[i] = s + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return tau, X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pgas-iterations", type=int, default=30, help="plain-PGAS iterations (reference: 2400)")
    ap.add_argument("--iterations", type=int, default=30, help="Algorithm2 iterations (reference: 800)")
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--validation-steps", type=int, default=600)
    ap.add_argument("--burn-in", type=int, default=0, help="draws dropped from the front of the chain")
    ap.add_argument("--replicates", type=int, default=16, help="noisy replicates per draw for the predictive band")
    ap.add_argument("--seed", type=int, default=12345678)
    args = ap.parse_args()

    import torch

    import pgas_amd
    from pgas_amd import experiments

    pb = experiments.emps_pgas(T=args.steps, seed=args.seed)
    pg = pgas_amd.PGAS(args.particles, args.pgas_iterations, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn,
                       pb.GP_prior, pb.basis_fcn)                                    # src/EMPS.py:243-255
    y = pb.observations
    Sigma_X, _ = pg(pgas_amd.random.key(args.seed), np.stack([y, np.gradient(y, 0.01)], axis=1))
    eng = pg.cSMC.engine
    K = Sigma_X.shape[1]
    kept = pg.chain_log["params"][args.burn_in:]
    As, Ss = torch.stack([p[0] for p in kept]), torch.stack([p[1] for p in kept])
    acc = None
    for k in range(K):                                                              # EMPS_Simulation.py:104-117: posterior-mean matrix
        st = eng.suffstats(Sigma_X[:, k].contiguous())
        acc = [a + b for a, b in zip(acc, st)] if acc else list(st)
    post = [pb.GP_prior[j] + (acc[j] / K).cpu().numpy() for j in range(3)] + [pb.GP_prior[3] + acc[3] / K]
    mean = pgas_amd.prior_mniw_2naturalPara_inv(*post)[0]

    tau, X = validation_data(args.validation_steps)
    shifted = np.concatenate([tau[:1], tau[:-1]])                                   # row t holds tau[t - 1] (row 0 is not read)
    sim = pgas_amd.Rollout(shifted, pb.basis_fcn, 2, device=eng.device)
    x0 = np.zeros(2)                                                                # src/EMPS.py:141-142 (the synthetic truth starts at rest)
    H = pb.likelihood_fcn.H
    of_mean = pgas_amd.rollout_summary(sim(mean[None], init_state=x0), H, X[:, 0])            # what the reference simulates
    of_draws = pgas_amd.rollout_summary(sim(As, init_state=x0), H, X[:, 0])                   # every kept draw, noise-free
    keys = pgas_amd.random.split(pgas_amd.random.key(args.seed + 1), As.shape[0])
    band = pgas_amd.rollout_summary(sim(As, Ss, keys, replicates=args.replicates, init_state=x0), H, X[:, 0])   # posterior predictive
    torch.cuda.synchronize()
    print(f"RMSE_PGAS, posterior-mean parameters (one simulation):        {float(of_mean['rmse']):.5f}")
    print(f"RMSE_PGAS, mean of {As.shape[0]:4d} simulated draws (noise-free):       {float(of_draws['rmse']):.5f}")
    print(f"RMSE_PGAS, posterior predictive mean ({args.replicates} noisy replicates): {float(band['rmse']):.5f}")
    print(f"predictive standard deviation of the position, mean over time: draws only {float(of_draws['std'][:, 0].mean()):.5f}, "
          f"with process noise {float(band['std'][:, 0].mean()):.5f}")

    # the predictive of the OBSERVATIONS without the (K, T, P, 2) cloud: moments and log score reduced over the replicates in the kernel
    scored = pgas_amd.Rollout(shifted, pb.basis_fcn, 2, device=eng.device, likelihood_fcn=pb.likelihood_fcn, observations=X[:, 0])
    stats = scored.predict(As, Ss, keys, replicates=args.replicates, init_state=x0, observation_noise=True)
    pred = pgas_amd.predictive_summary(stats, y=X[:, 0])
    torch.cuda.synchronize()
    print(f"predict: RMSE of the predicted observation's mean {float(pred['rmse']):.5f}; its standard deviation (process and measurement noise), "
          f"mean over time {float(pred['y_std_pooled'][:, 0].mean()):.5f}; log predictive density of the validation positions "
          f"{float(pred['elpd']):.2f} ({float(pred['elpd']) / len(tau):.3f} per step)")

    # calibration of that predictive: the PIT of the validation positions from CDF counts pooled over the draws, again without a cloud
    cal = pgas_amd.calibration_summary(scored.cdf(As, Ss, keys, replicates=args.replicates, init_state=x0, observation_noise=True), levels=(0.5, 0.9, 0.95))
    torch.cuda.synchronize()
    print("cdf: coverage of the 50 / 90 / 95 % predictive intervals of the validation positions "
          + " / ".join(f"{100 * float(cal['coverage'][lv]):.1f}" for lv in (0.5, 0.9, 0.95)) + f" %; KS distance of the PIT from uniform {float(cal['ks']):.3f}")

    # ---- the grey-box half: known physics, the learned friction curve F(dq) = A phi(dq) as its interface variable (src/EMPS.py:143-146)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from EMPS_Simulation import run_marginal, validation_rmse

    marg, mpb = run_marginal(args.iterations, args.particles, args.steps, seed=args.seed, log=lambda *a, **k: None)
    means = pgas_amd.mniw_posterior_means(mpb.GP_prior[0], marg["offline_T0"], marg["offline_T1"])    # (iterations, 1, 9): one model per iteration
    grey = pgas_amd.ModelRollout(tau, mpb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel), mpb.basis, device=eng.device)   # inputs as they are
    g_mean = pgas_amd.rollout_summary(grey([marg["offline_mean"][None]], init_state=x0, process_noise=False), H, X[:, 0])
    g_iter = pgas_amd.rollout_summary(grey([means], init_state=x0, process_noise=False), H, X[:, 0])
    host_alg2, host_pgas = validation_rmse(marg["offline_mean"], mean, mpb, pb, steps=args.validation_steps)
    torch.cuda.synchronize()
    print(f"RMSE_Alg2, averaged posterior mean, host loop (validation_rmse):  {host_alg2:.5f}   (its RMSE_PGAS: {host_pgas:.5f})")
    print(f"RMSE_Alg2, averaged posterior mean, one launch:                   {float(g_mean['rmse']):.5f}")
    print(f"RMSE_Alg2, mean of {means.shape[0]:4d} per-iteration models, one launch:       {float(g_iter['rmse']):.5f}, "
          f"predictive standard deviation of the position {float(g_iter['std'][:, 0].mean()):.5f}")

    # the same three figures as for the black-box model above: process and observation noise, reduced over the replicates in the kernel
    g_scored = pgas_amd.ModelRollout(tau, mpb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel), mpb.basis, device=eng.device, observations=X[:, 0])
    g_keys = pgas_amd.random.split(pgas_amd.random.key(args.seed + 2), means.shape[0])
    g_pred = pgas_amd.predictive_summary(g_scored.predict([means], g_keys, replicates=args.replicates, init_state=x0, observation_noise=True), y=X[:, 0])
    torch.cuda.synchronize()
    print(f"predict, Alg2: RMSE of the predicted observation's mean {float(g_pred['rmse']):.5f}; its standard deviation (process and measurement "
          f"noise), mean over time {float(g_pred['y_std_pooled'][:, 0].mean()):.5f}; log predictive density of the validation positions "
          f"{float(g_pred['elpd']):.2f} ({float(g_pred['elpd']) / len(tau):.3f} per step)")

    # and its calibration, beside the black-box figures above: the PIT of the validation positions from counts pooled over the models
    g_cal = pgas_amd.calibration_summary(g_scored.cdf([means], g_keys, replicates=args.replicates, init_state=x0, observation_noise=True), levels=(0.5, 0.9, 0.95))
    torch.cuda.synchronize()
    print("cdf, Alg2: coverage of the 50 / 90 / 95 % predictive intervals of the validation positions "
          + " / ".join(f"{100 * float(g_cal['coverage'][lv]):.1f}" for lv in (0.5, 0.9, 0.95))
          + f" %; KS distance of the PIT from uniform {float(g_cal['ks']):.3f}   (black-box: "
          + " / ".join(f"{100 * float(cal['coverage'][lv]):.1f}" for lv in (0.5, 0.9, 0.95)) + f" %, {float(cal['ks']):.3f})")


if __name__ == "__main__":
    main()
