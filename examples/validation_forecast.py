#!/usr/bin/env python3
"""Prediction error against the horizon: the plain-PGAS baseline is learned on the synthetic EMPS data as in
examples/validation_rollout.py, then EVERY kept draw (A_k, S_k) of the chain is run over a held-out record (the synthetic pulse input,
positions measured with the training noise level) by pgas_amd.HeldOutFilter.forecast -- a bootstrap particle filter per draw and, from
every row of its particle trace, an open-loop rollout of H - 1 steps: the h-step-ahead prediction p(y_tau | y_{0:tau-h}) for h = 1 .. H
and every row tau, all draws and origins in two launches.  Prints the RMSE of the predicted position and the log score per step against
the horizon, and beside them the open-loop figures of Rollout.predict on the same record (horizon "infinity": the cloud never sees the
observations).  The grey-box model of examples/validation_filter.py -- the known EMPS physics with the friction curve learned by
Algorithm1 + Algorithm2, one coefficient set per iteration -- is then forecast on the same record by pgas_amd.ModelRollout.forecast, and its
RMSE and log score per horizon are printed beside the black-box ones.

    python examples/validation_forecast.py [--pgas-iterations K] [--particles N] [--filter-particles NF] [--steps T] [--validation-steps V]
                                           [--burn-in B] [--horizon H] [--iterations I]

The reference's loop pairs x_{i-1} with the input of step i - 1 (src/EMPS.py:147).  The PGAS engine's step t reads input row t, so the
input sequence is handed to HeldOutFilter (and Rollout) shifted by one row.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pgas-iterations", type=int, default=30, help="plain-PGAS iterations (reference: 2400)")
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--filter-particles", type=int, default=512, help="particles of the held-out filter and of every forecast cloud (<= 1024)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--validation-steps", type=int, default=600)
    ap.add_argument("--burn-in", type=int, default=0, help="draws dropped from the front of the chain")
    ap.add_argument("--horizon", type=int, default=16, help="largest horizon H (<= validation steps)")
    ap.add_argument("--iterations", type=int, default=10, help="Algorithm2 iterations of the grey-box model (reference: 100)")
    ap.add_argument("--seed", type=int, default=12345678)
    args = ap.parse_args()

    import torch

    import pgas_amd
    from pgas_amd import experiments
    from validation_rollout import validation_data

    pb = experiments.emps_pgas(T=args.steps, seed=args.seed)
    pg = pgas_amd.PGAS(args.particles, args.pgas_iterations, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn,
                       pb.GP_prior, pb.basis_fcn)                                    # src/EMPS.py:243-255
    y = pb.observations
    pg(pgas_amd.random.key(args.seed), np.stack([y, np.gradient(y, 0.01)], axis=1))
    dev = pg.cSMC.engine.device
    kept = pg.chain_log["params"][args.burn_in:]
    As, Ss = torch.stack([p[0] for p in kept]), torch.stack([p[1] for p in kept])
    K = As.shape[0]

    tau, X = validation_data(args.validation_steps)
    lik = pb.likelihood_fcn
    rng = np.random.default_rng(args.seed + 3)
    y_val = X @ lik.H.T + rng.standard_normal((len(tau), lik.ny)) @ lik.LR.T        # the held-out record: noisy positions
    shifted = np.concatenate([tau[:1], tau[:-1]])                                   # row t holds tau[t - 1] (row 0 is not read)
    keys = pgas_amd.random.split(pgas_amd.random.key(args.seed + 1), K)

    flt = pgas_amd.HeldOutFilter(y_val, shifted, pb.basis_fcn, lik, 2, args.filter_particles, pb.init_state_mean, pb.init_state_cov, device=dev)
    res = flt.forecast(As, Ss, keys, args.horizon)                                   # the filter, then every origin of every draw at once
    fs = pgas_amd.forecast_summary(res, y=y_val)
    torch.cuda.synchronize()
    rmse, score = fs["rmse"].cpu().numpy(), fs["log_score"].cpu().numpy()
    width = torch.nanmean(fs["y_pred_std"][:, :, 0], dim=1).cpu().numpy()
    print(f"h-step-ahead prediction of the held-out record, {K} draws, {res.n} particles per cloud, {len(tau)} rows:")
    print("  horizon   RMSE of the position   log score per step   predicted std, mean over time")
    for h in range(args.horizon):
        print(f"  {h + 1:7d}   {rmse[h]:20.5f}   {score[h]:18.3f}   {width[h]:.5f}")

    # the open-loop figures on the same record: horizon "infinity"
    sim = pgas_amd.Rollout(shifted, pb.basis_fcn, 2, device=dev, likelihood_fcn=lik, observations=y_val)
    stats = sim.predict(As, Ss, keys, replicates=args.filter_particles, init_state=np.zeros(2))
    pred = pgas_amd.predictive_summary(stats, y=y_val)
    torch.cuda.synchronize()
    print(f"  open loop (Rollout.predict): RMSE {float(pred['rmse']):.5f}, log predictive density per step {float(pred['elpd']) / len(tau):.3f}")

    # calibration against the horizon: the PIT of the record from CDF counts of the same clouds (measurement noise on), pooled over the draws
    levels = (0.5, 0.9, 0.95)
    cal = pgas_amd.calibration_summary(flt.forecast_cdf(As, Ss, keys, args.horizon), levels=levels)
    cal_open = pgas_amd.calibration_summary(sim.cdf(As, Ss, keys, replicates=args.filter_particles, init_state=np.zeros(2), observation_noise=True), levels=levels)
    torch.cuda.synchronize()
    print("  horizon   coverage of the 50 / 90 / 95 % intervals   KS distance of the PIT from uniform")
    for h in range(args.horizon):
        print(f"  {h + 1:7d}   " + " / ".join(f"{100 * float(cal['coverage'][lv][h]):5.1f}" for lv in levels) + f" %   {float(cal['ks'][h]):.3f}")
    print("  open loop " + " / ".join(f"{100 * float(cal_open['coverage'][lv]):5.1f}" for lv in levels) + f" %   {float(cal_open['ks']):.3f}")

    # ---- the grey-box model at the same horizons: known physics, the learned friction curve as its interface variable; the draws are the
    # per-iteration posterior means of Algorithm2's statistics trace.  ModelRollout takes the input sequence as it is.
    from EMPS_Simulation import run_marginal

    marg, mpb = run_marginal(args.iterations, args.particles, args.steps, seed=args.seed, log=lambda *a, **k: None)
    means = pgas_amd.mniw_posterior_means(mpb.GP_prior[0], marg["offline_T0"], marg["offline_T1"])
    grey = pgas_amd.ModelRollout(tau, mpb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel), mpb.basis, mpb.init_state_mean, mpb.init_state_cov, device=dev,
                                 observations=y_val)
    g_keys = pgas_amd.random.split(pgas_amd.random.key(args.seed + 2), means.shape[0])
    g_res = grey.forecast([means], g_keys, min(args.filter_particles, grey.max_particles()), args.horizon)   # the filter, then every origin at once
    g_fs = pgas_amd.forecast_summary(g_res, y=y_val)
    torch.cuda.synchronize()
    g_rmse, g_score = g_fs["rmse"].cpu().numpy(), g_fs["log_score"].cpu().numpy()
    print(f"grey-box model (Algorithm2, {means.shape[0]} per-iteration models, {g_res.n} particles per cloud) beside the black-box model:")
    print("  horizon   RMSE grey-box   RMSE black-box   log score grey-box   log score black-box")
    for h in range(args.horizon):
        print(f"  {h + 1:7d}   {g_rmse[h]:13.5f}   {rmse[h]:14.5f}   {g_score[h]:18.3f}   {score[h]:19.3f}")

    # the grey-box model's calibration against the horizon: the PIT of the record from counts of the same clouds with observation noise
    g_cal = pgas_amd.calibration_summary(grey.forecast_cdf([means], g_keys, g_res.n, args.horizon), levels=levels)
    torch.cuda.synchronize()
    print("  horizon   grey-box coverage of the 50 / 90 / 95 % intervals, KS   black-box coverage, KS")
    for h in range(args.horizon):
        print(f"  {h + 1:7d}   " + " / ".join(f"{100 * float(g_cal['coverage'][lv][h]):5.1f}" for lv in levels) + f" %   {float(g_cal['ks'][h]):.3f}   "
              + " / ".join(f"{100 * float(cal['coverage'][lv][h]):5.1f}" for lv in levels) + f" %   {float(cal['ks'][h]):.3f}")


if __name__ == "__main__":
    main()
