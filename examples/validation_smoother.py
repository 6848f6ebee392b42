#!/usr/bin/env python3
"""What the state did on a record, given all of it: the plain-PGAS baseline is learned on the synthetic EMPS data as in
examples/validation_filter.py, then EVERY kept draw (A_k, S_k) of the chain is run over the held-out record (the synthetic pulse input,
positions measured with the training noise level) by pgas_amd.HeldOutFilter.smooth -- the bootstrap particle filter per draw, then
backward simulation (FFBSi) over its trace, every draw and trajectory in one launch per 256 trajectories.  Prints filtered against
smoothed: the RMSE of the position and of the UNMEASURED velocity against the truth, the smoothed standard deviation, and the RMSE of the
smoothed H x against the record.
The grey-box model of examples/validation_filter.py -- the known EMPS physics with the friction curve learned by Algorithm1 + Algorithm2,
one coefficient set per iteration -- is then smoothed on the same record by pgas_amd.ModelRollout.smooth, which also gives the smoothed
INTERFACE variable: the friction force given the whole record.

    python examples/validation_smoother.py [--pgas-iterations K] [--particles N] [--filter-particles NF] [--trajectories B] [--steps T]
                                           [--validation-steps V] [--burn-in B]
                                           [--iterations I]

The reference's loop pairs x_{i-1} with the input of step i - 1 (src/EMPS.py:147).  The PGAS engine's step t reads input row t, so the
input sequence is handed to HeldOutFilter shifted by one row.
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
    ap.add_argument("--filter-particles", type=int, default=512, help="particles of the held-out filter (<= 1024)")
    ap.add_argument("--trajectories", type=int, default=64, help="backward-simulation trajectories per draw (<= 65536)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--validation-steps", type=int, default=600)
    ap.add_argument("--burn-in", type=int, default=0, help="draws dropped from the front of the chain")
    ap.add_argument("--seed", type=int, default=12345678)
    ap.add_argument("--iterations", type=int, default=10, help="Algorithm2 iterations of the grey-box model (reference: 100)")
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
    res = flt.smooth(As, Ss, keys, args.trajectories)          # the filter, then one launch per 256 trajectories for all K draws
    ev = pgas_amd.evidence_summary(res.filter, y=y_val)
    sm = pgas_amd.smoothing_summary(res, y=y_val)
    torch.cuda.synchronize()
    truth = torch.as_tensor(X, device=dev)
    rmse = lambda m: [float(torch.sqrt(torch.mean((m[:, j] - truth[:, j]) ** 2))) for j in range(2)]   # noqa: E731
    f_rmse, s_rmse = rmse(ev["x_filt_mean_pooled"]), rmse(sm["x_smooth_mean"])
    print(f"{K} draws, {res.n} particles, {res.n_trajectories} backward trajectories per draw, {len(tau)} rows")
    print(f"position against the truth: filtered RMSE {f_rmse[0]:.5f}, smoothed RMSE {s_rmse[0]:.5f}")
    print(f"velocity against the truth (not measured): filtered RMSE {f_rmse[1]:.5f}, smoothed RMSE {s_rmse[1]:.5f}")
    print(f"smoothed standard deviation, mean over time: position {float(sm['x_smooth_std'][:, 0].mean()):.5f}, velocity "
          f"{float(sm['x_smooth_std'][:, 1].mean()):.5f}; one-step-ahead predictive standard deviation of the position "
          f"{float(ev['y_pred_std'][:, 0].mean()):.5f}")
    print(f"smoothed H x against the record: RMSE {float(sm['rmse']):.5f} (one-step-ahead prediction: {float(ev['rmse']):.5f})")
    spread = sm["x_smooth_mean_draw"].std(dim=0).mean(dim=0)
    print(f"spread of the per-draw smoothed means over the draws, mean over time: position {float(spread[0]):.5f}, velocity {float(spread[1]):.5f}")

    # ---- the grey-box model on the same record: known physics, the learned friction curve as its interface variable; the draws are the
    # per-iteration posterior means of Algorithm2's statistics trace.  ModelRollout takes the input sequence as it is.
    from EMPS_Simulation import run_marginal

    marg, mpb = run_marginal(args.iterations, args.particles, args.steps, seed=args.seed, log=lambda *a, **k: None)
    means = pgas_amd.mniw_posterior_means(mpb.GP_prior[0], marg["offline_T0"], marg["offline_T1"])
    grey = pgas_amd.ModelRollout(tau, mpb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel), mpb.basis, mpb.init_state_mean, mpb.init_state_cov, device=dev,
                                 observations=y_val)
    g_keys = pgas_amd.random.split(pgas_amd.random.key(args.seed + 2), means.shape[0])
    g_res = grey.smooth([means], g_keys, min(args.filter_particles, grey.max_particles()), args.trajectories)   # the filter, then 256 trajectories per launch
    g_ev, g_sm, g_xi = pgas_amd.evidence_summary(g_res.filter, y=y_val), pgas_amd.smoothing_summary(g_res, y=y_val), pgas_amd.interface_summary(g_res)
    torch.cuda.synchronize()
    gf_rmse, gs_rmse = rmse(g_ev["x_filt_mean_pooled"]), rmse(g_sm["x_smooth_mean"])
    print(f"grey-box model (Algorithm2, {means.shape[0]} per-iteration models, {g_res.n} particles, {g_res.n_trajectories} backward trajectories per model): "
          f"position filtered RMSE {gf_rmse[0]:.5f}, smoothed RMSE {gs_rmse[0]:.5f}; velocity filtered RMSE {gf_rmse[1]:.5f}, smoothed RMSE {gs_rmse[1]:.5f}; "
          f"smoothed friction force (the interface variable): mean over time {float(g_xi['xi_smooth_mean'][:, 0].mean()):.4f}, range "
          f"[{float(g_xi['xi_smooth_mean'][:, 0].min()):.4f}, {float(g_xi['xi_smooth_mean'][:, 0].max()):.4f}], standard deviation, mean over time "
          f"{float(g_xi['xi_smooth_std'][:, 0].mean()):.4f}, spread of the per-model means {float(g_xi['xi_smooth_mean_draw'][:, :, 0].std(dim=0).mean()):.4f}")


if __name__ == "__main__":
    main()
