"""Shared body of the reference's *_Simulation.py drivers for the marginalised family: Algorithm1 (online), a second Algorithm1 run
that supplies the initial reference trajectory (index drawn from the cumulative sum of the FLATTENED (T,N) weights, the reference's
quirk Q13, e.g. SingleMassOscillator_Simulation.py:54), then Algorithm2 (offline Particle Gibbs).

Opt-in convergence check: ``chains=C`` (command line: ``python examples/_marginal_driver.py --model smo --chains 4``) runs C more
Particle-Gibbs chains from the same initial reference in one batched pass (pgas_amd.MultiChainAlgorithm2) and prints the split-R-hat of
the latent functions' coefficients over the chains.  Without it the run is what it always was."""
from __future__ import annotations

import os
import sys
import time as _time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_online_offline(pb, particles, iterations, seed=12345678, device=None, log=print, chains=0):
    import torch

    import pgas_amd
    from pgas_amd import random as prng

    ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)   # the model callables traced into one-launch programs (StateSpaceModel + torch callables works the same)
    common = dict(observations=pb.observations, inputs=pb.inputs, SSM=ssm, init_state_mean=pb.init_state_mean, init_state_cov=pb.init_state_cov,
                  init_int_var_mean=pb.init_int_var_mean, init_int_var_cov=pb.init_int_var_cov, GP_prior=pb.GP_prior, basis_fcn=pb.basis_fcn(),
                  device=device)
    alg1 = pgas_amd.Algorithm1(N_samples=particles, forgetting_factor=pb.forgetting_factor, **common)
    alg2 = pgas_amd.Algorithm2(N_samples=particles, N_iterations=iterations, **common)
    T = pb.T
    key = prng.key(seed)
    key, key_sim = prng.split(key, 2)
    t0 = _time.perf_counter()
    online = alg1(key_sim)
    torch.cuda.synchronize()
    t_on = _time.perf_counter() - t0
    log(f"online (Algorithm1): N={particles}, T={T}: {t_on:.2f} s = {particles * (T - 1) / t_on:.3e} particle-steps/s")
    key, key_sim, key_traj = prng.split(key, 3)
    r_X, r_iv, _, r_w, r_anc, _, _, _ = alg1(key_sim)
    u = float(prng.uniform(key_traj, 1)[0])
    idx = min(int(np.searchsorted(np.cumsum(r_w.cpu().numpy()), u)), particles - 1)
    ref_state = pgas_amd.reconstruct_trajectory(r_X, r_anc, idx)
    ref_iv = [pgas_amd.reconstruct_trajectory(v, r_anc, idx) for v in r_iv]
    t0 = _time.perf_counter()
    offline = alg2(key, ref_state, ref_iv)
    torch.cuda.synchronize()
    t_off = _time.perf_counter() - t0
    log(f"offline (Algorithm2): K={iterations}: {t_off:.2f} s = {particles * (T - 1) * max(iterations - 1, 1) / t_off:.3e} particle-steps/s")
    times = dict(seconds_online=t_on, seconds_offline=t_off)
    if chains:
        times.update(chains_rhat(pb, common, particles, iterations, chains, key, ref_state, ref_iv, log))
    return online, offline, times


def chain_coefficients(prior, stats):
    """MNIW posterior-mean coefficients eta1^-1 eta0 (BI:35-45) of prior + statistics for every chain and iteration: stats = (T0 (C, K, M, n),
    T1 (C, K, M, M), ...) on the device -> (C, K, M n)."""
    import torch

    T0, T1 = stats[0], stats[1]
    e0 = torch.as_tensor(np.asarray(prior[0], dtype=np.float64).reshape(T0.shape[2:]), device=T0.device) + T0
    e1 = torch.as_tensor(np.asarray(prior[1], dtype=np.float64), device=T0.device) + T1
    return torch.linalg.solve(e1, e0).reshape(T0.shape[0], T0.shape[1], -1)


def chains_rhat(pb, common, particles, iterations, chains, key, ref_state, ref_iv, log=print):
    """C Particle-Gibbs chains in one batched pass from one initial reference; split-R-hat (pgas_amd.split_rhat) of every latent function's
    coefficients over the second half of the iterations.  Needs at least 8 iterations (4 draws per half chain)."""
    import torch

    import pgas_amd

    alg = pgas_amd.MultiChainAlgorithm2(chains, N_samples=particles, N_iterations=iterations, **common)
    t0 = _time.perf_counter()
    out = alg(key, ref_state, ref_iv)
    torch.cuda.synchronize()
    secs = _time.perf_counter() - t0
    log(f"offline, {chains} chains in one batch (MultiChainAlgorithm2): K={iterations}: {secs:.2f} s = "
        f"{chains * particles * (pb.T - 1) * max(iterations - 1, 1) / secs:.3e} particle-steps/s")
    res = dict(seconds_chains=secs, chains_state_trace=out[0])
    for i, stats in enumerate(out[3]):
        coeff = chain_coefficients(pb.GP_prior[i], stats)[:, iterations // 2:]
        if coeff.shape[1] < 4 or chains < 2:
            log(f"latent function {i}: split-R-hat needs at least 2 chains and 8 iterations")
            continue
        rhat = pgas_amd.split_rhat(coeff)
        res[f"rhat_{i}"] = rhat.cpu().numpy()
        log(f"latent function {i}: split-R-hat of its {rhat.numel()} coefficients over {chains} chains, iterations {iterations // 2} .. {iterations - 1}: "
            f"median {rhat.median().item():.3f}, max {rhat.max().item():.3f}")
    return res


def posterior_mean(prior, stats):
    """MNIW posterior mean (1, M) of prior + stats (BI:35-45) for statistics given with the reference's shapes."""
    import pgas_amd

    e0 = np.asarray(prior[0]).reshape(-1, 1) + np.asarray(stats[0]).reshape(-1, 1)
    e1 = np.asarray(prior[1]) + np.asarray(stats[1])
    e2 = np.reshape(prior[2], (1, 1)) + np.reshape(stats[2], (1, 1))
    e3 = float(np.reshape(prior[3], -1)[0]) + float(np.reshape(stats[3], -1)[0])
    return pgas_amd.prior_mniw_2naturalPara_inv(e0, e1, e2, e3)[0]


def main():
    import argparse

    import pgas_amd  # noqa: F401
    from pgas_amd import experiments

    ap = argparse.ArgumentParser(description="online filter, offline Particle Gibbs and (opt-in) a batched multi-chain convergence check")
    ap.add_argument("--model", choices=("smo", "vehicle", "emps", "toy"), default="smo")
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=800)
    ap.add_argument("--steps", type=int, default=750)
    ap.add_argument("--chains", type=int, default=0, help="C > 0: C more chains in one batched pass, split-R-hat of the latent functions' coefficients")
    a = ap.parse_args()
    make = {"smo": experiments.smo_marginal, "vehicle": experiments.vehicle_marginal, "emps": experiments.emps_marginal, "toy": experiments.toy_marginal}[a.model]
    run_online_offline(make(T=a.steps), a.particles, a.iterations, chains=a.chains)


if __name__ == "__main__":
    main()
