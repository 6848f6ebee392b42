"""Device-event timing of C independent PGAS chains in batched launches: one batched sweep
(condSequentialMonteCarloChains) and one full batched Gibbs iteration (MultiChainPGAS.step: keys, sweep, statistics, MNIW algebra,
draws) for C in {1, 16, 64, 256, 512, 1024}, on SingleMassOscillator-PGAS and EMPS-729 at the reference's size (N = 200, T = 2000),
against the same C chains swept one after another through condSequentialMonteCarlo (C <= 64).  particle-steps/s = C N (T - 1) / wall.
Prints one table row and one JSON line per measurement.

usage: chains_time.py [--models smo,emps] [--chains 1,16,64,256,512,1024] [--reps 3] [--seq-max 64] [--gibbs-only C] [--json OUT]
(--gibbs-only C: one batched Gibbs iteration of C chains, warm-up plus three timed, nothing else -- the run profiled under rocprofv3.)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pgas_amd  # noqa: E402
from pgas_amd import chains as ch  # noqa: E402
from pgas_amd import experiments  # noqa: E402
from pgas_amd import random as prng  # noqa: E402


def timed(f, reps):
    """ms per call of f, device events around `reps` calls after one warm-up call."""
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def problem(name, T):
    return experiments.smo_pgas(T=T) if name == "smo" else experiments.emps_pgas(T=T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="smo,emps")
    ap.add_argument("--chains", default="1,16,64,256,512,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seq-max", type=int, default=64)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--gibbs-only", type=int, default=0)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    N, T = a.N, a.T
    rows = []
    for name in a.models.split(","):
        pb = problem(name, T)
        A, S = experiments.initial_params(pb)
        Cs = [a.gibbs_only] if a.gibbs_only else [int(c) for c in a.chains.split(",")]
        for C in Cs:
            dev = torch.device("cuda", torch.cuda.current_device())
            mc = pgas_amd.MultiChainPGAS(C, N, 2, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn,
                                         pb.GP_prior, pb.basis_fcn, keep_chain_log=False)
            eng = mc.cSMC.engine
            keys = ch.keys_tensor(prng.split(prng.key(12345678), C), dev)
            As = torch.as_tensor(np.repeat(A[None], C, axis=0), device=dev)
            Ss = torch.as_tensor(np.repeat(S[None], C, axis=0), device=dev)
            ref = torch.as_tensor(np.repeat(pb.X_true.reshape(1, T, -1), C, axis=0), device=dev)
            state = dict(k=keys, traj=ref, A=As, S=Ss)

            def gibbs():
                state["k"], state["traj"], state["A"], state["S"], _ = mc.step(state["k"], state["traj"], state["A"], state["S"])

            if a.gibbs_only:
                ms_gibbs = timed(gibbs, 3)
                print(f"{name} C={C}: one batched Gibbs iteration {ms_gibbs:.2f} ms")
                continue
            ms_sweep = timed(lambda: mc.cSMC(keys, ref, As, Ss), a.reps)
            ms_gibbs = timed(gibbs, a.reps)
            ps = C * N * (T - 1) / (ms_sweep * 1e-3)
            row = dict(model=name, M=eng.M, N=N, T=T, C=C, batched_sweep_ms=ms_sweep, batched_particle_steps_per_s=ps, gibbs_iteration_ms=ms_gibbs)
            if C <= a.seq_max:
                single = mc.cSMC.single
                refs = [ref[c] for c in range(C)]
                kl = prng.split(prng.key(12345678), C)

                def sequential():
                    for c in range(C):
                        single(kl[c], refs[c], As[c], Ss[c])

                ms_seq = timed(sequential, 1 if C > 16 else a.reps)
                row.update(sequential_ms=ms_seq, sequential_particle_steps_per_s=C * N * (T - 1) / (ms_seq * 1e-3), speedup=ms_seq / ms_sweep)
            rows.append(row)
            seq = f", one after another {row['sequential_ms']:8.2f} ms ({row['speedup']:.1f}x)" if "sequential_ms" in row else ""
            print(f"{name:5s} M={eng.M:4d} C={C:5d}: batched sweep {ms_sweep:8.2f} ms = {ps:.3e} particle-steps/s, Gibbs iteration "
                  f"{ms_gibbs:8.2f} ms{seq}", flush=True)
            print(json.dumps(row), flush=True)
            del mc, eng
            torch.cuda.empty_cache()
    # the hard bar of DESIGN.md section 11: 256 batched chains against chains swept one after another (the sequential rate measured on <= 64)
    for name in a.models.split(","):
        r256 = [r for r in rows if r["model"] == name and r["C"] == 256]
        seq = [r for r in rows if r["model"] == name and "sequential_particle_steps_per_s" in r]
        if r256 and seq:
            best_seq = max(r["sequential_particle_steps_per_s"] for r in seq)
            print(f"{name}: 256 batched chains deliver {r256[0]['batched_particle_steps_per_s'] / best_seq:.1f}x the particle-steps/s of the best "
                  f"sequential rate ({best_seq:.3e})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
