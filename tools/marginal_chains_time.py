"""Timing of one Gibbs iteration of C marginalised Particle-Gibbs chains in one batched pass (pgas_amd.MultiChainAlgorithm2, DESIGN.md
section 23) against the same C iterations of Algorithm2 one after another in the same process: SingleMassOscillator, N = 200 particles per
chain, traced model (SymbolicStateSpaceModel), C in {1, 4, 16, 64}.  One iteration = the conditional filter over the whole record (its
initialisation, the T - 1 steps, the final index draw and the trajectories) plus the trajectory statistics -- the body of the loop of
Algorithm2.__call__ / MultiChainAlgorithm2.__call__.  The batched side is timed graph-replayed and launch by launch (the default is the
replay when C N <= 4096), the sequential side as Algorithm2 runs it (replayed: N = 200).

Per configuration: one warm-up of every side, then `reps` rounds that time the sides one after another (interleaved, so that a neighbour's
load on the machine meets all of them), each between a device synchronisation and the next; the medians and their ratio are reported.
Prints one table row and one JSON line per (T, C).

usage: marginal_chains_time.py [--chains 1,4,16,64] [--N 200] [--T 750] [--reps 10] [--batched-only]
(--batched-only: nothing but the batched iterations in their default mode -- the run profiled under rocprofv3.)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pgas_amd  # noqa: E402
from pgas_amd import experiments  # noqa: E402
from pgas_amd import random as prng  # noqa: E402
from pgas_amd.chains import keys_tensor  # noqa: E402


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="1,4,16,64")
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--T", default="750")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batched-only", action="store_true")
    a = ap.parse_args()
    N = a.N
    print(f"{torch.cuda.get_device_name(0)}; SingleMassOscillator, N = {N} particles per chain, traced model; ms per Gibbs iteration of ALL C chains, "
          f"median of {a.reps} interleaved rounds", flush=True)
    for T in [int(t) for t in a.T.split(",")]:
        pb = experiments.smo_marginal(T=T)

        def args():
            return dict(observations=pb.observations, inputs=pb.inputs, SSM=pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel),
                        init_state_mean=pb.init_state_mean, init_state_cov=pb.init_state_cov, init_int_var_mean=pb.init_int_var_mean,
                        init_int_var_cov=pb.init_int_var_cov, GP_prior=pb.GP_prior, basis_fcn=pb.basis_fcn())

        single = pgas_amd.Algorithm2(N, 2, **args())
        dev = single.cSMC.device
        x1 = torch.as_tensor(np.asarray(pb.X_true, dtype=np.float64).reshape(T, -1), device=dev)
        iv1 = [torch.as_tensor(np.asarray(v, dtype=np.float64).reshape(T, -1), device=dev) for v in pb.int_var_true]
        st1 = [list(s) for s in single._trajectory_stats(x1, iv1)]

        def one_chain(key):
            x, iv = single.cSMC(key, x1, iv1, st1)
            single._trajectory_stats(x.reshape(T, -1), [v.reshape(T, -1) for v in iv])

        print(f"T = {T}", flush=True)
        print("    C | batched replayed | batched eager | sequential | sequential / batched (default mode)", flush=True)
        for C in [int(c) for c in a.chains.split(",")]:
            keys = prng.split(prng.key(12345678), C)
            multi = pgas_amd.MultiChainAlgorithm2(C, N, 2, **args())
            kd = keys_tensor(keys, dev)
            xC, ivC = x1.expand(C, *x1.shape).contiguous(), [v.expand(C, *v.shape).contiguous() for v in iv1]
            stC = [list(s) for s in multi._trajectory_stats(xC, ivC)]

            def batched(mode):
                x, iv = multi.cSMC(kd, xC, ivC, stC, use_graph=mode)
                multi._trajectory_stats(x, list(iv))

            def sequential():
                for k in keys:
                    one_chain(k)

            default_graph = C * N <= 4096
            sides = {"batched_default": lambda: batched(None)} if a.batched_only else \
                {"batched_replayed": lambda: batched(True), "batched_eager": lambda: batched(False), "sequential": sequential}
            for f in sides.values():
                f()   # warm-up of every side
            times = {k: [] for k in sides}
            for _ in range(a.reps):
                for k, f in sides.items():
                    times[k].append(wall(f))
            row = dict(C=C, N=N, T=T, reps=a.reps, default_mode="replayed" if default_graph else "eager")
            for k, v in times.items():
                row[k + "_ms"] = statistics.median(v)
                row[k + "_min_ms"], row[k + "_max_ms"] = min(v), max(v)
            if not a.batched_only:
                row["batched_default_ms"] = row["batched_replayed_ms"] if default_graph else row["batched_eager_ms"]
                row["ratio"] = row["sequential_ms"] / row["batched_default_ms"]
                print(f"{C:5d} | {row['batched_replayed_ms']:10.1f} ms    | {row['batched_eager_ms']:10.1f} ms | {row['sequential_ms']:10.1f} ms | {row['ratio']:6.2f}x "
                      f"({row['default_mode']})", flush=True)
            print(json.dumps(row), flush=True)
            del multi
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
