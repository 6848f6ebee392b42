"""Device-event timing of R independent runs of the marginalised online filter in one batched pass (pgas_amd.MultiRunAlgorithm1, DESIGN.md
section 12) against the same R runs of Algorithm1 one after another in the same process: SingleMassOscillator, N = 200, the driver's T,
traced model (SymbolicStateSpaceModel), R in {1, 4, 16, 64, 256}.  What is timed is the filter loop t = 1 .. T-1 with its initialisation
(not the output / log-likelihood passes of __call__ behind it), graph-replayed and eager; ms per step = time / (T - 1), for ALL R runs.
One warm-up pass per configuration, then `reps` timed passes between two device events (the sequential side: one pass, after one warm-up run).
Prints one table row and one JSON line per R.

usage: runs_time.py [--runs 1,4,16,64,256] [--N 200] [--T 750] [--reps 3] [--seq-max 256] [--batched-only]
(--batched-only: nothing but the replayed batched passes -- the run profiled under rocprofv3.)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pgas_amd  # noqa: E402
from pgas_amd import experiments  # noqa: E402
from pgas_amd import random as prng  # noqa: E402


def loop(alg, key, use_graph):
    """The filter loop of alg.__call__ without the passes over the traces behind it."""
    rand = alg._rand(key)
    st, iv, sst, lw, anc, stats = alg._init_algorithm(rand)
    traces, T = (st, iv, sst, lw, anc), alg.observations.shape[0]
    if use_graph:
        alg._graphed_loop(rand, traces, stats, T)
    else:
        for t in range(1, T):
            stats = alg._loop_body(rand, t, traces, stats)


def timed(f, reps, warm=True):
    if warm:
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="1,4,16,64,256")
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--T", type=int, default=750)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seq-max", type=int, default=256)
    ap.add_argument("--batched-only", action="store_true")
    a = ap.parse_args()
    N, T = a.N, a.T
    pb = experiments.smo_marginal(T=T)

    def args():
        return dict(observations=pb.observations, inputs=pb.inputs, SSM=pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel),
                    forgetting_factor=pb.forgetting_factor, init_state_mean=pb.init_state_mean, init_state_cov=pb.init_state_cov,
                    init_int_var_mean=pb.init_int_var_mean, init_int_var_cov=pb.init_int_var_cov, GP_prior=pb.GP_prior, basis_fcn=pb.basis_fcn())

    print(f"{torch.cuda.get_device_name(0)}; SingleMassOscillator, N = {N} particles per run, T = {T}, traced model; ms per filter step of ALL R runs",
          flush=True)
    single = pgas_amd.Algorithm1(N, **args())
    if not a.batched_only:
        for mode in (True, False):
            loop(single, 1, mode)   # warm-up of the sequential side
    print("    R | batched replayed | batched eager | sequential replayed | sequential eager | ratio replayed | ratio eager", flush=True)
    for R in [int(r) for r in a.runs.split(",")]:
        keys = prng.split(prng.key(12345678), R)
        multi = pgas_amd.MultiRunAlgorithm1(R, N, **args())
        reps = a.reps if R <= 64 else max(1, a.reps - 1)
        row = dict(R=R, N=N, T=T, batched_replayed_ms=timed(lambda: loop(multi, keys, True), reps) / (T - 1))
        if a.batched_only:
            print(json.dumps(row), flush=True)
            continue
        row["batched_eager_ms"] = timed(lambda: loop(multi, keys, False), reps) / (T - 1)
        if R <= a.seq_max:
            def sequential(mode):
                for k in keys:
                    loop(single, k, mode)

            row["sequential_replayed_ms"] = timed(lambda: sequential(True), 1, warm=False) / (T - 1)
            row["sequential_eager_ms"] = timed(lambda: sequential(False), 1, warm=False) / (T - 1)
            row["ratio_replayed"] = row["sequential_replayed_ms"] / row["batched_replayed_ms"]
            row["ratio_eager"] = row["sequential_eager_ms"] / row["batched_eager_ms"]
        f = lambda k: f"{row[k]:10.3f}" if k in row else "         -"   # noqa: E731
        print(f"{R:5d} | {f('batched_replayed_ms')} ms    | {f('batched_eager_ms')} ms | {f('sequential_replayed_ms')} ms       | {f('sequential_eager_ms')} ms    | "
              f"{f('ratio_replayed')}x    | {f('ratio_eager')}x", flush=True)
        print(json.dumps(row), flush=True)
        del multi
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
