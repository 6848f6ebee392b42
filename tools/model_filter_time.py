#!/usr/bin/env python3
"""Device-event timing of the grey-box held-out filter (pgas_amd.ModelRollout.filter) on SingleMassOscillator and
Vehicle at T = 2000, N = 200 particles: K in {1, 16, 64, 256} draws in one call, moments on and traces off; K = 64 also with
moments=False and with traces=True.

  filter     one launch of k_model_filter per call
  baseline   the best route to the same log-likelihood before it, from the primitives alone: a host loop per time step, batched over the
             K draws on a particle axis of K N -- per latent function hilbert_basis and a batched matmul with the draws' coefficients,
             expr_eval of g, expr_eval(mode=2), a logsumexp per draw, runs_uniform + runs_systematic(R = K), runs_normal and
             expr_eval(mode=1) with the gather of x and xi done inside that launch (draw_state_gather).  It forms ell and loglik only
             (none of the moments), which favours it.

The two are run INTERLEAVED, call by call, in one process: one warm-up call each, then --calls rounds, device events around every call.
Medians are reported, with the baseline's own max - min: the noise a difference has to clear.  The baseline draws from the filter's own
Philox streams, so the two log-likelihoods agree to rounding until a resampling threshold falls between their last bits; the largest
relative difference over the draws is printed as a sanity figure.

usage: model_filter_time.py [--models smo,vehicle] [--steps 2000] [--particles 200] [--calls 20] [--draws 1,16,64,256] [--out FILE]"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def one(fn, torch):
    """ms of one call of fn, device events around it."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="smo,vehicle")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--draws", default="1,16,64,256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import pgas_amd
    from pgas_amd import experiments
    from pgas_amd._lib import MarginalOps
    from pgas_amd.Algorithm1 import STREAM_INIT_STATE, STREAM_RESAMPLE, STREAM_STATE

    T, N = args.steps, args.particles
    ops = MarginalOps(1)
    dev = ops.device
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/model_filter_time.py --models {args.models} --steps {T} --particles {N} --calls {args.calls}: {torch.cuda.get_device_name(dev)}, "
        "device events, one warm-up call, filter / baseline interleaved call by call; medians")
    makes = {"smo": ("SMO", experiments.smo_marginal), "vehicle": ("Vehicle", experiments.vehicle_marginal)}
    logN = math.log(N)
    for key in args.models.split(","):
        name, make = makes[key]
        pb = make(T=T)
        ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
        ssm.bind(ops)
        sim = pgas_amd.ModelRollout(pb.inputs, ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, ops=ops, observations=pb.observations)
        nx = sim.nx
        y = torch.as_tensor(np.asarray(pb.observations, dtype=np.float64).reshape(T, sim.ny), device=dev)
        u = torch.as_tensor(np.asarray(pb.inputs, dtype=np.float64).reshape(T, -1), device=dev)
        m0 = torch.as_tensor(np.asarray(pb.init_state_mean, dtype=np.float64), device=dev)
        L0t = torch.as_tensor(np.linalg.cholesky(pb.init_state_cov).T.copy(), device=dev)
        say(f"{name:8s} file {sim._filter_file_bytes()} B, dynamic LDS {sim.filter_lds_bytes(N)} B at N = {N}, max_particles() = {sim.max_particles()}")
        rng = np.random.default_rng(1)
        for K in [int(k) for k in args.draws.split(",")]:
            A = []
            for g in pb.GP_prior:
                sd = np.diag(np.linalg.inv(np.asarray(g[1])))
                A.append(torch.as_tensor(0.1 * rng.standard_normal((K, 1, sd.size)) * sd, device=dev))
            At = [a.transpose(1, 2).contiguous() for a in A]
            keys = pgas_amd.chains.keys_tensor(list(range(1, K + 1)), dev)
            bops = MarginalOps(K * N, dev)          # the baseline's context: K runs of N particles on one particle axis
            bssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
            bssm.bind(bops)

            def xi_of(x, ut):
                out = []
                for i, b in enumerate(pb.basis):
                    phi = bops.hilbert_basis(b.map, b.alpha(x, ut).reshape(-1, 1).contiguous(), None) if hasattr(b, "feature") else bops.hilbert_basis(b, x, ut)
                    out.append(torch.bmm(phi.view(K, N, -1), At[i]).reshape(K * N, -1))
                return out

            def baseline():
                x = m0 + bops.runs_normal(keys, STREAM_INIT_STATE, 0, nx) @ L0t
                ell = torch.empty((K, T), dtype=torch.float64, device=dev)
                for t in range(T):
                    xi = xi_of(x, u[t])
                    bssm.output_mdl(x, u[t], *xi)                                        # g (the predicted observation of the step)
                    l = bssm.log_likelihood(y[t], x, u[t], *xi).view(K, N)
                    ell[:, t] = torch.logsumexp(l, dim=1) - logN
                    if t == T - 1:
                        break
                    _, glo = bops.runs_systematic(K, bops.runs_uniform(keys, STREAM_RESAMPLE, t), l)
                    x = bssm.draw_state_gather(bops.runs_normal(keys, STREAM_STATE, t + 1, nx), x, u[t], glo.view(-1), *xi)
                return ell, ell.sum(dim=1)

            variants = [("moments", lambda: sim.filter(A, keys, N))]
            if K == 64:
                variants += [("moments=False", lambda: sim.filter(A, keys, N, moments=False)), ("traces=True", lambda: sim.filter(A, keys, N, traces=True))]
            got, ref = variants[0][1](), baseline()                                      # the warm-up calls, compared as a sanity figure
            for _, fn in variants[1:]:
                fn()
            torch.cuda.synchronize()
            gap = float((got.loglik - ref[1]).abs().max() / ref[1].abs().max())           # the same Philox streams: equal to rounding until a threshold falls between the two
            del got, ref
            ms = {w: [] for w, _ in variants}
            ms["baseline"] = []
            for _ in range(args.calls):
                for w, fn in variants:
                    ms[w].append(one(fn, torch))
                ms["baseline"].append(one(baseline, torch))
            med = {w: float(np.median(v)) for w, v in ms.items()}
            spread = float(np.max(ms["baseline"]) - np.min(ms["baseline"]))
            gain = med["baseline"] - med["moments"]
            say(f"{name:8s} K={K:4d} N={N}: filter {med['moments']:9.3f} ms (min {np.min(ms['moments']):9.3f}, max {np.max(ms['moments']):9.3f}) = "
                f"{1e3 * med['moments'] / T:7.3f} us/step, {K * N * T / (med['moments'] * 1e-3):.3e} particle-steps/s; "
                f"baseline {med['baseline']:9.3f} ms (min {np.min(ms['baseline']):9.3f}, max {np.max(ms['baseline']):9.3f}, max - min {spread:8.3f})")
            say(f"{'':8s} baseline / filter {med['baseline'] / med['moments']:6.1f}x; baseline - filter = {gain:9.3f} ms {'>' if gain > spread else '<='} the baseline's "
                f"max - min; max rel. |loglik - baseline's| = {gap:.2e} (two Monte Carlo estimates)")
            for w, _ in variants[1:]:
                say(f"{'':8s} K={K:4d} {w}: {med[w]:9.3f} ms (min {np.min(ms[w]):9.3f}, max {np.max(ms[w]):9.3f})")
            del A, At, bops, bssm
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
