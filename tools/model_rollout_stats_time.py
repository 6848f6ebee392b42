#!/usr/bin/env python3
"""Device-event timing of the grey-box rollout's in-kernel predictive moments and log score (pgas_amd.ModelRollout.predict, DESIGN.md
section 14) on SingleMassOscillator and Vehicle at T = 2000.  Per (K, P) in {(64, 256), (64, 1024), (600, 1024)}, process noise on, x_0
drawn, the model's observations scored:

  predict      moments and log score in one call (k_model_rollout_stats + k_rollout_stats_finish): K T (2 (nx + ny) + 1) doubles out,
               K ceil(P / 64) T (2 (nx + ny) + 2) doubles of partial sums in between
  yardstick    the only route to the same numbers without it: ModelRollout.__call__(outputs=True) (both clouds), torch sums of x, x^2,
               y, y^2 over the replicates, then the Gaussian log-density of StateSpaceModel.log_likelihood on the stored outputs (one
               batched torch expression over (K, T, P), cheaper than a call per step) and a logsumexp over the replicates
  rollout      ModelRollout.__call__(outputs=True) alone: predict against it is the price of the reduction on the latency chain

The three are run INTERLEAVED, call by call, in one process: one warm-up call each, then --calls rounds of (predict, yardstick, rollout),
device events around every call.  Medians are reported, with the yardstick's own max - min: the noise a difference has to clear.  If the
yardstick cannot allocate its clouds at a point, that is reported and the point is repeated at half the draws.

usage: model_rollout_stats_time.py [--models smo,vehicle] [--steps 2000] [--calls 20] [--out FILE]"""
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import pgas_amd
    from pgas_amd import experiments
    from pgas_amd._lib import MarginalOps

    T = args.steps
    ops = MarginalOps(1)
    dev = ops.device
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/model_rollout_stats_time.py --models {args.models} --steps {T} --calls {args.calls}: {torch.cuda.get_device_name(dev)}, device events, "
        "one warm-up call, predict / yardstick / rollout interleaved call by call; medians")
    makes = {"smo": ("SMO", experiments.smo_marginal), "vehicle": ("Vehicle", experiments.vehicle_marginal)}
    for key in args.models.split(","):
        name, make = makes[key]
        pb = make(T=T)
        ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
        ssm.bind(ops)
        sim = pgas_amd.ModelRollout(pb.inputs, ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, ops=ops, observations=pb.observations)
        nx, ny = sim.nx, sim.ny
        y = torch.as_tensor(np.asarray(pb.observations, dtype=np.float64).reshape(T, ny), device=dev)
        LRinvT = torch.as_tensor(ssm._LRinv, device=dev).T.contiguous()
        rng = np.random.default_rng(1)
        todo = [(64, 256), (64, 1024), (600, 1024)]
        while todo:
            K, P = todo.pop(0)
            A = []
            for g in pb.GP_prior:
                sd = np.diag(np.linalg.inv(np.asarray(g[1])))
                A.append(torch.as_tensor(0.1 * rng.standard_normal((K, 1, sd.size)) * sd, device=dev))
            keys = pgas_amd.chains.keys_tensor(list(range(1, K + 1)), dev)

            def predict():
                return sim.predict(A, keys, replicates=P)

            def rollout():
                return sim(A, keys, replicates=P, outputs=True)

            def yardstick():
                ox, oy = sim(A, keys, replicates=P, outputs=True)
                mom = ox.sum(dim=2), (ox * ox).sum(dim=2), oy.sum(dim=2), (oy * oy).sum(dim=2)
                e = (y[None, :, None, :] - oy) @ LRinvT                               # StateSpaceModel.log_likelihood on the stored outputs
                ll = ssm._cR - 0.5 * (e * e).sum(dim=-1)
                return mom, torch.logsumexp(ll, dim=2) - math.log(P)

            fns = (("predict", predict), ("yardstick", yardstick), ("rollout", rollout))
            C = 2 * (nx + ny) + 2
            part_mb, out_mb = K * ((P + 63) // 64) * T * C * 8 / 1e6, K * T * (C - 1) * 8 / 1e6
            cloud_mb = K * T * P * (nx + ny) * 8 / 1e6
            try:
                got, ref = predict(), yardstick()                                     # the warm-up calls, compared as a sanity figure
                rollout()
                torch.cuda.synchronize()
                err = max(float(((a - b).abs() / (1e-300 + b.abs()).clamp(min=1.0)).max()) for a, b in
                          zip((got.x_sum, got.x_sumsq, got.y_sum, got.y_sumsq, got.lpd), ref[0] + (ref[1],)))
                del got, ref
                ms = {w: [] for w, _ in fns}
                for _ in range(args.calls):
                    for w, fn in fns:
                        ms[w].append(one(fn, torch))
            except torch.cuda.OutOfMemoryError as e:
                say(f"{name:8s} K={K:4d} P={P:5d}: the yardstick cannot allocate its clouds of {cloud_mb:.1f} MB (+ temporaries): {str(e).splitlines()[0]}")
                torch.cuda.empty_cache()
                if K > 1:
                    todo.insert(0, (K // 2, P))
                continue
            med = {w: float(np.median(v)) for w, v in ms.items()}
            spread = float(np.max(ms["yardstick"]) - np.min(ms["yardstick"]))
            gain = med["yardstick"] - med["predict"]
            say(f"{name:8s} K={K:4d} P={P:5d}: predict {med['predict']:9.3f} ms (min {np.min(ms['predict']):9.3f}, max {np.max(ms['predict']):9.3f}), "
                f"yardstick {med['yardstick']:9.3f} ms (min {np.min(ms['yardstick']):9.3f}, max {np.max(ms['yardstick']):9.3f}, max - min {spread:8.3f}), "
                f"rollout alone {med['rollout']:9.3f} ms")
            say(f"{'':8s} yardstick / predict {med['yardstick'] / med['predict']:5.2f}x, predict / rollout {med['predict'] / med['rollout']:5.2f}, "
                f"reduction {1e3 * (med['predict'] - med['rollout']) / T:+7.3f} us/step over the rollout's {1e3 * med['rollout'] / T:7.3f}; "
                f"yardstick - predict = {gain:9.3f} ms {'>' if gain > spread else '<='} the yardstick's max - min")
            say(f"{'':8s} part {part_mb:.1f} MB, output {out_mb:.3f} MB, against clouds of {cloud_mb:.1f} MB; max rel. |predict - yardstick| = {err:.2e}")
            del A
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
