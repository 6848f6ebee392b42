"""Device-event timing of the in-kernel predictive moments and log score (pgas_amd.Rollout.predict) on
SingleMassOscillator (M = 41) and EMPS-729 at T = 2000.  Per (K, P) in {(64, 256), (64, 1024), (600, 1024)}:

  predict      moments and log score in one call (k_rollout_stats + k_rollout_stats_finish), output K T (2 (nx + ny) + 1) doubles
  yardstick    the only route to the same moments before: Rollout.__call__ (the (K, T, P, nx) cloud) followed by torch sums of x, x^2,
               H x and (H x)^2 over the replicates
  rollout      Rollout.__call__ alone: predict against it is the price of the reduction on the latency chain

and predict alone at P = 65 536, K = 1 and 64 (64 blocks per draw).  One warm-up call and --reps timed calls each.

usage: rollout_stats_time.py [--models smo,emps] [--T 2000] [--reps 20] [--out FILE]"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="smo,emps")
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/rollout_stats_time.py --models {a.models} --T {T} --reps {a.reps}: {torch.cuda.get_device_name(0)}, device events, one warm-up call")
    for name in a.models.split(","):
        pb = experiments.smo_pgas(T=T) if name == "smo" else experiments.emps_pgas(T=T)
        A, S = experiments.initial_params(pb)
        sim = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov, likelihood_fcn=pb.likelihood_fcn,
                               observations=pb.observations)
        dev = sim.engine.device
        M, nx, ny = sim.engine.M, sim.engine.nx, sim.engine.ny
        Ht = torch.as_tensor(pb.likelihood_fcn.H, device=dev).T.contiguous()

        def params(K):
            As = torch.as_tensor(np.stack([A * (1.0 + 1e-4 * k) for k in range(K)]), device=dev)
            Ss = torch.as_tensor(np.stack([S * (1.0 + 1e-3 * k) for k in range(K)]), device=dev)
            return As, Ss, ch.keys_tensor(prng.split(prng.key(12345678), K), dev)

        for K, P in ((64, 256), (64, 1024), (600, 1024)):
            As, Ss, kd = params(K)

            def yardstick():
                x = sim(As, Ss, kd, replicates=P)
                yh = x @ Ht
                return x.sum(dim=2), (x * x).sum(dim=2), yh.sum(dim=2), (yh * yh).sum(dim=2)

            ms_p = timed(lambda: sim.predict(As, Ss, kd, replicates=P), a.reps)
            ms_m = timed(lambda: sim.predict(As, Ss, kd, replicates=P, log_score=False), a.reps)
            ms_r = timed(lambda: sim(As, Ss, kd, replicates=P), a.reps)
            ms_y = timed(yardstick, a.reps)
            out_b, cloud_b = K * T * (2 * (nx + ny) + 1) * 8, K * T * P * nx * 8
            say(f"{name:5s} M={M:4d} K={K:4d} P={P:6d}: predict {ms_p:9.3f} ms (moments only {ms_m:9.3f} ms), yardstick {ms_y:9.3f} ms ({ms_y / ms_p:6.2f}x), "
                f"rollout alone {ms_r:9.3f} ms (predict / rollout {ms_p / ms_r:5.2f}); output {out_b / 1e6:.3f} MB against a cloud of {cloud_b / 1e6:.1f} MB")
            torch.cuda.empty_cache()
        for K in (1, 64):
            P = 65536
            As, Ss, kd = params(K)
            ms_p = timed(lambda: sim.predict(As, Ss, kd, replicates=P), a.reps)
            say(f"{name:5s} M={M:4d} K={K:4d} P={P:6d}: predict {ms_p:9.3f} ms = {K * P * (T - 1) / (ms_p * 1e-3):.3e} particle-steps/s ({(P + 1023) // 1024} blocks per draw)")
        del sim
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
