"""Device-event timing of the batched open-loop simulation (pgas_amd.Rollout) on SingleMassOscillator (M = 41) and
EMPS-729 at T = 2000: noise-free K in {1, 16, 64, 600} draws at P = 1 replicate, noisy K = 64 at P in {1, 64, 256}, against the only
device path there was before -- per draw, set_params plus T - 1 dependent aux_states launches (timed for 16 draws one after another,
reported per draw).  particle-steps/s = K P (T - 1) / wall.  Prints one table row per measurement.

usage: rollout_time.py [--models smo,emps] [--T 2000] [--reps 20] [--baseline-draws 16] [--out FILE]"""
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
from pgas_amd._lib import Engine  # noqa: E402


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
    ap.add_argument("--baseline-draws", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/rollout_time.py --models {a.models} --T {T} --reps {a.reps}: {torch.cuda.get_device_name(0)}, device events, one warm-up call")
    for name in a.models.split(","):
        pb = experiments.smo_pgas(T=T) if name == "smo" else experiments.emps_pgas(T=T)
        A, S = experiments.initial_params(pb)
        sim = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov)
        dev = sim.engine.device
        M = sim.engine.M
        x0 = torch.as_tensor(pb.X_true[0], device=dev)

        def params(K):
            As = torch.as_tensor(np.stack([A * (1.0 + 1e-4 * k) for k in range(K)]), device=dev)
            Ss = torch.as_tensor(np.stack([S * (1.0 + 1e-3 * k) for k in range(K)]), device=dev)
            return As, Ss, ch.keys_tensor(prng.split(prng.key(12345678), K), dev)

        # baseline: what a caller could do before -- a context of one particle, per draw set_params and T - 1 dependent launches
        Kb = a.baseline_draws
        As, Ss, _ = params(Kb)
        base = Engine(1, np.zeros((T, 1)), pb.inputs, pb.init_state_mean, pb.init_state_cov, pgas_amd.GaussianLikelihood(np.eye(1, pb.nx), np.eye(1)),
                      pb.basis_fcn)

        def baseline():
            for k in range(Kb):
                base.set_params(As[k], Ss[k])
                x = x0.reshape(1, -1)
                for t in range(1, T):
                    x = base.aux_states(x, t)

        ms_base = timed(baseline, 1) / Kb
        say(f"{name:5s} M={M:4d} baseline (set_params + {T - 1} aux_states launches), per draw of {Kb}: {ms_base:9.3f} ms = {(T - 1) / (ms_base * 1e-3):.3e} particle-steps/s")
        for K in (1, 16, 64, 600):
            As, Ss, _ = params(K)
            ms = timed(lambda: sim(As, init_state=x0), a.reps)
            say(f"{name:5s} M={M:4d} noise-free K={K:4d} P=   1: {ms:9.3f} ms = {K * (T - 1) / (ms * 1e-3):.3e} particle-steps/s; "
                f"{K} draws through the baseline {K * ms_base:10.2f} ms ({K * ms_base / ms:7.1f}x)")
        K = 64
        As, Ss, kd = params(K)
        for P in (1, 64, 256):
            ms = timed(lambda: sim(As, Ss, kd, replicates=P), a.reps)
            say(f"{name:5s} M={M:4d} noisy      K={K:4d} P={P:4d}: {ms:9.3f} ms = {K * P * (T - 1) / (ms * 1e-3):.3e} particle-steps/s")
        del sim, base
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
