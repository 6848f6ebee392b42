"""Device-event timing of the batched bootstrap particle filter (pgas_amd.HeldOutFilter) on SingleMassOscillator
(M = 41) and EMPS-729 at T = 2000, N = 200 particles: K in {1, 16, 64, 256} draws in one call (log-likelihood and moments, no traces),
against the only route there was before -- a host loop per draw and per step over aux_states, torch noise, a torch log-density and
logsumexp, systematic_SISR and a gather (timed for 4 draws one after another, reported per draw).  particle-steps/s = K N T / wall.
Prints one table row per measurement.

usage: filter_time.py [--models smo,emps] [--T 2000] [--N 200] [--reps 20] [--baseline-draws 4] [--out FILE]"""
import argparse
import math
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
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-draws", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T, N = a.T, a.N
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/filter_time.py --models {a.models} --T {T} --N {N} --reps {a.reps}: {torch.cuda.get_device_name(0)}, device events, one warm-up call")
    for name in a.models.split(","):
        pb = experiments.smo_pgas(T=T) if name == "smo" else experiments.emps_pgas(T=T)
        A, S = experiments.initial_params(pb)
        lik = pb.likelihood_fcn
        flt = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, lik, pb.nx, N, pb.init_state_mean, pb.init_state_cov)
        dev = flt.engine.device
        M = flt.engine.M

        def params(K):
            As = torch.as_tensor(np.stack([A * (1.0 + 1e-4 * k) for k in range(K)]), device=dev)
            Ss = torch.as_tensor(np.stack([S * (1.0 + 1e-3 * k) for k in range(K)]), device=dev)
            return As, Ss, ch.keys_tensor(prng.split(prng.key(12345678), K), dev)

        # baseline: what a caller could do before -- per draw and per step, dependent launches of existing pieces
        Kb = a.baseline_draws
        As, Ss, _ = params(Kb)
        base = Engine(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, lik, pb.basis_fcn)
        y = torch.as_tensor(np.asarray(pb.observations, dtype=np.float64).reshape(T, -1), device=dev)
        Ht = torch.as_tensor(lik.H.T.copy(), device=dev)
        LRinv_t = torch.as_tensor(lik.LRinv.T.copy(), device=dev)
        m0 = torch.as_tensor(pb.init_state_mean, device=dev)
        L0t = torch.as_tensor(np.linalg.cholesky(pb.init_state_cov).T.copy(), device=dev)
        logN = math.log(N)

        def baseline():
            out = []
            for k in range(Kb):
                base.set_params(As[k], Ss[k])
                LSt = torch.linalg.cholesky(Ss[k]).T
                x = m0 + torch.randn((N, pb.nx), dtype=torch.float64, device=dev) @ L0t
                total = torch.zeros((), dtype=torch.float64, device=dev)
                for t in range(T):
                    if t > 0:
                        x = base.aux_states(x, t) + torch.randn((N, pb.nx), dtype=torch.float64, device=dev) @ LSt
                    w = (y[t] - x @ Ht) @ LRinv_t
                    l = lik.cR - 0.5 * (w * w).sum(dim=1)
                    m = l.max()
                    total = total + (torch.logsumexp(l, dim=0) - logN)
                    anc = pgas_amd.systematic_SISR(1000 * k + t, torch.exp(l - m), device=dev)
                    x = x[anc.long()]
                out.append(total)
            return out

        ms_base = timed(baseline, 1) / Kb
        say(f"{name:5s} M={M:4d} N={N} baseline (per step: aux_states, torch noise, log-density, logsumexp, systematic_SISR, gather), per draw of {Kb}: "
            f"{ms_base:9.3f} ms = {N * T / (ms_base * 1e-3):.3e} particle-steps/s")
        for K in (1, 16, 64, 256):
            As, Ss, kd = params(K)
            ms = timed(lambda: flt(As, Ss, kd), a.reps)
            say(f"{name:5s} M={M:4d} N={N} filter K={K:4d}: {ms:9.3f} ms = {K * N * T / (ms * 1e-3):.3e} particle-steps/s; "
                f"{K} draws through the baseline {K * ms_base:10.2f} ms ({K * ms_base / ms:7.1f}x)")
        As, Ss, kd = params(64)
        ms = timed(lambda: flt(As, Ss, kd, moments=False), a.reps)
        say(f"{name:5s} M={M:4d} N={N} filter K=  64, log-likelihood only (moments=False): {ms:9.3f} ms")
        ms = timed(lambda: flt(As, Ss, kd, traces=True), a.reps)
        say(f"{name:5s} M={M:4d} N={N} filter K=  64, with traces (x, anc): {ms:9.3f} ms")
        del flt, base
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
