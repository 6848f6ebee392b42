"""Device-event timing of the held-out smoother (pgas_amd.HeldOutFilter.smooth) on SingleMassOscillator (M = 41)
and EMPS-729 at T = 2000, N = 200 particles: the pgas_smooth launch alone (from the traces of one filter call) and smooth() in all, the
filter included, for K in {1, 16, 64, 256} draws of B = 64 trajectories, and at K = 64 for B in {1, 4, 16, 64, 256} -- one trajectory
costs a wave its per-row work, B = 1 and B = 4 cost the same (a wave each), so the intercept is the part every row pays once (the
transition means, the barriers) and the slope from B = 4 upwards is the wave work per trajectory-row.  trajectory-rows/s = K B T / time.

Baseline, the only route there was before: one filter call with traces, then a host loop per draw, per trajectory and per row over
aux_states, a torch Gaussian log-density against the next smoothed state, a logsumexp and a draw on the host.  Timed for
`--baseline-draws` draws x `--baseline-trajectories` trajectories and scaled to 64 x 64.

usage: smooth_time.py [--models smo,emps] [--T 2000] [--N 200] [--B 64] [--reps 20] [--baseline-draws 4] [--baseline-trajectories 4] [--out FILE]"""
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
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-draws", type=int, default=4)
    ap.add_argument("--baseline-trajectories", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T, N, B = a.T, a.N, a.B
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/smooth_time.py --models {a.models} --T {T} --N {N} --B {B} --reps {a.reps}: {torch.cuda.get_device_name(0)}, device events, one warm-up call")
    for name in a.models.split(","):
        pb = experiments.smo_pgas(T=T) if name == "smo" else experiments.emps_pgas(T=T)
        A, S = experiments.initial_params(pb)
        lik = pb.likelihood_fcn
        flt = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, lik, pb.nx, N, pb.init_state_mean, pb.init_state_cov)
        eng = flt.engine
        dev, M, nx = eng.device, eng.M, pb.nx

        def params(K):
            As = torch.as_tensor(np.stack([A * (1.0 + 1e-4 * k) for k in range(K)]), device=dev)
            Ss = torch.as_tensor(np.stack([S * (1.0 + 1e-3 * k) for k in range(K)]), device=dev)
            return As, Ss, ch.keys_tensor(prng.split(prng.key(12345678), K), dev)

        # ---- baseline: per draw, per trajectory and per row, dependent launches of existing pieces and a draw on the host
        Kb, Bb = a.baseline_draws, a.baseline_trajectories
        As, Ss, kd = params(Kb)
        ms_filter_b = timed(lambda: flt(As, Ss, kd, traces=True), a.reps)
        tr = flt(As, Ss, kd, traces=True)
        base = Engine(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, lik, pb.basis_fcn)
        y = torch.as_tensor(np.asarray(pb.observations, dtype=np.float64).reshape(T, -1), device=dev)
        Ht = torch.as_tensor(lik.H.T.copy(), device=dev)
        LRinv_t = torch.as_tensor(lik.LRinv.T.copy(), device=dev)
        rng = np.random.default_rng(1)

        def baseline():
            out = []
            for k in range(Kb):
                base.set_params(As[k], Ss[k])
                LSinv_t = torch.linalg.inv(torch.linalg.cholesky(Ss[k])).T
                for _ in range(Bb):
                    xn, path = None, []
                    for t in range(T - 1, -1, -1):
                        x = tr.x[k, t]
                        w = (y[t] - x @ Ht) @ LRinv_t
                        v = -0.5 * (w * w).sum(dim=1)
                        if xn is not None:
                            d = (xn - base.aux_states(x, t + 1)) @ LSinv_t
                            v = v - 0.5 * (d * d).sum(dim=1)
                        cdf = torch.cumsum(torch.exp(v - torch.logsumexp(v, dim=0)), dim=0)
                        j = min(int(torch.searchsorted(cdf, rng.uniform())), N - 1)   # the host-side draw
                        xn = x[j]
                        path.append(j)
                    out.append(path)
            return out

        ms_traj = timed(baseline, 1) / (Kb * Bb)
        ms_base = 64 * ms_filter_b / Kb + 64 * 64 * ms_traj
        say(f"{name:5s} M={M:4d} N={N} baseline (per row: aux_states, torch log-densities, logsumexp, cumsum, a draw on the host), per trajectory of "
            f"{Kb} x {Bb}: {ms_traj:9.3f} ms = {ms_traj * 1e3 / T:7.1f} us per row; 64 draws x 64 trajectories with the filter: {ms_base:11.1f} ms")
        del tr, base

        def row(K, Bn, with_all):
            As, Ss, kd = params(K)
            f = flt(As, Ss, kd, traces=True)
            ms_s = timed(lambda: eng.smooth(As, Ss, kd, f.x, f.anc, min(Bn, 256), 0, True, False, False), a.reps)
            ms_x = timed(lambda: eng.smooth(As, Ss, kd, f.x, f.anc, min(Bn, 256), 0, True, True, True), a.reps)
            del f
            txt = (f"{name:5s} M={M:4d} N={N} K={K:4d} B={Bn:4d}: pgas_smooth {ms_s:9.3f} ms (with xs and idx {ms_x:9.3f} ms) = "
                   f"{K * Bn * T / (ms_s * 1e-3):.3e} trajectory-rows/s, {ms_s * 1e3 / T:7.2f} us per row")
            if with_all:
                ms_f = timed(lambda: flt(As, Ss, kd, traces=True), a.reps)
                ms_all = timed(lambda: flt.smooth(As, Ss, kd, Bn), a.reps)
                txt += f"; filter with traces {ms_f:9.3f} ms; smooth() in all {ms_all:9.3f} ms"
                if K == 64 and Bn == 64:
                    txt += f"; baseline {ms_base:11.1f} ms ({ms_base / ms_all:8.1f}x)"
            say(txt)

        for K in (1, 16, 64, 256):
            row(K, B, True)
        for Bn in (1, 4, 16, 64, 256):
            if Bn != B:
                row(64, Bn, False)
        del flt, eng
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
