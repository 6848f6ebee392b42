#!/usr/bin/env python3
"""Device-event timing of the grey-box held-out smoother (pgas_amd.ModelRollout.smooth) on SingleMassOscillator and
Vehicle at T = 2000, N = 200 particles: the pgas_m_smooth launch alone (from the traces of one filter call), the filter with traces, and
smooth() in all, for K in {1, 16, 64, 256} draws of B = 64 trajectories, and at K = 64 for B in {1, 4, 16, 64, 256} -- B = 1 and B = 4
cost the same (a wave each), so their time is what every row pays once (the interface variables, the transition program, the barriers)
and the slope from B = 4 upwards is the wave work per trajectory-row.  trajectory-rows/s = K B T / time.

Baseline, the only route there was before: one filter call with traces, then a host loop per draw, per trajectory and per row -- a
SymbolicStateSpaceModel.transition_logpdf launch against the next smoothed state (the interface variables of the draw's rows are formed
once per draw with hilbert_basis and a matmul, not once per trajectory, which favours it), a logsumexp, a cumsum and a draw on the host.
Timed for `--baseline-draws` draws x `--baseline-trajectories` trajectories and scaled to 64 x 64 (one filter call, whose time does not
depend on the number of draws, plus 64 x 64 trajectories).

At K = 64 and B in {4, 64} the instance of the kernel that reads nx at run time (PGAS_M_SMOOTH_RUNTIME_NX=1; what a model with nx >= 5
runs) is timed against the constant-nx instance, the two ALTERNATED call by call in the same process.

One warm-up call, then --calls calls with device events around every call; medians.

usage: model_smooth_time.py [--models smo,vehicle] [--steps 2000] [--particles 200] [--B 64] [--calls 20] [--baseline-draws 4]
                            [--baseline-trajectories 4] [--no-baseline] [--out FILE]"""
from __future__ import annotations

import argparse
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


def median(fn, calls, torch):
    fn()
    torch.cuda.synchronize()
    return float(np.median([one(fn, torch) for _ in range(calls)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="smo,vehicle")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--baseline-draws", type=int, default=4)
    ap.add_argument("--baseline-trajectories", type=int, default=4)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import pgas_amd
    from pgas_amd import experiments
    from pgas_amd._lib import MarginalOps

    T, N, B = args.steps, args.particles, args.B
    ops = MarginalOps(1)
    dev = ops.device
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/model_smooth_time.py --models {args.models} --steps {T} --particles {N} --B {B} --calls {args.calls}: {torch.cuda.get_device_name(dev)}, "
        "device events around every call, one warm-up call; medians")
    makes = {"smo": ("SMO", experiments.smo_marginal), "vehicle": ("Vehicle", experiments.vehicle_marginal)}
    for key in args.models.split(","):
        name, make = makes[key]
        pb = make(T=T)
        ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
        ssm.bind(ops)
        sim = pgas_amd.ModelRollout(pb.inputs, ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, ops=ops, observations=pb.observations)
        y = torch.as_tensor(np.asarray(pb.observations, dtype=np.float64).reshape(T, sim.ny), device=dev)
        u = torch.as_tensor(np.asarray(pb.inputs, dtype=np.float64).reshape(T, -1), device=dev)
        say(f"{name:8s} file {sim._filter_file_bytes()} B, dynamic LDS {sim.filter_lds_bytes(N)} B at N = {N}, max_particles() = {sim.max_particles()}")
        rng = np.random.default_rng(1)

        def params(K):
            A = []
            for g in pb.GP_prior:
                sd = np.diag(np.linalg.inv(np.asarray(g[1])))
                A.append(torch.as_tensor(0.1 * rng.standard_normal((K, 1, sd.size)) * sd, device=dev))
            return A, pgas_amd.chains.keys_tensor(list(range(1, K + 1)), dev)

        # ---- baseline: per draw, per trajectory and per row, dependent launches of existing pieces and a draw on the host
        ms_base = None
        if not args.no_baseline:
            Kb, Bb = args.baseline_draws, args.baseline_trajectories
            A, keys = params(Kb)
            ms_filter_b = median(lambda: sim.filter(A, keys, N, traces=True), args.calls, torch)
            tr = sim.filter(A, keys, N, traces=True)
            hrng = np.random.default_rng(2)

            def xi_of(k, x, ut):
                out = []
                for i, b in enumerate(pb.basis):
                    phi = ops.hilbert_basis(b.map, b.alpha(x, ut).reshape(-1, 1).contiguous(), None) if hasattr(b, "feature") else ops.hilbert_basis(b, x, ut)
                    out.append((phi @ A[i][k].T).contiguous())
                return out

            def baseline():
                out = []
                for k in range(Kb):
                    xi = [xi_of(k, tr.x[k, t].contiguous(), u[t]) for t in range(T)]   # once per draw
                    for _ in range(Bb):
                        xn, path = None, []
                        for t in range(T - 1, -1, -1):
                            v = tr.lw[k, t]
                            if xn is not None:
                                v = v + ssm.transition_logpdf(xn, tr.x[k, t].contiguous(), u[t], *xi[t])
                            cdf = torch.cumsum(torch.exp(v - torch.logsumexp(v, dim=0)), dim=0)
                            j = min(int(torch.searchsorted(cdf, hrng.uniform())), N - 1)   # the host-side draw
                            xn = tr.x[k, t, j]
                            path.append(j)
                        out.append(path)
                return out

            ms_traj = median(baseline, 1, torch) / (Kb * Bb)
            ms_base = ms_filter_b + 64 * 64 * ms_traj   # ONE filter call: its time does not depend on the number of draws (below)
            say(f"{name:8s} N={N} baseline (per row: transition_logpdf, logsumexp, cumsum, a draw on the host; xi once per draw), per trajectory of "
                f"{Kb} x {Bb}: {ms_traj:9.3f} ms = {ms_traj * 1e3 / T:7.1f} us per row; 64 draws x 64 trajectories with the filter: {ms_base:11.1f} ms")
            del tr

        def row(K, Bn, with_all):
            A, keys = params(K)
            sim.check_smooth(A, keys, N, Bn)
            flt = sim.filter(A, keys, N, traces=True)   # its operands stay in sim._keep for the launches below
            ms_s = median(lambda: sim._smooth_from(flt, K, N, 0, True, Bn, False, False, True), args.calls, torch)
            ms_n = median(lambda: sim._smooth_from(flt, K, N, 0, True, Bn, False, False, False), args.calls, torch)
            ms_x = median(lambda: sim._smooth_from(flt, K, N, 0, True, Bn, True, True, True), args.calls, torch)
            del flt
            txt = (f"{name:8s} N={N} K={K:4d} B={Bn:4d}: pgas_m_smooth {ms_s:9.3f} ms (interface=False {ms_n:9.3f} ms, with xs, xis and idx {ms_x:9.3f} ms) = "
                   f"{K * Bn * T / (ms_s * 1e-3):.3e} trajectory-rows/s, {ms_s * 1e3 / T:7.2f} us per row")
            if K == 64 and Bn in (4, 64):   # constant nx against run-time nx, alternated call by call
                fn = lambda: sim._smooth_from(flt2, K, N, 0, True, Bn, False, False, True)  # noqa: E731
                flt2 = sim.filter(A, keys, N, traces=True)
                ms = {"0": [], "1": []}
                for v in ("0", "1"):
                    os.environ["PGAS_M_SMOOTH_RUNTIME_NX"] = v
                    fn()
                torch.cuda.synchronize()
                for _ in range(args.calls):
                    for v in ("0", "1"):
                        os.environ["PGAS_M_SMOOTH_RUNTIME_NX"] = v
                        ms[v].append(one(fn, torch))
                os.environ.pop("PGAS_M_SMOOTH_RUNTIME_NX")
                del flt2
                c, r = float(np.median(ms["0"])), float(np.median(ms["1"]))
                txt += (f"; alternated: constant nx {c:9.3f} ms (min {min(ms['0']):9.3f}, max {max(ms['0']):9.3f}), run-time nx {r:9.3f} ms "
                        f"(min {min(ms['1']):9.3f}, max {max(ms['1']):9.3f})")
            if with_all:
                ms_f = median(lambda: sim.filter(A, keys, N, traces=True), args.calls, torch)
                ms_all = median(lambda: sim.smooth(A, keys, N, Bn), args.calls, torch)
                txt += f"; filter with moments and traces {ms_f:9.3f} ms; smooth() in all {ms_all:9.3f} ms"
                if K == 64 and Bn == 64 and ms_base is not None:
                    txt += f"; baseline {ms_base:11.1f} ms ({ms_base / ms_all:8.1f}x)"
            say(txt)

        for K in (1, 16, 64, 256):
            row(K, B, True)
        for Bn in (1, 4, 16, 64, 256):
            if Bn != B:
                row(64, Bn, False)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
