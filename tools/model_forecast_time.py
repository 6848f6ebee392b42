#!/usr/bin/env python3
"""Device-event timing of the grey-box h-step-ahead forecast (pgas_amd.ModelRollout.forecast) on SingleMassOscillator
and Vehicle at T = 2000, N = 200 particles, H = 16 horizons: K in {1, 16, 64, 256} draws -- the filter call with traces, pgas_m_forecast
alone with and without the log score, and forecast() in all.  particle-steps/s of pgas_m_forecast = K N sum_s (min(H, T - s) - 1) / time.
One warm-up call, then --calls calls with device events around each; medians.

Baseline, the only route there was before: one filter call with traces, then per origin row s a fresh ModelRollout over rows s .. s + H - 1
of the record and one predict call from the trace row (init_state = trace row, replicates = N, log score on).  Timed on the host clock
(the construction traces the model on the host) for `--baseline-origins` origins spread over the record at K = 64 and scaled to T origins.

--tb 1,2,4,8,16: also times pgas_m_forecast with that many origin rows per workgroup (PGAS_M_FORECAST_TB) at K = 1 and K = 64.

usage: model_forecast_time.py [--models smo,vehicle] [--steps 2000] [--particles 200] [--horizon 16] [--calls 20] [--draws 1,16,64,256]
                              [--baseline-origins 8] [--tb LIST] [--out FILE]"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def median_ms(fn, calls, torch):
    """Median ms of `calls` calls of fn after one warm-up call, device events around every call."""
    out = fn()
    torch.cuda.synchronize()
    del out
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        del out
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="smo,vehicle")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--draws", default="1,16,64,256")
    ap.add_argument("--baseline-origins", type=int, default=8)
    ap.add_argument("--tb", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import pgas_amd
    from pgas_amd import experiments
    from pgas_amd._lib import MarginalOps

    T, N, H = args.steps, args.particles, args.horizon
    steps = sum(min(H, T - s) - 1 for s in range(T))   # propagations per particle and draw
    ops = MarginalOps(1)
    dev = ops.device
    lib = ops.eng.lib
    tb0 = int(lib.pgas_m_forecast_origins_per_block())
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/model_forecast_time.py --models {args.models} --steps {T} --particles {N} --horizon {H} --calls {args.calls}: "
        f"{torch.cuda.get_device_name(dev)}, device events, one warm-up call; medians")
    makes = {"smo": ("SMO", experiments.smo_marginal), "vehicle": ("Vehicle", experiments.vehicle_marginal)}
    for key in args.models.split(","):
        name, make = makes[key]
        pb = make(T=T)
        ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
        sim = pgas_amd.ModelRollout(pb.inputs, ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, ops=ops, observations=pb.observations)
        say(f"{name:8s} file {sim._filter_file_bytes()} B, dynamic LDS {sim.filter_lds_bytes(N)} B at N = {N}")
        rng = np.random.default_rng(1)

        def draws(K):
            A = []
            for g in pb.GP_prior:
                sd = np.diag(np.linalg.inv(np.asarray(g[1])))
                A.append(torch.as_tensor(0.1 * rng.standard_normal((K, 1, sd.size)) * sd, device=dev))
            return A, pgas_amd.chains.keys_tensor(list(range(1, K + 1)), dev)

        def launches(A, keys, K, score):
            """-> (the filter's result, a callable that runs pgas_m_forecast alone from it)."""
            flt = sim.filter(A, keys, N, traces=True)
            _, _, mode, noisy_state, _, _ = sim.check_forecast(A, keys, N, H)
            return flt, lambda: sim._forecast_from(flt, K, N, mode, noisy_state, H, score, False)

        # ---- baseline at K = 64: a ModelRollout and a predict call per origin row
        Kb = 64
        A, keys = draws(Kb)
        ms_filter_b = median_ms(lambda: sim.filter(A, keys, N, traces=True), args.calls, torch)
        trace = sim.filter(A, keys, N, traces=True).x
        obs = np.asarray(pb.observations, dtype=np.float64).reshape(T, -1)
        inp = np.asarray(pb.inputs, dtype=np.float64).reshape(T, -1)
        origins = [int(s) for s in np.linspace(0, T - H, args.baseline_origins)]

        def baseline():
            out = []
            for s in origins:
                sub = pgas_amd.ModelRollout(inp[s:s + H], ssm, pb.basis, ops=ops, observations=obs[s:s + H])
                out.append(sub.predict(A, keys, replicates=N, init_state=trace[:, s].contiguous(), log_score=True))
            torch.cuda.synchronize()
            return out

        baseline()   # warm-up
        t0 = time.perf_counter()
        baseline()
        ms_origin = (time.perf_counter() - t0) * 1e3 / len(origins)
        ms_base = ms_filter_b + T * ms_origin
        say(f"{name:8s} N={N} H={H} baseline K={Kb}: filter with traces {ms_filter_b:9.3f} ms + {T} origins x {ms_origin:8.3f} ms "
            f"(a ModelRollout and one predict call each, host clock, mean of {len(origins)}) = {ms_base:11.1f} ms")
        del trace

        for K in [int(k) for k in args.draws.split(",")]:
            A, keys = draws(K)
            ms_f = median_ms(lambda: sim.filter(A, keys, N, traces=True), args.calls, torch)
            flt, run = launches(A, keys, K, True)
            ms_c = median_ms(run, args.calls, torch)
            flt, run = launches(A, keys, K, False)
            ms_m = median_ms(run, args.calls, torch)
            del flt, run
            ms_all = median_ms(lambda: sim.forecast(A, keys, N, H), args.calls, torch)
            say(f"{name:8s} N={N} H={H} TB={tb0} K={K:4d}: filter with traces {ms_f:9.3f} ms, pgas_m_forecast {ms_c:9.3f} ms "
                f"(moments only {ms_m:9.3f} ms) = {K * N * steps / (ms_c * 1e-3):.3e} particle-steps/s; forecast() in all {ms_all:9.3f} ms"
                + (f"; baseline {ms_base:11.1f} ms ({ms_base / ms_all:8.1f}x)" if K == Kb else ""))
        for tb in [int(v) for v in args.tb.split(",") if v]:
            os.environ["PGAS_M_FORECAST_TB"] = str(tb)
            for K in (1, 64):
                A, keys = draws(K)
                flt, run = launches(A, keys, K, True)
                ms_c = median_ms(run, args.calls, torch)
                say(f"{name:8s} N={N} H={H} TB={int(lib.pgas_m_forecast_origins_per_block()):3d} K={K:4d}: pgas_m_forecast {ms_c:9.3f} ms")
                del flt, run
            del os.environ["PGAS_M_FORECAST_TB"]
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
