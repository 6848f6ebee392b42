"""Device-event timing of the h-step-ahead forecast (pgas_amd.HeldOutFilter.forecast) on SingleMassOscillator
(M = 41) and EMPS-729 at T = 2000, N = 200 particles, H = 16 horizons: K in {1, 16, 64, 256} draws, the filter call with traces and the
pgas_forecast call timed separately.  particle-steps/s of pgas_forecast = K N sum_s (min(H, T - s) - 1) / time, next to the rate of
rollout_stats (K draws, P = N replicates, the whole record, log score on) on the same context.

Baseline, the only route there was before: one filter call with traces, then per origin row s a fresh context over rows s .. s + H - 1 of
the record and one rollout_stats call from the trace row (x0_mode 3, P = N, log score on).  Timed on the host clock (a context creation
synchronises) for `--baseline-origins` origins spread over the record at K = 64 and scaled to T origins.

--tb 4,8,16: also times pgas_forecast with that many origin rows per workgroup (PGAS_FORECAST_TB) at K = 1 and K = 64.

usage: forecast_time.py [--models smo,emps] [--T 2000] [--N 200] [--H 16] [--reps 20] [--baseline-origins 8] [--tb LIST] [--out FILE]"""
import argparse
import os
import sys
import time

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
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-origins", type=int, default=8)
    ap.add_argument("--tb", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T, N, H = a.T, a.N, a.H
    steps = sum(min(H, T - s) - 1 for s in range(T))   # propagations per particle and draw
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/forecast_time.py --models {a.models} --T {T} --N {N} --H {H} --reps {a.reps}: {torch.cuda.get_device_name(0)}, device events, one warm-up call")
    for name in a.models.split(","):
        pb = experiments.smo_pgas(T=T) if name == "smo" else experiments.emps_pgas(T=T)
        A, S = experiments.initial_params(pb)
        lik = pb.likelihood_fcn
        flt = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, lik, pb.nx, N, pb.init_state_mean, pb.init_state_cov)
        eng = flt.engine
        dev, M = eng.device, eng.M
        tb0 = int(eng.lib.pgas_forecast_origins_per_block())

        def params(K):
            As = torch.as_tensor(np.stack([A * (1.0 + 1e-4 * k) for k in range(K)]), device=dev)
            Ss = torch.as_tensor(np.stack([S * (1.0 + 1e-3 * k) for k in range(K)]), device=dev)
            return As, Ss, ch.keys_tensor(prng.split(prng.key(12345678), K), dev)

        # ---- baseline at K = 64: a context and a rollout_stats call per origin row
        Kb = 64
        As, Ss, kd = params(Kb)
        ms_filter64 = timed(lambda: flt(As, Ss, kd, traces=True), a.reps)
        trace = flt(As, Ss, kd, traces=True).x
        obs = np.asarray(pb.observations, dtype=np.float64).reshape(T, -1)
        inp = np.asarray(pb.inputs, dtype=np.float64).reshape(T, -1)
        origins = [int(s) for s in np.linspace(0, T - H, a.baseline_origins)]

        def baseline():
            out = []
            for s in origins:
                e = Engine(N, obs[s:s + H], inp[s:s + H], pb.init_state_mean, pb.init_state_cov, lik, pb.basis_fcn)
                out.append(e.rollout_stats(As, Ss, kd, replicates=N, x0=trace[:, s].contiguous(), x0_mode=3, log_score=True))
            torch.cuda.synchronize()
            return out

        baseline()   # warm-up
        t0 = time.perf_counter()
        baseline()
        ms_origin = (time.perf_counter() - t0) * 1e3 / len(origins)
        ms_base = ms_filter64 + T * ms_origin
        say(f"{name:5s} M={M:4d} N={N} H={H} baseline K={Kb}: filter with traces {ms_filter64:9.3f} ms + {T} origins x {ms_origin:8.3f} ms "
            f"(a context and one rollout_stats call each, host clock, mean of {len(origins)}) = {ms_base:11.1f} ms")
        del trace

        for K in (1, 16, 64, 256):
            As, Ss, kd = params(K)
            ms_f = timed(lambda: flt(As, Ss, kd, traces=True), a.reps)
            x = flt(As, Ss, kd, traces=True).x
            ms_c = timed(lambda: eng.forecast(As, Ss, kd, x, H, True), a.reps)
            ms_m = timed(lambda: eng.forecast(As, Ss, kd, x, H, False), a.reps)
            del x
            ms_all = timed(lambda: flt.forecast(As, Ss, kd, H), a.reps)
            ms_rs = timed(lambda: eng.rollout_stats(As, Ss, kd, replicates=N, log_score=True), a.reps)
            say(f"{name:5s} M={M:4d} N={N} H={H} TB={tb0} K={K:4d}: filter with traces {ms_f:9.3f} ms, pgas_forecast {ms_c:9.3f} ms "
                f"(moments only {ms_m:9.3f} ms) = {K * N * steps / (ms_c * 1e-3):.3e} particle-steps/s; forecast() in all {ms_all:9.3f} ms; "
                f"rollout_stats K={K} P={N} {ms_rs:9.3f} ms = {K * N * (T - 1) / (ms_rs * 1e-3):.3e} particle-steps/s"
                + (f"; baseline {ms_base:11.1f} ms ({ms_base / ms_all:8.1f}x)" if K == Kb else ""))
        for tb in [int(v) for v in a.tb.split(",") if v]:
            os.environ["PGAS_FORECAST_TB"] = str(tb)
            for K in (1, 64):
                As, Ss, kd = params(K)
                x = flt(As, Ss, kd, traces=True).x
                ms_c = timed(lambda: eng.forecast(As, Ss, kd, x, H, True), a.reps)
                say(f"{name:5s} M={M:4d} N={N} H={H} TB={int(eng.lib.pgas_forecast_origins_per_block()):3d} K={K:4d}: pgas_forecast {ms_c:9.3f} ms")
                del x
            del os.environ["PGAS_FORECAST_TB"]
        del flt, eng
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
