"""Device-event timing of the in-kernel predictive CDF counts (pgas_amd.Rollout.cdf and pgas_amd.HeldOutFilter.forecast_cdf, DESIGN.md
section 19) on SingleMassOscillator (M = 41) and EMPS-729 at T = 2000.

Part A, per (K, P) in {(64, 256), (600, 1024)} and J in {1, 16}, with observation noise:

  cdf          the counts in one call (k_rollout_cdf), output K T (nx + ny) J int32
  predict      Rollout.predict on the same draws (moments only, observation noise): it shares the propagation, so the difference is the
               price of counting against the moments
  yardstick    the only route to the same counts before: Rollout.__call__ (the (K, T, P, nx) cloud), then torch measurement noise
               (randn @ LR^T) and (v[..., None] <= thr).sum over the replicates, in chunks of --chunk draws so that the boolean
               (chunk, T, P, nx + ny, J) tensor fits

Part B, N = 200 particles, H = 16 horizons, K = 64, J in {1, 16}: pgas_forecast_cdf from a stored trace against pgas_forecast (moments and
log score) from the same trace, and forecast_cdf() against forecast() with the filter included.  There was no route to these counts
before: the forecast returns no cloud.

One warm-up call and --reps timed calls each.

usage: cdf_time.py [--models smo,emps] [--T 2000] [--reps 20] [--chunk 50] [--out FILE]"""
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
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/cdf_time.py --models {a.models} --T {T} --reps {a.reps} --chunk {a.chunk}: {torch.cuda.get_device_name(0)}, device events, one warm-up call")
    for name in a.models.split(","):
        pb = experiments.smo_pgas(T=T) if name == "smo" else experiments.emps_pgas(T=T)
        A, S = experiments.initial_params(pb)
        lik = pb.likelihood_fcn
        sim = pgas_amd.Rollout(pb.inputs, pb.basis_fcn, pb.nx, pb.init_state_mean, pb.init_state_cov, likelihood_fcn=lik, observations=pb.observations)
        dev = sim.engine.device
        M, nx, ny = sim.engine.M, sim.engine.nx, sim.engine.ny
        Ht = torch.as_tensor(lik.H, device=dev).T.contiguous()
        LRt = torch.as_tensor(np.atleast_2d(lik.LR), device=dev).T.contiguous()

        def params(K):
            As = torch.as_tensor(np.stack([A * (1.0 + 1e-4 * k) for k in range(K)]), device=dev)
            Ss = torch.as_tensor(np.stack([S * (1.0 + 1e-3 * k) for k in range(K)]), device=dev)
            return As, Ss, ch.keys_tensor(prng.split(prng.key(12345678), K), dev)

        # ---- Part A
        for K, P in ((64, 256), (600, 1024)):
            As, Ss, kd = params(K)
            st = sim.predict(As, Ss, kd, replicates=P, observation_noise=True, log_score=False)
            summ = pgas_amd.predictive_summary(st)
            mean = torch.cat([summ["x_mean_pooled"], summ["y_mean_pooled"]], dim=1)
            std = torch.cat([summ["x_std_pooled"], summ["y_std_pooled"]], dim=1)
            ms_p = timed(lambda: sim.predict(As, Ss, kd, replicates=P, observation_noise=True, log_score=False), a.reps)
            for J in (1, 16):
                thr = pgas_amd.threshold_grid(mean, std, J, width=2.0 if J > 1 else 0.0).contiguous()
                kc = min(K, a.chunk)

                def yardstick():
                    out = torch.empty((K, T, nx + ny, J), dtype=torch.int32, device=dev)
                    for lo in range(0, K, kc):
                        x = sim(As[lo:lo + kc], Ss[lo:lo + kc], kd[lo:lo + kc], replicates=P)
                        yh = x @ Ht + torch.randn(x.shape[:3] + (ny,), dtype=torch.float64, device=dev) @ LRt
                        v = torch.cat([x, yh], dim=-1)
                        out[lo:lo + kc] = (v[..., None] <= thr[None, :, None]).sum(dim=2, dtype=torch.int32)
                    return out

                ms_c = timed(lambda: sim.cdf(As, Ss, kd, replicates=P, thresholds=thr, observation_noise=True), a.reps)
                ms_y = timed(yardstick, a.reps)
                say(f"{name:5s} M={M:4d} K={K:4d} P={P:5d} J={J:2d}: cdf {ms_c:9.3f} ms, predict (moments, noise) {ms_p:9.3f} ms (cdf / predict {ms_c / ms_p:5.2f}), "
                    f"yardstick {ms_y:9.3f} ms in chunks of {kc} draws ({ms_y / ms_c:6.2f}x); output {K * T * (nx + ny) * J * 4 / 1e6:.3f} MB "
                    f"against a cloud of {K * T * P * nx * 8 / 1e6:.1f} MB")
                torch.cuda.empty_cache()
        del sim
        torch.cuda.empty_cache()

        # ---- Part B
        K, N, H = 64, a.N, a.H
        flt = pgas_amd.HeldOutFilter(pb.observations, pb.inputs, pb.basis_fcn, lik, pb.nx, N, pb.init_state_mean, pb.init_state_cov)
        eng = flt.engine
        As, Ss, kd = params(K)
        res = flt.forecast(As, Ss, kd, H)
        x = res.filter.x
        fs = pgas_amd.forecast_summary(res)
        mean = torch.cat([fs["x_pred_mean"][0], fs["y_pred_mean"][0]], dim=1)
        std = torch.cat([fs["x_pred_std"][0], fs["y_pred_std"][0]], dim=1) + float(np.sqrt(np.trace(np.atleast_2d(lik.R))))
        ms_f = timed(lambda: eng.forecast(As, Ss, kd, x, H, True), a.reps)
        ms_fm = timed(lambda: eng.forecast(As, Ss, kd, x, H, False), a.reps)
        ms_all_f = timed(lambda: flt.forecast(As, Ss, kd, H), a.reps)
        for J in (1, 16):
            thr = pgas_amd.threshold_grid(mean, std, J, width=2.0 if J > 1 else 0.0).contiguous()
            ms_c = timed(lambda: eng.forecast_cdf(As, Ss, kd, x, H, thr, True), a.reps)
            ms_all_c = timed(lambda: flt.forecast_cdf(As, Ss, kd, H, thresholds=thr), a.reps)
            say(f"{name:5s} M={M:4d} K={K:4d} N={N} H={H} J={J:2d}: pgas_forecast_cdf {ms_c:9.3f} ms, pgas_forecast {ms_f:9.3f} ms (moments only {ms_fm:9.3f} ms; "
                f"cdf / forecast {ms_c / ms_f:5.2f}); forecast_cdf() in all {ms_all_c:9.3f} ms, forecast() in all {ms_all_f:9.3f} ms; "
                f"output {K * H * T * (nx + ny) * J * 4 / 1e6:.1f} MB; no route to these counts before")
        del flt, eng, x, res
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
