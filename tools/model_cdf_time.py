#!/usr/bin/env python3
"""Device-event timing of the grey-box in-kernel predictive CDF counts (pgas_amd.ModelRollout.cdf and ModelRollout.forecast_cdf, DESIGN.md
section 20) on SingleMassOscillator and Vehicle at T = 2000.

Part A, per (K, P) in {(64, 256), (600, 1024)} and J in {1, 16}, with observation noise:

  cdf          the counts in one call (k_model_rollout_cdf), output K T (nx + ny) J int32
  predict      ModelRollout.predict on the same draws (moments only, observation noise): it shares the propagation, so the difference is
               the price of counting against the moments
  yardstick    the only route to the same counts before: ModelRollout.__call__(outputs=True) (both clouds), then torch observation noise
               (randn @ LR^T) and (v[..., None] <= thr).sum over the replicates, in chunks of --chunk draws so that the clouds and the
               boolean (chunk, T, P, nx + ny, J) tensor fit

Part B, N = 200 particles, H = 16 horizons, K = 64, J in {1, 16}: pgas_m_forecast_cdf from a stored trace against pgas_m_forecast (moments
and log score; moments only) from the same trace; forecast_cdf() against forecast() with the filter included; and the only route before,
forecast(clouds=True) followed by the compare (no observation noise in it: ModelRollout.forecast has none), at --cloud-draws draws because
its clouds are K H T N (nx + ny) doubles.

One warm-up call and --reps timed calls each.

usage: model_cdf_time.py [--models smo,vehicle] [--T 2000] [--reps 20] [--chunk 25] [--cloud-draws 8] [--parts A,B] [--points 64x256,600x1024]
                         [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pgas_amd  # noqa: E402
from pgas_amd import experiments  # noqa: E402
from pgas_amd._lib import MarginalOps  # noqa: E402


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
    ap.add_argument("--models", default="smo,vehicle")
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=25)
    ap.add_argument("--cloud-draws", type=int, default=8)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--parts", default="A,B")
    ap.add_argument("--points", default="64x256,600x1024")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    ops = MarginalOps(1)
    dev = ops.device
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept up to date: a run that is cut short leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"# tools/model_cdf_time.py --models {a.models} --T {T} --reps {a.reps} --chunk {a.chunk} --cloud-draws {a.cloud_draws} --parts {a.parts} "
        f"--points {a.points}: {torch.cuda.get_device_name(dev)}, device events, one warm-up call")
    makes = {"smo": ("SMO", experiments.smo_marginal), "vehicle": ("Vehicle", experiments.vehicle_marginal)}
    for key in a.models.split(","):
        name, make = makes[key]
        pb = make(T=T)
        ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
        sim = pgas_amd.ModelRollout(pb.inputs, ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, ops=ops, observations=pb.observations)
        nx, ny = sim.nx, sim.ny
        LRt = torch.as_tensor(np.linalg.cholesky(np.atleast_2d(ssm.output_noise)), device=dev).T.contiguous()
        rng = np.random.default_rng(1)

        def draws(K):
            A = []
            for g in pb.GP_prior:
                sd = np.diag(np.linalg.inv(np.asarray(g[1])))
                A.append(torch.as_tensor(0.1 * rng.standard_normal((K, 1, sd.size)) * sd, device=dev))
            return A, pgas_amd.chains.keys_tensor(list(range(1, K + 1)), dev)

        # ---- Part A
        for K, P in [tuple(int(v) for v in p.split("x")) for p in a.points.split(",")] if "A" in a.parts else []:
            A, kd = draws(K)
            st = sim.predict(A, kd, replicates=P, observation_noise=True, log_score=False)
            summ = pgas_amd.predictive_summary(st)
            mean = torch.cat([summ["x_mean_pooled"], summ["y_mean_pooled"]], dim=1)
            std = torch.cat([summ["x_std_pooled"], summ["y_std_pooled"]], dim=1)
            ms_p = timed(lambda: sim.predict(A, kd, replicates=P, observation_noise=True, log_score=False), a.reps)
            for J in (1, 16):
                thr = pgas_amd.threshold_grid(mean, std, J, width=2.0 if J > 1 else 0.0).contiguous()
                kc = min(K, a.chunk)

                def yardstick():
                    out = torch.empty((K, T, nx + ny, J), dtype=torch.int32, device=dev)
                    for lo in range(0, K, kc):
                        x, g = sim([m[lo:lo + kc] for m in A], kd[lo:lo + kc], replicates=P, outputs=True)
                        v = torch.cat([x, g + torch.randn(g.shape, dtype=torch.float64, device=dev) @ LRt], dim=-1)
                        del x, g
                        for c in range(nx + ny):   # a channel at a time: the boolean tensor is (chunk, T, P, J)
                            out[lo:lo + kc, :, c] = (v[..., c, None] <= thr[None, :, None, c]).sum(dim=2, dtype=torch.int32)
                    return out

                ms_c = timed(lambda: sim.cdf(A, kd, replicates=P, thresholds=thr, observation_noise=True), a.reps)
                ms_y = timed(yardstick, max(1, a.reps // 4))
                say(f"{name:8s} K={K:4d} P={P:5d} J={J:2d}: cdf {ms_c:9.3f} ms, predict (moments, noise) {ms_p:9.3f} ms (cdf / predict {ms_c / ms_p:5.2f}), "
                    f"yardstick {ms_y:9.3f} ms in chunks of {kc} draws, {max(1, a.reps // 4)} calls ({ms_y / ms_c:6.2f}x); "
                    f"output {K * T * (nx + ny) * J * 4 / 1e6:.3f} MB, {K * T * (nx + ny) * J * ((P + 63) // 64) / 1e6:.1f} M atomic adds, "
                    f"against clouds of {K * T * P * (nx + ny) * 8 / 1e6:.1f} MB")
                torch.cuda.empty_cache()
            del A

        # ---- Part B
        if "B" in a.parts:
            K, N, H = 64, a.N, a.H
            A, kd = draws(K)
            from pgas_amd._lib import ModelForecastCdfDesc

            res = sim.forecast(A, kd, N, H)
            fs = pgas_amd.forecast_summary(res)
            mean = torch.cat([fs["x_pred_mean"][0], fs["y_pred_mean"][0]], dim=1)
            std = torch.cat([fs["x_pred_std"][0], fs["y_pred_std"][0]], dim=1) + float(np.sqrt(np.trace(np.atleast_2d(ssm.output_noise))))
            flt = sim.filter(A, kd, N, traces=True)
            _, _, mode, noisy_state, _, _ = sim.check_forecast(A, kd, N, H)
            ms_f = timed(lambda: sim._forecast_from(flt, K, N, mode, noisy_state, H, True, False), a.reps)
            ms_fm = timed(lambda: sim._forecast_from(flt, K, N, mode, noisy_state, H, False, False), a.reps)
            ms_all_f = timed(lambda: sim.forecast(A, kd, N, H), a.reps)
            Kc = min(K, a.cloud_draws)
            Ac, kc_ = [m[:Kc].contiguous() for m in A], kd[:Kc].contiguous()
            for J in (1, 16):
                thr = pgas_amd.threshold_grid(mean, std, J, width=2.0 if J > 1 else 0.0).contiguous()
                count = torch.empty((K, H, T, nx + ny, J), dtype=torch.int32, device=dev)
                fc = ModelForecastCdfDesc()
                fc.x_dev, fc.thr_dev, fc.count_dev, fc.H, fc.J, fc.noise = flt.x.data_ptr(), thr.data_ptr(), count.data_ptr(), H, J, 1
                sim._LR(fc)
                sim.filter(A, kd, N, traces=True)   # sim._keep: the operands of the descriptor
                Ak, rows, seeds, x0 = sim._keep
                d = sim._desc(K, N, 0, mode, Ak, rows, seeds, x0, noisy_state, None, None)
                ms_c = timed(lambda: ops.model_forecast_cdf(d, fc), a.reps)
                ms_all_c = timed(lambda: sim.forecast_cdf(A, kd, N, H, thresholds=thr), a.reps)

                def clouds_route():
                    r = sim.forecast(Ac, kc_, N, H, log_score=False, clouds=True)
                    out = torch.empty((Kc, H, T, nx + ny, J), dtype=torch.int32, device=dev)
                    for c in range(nx + ny):
                        v = r.cloud_x[..., c] if c < nx else r.cloud_y[..., c - nx]
                        out[..., c, :] = (v[..., None] <= thr[None, None, :, None, c]).sum(dim=3, dtype=torch.int32)
                    return out

                ms_cl = timed(clouds_route, max(1, a.reps // 4))
                say(f"{name:8s} K={K:4d} N={N} H={H} J={J:2d}: pgas_m_forecast_cdf {ms_c:9.3f} ms, pgas_m_forecast {ms_f:9.3f} ms (moments only {ms_fm:9.3f} ms; "
                    f"cdf / forecast {ms_c / ms_f:5.2f}); forecast_cdf() in all {ms_all_c:9.3f} ms, forecast() in all {ms_all_f:9.3f} ms; "
                    f"forecast(clouds=True) + compare at K={Kc}: {ms_cl:9.3f} ms = {ms_cl / Kc:8.3f} ms/draw against {ms_all_c / K:8.3f} ms/draw, "
                    f"{max(1, a.reps // 4)} calls, without observation noise; output {K * H * T * (nx + ny) * J * 4 / 1e6:.1f} MB")
                del count
                torch.cuda.empty_cache()
            del flt, res, A
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
