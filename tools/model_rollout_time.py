#!/usr/bin/env python3
"""Time pgas_amd.ModelRollout (one launch) against the per-step loop of the primitives it fuses.

    python tools/model_rollout_time.py [--steps 2000] [--calls 20] [--out profiles/model_rollout_time.txt]

Models: SMO (2-D basis, M = 41) and Vehicle (two latent functions with traced features, the longest program).  Configurations:
K in {1, 16, 64, 600} draws at P = 1 replicate, and K = 64 at P in {64, 256}.  Device events around every call, one warm-up call and
`--calls` timed calls; the table reports the median with the minimum, microseconds per step and particle-steps per second.

fused        ModelRollout, noise-free, x_0 given per replicate;  fused+noise: the same call with process noise and keys.
loop         the per-step loop over a particle axis of K P: per latent function one basis launch (for the Vehicle one expr_eval of the
             traced slip angle in front of it), one batched matmul, then one expr_eval of the transition -- noise-free, on preallocated
             coefficient tensors.  This is what the primitives allowed before the fused kernel.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, calls, torch):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import pgas_amd
    from pgas_amd import experiments, exprs
    from pgas_amd._lib import MarginalOps

    T = args.steps
    ops = MarginalOps(1)
    dev = ops.device
    lines = [f"# pgas_amd.ModelRollout against the per-step loop of its primitives; T = {T} steps, {args.calls} timed calls after one warm-up, "
             f"device events; {torch.cuda.get_device_name(dev)}",
             f"{'model':8s} {'K':>4s} {'P':>4s} {'what':12s} {'median ms':>10s} {'min ms':>9s} {'us/step':>9s} {'particle-steps/s':>17s} {'loop/fused':>10s}"]
    for name, make in (("SMO", experiments.smo_marginal), ("Vehicle", experiments.vehicle_marginal)):
        pb = make(T=T)
        ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
        ssm.bind(ops)
        sim = pgas_amd.ModelRollout(pb.inputs, ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, ops=ops)
        U = torch.as_tensor(np.asarray(pb.inputs, dtype=np.float64).reshape(T, -1), device=dev)
        feats = [exprs.trace(lambda st, u, b=b: b.feature(exprs.SymNamespace(st.tr))(st, u), sim.nx, sim.nu, ()) if hasattr(b, "feature") else None
                 for b in pb.basis]
        maps = [b.map if hasattr(b, "feature") else b for b in pb.basis]
        rng = np.random.default_rng(1)
        for K, P in ((1, 1), (16, 1), (64, 1), (600, 1), (64, 64), (64, 256)):
            A = []
            for g in pb.GP_prior:
                sd = np.diag(np.linalg.inv(np.asarray(g[1])))
                A.append(torch.as_tensor(0.1 * rng.standard_normal((K, 1, sd.size)) * sd, device=dev))
            x0 = torch.as_tensor(np.asarray(pb.init_state_mean) + 0.01 * rng.standard_normal((K, P, sim.nx)), device=dev)
            keys = pgas_amd.chains.keys_tensor(list(range(1, K + 1)), dev)
            At = [a.transpose(1, 2).contiguous() for a in A]   # (K, M, 1) for the batched product

            def fused():
                return sim(A, None, replicates=P, init_state=x0, process_noise=False)

            def fused_noise():
                return sim(A, keys, replicates=P, init_state=x0)

            def loop():
                x = x0.reshape(K * P, sim.nx)
                for t in range(T - 1):
                    u = U[t]
                    xi = []
                    for i, bm in enumerate(maps):
                        if feats[i] is None:
                            phi = ops.hilbert_basis(bm, x, u)
                        else:
                            phi = ops.hilbert_basis(bm, ops.expr_eval(feats[i], x, u, []), None)
                        xi.append(torch.bmm(phi.view(K, P, -1), At[i]).view(K * P, 1))
                    x = ops.expr_eval(ssm._program(0, x, u, xi), x, u, xi)
                return x

            ref = loop()
            got = fused()[:, -1].reshape(K * P, sim.nx)
            err = float((got - ref).abs().max())   # free-running, so only a sanity figure: both simulate the same system
            res = {}
            for what, fn in (("fused", fused), ("fused+noise", fused_noise), ("loop", loop)):
                res[what] = timed(fn, args.calls, torch)
            for what in ("fused", "fused+noise", "loop"):
                med, mn = res[what]
                ratio = f"{res['loop'][0] / res['fused'][0]:10.1f}" if what == "fused" else f"{'':10s}"
                lines.append(f"{name:8s} {K:4d} {P:4d} {what:12s} {med:10.3f} {mn:9.3f} {1e3 * med / T:9.3f} {K * P * T / (med * 1e-3):17.3e} {ratio}")
            lines.append(f"# {name} K={K} P={P}: max |fused - loop| at the last step = {err:.2e}")
            print("\n".join(lines[-4:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
