#!/usr/bin/env python3
"""Census of the resampling search's sources in the bench's regime, from the canonical C oracle alone (CPU, no GPU; development aid).
usage: tools/ns_census.py [--particles N] [--T T] [--steps K] [--first F] [--seed S]
Runs the first K steps of the SingleMassOscillator sweep at N particles with (A, S) = experiments.initial_params of the T-step problem
(what bench.py sweeps) and prints, for every step from F on, what k_step's search of that step meets:
  distinct   share of the N ancestors that are distinct particles
  ns median  source segments (of 1024 particles) a workgroup's 1024 ancestors come from: median and maximum over the workgroups
  ns > 8     workgroups with more source segments than PG_NCAND = 8, the ones that leave the staged search for the per-slot path
The ancestors of the conditioned particle (the last one) come from another draw and are left out."""
import argparse
import os
import sys

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(root, "tests"))
from common import canon_model, experiments  # noqa: E402

SEG, NCAND = 1024, 8
ap = argparse.ArgumentParser()
ap.add_argument("--particles", type=int, default=1 << 20)
ap.add_argument("--T", type=int, default=2000)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--first", type=int, default=16)
ap.add_argument("--seed", type=int, default=12345678)
a = ap.parse_args()
N = a.particles
pb = experiments.smo_pgas(T=a.T)
A, S = experiments.initial_params(pb)
cm = canon_model(pb, N)
LS, LSinv, cS = cm.chol_parts(S)
x = cm.init_state(a.seed, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), pb.X_true[0])
lw = None
nwg = (N + SEG - 1) // SEG
print(f"N = {N}, {nwg} workgroups, T = {a.T}, seed {a.seed}")
print("step  distinct %  ns median  ns max  workgroups with ns > 8")
over = 0
for t in range(1, a.steps):
    lw, x, anc = cm.step(t, a.seed, x, lw, A, LS, LSinv, cS, pb.X_true[t])[:3]
    if t < a.first:
        continue
    src = np.asarray(anc[: N - 1]) // SEG
    ns = np.array([len(np.unique(src[w * SEG:(w + 1) * SEG])) for w in range(nwg)])
    over += int((ns > NCAND).sum() > 0)
    print(f"{t:4d}  {100.0 * len(np.unique(anc[: N - 1])) / (N - 1):9.2f}  {int(np.median(ns)):9d}  {int(ns.max()):6d}  {int((ns > NCAND).sum()):6d}", flush=True)
print(f"steps with a workgroup above {NCAND} source segments: {over} of {a.steps - max(a.first, 1)}")
