"""Device-event timing of one Gibbs iteration over E records that share one model: MultiRecordPGAS.step (keys,
seeds, one sweep launch of E x C workgroups, seam-aware statistics, MNIW algebra, draws) against the same E records taken one after
another through E single-record MultiChainPGAS contexts on the same build (E sweeps, E sets of statistics; what a user could do
before, and no shared posterior).  SingleMassOscillator-PGAS, N = 200, records of 500 rows, E in {1, 4, 16}, C in {1, 16}.  At E = 1
the two are the same launches but for the seed kernel and the seam flag: the expectation is a ratio within run-to-run noise.
The two are timed in turn within every repetition.  Prints one table row and one JSON line per measurement (median, minimum and
maximum of the timed repetitions).

usage: records_time.py [--records 1,4,16] [--chains 1,16] [--rows 500] [--N 200] [--reps 7] [--json OUT]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pgas_amd  # noqa: E402
from pgas_amd import chains as ch  # noqa: E402
from pgas_amd import experiments  # noqa: E402
from pgas_amd import random as prng  # noqa: E402


def timed(fs, reps):
    """Per function of `fs`: (median, min, max) ms per call -- device events around each call, the functions taken in turn within every
    one of `reps` rounds (so that drift of the machine falls on all of them alike), after two warm-up rounds."""
    for _ in range(2):
        for f in fs:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fs]
    for _ in range(reps):
        for f, m in zip(fs, ms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            m.append(e0.elapsed_time(e1))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def stepper(mc, keys, ref, A, S):
    """A closure that advances `mc` by one Gibbs iteration per call, its state carried on the device."""
    state = dict(k=keys, traj=ref, A=A, S=S)

    def step():
        state["k"], state["traj"], state["A"], state["S"], _ = mc.step(state["k"], state["traj"], state["A"], state["S"])

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="1,4,16")
    ap.add_argument("--chains", default="1,16")
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    N, Te = a.N, a.rows
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for E in [int(v) for v in a.records.split(",")]:
        pb = experiments.smo_pgas(T=E * Te)
        A0, S0 = experiments.initial_params(pb)
        cut = [slice(e * Te, (e + 1) * Te) for e in range(E)]
        model = (pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.GP_prior, pb.basis_fcn)
        for C in [int(v) for v in a.chains.split(",")]:
            keys = ch.keys_tensor(prng.split(prng.key(12345678), C), dev)
            A = torch.as_tensor(np.repeat(A0[None], C, axis=0), device=dev)
            S = torch.as_tensor(np.repeat(S0[None], C, axis=0), device=dev)
            mr = pgas_amd.MultiRecordPGAS(C, N, 2, [pb.observations[s] for s in cut], [pb.inputs[s] for s in cut], *model, keep_chain_log=False)
            together = stepper(mr, keys, mr.cSMC._refs(pb.X_true), A, S)
            singles = [pgas_amd.MultiChainPGAS(C, N, 2, pb.observations[s], pb.inputs[s], *model, keep_chain_log=False) for s in cut]
            steps = [stepper(m, keys, m.cSMC._refs(pb.X_true[s]), A, S) for m, s in zip(singles, cut)]
            joint, apart = timed([together, lambda: [f() for f in steps]], a.reps)
            row = dict(model="smo", N=N, rows_per_record=Te, E=E, C=C, records_ms=joint[0], records_ms_min=joint[1], records_ms_max=joint[2],
                       one_after_another_ms=apart[0], one_after_another_ms_min=apart[1], one_after_another_ms_max=apart[2], ratio=apart[0] / joint[0])
            rows.append(row)
            print(f"E={E:3d} C={C:3d}: one multi-record iteration {joint[0]:8.2f} ms ({joint[1]:.2f}..{joint[2]:.2f}), {E} single-record iterations one "
                  f"after another {apart[0]:8.2f} ms ({apart[1]:.2f}..{apart[2]:.2f}): {row['ratio']:.2f}x", flush=True)
            print(json.dumps(row), flush=True)
            del mr, singles, steps, together
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
