"""Kernel launches per step of the batched marginalised filter's eager loop (pgas_amd.MultiRunAlgorithm1; development aid): run under
   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/runs_launches.py [R] [T]   (traced model callables)
and divide the `Calls` column by T - 1; tools/alg1_launches.py is the single run's count."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import pgas_amd
from pgas_amd import experiments
from pgas_amd import random as prng
N, R, T = 200, int(sys.argv[1]) if len(sys.argv) > 1 else 64, int(sys.argv[2]) if len(sys.argv) > 2 else 201
pb = experiments.smo_marginal(T=T)
alg = pgas_amd.MultiRunAlgorithm1(R, N, observations=pb.observations, inputs=pb.inputs, SSM=pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel),
                                  forgetting_factor=pb.forgetting_factor, init_state_mean=pb.init_state_mean, init_state_cov=pb.init_state_cov,
                                  init_int_var_mean=pb.init_int_var_mean, init_int_var_cov=pb.init_int_var_cov, GP_prior=pb.GP_prior,
                                  basis_fcn=pb.basis_fcn())
rand = alg._rand(prng.split(prng.key(12345678), R))
st, iv, sst, lw, anc, stats = alg._init_algorithm(rand)
traces = (st, iv, sst, lw, anc)
for t in range(1, T):
    stats = alg._loop_body(rand, t, traces, stats)
torch.cuda.synchronize()
