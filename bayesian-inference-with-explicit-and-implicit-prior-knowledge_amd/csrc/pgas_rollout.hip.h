// pgas_rollout.hip.h -- open-loop simulation of the learned transition model under K posterior draws (A_k, S_k) in ONE launch
// (DESIGN.md section 13): x_t = A_k phi(x_{t-1}, u_t) [+ LS_k z_t], t = 1 .. T - 1, for P replicates per draw.
//
//   k_rollout   one workgroup per draw (blockIdx.x = draw); lanes and NR registers per lane are the replicates (p = r * 256 + tid)
//
// The step is the propagation of the one-workgroup sweep (small_particle_step, pgas_resample.hip.h) without its weights: the same input
// row u_t, the same eval_mean instantiation on the draw's coefficient tensor in LDS, the same ascending fma chain for LS z, and the
// same Philox counters (seed, PGAS_STREAM_PROP, t, particle).  The reference propagates particle i from its own previous state
// (quirk Q1), so particle i < N - 1 of a sweep IS a free noisy rollout: replicate p0 + p of draw k equals particle p0 + p of a sweep
// with seed_k, A_k, S_k, bit for bit.  Every replicate's state stays in registers for all T steps; the only traffic is the coalesced
// store of out[k, t, :, :].  Draws never wait for each other: no flag, counter or barrier crosses a workgroup, so K may exceed what
// the GPU holds at once.  Per-draw G_k and (LS, LS^-1, cS) come from k_chains_pack (pgas_chains.hip.h) on the rollout's own buffers.
#pragma once

#include "pgas_chains.hip.h"

#define PG_ROLLOUT_X0_DRAWN 0   // x_0 ~ N(m0, P0) on PGAS_STREAM_INIT, as the sweep draws it
#define PG_ROLLOUT_X0_ONE 1     // x0 (nx): every draw and replicate
#define PG_ROLLOUT_X0_DRAW 2    // x0 (K, nx): per draw
#define PG_ROLLOUT_X0_EACH 3    // x0 (K, P, nx): per draw and replicate

// per draw k: tp_all[k], G_all + k gstride, seeds[k] (seeds == NULL: no process noise, tp_all is not read), out (K, T, P, NX)
template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_rollout(DevModel md, const TransParams* __restrict__ tp_all, const double* __restrict__ G_all, int64_t gstride,
                                                    const uint64_t* __restrict__ seeds, const double* __restrict__ m0L0, const double* __restrict__ x0,
                                                    int x0_mode, int P, int64_t p0, double* __restrict__ out_all) {
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_rollout[];   // the draw's coefficient tensor
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, T = md.T;
    const double* __restrict__ G_arg = G_all + draw * (size_t)gstride;
    double* __restrict__ out = out_all + draw * (size_t)T * P * NX;
    const size_t row = (size_t)P * NX;
    {
        int gtot = NX;
#pragma unroll
        for (int d = 0; d < D; ++d) gtot *= (d == D - 1 && D > 1) ? JIN : md.J[d];
        for (int i = tid; i < gtot; i += PG_BLK) pg_g_lds_rollout[i] = G_arg[i];
        lds_barrier();
    }
    const double* Guse = pg_g_lds_rollout;
    const bool noisy = seeds != nullptr;
    const uint64_t seed = noisy ? ld_const(seeds + draw) : 0ull;
    double LS[4] = {0.0, 0.0, 0.0, 0.0};
    if (noisy) {
#pragma unroll
        for (int q = 0; q < 4; ++q) LS[q] = ld_const(&tp_all[draw].LS[q]);
    }
    // a wave all of whose replicates lie past P has nothing to do (nothing below crosses a wave)
    if ((tid & ~63) >= P) return;

    // ---- row 0: given, or x_0 ~ N(m0, P0) with the sweep's counters (src/PGAS.py:155-174)
    double x[NR][NX];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int p = r * PG_BLK + tid, pc = p < P ? p : P - 1;
        if (x0_mode == PG_ROLLOUT_X0_DRAWN) {
            double z[2] = {0.0, 0.0};
            pgas_rng_normals(seed, PGAS_STREAM_INIT, 0u, (uint64_t)(p0 + pc), NX, z);
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                double v = m0L0[k];
#pragma unroll
                for (int l = 0; l <= k; ++l) v = PGAS_FMA(m0L0[NX + k * NX + l], z[l], v);
                x[r][k] = v;
            }
        } else {
            const size_t off = x0_mode == PG_ROLLOUT_X0_ONE ? 0 : x0_mode == PG_ROLLOUT_X0_DRAW ? draw * NX : (draw * (size_t)P + pc) * NX;
#pragma unroll
            for (int k = 0; k < NX; ++k) x[r][k] = x0[off + k];
        }
        if (p < P) {
#pragma unroll
            for (int k = 0; k < NX; ++k) out[(size_t)p * NX + k] = x[r][k];
        }
    }

    // ---- the time loop: the propagation of src/PGAS.py:45-77,130-133 from the replicate's own previous state
    for (int t = 1; t < T; ++t) {
        const double* __restrict__ ut = md.u + (size_t)t * md.nu;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int p = r * PG_BLK + tid, pc = p < P ? p : P - 1;
            if (r * PG_BLK + (tid & ~63) < P) {   // wave-uniform: register rows past P hold no replicate
                double xin[1][NX], aux[1][NX];
#pragma unroll
                for (int k = 0; k < NX; ++k) xin[0][k] = x[r][k];
                eval_mean<NX, D, JIN, 1, J0T, true>(md, Guse, ut, xin, aux);
                if (noisy) {
                    double z[2] = {0.0, 0.0};
                    pgas_rng_normals(seed, PGAS_STREAM_PROP, (uint32_t)t, (uint64_t)(p0 + pc), NX, z);
#pragma unroll
                    for (int k = 0; k < NX; ++k) {
                        double v = aux[0][k];
#pragma unroll
                        for (int l = 0; l <= k; ++l) v = PGAS_FMA(LS[k * NX + l], z[l], v);
                        x[r][k] = v;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < NX; ++k) x[r][k] = aux[0][k];
                }
                if (p < P) {
#pragma unroll
                    for (int k = 0; k < NX; ++k) st_stream(&out[(size_t)t * row + (size_t)p * NX + k], x[r][k]);
                }
            }
        }
    }
}
