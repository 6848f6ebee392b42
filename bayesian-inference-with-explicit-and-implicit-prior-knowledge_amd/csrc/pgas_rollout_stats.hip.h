// pgas_rollout_stats.hip.h -- the posterior predictive of the OBSERVATIONS from the rollout of pgas_rollout.hip.h, reduced over the
// replicates inside the kernel ("Predictive moments and log score"): nothing per replicate is written to memory.
//
//   k_rollout_stats         grid (K, B = ceil(P / 1024)): blockIdx.x = draw, blockIdx.y = block of 1024 replicates,
//                           replicate p = 1024 b + 256 r + lane; per step the block's partial sums go to part (K, B, T, C)
//   k_rollout_stats_finish  one thread per (k, t, channel): the blocks' partials in ascending b; the log predictive density
//
// The propagation is k_rollout's, operation for operation (the staging of G_k, the eval_mean instantiation, the fma chain of LS z, the
// Philox counters, the four x0 modes), so replicate p0 + p carries exactly the state pgas_rollout stores for it.  Per step t (row 0
// included) and replicate the value channels are the state x_j, the predicted observation yhat_j = sum_k H[j,k] x_k (ascending fma
// chain from +0.0, continued with LR[j,l] e_l, l = 0 .. j, e on PGAS_STREAM_OBS, when measurement noise is asked for) and, for the log
// score, l = loglik<NX>(md, y_t, x).  Every value channel v is reduced to S1 = sum v and S2 = sum (v * v) (product rounded, then added)
// in a DEFINED order that depends neither on NR nor on the wave layout:
//   1. lane-local   s = (((+0.0 + v[r = 0]) + v[r = 1]) + ...), ascending r, over the replicates < P only
//   2. 256 lanes    the balanced adjacent-pair tree v <- v[0::2] + v[1::2], eight times; lanes without a replicate hold +0.0.  An xor
//                   butterfly is that tree (IEEE addition commutes): DPP quad permutes and row mirrors for offsets 1 .. 8, the four rows
//                   and then the four waves as (a0 + a1) + (a2 + a3)
//   3. blocks       ascending b from +0.0 (k_rollout_stats_finish)
// Log score per block: m_b = max l (exact; NaN takes no part), s_b = sum pgas_exp(l - m_b) in the order of 1-2 (a NaN l adds +0.0; a
// block without a finite l has m_b = -inf, s_b = 0).
//
// Barriers: every wave reaches every barrier -- a wave without replicates runs the reduction on +0.0 / -inf and skips the propagation
// only.  One LDS slot set per step parity makes ONE barrier per step enough: the wave partials of step t (moments, max l) are written
// before barrier t and read after it; the wave sums of exp(l_t - m_b), which need m_b, are written after barrier t and read after
// barrier t + 1 (one more barrier after the last step).  Slot set t & 1 is next written after barrier t + 1, which no wave passes
// before every wave has finished reading step t.  The partials leave through global stores of wave 0 that nothing waits for.
#pragma once

#include "pgas_rollout.hip.h"

#define PG_RS_NV (2 + PGAS_MAX_NY)       // value channels a slot set has room for: x (<= 2), yhat (<= PGAS_MAX_NY)
#define PG_RS_SLOTS (2 * PG_RS_NV + 2)   // S1, S2 per value channel, wave max of l, wave sum of exp(l - m_b)

struct RolloutObs {   // by value: what the predicted observations need beside the context's model
    double LR[PGAS_MAX_NY * PGAS_MAX_NY];   // lower Cholesky factor of R, row-major ny x ny
    int32_t noise;                          // 1: yhat = H x + LR e
    int32_t score;                          // 1: the log score channels are formed (loglik is evaluated)
};

// the sum over the wave's 64 lanes in the order of the adjacent-pair tree; every lane must be active.  Wave-uniform result.
__device__ __forceinline__ double wave_sum_tree(double v) {
    v = v + dpp_keep_f64<0xB1 /* quad_perm [1,0,3,2]: lane ^ 1 */, 0xf>(v);
    v = v + dpp_keep_f64<0x4E /* quad_perm [2,3,0,1]: lane ^ 2 */, 0xf>(v);
    v = v + dpp_keep_f64<0x141 /* row_half_mirror: the other quad of 8 lanes (quads are uniform by now) */, 0xf>(v);
    v = v + dpp_keep_f64<0x140 /* row_mirror: the other half of the row of 16 */, 0xf>(v);
    const double a0 = readlane_f64(v, 0), a1 = readlane_f64(v, 16), a2 = readlane_f64(v, 32), a3 = readlane_f64(v, 48);
    return (a0 + a1) + (a2 + a3);
}

// number of doubles per (k, b, t) in part: S1 (nx + ny), S2 (nx + ny), m_b, s_b
__host__ __device__ __forceinline__ int rollout_stats_channels(int nx, int ny) { return 2 * (nx + ny) + 2; }

template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_rollout_stats(DevModel md, const TransParams* __restrict__ tp_all, const double* __restrict__ G_all, int64_t gstride,
                                                          const uint64_t* __restrict__ seeds, const double* __restrict__ m0L0, const double* __restrict__ x0,
                                                          int x0_mode, int P, int64_t p0, RolloutObs ob, double* __restrict__ part_all) {
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_rstats[];   // the draw's coefficient tensor
    __shared__ double red[2][4][PG_RS_SLOTS];                                    // [step parity][wave][slot]
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, T = md.T, ny = md.ny;
    const int pbase = (int)blockIdx.y * PGAS_SEG;   // P <= 2^20
    const int nv = NX + ny, C = rollout_stats_channels(NX, ny);
    const double* __restrict__ G_arg = G_all + draw * (size_t)gstride;
    double* __restrict__ part = part_all + (draw * gridDim.y + blockIdx.y) * (size_t)T * C;
    {
        int gtot = NX;
#pragma unroll
        for (int d = 0; d < D; ++d) gtot *= (d == D - 1 && D > 1) ? JIN : md.J[d];
        for (int i = tid; i < gtot; i += PG_BLK) pg_g_lds_rstats[i] = G_arg[i];
        lds_barrier();
    }
    const double* Guse = pg_g_lds_rstats;
    const bool noisy = seeds != nullptr;
    const uint64_t seed = noisy ? ld_const(seeds + draw) : 0ull;
    double LS[4] = {0.0, 0.0, 0.0, 0.0};
    if (noisy) {
#pragma unroll
        for (int q = 0; q < 4; ++q) LS[q] = ld_const(&tp_all[draw].LS[q]);
    }
    const double ninf = -__builtin_inf();

    double x[NR][NX];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int k = 0; k < NX; ++k) x[r][k] = 0.0;
    }

    for (int t = 0; t < T; ++t) {
        const int par = t & 1;
        if (t == 0) {
            // ---- row 0: given, or x_0 ~ N(m0, P0) with the sweep's counters (src/PGAS.py:155-174)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int p = pbase + r * PG_BLK + tid, pc = p < P ? p : P - 1;
                if (pbase + r * PG_BLK + (tid & ~63) < P) {
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
                }
            }
        } else {
            // ---- the propagation of src/PGAS.py:45-77,130-133 from the replicate's own previous state (k_rollout's time loop)
            const double* __restrict__ ut = md.u + (size_t)t * md.nu;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int p = pbase + r * PG_BLK + tid, pc = p < P ? p : P - 1;
                if (pbase + r * PG_BLK + (tid & ~63) < P) {   // wave-uniform: register rows past P hold no replicate
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
                }
            }
        }

        // ---- the channels of step t, one at a time: lane-local sums in ascending r, the wave's tree, lane 0 of the wave to LDS
        const double* __restrict__ yt = md.y + (size_t)t * ny;
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const bool has = pbase + r * PG_BLK + tid < P;
                const double v = x[r][k], vv = v * v;
                s1 = has ? s1 + v : s1;
                s2 = has ? s2 + vv : s2;
            }
            s1 = wave_sum_tree(s1);
            s2 = wave_sum_tree(s2);
            if ((tid & 63) == 0) {
                red[par][wave][k] = s1;
                red[par][wave][PG_RS_NV + k] = s2;
            }
        }
#pragma unroll
        for (int j = 0; j < PGAS_MAX_NY; ++j) {
            if (j < ny) {
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const int p = pbase + r * PG_BLK + tid, pc = p < P ? p : P - 1;
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < NX; ++k) acc = PGAS_FMA(md.H[j * NX + k], x[r][k], acc);
                    if (ob.noise) {
                        double e[PGAS_MAX_NY] = {0.0, 0.0};
                        pgas_rng_normals(seed, PGAS_STREAM_OBS, (uint32_t)t, (uint64_t)(p0 + pc), ny, e);
#pragma unroll
                        for (int l = 0; l <= j; ++l) acc = PGAS_FMA(ob.LR[j * ny + l], e[l], acc);
                    }
                    const double vv = acc * acc;
                    s1 = p < P ? s1 + acc : s1;
                    s2 = p < P ? s2 + vv : s2;
                }
                s1 = wave_sum_tree(s1);
                s2 = wave_sum_tree(s2);
                if ((tid & 63) == 0) {
                    red[par][wave][NX + j] = s1;
                    red[par][wave][PG_RS_NV + NX + j] = s2;
                }
            }
        }
        double lcur[NR];
        if (ob.score) {
            double m = ninf;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                lcur[r] = loglik<NX>(md, yt, x[r]);
                if (!(pbase + r * PG_BLK + tid < P)) lcur[r] = ninf;
                m = __builtin_fmax(m, lcur[r]);   // NaN takes no part
            }
            m = wave_max(m);
            if ((tid & 63) == 0) red[par][wave][2 * PG_RS_NV] = m;
        }
        lds_barrier();   // barrier t

        // ---- after the barrier: wave 0 sends the block's partials of step t on their way; every wave needs m_b
        if (tid < 2 * nv) {
            const int slot = tid < nv ? tid : PG_RS_NV + (tid - nv);
            st_stream(&part[(size_t)t * C + tid], (red[par][0][slot] + red[par][1][slot]) + (red[par][2][slot] + red[par][3][slot]));
        }
        if (ob.score) {
            if (t > 0 && tid == 2 * nv + 1) {   // s_b of step t - 1: written after barrier t - 1
                const int q = par ^ 1, slot = 2 * PG_RS_NV + 1;
                st_stream(&part[(size_t)(t - 1) * C + tid], (red[q][0][slot] + red[q][1][slot]) + (red[q][2][slot] + red[q][3][slot]));
            }
            const int slot = 2 * PG_RS_NV;
            const double mb = __builtin_fmax(__builtin_fmax(red[par][0][slot], red[par][1][slot]), __builtin_fmax(red[par][2][slot], red[par][3][slot]));
            if (tid == 2 * nv) st_stream(&part[(size_t)t * C + tid], mb);
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const double l = lcur[r];
                const double ex = pgas_exp(l - mb);
                const bool takes = (l == l) && mb != ninf && pbase + r * PG_BLK + tid < P;
                s = takes ? s + ex : s;
            }
            s = wave_sum_tree(s);
            if ((tid & 63) == 0) red[par][wave][2 * PG_RS_NV + 1] = s;
        }
    }
    if (ob.score) {
        lds_barrier();
        if (tid == 2 * nv + 1) {
            const int q = (T - 1) & 1, slot = 2 * PG_RS_NV + 1;
            st_stream(&part[(size_t)(T - 1) * C + tid], (red[q][0][slot] + red[q][1][slot]) + (red[q][2][slot] + red[q][3][slot]));
        }
    }
}

// One thread per (k, t, channel): sum[k, t, c] / sumsq[k, t, c] = the blocks' partials in ascending b from +0.0; channel nx + ny is the
// log predictive density lpd[k, t] = (M + log S) - log P with M = max_b m_b, S = sum_b s_b exp(m_b - M) in ascending b from +0.0 over
// the blocks with m_b > -inf; -inf when S = 0; NaN when y_t holds a NaN (tested here, not left to propagation).  Runs for B = 1 too.
__global__ __launch_bounds__(256) void k_rollout_stats_finish(const double* __restrict__ part, const double* __restrict__ y, int K, int B, int T, int nx, int ny, int P,
                                                              double* __restrict__ sum, double* __restrict__ sumsq, double* __restrict__ lpd) {
    const int nv = nx + ny, C = rollout_stats_channels(nx, ny), nch = nv + (lpd ? 1 : 0);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)K * T * nch) return;
    const int c = (int)(i % nch);
    const size_t kt = i / nch, k = kt / T, t = kt % T;
    const double* __restrict__ row = part + (k * B * T + t) * (size_t)C;   // block b: + b T C
    const size_t bstride = (size_t)T * C;
    if (c < nv) {
        double s1 = 0.0, s2 = 0.0;
        for (int b = 0; b < B; ++b) {
            s1 = s1 + row[b * bstride + c];
            s2 = s2 + row[b * bstride + nv + c];
        }
        sum[kt * nv + c] = s1;
        sumsq[kt * nv + c] = s2;
        return;
    }
    const double ninf = -__builtin_inf();
    double M = ninf;
    for (int b = 0; b < B; ++b) M = __builtin_fmax(M, row[b * bstride + 2 * nv]);
    double S = 0.0;
    for (int b = 0; b < B; ++b) {
        const double mb = row[b * bstride + 2 * nv];
        if (mb != ninf) S = S + row[b * bstride + 2 * nv + 1] * pgas_exp(mb - M);
    }
    double v = S == 0.0 ? ninf : (M + pgas_log(S)) - pgas_log((double)P);
    bool ynan = false;
    for (int j = 0; j < ny; ++j) ynan = ynan || y[t * ny + j] != y[t * ny + j];
    if (ynan) v = __builtin_nan("");
    lpd[kt] = v;
}
