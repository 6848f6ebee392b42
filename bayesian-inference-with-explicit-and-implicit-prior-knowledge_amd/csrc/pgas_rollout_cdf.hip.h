// pgas_rollout_cdf.hip.h -- the empirical predictive CDF of the rollout of pgas_rollout.hip.h at given thresholds, counted over the
// replicates inside the kernel: count[k, t, c, j] = #{replicates p < P : v_c <= thr[t, c, j]}, an int32.
//
//   k_rollout_cdf   grid (K, B = ceil(P / 1024)): blockIdx.x = draw, blockIdx.y = block of 1024 replicates,
//                   replicate p = 1024 b + 256 r + lane; B = 1 stores the counts, B > 1 adds them with integer atomics onto an
//                   output the host zeroed on the same stream
//
// The propagation is k_rollout_stats', operation for operation (the staging of G_k, the eval_mean instantiation, the fma chain of LS z,
// the Philox counters, the four x0 modes), so replicate p0 + p carries exactly the state pgas_rollout stores for it; the value channels
// are k_rollout_stats' too: the state x_j, then yhat_j = sum_k H[j,k] x_k (ascending fma chain from +0.0, continued with LR[j,l] e_l,
// l = 0 .. j, e on PGAS_STREAM_OBS, when measurement noise is asked for).
//
// The counting stage (shared with pgas_forecast_cdf.hip.h).  Slot i = c J + j < (nx + ny) J <= 64 names (channel, threshold):
//   thresholds   lane i of every wave holds thr[row, i] in a register, fetched one step ahead; the stage reads it with v_readlane, so a
//                threshold is wave-uniform (an SGPR pair) where it is compared
//   count        per slot and register row r: popcount of the 64-lane ballot of (replicate < P and v <= threshold), the IEEE comparison
//                (a NaN on either side counts nothing); the rows' popcounts are added in scalar registers and lane i of one VGPR keeps
//                the wave's total (a select on lane == i)
//   waves        the 64 lanes of every wave write that VGPR to cnt[step parity][wave][lane]; after the step's barrier lane i of wave 0
//                adds the four waves' words and sends the total on its way
// Integer addition is exact: no result bit depends on NR, the wave layout or the block split.
//
// Barriers: every wave reaches every barrier -- a wave without replicates counts nothing and skips the propagation only.  ONE barrier
// per step.  LDS hazards (slot set t & 1 of cnt; barrier t is the one of step t):
//   cnt[t & 1][wave][0 .. 63]   written by every wave before barrier t, read by wave 0 after it; next written before barrier t + 2, that
//                               is after barrier t + 1, which no wave passes before wave 0 has read step t (lds_barrier waits for its
//                               LDS reads)
// The counts leave through global stores (or atomics) of wave 0 that nothing waits for.
#pragma once

#include "pgas_rollout_stats.hip.h"

#define PG_CDF_SLOTS 64   // (nx + ny) J <= (2 + PGAS_MAX_NY) PGAS_CDF_MAX_J
static_assert((2 + PGAS_MAX_NY) * PGAS_CDF_MAX_J <= PG_CDF_SLOTS, "a wave's lanes hold one (channel, threshold) slot each");

// lane i < nslots: thr_row[i]; the other lanes: NaN (a slot that is never read)
__device__ __forceinline__ double cdf_fetch_thresholds(const double* __restrict__ thr_row, int lane, int nslots) {
    return lane < nslots ? thr_row[lane] : __builtin_nan("");
}

// One value channel of NR register rows against its J thresholds (slots base .. base + J - 1 of thv): row r of lane `tid` holds a
// replicate when r * PG_BLK + tid < nrem.  Every lane of the wave must be active.  Returns `mine` with the wave's counts in lanes
// base .. base + J - 1.
template <int NR>
__device__ __forceinline__ int cdf_count_channel(const double (&v)[NR], int tid, int nrem, double thv, int base, int J, int mine) {
    const int lane = tid & 63;
    for (int j = 0; j < J; ++j) {
        const double th = readlane_f64(thv, base + j);
        int n = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) n += __popcll(__ballot(r * PG_BLK + tid < nrem && v[r] <= th));
        mine = lane == base + j ? n : mine;
    }
    return mine;
}

// the block's total of slot `slot` after the step's barrier
__device__ __forceinline__ int cdf_block_total(const int (&cnt)[4][PG_CDF_SLOTS], int slot) {
    return (cnt[0][slot] + cnt[1][slot]) + (cnt[2][slot] + cnt[3][slot]);
}

template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_rollout_cdf(DevModel md, const TransParams* __restrict__ tp_all, const double* __restrict__ G_all, int64_t gstride,
                                                        const uint64_t* __restrict__ seeds, const double* __restrict__ m0L0, const double* __restrict__ x0,
                                                        int x0_mode, int P, int64_t p0, RolloutObs ob, const double* __restrict__ thr, int J,
                                                        int32_t* __restrict__ count_all) {
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_rcdf[];   // the draw's coefficient tensor
    __shared__ int cnt[2][4][PG_CDF_SLOTS];                                    // [step parity][wave][slot]
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, T = md.T, ny = md.ny;
    const int pbase = (int)blockIdx.y * PGAS_SEG;   // P <= 2^20
    const int nv = NX + ny, nslots = nv * J, nrem = P - pbase;
    const bool add = gridDim.y > 1;
    const double* __restrict__ G_arg = G_all + draw * (size_t)gstride;
    int32_t* __restrict__ count = count_all + draw * (size_t)T * nslots;
    {
        int gtot = NX;
#pragma unroll
        for (int d = 0; d < D; ++d) gtot *= (d == D - 1 && D > 1) ? JIN : md.J[d];
        for (int i = tid; i < gtot; i += PG_BLK) pg_g_lds_rcdf[i] = G_arg[i];
        lds_barrier();
    }
    const double* Guse = pg_g_lds_rcdf;
    const bool noisy = seeds != nullptr;
    const uint64_t seed = noisy ? ld_const(seeds + draw) : 0ull;
    double LS[4] = {0.0, 0.0, 0.0, 0.0};
    if (noisy) {
#pragma unroll
        for (int q = 0; q < 4; ++q) LS[q] = ld_const(&tp_all[draw].LS[q]);
    }

    double x[NR][NX];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int k = 0; k < NX; ++k) x[r][k] = 0.0;
    }
    double thnext = cdf_fetch_thresholds(thr, lane, nslots);   // row 0

    for (int t = 0; t < T; ++t) {
        const int par = t & 1;
        const double thv = thnext;
        if (t + 1 < T) thnext = cdf_fetch_thresholds(thr + (size_t)(t + 1) * nslots, lane, nslots);   // one step ahead
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

        // ---- the channels of step t, one at a time, against their thresholds: the wave's counts gather in `mine`
        int mine = 0;
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            double v[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) v[r] = x[r][k];
            mine = cdf_count_channel<NR>(v, tid, nrem, thv, k * J, J, mine);
        }
#pragma unroll
        for (int j = 0; j < PGAS_MAX_NY; ++j) {
            if (j < ny) {
                double v[NR];
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
                    v[r] = acc;
                }
                mine = cdf_count_channel<NR>(v, tid, nrem, thv, (NX + j) * J, J, mine);
            }
        }
        cnt[par][wave][lane] = mine;
        lds_barrier();   // barrier t

        // ---- after the barrier: wave 0 sends the block's counts of step t on their way
        if (tid < nslots) {
            const int total = cdf_block_total(cnt[par], tid);
            int32_t* dst = &count[(size_t)t * nslots + tid];
            if (add) atomicAdd(dst, total);
            else st_stream(dst, (int32_t)total);
        }
    }
}
