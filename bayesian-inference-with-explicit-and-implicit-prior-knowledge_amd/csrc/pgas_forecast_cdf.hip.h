// pgas_forecast_cdf.hip.h -- the empirical CDF of the h-step-ahead clouds of pgas_forecast.hip.h at given thresholds, every origin row
// of every draw in ONE launch: count[k, h - 1, tau, c, j] = #{particles i < N : v_c <= thr[tau, c, j]}, an int32.
//
//   k_forecast_cdf   grid (K, ceil(T / TB)): blockIdx.x = draw, blockIdx.y = chunk of TB origin rows; particle i = 256 r + tid, r < NR
//
// The clouds are k_forecast's, bit for bit: per origin s and lead l = 0 .. min(H, T - s) - 1 (target row tau = s + l, horizon h = l + 1)
//   1. cloud     l = 0: c[i] = x[k, s, i]; l >= 1: c[i] = A_k phi(c[i], u_{s+l}) + LS_k z, z on (seed_k, PGAS_STREAM_FORECAST, t = s + l,
//                particle = l << 32 | i)
//   2. channels  the state c_j, then yhat_j = sum_k H[j,k] c_k (fma chain from +0.0), continued with LR[j,q] e_q, q = 0 .. j, when
//                measurement noise is asked for: e on (seed_k, PGAS_STREAM_OBS, t = tau, particle = (l + 1) << 32 | i) -- the high word
//                is never 0, so no counter is shared with the open loop's noise (pgas_rollout_cdf.hip.h, particle = p0 + p < 2^32)
//   3. counts    the counting stage of pgas_rollout_cdf.hip.h against the thresholds of the TARGET row, thr[tau]: one threshold set
//                serves every horizon
//   4. the entries without an origin row (tau < l) are -1: written by the draw's chunk 0
// Every defined entry (l, tau) belongs to origin tau - l alone, so it has one writer and plain stores do; no flag, counter or barrier
// crosses a workgroup, so K x chunks may exceed what the GPU holds.
//
// Barriers: the lead-loop bound min(H, T - s) and the origin range are workgroup-uniform, and a wave or register row without particles
// skips the propagation only (it counts nothing), so every wave reaches every barrier.  The steps of a workgroup (all leads of all its
// origins) are numbered n = 0, 1, ...; there is ONE barrier per step.
//
// LDS hazards (slot set n & 1 of cnt; barrier n is the one of step n):
//   cnt[n & 1][wave][0 .. 63]   written by every wave before barrier n, read by wave 0 after it; next written before barrier n + 2, that
//                               is after barrier n + 1, which no wave passes before wave 0 has read step n
// The thresholds of step n + 1 (target row t + 1 within an origin, s + 1 at the next origin's lead 0) are fetched during step n.  The
// counts leave through global stores of wave 0 that nothing waits for.
#pragma once

#include "pgas_rollout_cdf.hip.h"

template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_forecast_cdf(DevModel md, const TransParams* __restrict__ tp_all, const double* __restrict__ G_all, int64_t gstride,
                                                         const uint64_t* __restrict__ seeds, const double* __restrict__ x_all, int Hz, int TB, RolloutObs ob,
                                                         const double* __restrict__ thr, int J, int32_t* __restrict__ count_all) {
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_fcdf[];   // the draw's coefficient tensor
    __shared__ int cnt[2][4][PG_CDF_SLOTS];                                    // [step parity][wave][slot]
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, N = md.N, T = md.T, ny = md.ny, nv = NX + ny, nslots = nv * J;
    const int s_lo = (int)blockIdx.y * TB, s_hi = s_lo + TB < T ? s_lo + TB : T;
    const double* __restrict__ G_arg = G_all + draw * (size_t)gstride;
    const double* __restrict__ x_trace = x_all + draw * (size_t)T * N * NX;
    int32_t* __restrict__ count = count_all + draw * (size_t)Hz * T * nslots;   // (H, T, nv, J)
    {
        int gtot = NX;
#pragma unroll
        for (int d = 0; d < D; ++d) gtot *= (d == D - 1 && D > 1) ? JIN : md.J[d];
        for (int i = tid; i < gtot; i += PG_BLK) pg_g_lds_fcdf[i] = G_arg[i];
        lds_barrier();
    }
    const double* Guse = pg_g_lds_fcdf;
    const uint64_t seed = ld_const(seeds + draw);
    double LS[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) LS[q] = ld_const(&tp_all[draw].LS[q]);

    // ---- 4. the entries no origin row reaches: horizon index l > tau
    if (blockIdx.y == 0) {
        for (int l = 1; l < Hz; ++l)
            for (int e = tid; e < l * nslots; e += PG_BLK) st_stream(&count[(size_t)l * T * nslots + e], (int32_t)-1);   // rows tau = 0 .. l - 1: contiguous
    }

    double x[NR][NX];
    int n = 0;   // the workgroup's step counter: the slot set's parity
    double thnext = cdf_fetch_thresholds(thr + (size_t)s_lo * nslots, lane, nslots);   // step 0: target row s_lo

    for (int s = s_lo; s < s_hi; ++s) {
        // ---- the origin's cloud: row s of the trace (lanes read consecutive particles)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int i = r * PG_BLK + tid, ic = i < N ? i : N - 1;
#pragma unroll
            for (int k = 0; k < NX; ++k) x[r][k] = x_trace[((size_t)s * N + ic) * NX + k];
        }
        const int L = Hz < T - s ? Hz : T - s;   // workgroup-uniform
        for (int l = 0; l < L; ++l, ++n) {
            const int par = n & 1, t = s + l;
            const double thv = thnext;
            {
                const int tn = l + 1 < L ? t + 1 : s + 1;   // the next step's target row; s + 1 < T is tested, s + 1 >= s_hi fetches a row nobody uses
                if (tn < T) thnext = cdf_fetch_thresholds(thr + (size_t)tn * nslots, lane, nslots);
            }
            if (l > 0) {
                // ---- 1. the propagation of k_rollout from the particle's own previous state, on the forecast's stream
                const double* __restrict__ ut = md.u + (size_t)t * md.nu;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const int i = r * PG_BLK + tid, ic = i < N ? i : N - 1;
                    if (r * PG_BLK + (tid & ~63) < N) {   // wave-uniform: register rows past N hold no particle
                        double xin[1][NX], aux[1][NX];
#pragma unroll
                        for (int k = 0; k < NX; ++k) xin[0][k] = x[r][k];
                        eval_mean<NX, D, JIN, 1, J0T, true>(md, Guse, ut, xin, aux);
                        double z[2] = {0.0, 0.0};
                        pgas_rng_normals(seed, PGAS_STREAM_FORECAST, (uint32_t)t, ((uint64_t)l << 32) | (uint64_t)ic, NX, z);
#pragma unroll
                        for (int k = 0; k < NX; ++k) {
                            double v = aux[0][k];
#pragma unroll
                            for (int q = 0; q <= k; ++q) v = PGAS_FMA(LS[k * NX + q], z[q], v);
                            x[r][k] = v;
                        }
                    }
                }
            }

            // ---- 2., 3. the channels of the step, one at a time, against the target row's thresholds
            int mine = 0;
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                double v[NR];
#pragma unroll
                for (int r = 0; r < NR; ++r) v[r] = x[r][k];
                mine = cdf_count_channel<NR>(v, tid, N, thv, k * J, J, mine);
            }
#pragma unroll
            for (int j = 0; j < PGAS_MAX_NY; ++j) {
                if (j < ny) {
                    double v[NR];
#pragma unroll
                    for (int r = 0; r < NR; ++r) {
                        const int i = r * PG_BLK + tid, ic = i < N ? i : N - 1;
                        double acc = 0.0;
#pragma unroll
                        for (int k = 0; k < NX; ++k) acc = PGAS_FMA(md.H[j * NX + k], x[r][k], acc);
                        if (ob.noise) {
                            double e[PGAS_MAX_NY] = {0.0, 0.0};
                            pgas_rng_normals(seed, PGAS_STREAM_OBS, (uint32_t)t, ((uint64_t)(l + 1) << 32) | (uint64_t)ic, ny, e);
#pragma unroll
                            for (int q = 0; q <= j; ++q) acc = PGAS_FMA(ob.LR[j * ny + q], e[q], acc);
                        }
                        v[r] = acc;
                    }
                    mine = cdf_count_channel<NR>(v, tid, N, thv, (NX + j) * J, J, mine);
                }
            }
            cnt[par][wave][lane] = mine;
            lds_barrier();   // barrier n

            // ---- after the barrier: wave 0 sends the step's counts on their way
            if (tid < nslots) st_stream(&count[((size_t)l * T + t) * nslots + tid], (int32_t)cdf_block_total(cnt[par], tid));
        }
    }
}
