// pgas_forecast.hip.h -- h-step-ahead predictions from the held-out filter's particle trace, every origin row of every draw in ONE
// launch: p(y_tau | y_{0:tau-h}, A_k, S_k) for h = 1 .. H, as predictive moments and as a log score.
//
//   k_forecast   grid (K, ceil(T / TB)): blockIdx.x = draw, blockIdx.y = chunk of TB origin rows; particle i = 256 r + tid, r < NR
//
// Row s of pgas_filter's trace x (K, T, N, nx) is stored before y_s is used: a sample of p(x_s | y_{0:s-1}).  Per origin s and lead
// l = 0 .. min(H, T - s) - 1 (target row tau = s + l, horizon h = l + 1), in this order:
//   1. cloud     l = 0: c[i] = x[k, s, i] (nothing is propagated); l >= 1: c[i] = A_k phi(c[i], u_{s+l}) + LS_k z, the eval_mean
//                instantiation and the noise chain of k_rollout, z on (seed_k, PGAS_STREAM_FORECAST, t = s + l, particle = l << 32 | i):
//                the counter names (target row, lead, particle) and nothing else -- not H, not TB, not the draws of the launch
//   2. channels  the state c_j, then yhat_j = sum_k H[j,k] c_k (fma chain from +0.0, no measurement noise): k_filter's step 3
//   3. moments   sum[k, l, tau, :] = sum_i v, sumsq = sum_i (v v) (product rounded, then added) in the order of pgas_rollout_stats.hip.h
//                levels 1-2; at l = 0 the operation sequence of k_filter's pred_sum / pred_sumsq
//   4. log score l_i = loglik<NX>(y_tau, c[i]); m = max l (NaN takes no part), s = sum_i pgas_exp(l_i - m) in the order of 3 (a NaN l adds
//                +0.0); lpd[k, l, tau] = (m + pgas_log(s)) - pgas_log(N); -inf when s = 0; NaN when y_tau holds a NaN (tested)
//   5. the entries without an origin row (tau < l) are NaN: written by the draw's chunk 0
// Every defined entry (l, tau) belongs to origin tau - l alone, so it has one writer; no flag, counter or barrier crosses a workgroup,
// so K x chunks may exceed what the GPU holds.
//
// Barriers: the lead-loop bound min(H, T - s) and the origin range are workgroup-uniform, and a wave or register row without particles
// skips the propagation only (it adds +0.0 / -inf), so every wave reaches every barrier.  The steps of a workgroup (all leads of all its
// origins) are numbered n = 0, 1, ...; there is ONE barrier per step and one more after the last.
//
// LDS hazards (slot set n & 1 of red; barrier n is the one of step n):
//   moment slots, max slot   written before barrier n, read after it (wave 0 the moments, every wave the maximum); next written before
//                            barrier n + 2, that is after barrier n + 1, which no wave passes before every wave has read step n
//   exp-sum slot             needs the maximum: written after barrier n, read after barrier n + 1 (by the thread that stores lpd of step
//                            n, whose maximum, target and NaN flag it kept in registers); next written after barrier n + 2
// The outputs leave through global stores of wave 0 that nothing waits for.
#pragma once

#include "pgas_rollout_stats.hip.h"

template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_forecast(DevModel md, const TransParams* __restrict__ tp_all, const double* __restrict__ G_all, int64_t gstride,
                                                     const uint64_t* __restrict__ seeds, const double* __restrict__ x_all, int Hz, int TB, int score,
                                                     double* __restrict__ sum_all, double* __restrict__ sumsq_all, double* __restrict__ lpd_all) {
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_forecast[];   // the draw's coefficient tensor
    __shared__ double red[2][4][PG_RS_SLOTS];                                      // [step parity][wave][slot]
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, N = md.N, T = md.T, ny = md.ny, nv = NX + ny;
    const int s_lo = (int)blockIdx.y * TB, s_hi = s_lo + TB < T ? s_lo + TB : T;
    const double* __restrict__ G_arg = G_all + draw * (size_t)gstride;
    const double* __restrict__ x_trace = x_all + draw * (size_t)T * N * NX;
    double* __restrict__ sum_out = sum_all + draw * (size_t)Hz * T * nv;     // (H, T, nv)
    double* __restrict__ sumsq_out = sumsq_all + draw * (size_t)Hz * T * nv;
    double* __restrict__ lpd_out = score ? lpd_all + draw * (size_t)Hz * T : nullptr;   // (H, T)
    {
        int gtot = NX;
#pragma unroll
        for (int d = 0; d < D; ++d) gtot *= (d == D - 1 && D > 1) ? JIN : md.J[d];
        for (int i = tid; i < gtot; i += PG_BLK) pg_g_lds_forecast[i] = G_arg[i];
        lds_barrier();
    }
    const double* Guse = pg_g_lds_forecast;
    const uint64_t seed = ld_const(seeds + draw);
    double LS[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) LS[q] = ld_const(&tp_all[draw].LS[q]);
    const double ninf = -__builtin_inf(), qnan = __builtin_nan("");

    // ---- 5. the entries no origin row reaches: horizon index l > tau
    if (blockIdx.y == 0) {
        for (int l = 1; l < Hz; ++l) {
            for (int e = tid; e < l * nv; e += PG_BLK) {   // rows tau = 0 .. l - 1 of horizon index l are contiguous
                st_stream(&sum_out[(size_t)l * T * nv + e], qnan);
                st_stream(&sumsq_out[(size_t)l * T * nv + e], qnan);
            }
            if (score)
                for (int e = tid; e < l; e += PG_BLK) st_stream(&lpd_out[(size_t)l * T + e], qnan);
        }
    }

    double x[NR][NX];
    int n = 0;                 // the workgroup's step counter: the slot set's parity
    double m_prev = ninf;      // step n - 1: its maximum, where its lpd goes, whether its observation row holds a NaN
    size_t lpd_prev = 0;
    bool ynan_prev = false;

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

            // ---- 2., 3. the channels of the step, one at a time: lane-local sums in ascending r, the wave's tree, lane 0 of the wave to LDS
            const double* __restrict__ yt = md.y + (size_t)t * ny;
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const bool has = r * PG_BLK + tid < N;
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
                        const bool has = r * PG_BLK + tid < N;
                        double acc = 0.0;
#pragma unroll
                        for (int k = 0; k < NX; ++k) acc = PGAS_FMA(md.H[j * NX + k], x[r][k], acc);
                        const double vv = acc * acc;
                        s1 = has ? s1 + acc : s1;
                        s2 = has ? s2 + vv : s2;
                    }
                    s1 = wave_sum_tree(s1);
                    s2 = wave_sum_tree(s2);
                    if ((tid & 63) == 0) {
                        red[par][wave][NX + j] = s1;
                        red[par][wave][PG_RS_NV + NX + j] = s2;
                    }
                }
            }
            // ---- 4. log score: the wave's maximum before the barrier
            double lcur[NR];
            bool ynan = false;
            if (score) {
#pragma unroll
                for (int j = 0; j < PGAS_MAX_NY; ++j) ynan = ynan || (j < ny && yt[j] != yt[j]);
                double m = ninf;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    lcur[r] = loglik<NX>(md, yt, x[r]);
                    if (!(r * PG_BLK + tid < N)) lcur[r] = ninf;
                    m = __builtin_fmax(m, lcur[r]);   // NaN takes no part
                }
                m = wave_max(m);
                if ((tid & 63) == 0) red[par][wave][2 * PG_RS_NV] = m;
            }
            lds_barrier();   // barrier n

            // ---- after the barrier: wave 0 sends the step's moments on their way; every wave needs the maximum
            const size_t row = (size_t)l * T + t;   // (horizon index, target row)
            if (tid < 2 * nv) {
                const int c = tid < nv ? tid : tid - nv, slot = tid < nv ? c : PG_RS_NV + c;
                double* __restrict__ dst = (tid < nv ? sum_out : sumsq_out) + row * nv + c;
                st_stream(dst, (red[par][0][slot] + red[par][1][slot]) + (red[par][2][slot] + red[par][3][slot]));
            }
            if (score) {
                if (n > 0 && tid == 2 * nv) {   // lpd of step n - 1: its exp sums were written after barrier n - 1
                    const int q = par ^ 1, slot = 2 * PG_RS_NV + 1;
                    const double S = (red[q][0][slot] + red[q][1][slot]) + (red[q][2][slot] + red[q][3][slot]);
                    const double v = S == 0.0 ? ninf : (m_prev + pgas_log(S)) - pgas_log((double)N);
                    st_stream(&lpd_out[lpd_prev], ynan_prev ? qnan : v);
                }
                const int slot = 2 * PG_RS_NV;
                const double mb = __builtin_fmax(__builtin_fmax(red[par][0][slot], red[par][1][slot]), __builtin_fmax(red[par][2][slot], red[par][3][slot]));
                double sx = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const double lv = lcur[r];
                    const double ex = pgas_exp(lv - mb);
                    const bool takes = (lv == lv) && mb != ninf && r * PG_BLK + tid < N;
                    sx = takes ? sx + ex : sx;
                }
                sx = wave_sum_tree(sx);
                if ((tid & 63) == 0) red[par][wave][2 * PG_RS_NV + 1] = sx;
                m_prev = mb;
                lpd_prev = row;
                ynan_prev = ynan;
            }
        }
    }
    if (score && n > 0) {   // n > 0 always (s_lo < T and L >= 1): kept for the reader
        lds_barrier();
        if (tid == 2 * nv) {
            const int q = (n - 1) & 1, slot = 2 * PG_RS_NV + 1;
            const double S = (red[q][0][slot] + red[q][1][slot]) + (red[q][2][slot] + red[q][3][slot]);
            const double v = S == 0.0 ? ninf : (m_prev + pgas_log(S)) - pgas_log((double)N);
            st_stream(&lpd_out[lpd_prev], ynan_prev ? qnan : v);
        }
    }
}
