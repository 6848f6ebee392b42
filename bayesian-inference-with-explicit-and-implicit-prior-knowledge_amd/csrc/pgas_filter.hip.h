// pgas_filter.hip.h -- a bootstrap particle filter per posterior draw (A_k, S_k, seed_k) on the context's observations, K draws in ONE
// launch: the one-step-ahead predictive density p(y_t | y_{0:t-1}, A_k, S_k), its sum over t (the log marginal
// likelihood of the record) and the filtered state.
//
//   k_filter   one workgroup per draw (blockIdx.x = draw); particle i = r * 256 + tid, r < NR
//
// Per step t, in this order:
//   1. state     t = 0: x_0 drawn as the sweep draws it (PGAS_STREAM_INIT, every i < N: no conditioned particle) or given (pgas_rollout's
//                x0 modes); t >= 1: x_t[i] = A_k phi(x_{t-1}[a_{t-1}[i]], u_t) + LS_k z, z on (seed_k, PGAS_STREAM_PROP, t, i) -- the
//                eval_mean instantiation and the noise chain of small_particle_step, from the RESAMPLED state (not quirk Q1)
//   2. l_i = loglik<NX>(y_t, x_t[i])
//   3. predictive channels (the unweighted cloud, before y_t is used): x_j, then yhat_j = sum_k H[j,k] x_k (fma chain from +0.0); sum
//      and sum of squares in the order of pgas_rollout_stats.hip.h levels 1-2
//   4. small_scan<1, NR>: k = pgas_seg_ref(max l), numerators q_i, integer cumsum c, S = s 2^-51; valid = 0 < S < inf
//   5. ell[t] = filter_ell(k, S, N); -inf when S == 0; NaN when y_t holds a NaN
//   6. filtered channels: w_i = q_i 2^-51; filt_sum_j = sum_i (w_i x_ij) (product rounded, then added, order of 3), wtot = S,
//      ess = (S S) / sum_i (w_i w_i), 0 when not valid
//   7. a_t[i] = min(#{j : c_j 2^-51 < U_i S}, N - 1), U_i = slot_U(u, i), u = pgas_rng_uniform(seed_k, PGAS_STREAM_RESAMPLE, t); identity
//      when not valid (a NaN observation row is a pure prediction step)
//   8. loglik = sum_t ell[t], ascending t from +0.0 over the rows whose y_t holds no NaN
//
// The states live in registers; the resampled state reaches its new owner through the LDS array xs (N nx doubles): the owner writes
// its row, a barrier, each thread reads row a.  Every wave reaches every barrier: a wave without particles skips the propagation
// only.  Draws never wait for each other: no flag, counter or barrier crosses a workgroup, so K may exceed what the GPU holds.
//
// LDS hazards (B1..B3 the barriers of small_scan, B4 the one after the gather rows are written):
//   red[][pred slots]   written before B1 of step t, read by wave 0 after B3; next written after B4
//   sm.red[0][]         written before B1, read (the maximum, for k and q_i) after B3; next written after B4
//   sm.num[0]           written before B3, searched after B3; next written after B4 (and after B1, B2 of step t + 1)
//   red[][filt slots], xs   written after B3, read after B4; next written after B3 of step t + 1
#pragma once

#include "pgas_rollout_stats.hip.h"

#define PG_FL_PRED (2 * PG_RS_NV)     // S1, S2 of the predictive channels: x (<= 2), yhat (<= PGAS_MAX_NY)
#define PG_FL_SLOTS (PG_FL_PRED + 3)  // + sum w x_j (<= 2), sum w w

struct FilterOut {   // by value: the outputs of pgas_filter, per draw k slice k of each; nullable ones as documented in include/pgas_hip.h
    double* ell;        // (K, T)
    double* loglik;     // (K)
    double* ess;        // (K, T) or NULL
    double* pred_sum;   // (K, T, nx + ny) or NULL
    double* pred_sumsq; // with pred_sum
    double* filt_sum;   // (K, T, nx) or NULL
    double* wtot;       // with filt_sum
    double* x;          // (K, T, N, nx) or NULL
    int32_t* anc;       // (K, T, N) or NULL
};

// log((1/N) sum_i exp l_i) from the scan's exact pair: the power-of-two reference k (an integer-valued double) and S = s 2^-51
__device__ __forceinline__ double filter_ell(double kref, double S, int N) {
    return PGAS_FMA(kref, PGAS_SEG_LN2_LO, PGAS_FMA(kref, PGAS_SEG_LN2_HI, pgas_log(S))) - pgas_log((double)N);
}

// ---- the pieces of the weight stage that k_filter and k_model_filter (pgas_marginal_filter.hip.h) share: what follows small_scan<1, NR>.
// The ancestor search and the three stores of filt_sum / wtot / ess stay in each kernel: as shared pieces they changed k_filter's code
// (registers across an occupancy step, and a measured 1 - 2 % per call).

// the four waves' partials of one slot, as (w0 + w1) + (w2 + w3)
template <int W>
__device__ __forceinline__ double sum4(const double (&red)[4][W], int slot) {
    return (red[0][slot] + red[1][slot]) + (red[2][slot] + red[3][slot]);
}

// k = pgas_seg_ref(max l) from the wave maxima small_scan left in sm.red[0]
__device__ __forceinline__ double filter_ref(const SmallSmem& sm) {
    double m = sm.red[0][0];
#pragma unroll
    for (int v = 1; v < PG_BLK / 64; ++v) m = __builtin_fmax(m, sm.red[0][v]);
    return pgas_seg_ref(m);
}

// ell[t]: NaN when y_t holds a NaN, -inf when no particle has weight
__device__ __forceinline__ double filter_increment(bool ynan, double kref, double S, int N) {
    return ynan ? __builtin_nan("") : (S == 0.0 ? -__builtin_inf() : filter_ell(kref, S, N));
}

// w_i = q_i 2^-51 with the numerators small_scan summed
template <int NR>
__device__ __forceinline__ void filter_weights(const double (&lw)[NR], double kref, double (&w)[NR]) {
    double arg[NR];
    uint64_t qv[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) arg[r] = pgas_seg_arg(lw[r], kref);
    dev_exp_q51_n<NR>(arg, qv);
#pragma unroll
    for (int r = 0; r < NR; ++r) w[r] = pgas_u64_to_double(qv[r]) * PGAS_FIX_INV;   // exact: q <= 2^51
}

template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_filter(DevModel md, const TransParams* __restrict__ tp_all, const double* __restrict__ G_all, int64_t gstride,
                                                   const uint64_t* __restrict__ seeds, const double* __restrict__ m0L0, const double* __restrict__ x0,
                                                   int x0_mode, FilterOut out) {
    __shared__ SmallSmem sm;
    __shared__ double xs[NR * PG_BLK * NX];      // the step's states by particle, for the gather of the resampled state
    __shared__ double red[PG_BLK / 64][PG_FL_SLOTS];
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_filter[];   // the draw's coefficient tensor
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, N = md.N, T = md.T, ny = md.ny, nv = NX + ny;
    const double* __restrict__ G_arg = G_all + draw * (size_t)gstride;
    {
        int gtot = NX;
#pragma unroll
        for (int d = 0; d < D; ++d) gtot *= (d == D - 1 && D > 1) ? JIN : md.J[d];
        for (int i = tid; i < gtot; i += PG_BLK) pg_g_lds_filter[i] = G_arg[i];
        lds_barrier();
    }
    const double* Guse = pg_g_lds_filter;
    const uint64_t seed = ld_const(seeds + draw);
    double LS[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) LS[q] = ld_const(&tp_all[draw].LS[q]);
    const bool pow2 = (N & (N - 1)) == 0;
    const double invN = 1.0 / (double)N, ninf = -__builtin_inf();
    const size_t row = (size_t)N * NX;
    double* __restrict__ ell_out = out.ell + draw * (size_t)T;
    double* __restrict__ x_trace = out.x ? out.x + draw * (size_t)T * row : nullptr;
    int32_t* __restrict__ anc_trace = out.anc ? out.anc + draw * (size_t)T * N : nullptr;
    const bool want_pred = out.pred_sum != nullptr, want_filt = out.filt_sum != nullptr, want_w = want_filt || out.ess != nullptr;

    double x[NR][NX];
    int anc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        anc[r] = r * PG_BLK + tid;
#pragma unroll
        for (int k = 0; k < NX; ++k) x[r][k] = 0.0;
    }
    double total = 0.0;

    // y_t is fetched one step ahead (u_t is read by eval_mean through addresses that depend on t alone)
    double yn[PGAS_MAX_NY];
#pragma unroll
    for (int k = 0; k < PGAS_MAX_NY; ++k) yn[k] = k < ny ? md.y[k] : 0.0;

    for (int t = 0; t < T; ++t) {
        double yt[PGAS_MAX_NY];
#pragma unroll
        for (int k = 0; k < PGAS_MAX_NY; ++k) yt[k] = yn[k];
        {
            const int tn = t + 1 < T ? t + 1 : t;
#pragma unroll
            for (int k = 0; k < PGAS_MAX_NY; ++k) yn[k] = k < ny ? md.y[(size_t)tn * ny + k] : 0.0;
        }
        const double u1 = pgas_rng_uniform(seed, PGAS_STREAM_RESAMPLE, (uint32_t)t);

        // ---- 1. state
        if (t == 0) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int i = r * PG_BLK + tid, ic = i < N ? i : N - 1;
                if (r * PG_BLK + (tid & ~63) < N) {   // wave-uniform: register rows past N hold no particle
                    if (x0_mode == PG_ROLLOUT_X0_DRAWN) {
                        double z[2] = {0.0, 0.0};
                        pgas_rng_normals(seed, PGAS_STREAM_INIT, 0u, (uint64_t)ic, NX, z);
#pragma unroll
                        for (int k = 0; k < NX; ++k) {
                            double v = m0L0[k];
#pragma unroll
                            for (int l = 0; l <= k; ++l) v = PGAS_FMA(m0L0[NX + k * NX + l], z[l], v);
                            x[r][k] = v;
                        }
                    } else {
                        const size_t off = x0_mode == PG_ROLLOUT_X0_ONE ? 0 : x0_mode == PG_ROLLOUT_X0_DRAW ? draw * NX : (draw * (size_t)N + ic) * NX;
#pragma unroll
                        for (int k = 0; k < NX; ++k) x[r][k] = x0[off + k];
                    }
                }
            }
        } else {
            const double* __restrict__ ut = md.u + (size_t)t * md.nu;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int i = r * PG_BLK + tid, ic = i < N ? i : N - 1;
                if (r * PG_BLK + (tid & ~63) < N) {
                    double xin[1][NX], aux[1][NX];
#pragma unroll
                    for (int k = 0; k < NX; ++k) xin[0][k] = xs[anc[r] * NX + k];   // anc[r] < NR * 256: inside xs
                    eval_mean<NX, D, JIN, 1, J0T, true>(md, Guse, ut, xin, aux);
                    double z[2] = {0.0, 0.0};
                    pgas_rng_normals(seed, PGAS_STREAM_PROP, (uint32_t)t, (uint64_t)ic, NX, z);
#pragma unroll
                    for (int k = 0; k < NX; ++k) {
                        double v = aux[0][k];
#pragma unroll
                        for (int l = 0; l <= k; ++l) v = PGAS_FMA(LS[k * NX + l], z[l], v);
                        x[r][k] = v;
                    }
                }
            }
        }
        if (x_trace) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int i = r * PG_BLK + tid;
                if (i < N) {
#pragma unroll
                    for (int k = 0; k < NX; ++k) st_stream(&x_trace[(size_t)t * row + (size_t)i * NX + k], x[r][k]);
                }
            }
        }

        // ---- 2. particle log-likelihoods
        double lw[1][NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) lw[0][r] = r * PG_BLK + tid < N ? loglik<NX>(md, yt, x[r]) : ninf;

        // ---- 3. predictive channels: lane-local sums in ascending r, the wave's tree, lane 0 of the wave to LDS
        if (want_pred) {
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
                    red[wave][k] = s1;
                    red[wave][PG_RS_NV + k] = s2;
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
                        red[wave][NX + j] = s1;
                        red[wave][PG_RS_NV + NX + j] = s2;
                    }
                }
            }
        }

        // ---- 4. fixed-point scan (ends with a barrier: sm.num, sm.red and the predictive slots are visible)
        double S[1];
        small_scan<1, NR>(sm, lw, N, S);
        const bool valid = (S[0] > 0.0) && (S[0] < __builtin_inf());
        const double kref = filter_ref(sm);
        if (want_pred && tid < 2 * nv) {
            const int c = tid < nv ? tid : tid - nv, slot = tid < nv ? c : PG_RS_NV + c;
            double* __restrict__ dst = (tid < nv ? out.pred_sum : out.pred_sumsq) + (draw * T + t) * (size_t)nv + c;
            st_stream(dst, sum4(red, slot));
        }

        // ---- 5. evidence increment
        bool ynan = false;
#pragma unroll
        for (int j = 0; j < PGAS_MAX_NY; ++j) ynan = ynan || (j < ny && yt[j] != yt[j]);
        if (tid == 0) {
            const double e = filter_increment(ynan, kref, S[0], N);
            st_stream(&ell_out[t], e);
            if (!ynan) total = total + e;
        }

        // ---- 6. filtered channels
        if (want_w) {
            double w[NR];
            filter_weights<NR>(lw[0], kref, w);
            double sx[NX], sw = 0.0;
#pragma unroll
            for (int k = 0; k < NX; ++k) sx[k] = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const bool has = r * PG_BLK + tid < N;
                const double ww = w[r] * w[r];
                sw = has ? sw + ww : sw;
#pragma unroll
                for (int k = 0; k < NX; ++k) {
                    const double wx = w[r] * x[r][k];
                    sx[k] = has ? sx[k] + wx : sx[k];
                }
            }
            sw = wave_sum_tree(sw);
#pragma unroll
            for (int k = 0; k < NX; ++k) sx[k] = wave_sum_tree(sx[k]);
            if ((tid & 63) == 0) {
                red[wave][PG_FL_PRED + 2] = sw;
#pragma unroll
                for (int k = 0; k < NX; ++k) red[wave][PG_FL_PRED + k] = sx[k];
            }
        }

        // ---- 7. systematic resampling at every step; the owner publishes its state
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int i = r * PG_BLK + tid;
            int a = i;   // no positive weight, or no particle: identity
            if (valid && i < N) {
                const int p = small_lower_bound<NR * PG_BLK>(sm.num[0], slot_U(u1, i, N, invN, pow2) * S[0]);
                a = p > N - 1 ? N - 1 : p;
            }
            anc[r] = a;
            if (anc_trace && i < N) st_stream(&anc_trace[(size_t)t * N + i], (int32_t)a);
#pragma unroll
            for (int k = 0; k < NX; ++k) xs[i * NX + k] = x[r][k];
        }
        lds_barrier();   // B4: xs and the filtered slots are visible; sm.num / sm.red are free for the next step
        if (want_w) {
            const int slot = PG_FL_PRED + (tid < NX ? tid : 2);
            const double s = sum4(red, slot);
            if (want_filt && tid < NX) st_stream(&out.filt_sum[(draw * T + t) * (size_t)NX + tid], s);
            if (want_filt && tid == NX) st_stream(&out.wtot[draw * T + t], S[0]);
            if (out.ess && tid == NX + 1) st_stream(&out.ess[draw * T + t], valid ? (S[0] * S[0]) / s : 0.0);
        }
    }
    if (tid == 0) out.loglik[draw] = total;
}
