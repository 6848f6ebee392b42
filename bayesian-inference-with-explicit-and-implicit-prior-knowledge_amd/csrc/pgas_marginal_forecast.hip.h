// pgas_marginal_forecast.hip.h -- h-step-ahead predictions of a GREY-BOX model (traced physics f / g, learned xi_i = A_k,i phi_i) from
// the particle trace of pgas_m_filter, every origin row of every coefficient draw in ONE launch:
// p(y_tau | y_{0:tau-h}, A_k) for h = 1 .. H, as predictive moments and as a log score.
//
//   k_model_forecast<NR>   grid (K, ceil(T / TB)): blockIdx.x = draw, blockIdx.y = chunk of TB origin rows; one workgroup of 256;
//                          particle i = 256 r + tid, r < NR (k_model_filter's geometry)
//
// Inputs per draw k: the trace x (K, T, N, nx) exactly as pgas_m_filter stores it, the draw's coefficient rows A_k,i [and Lrow_k,i], seed_k,
// the descriptor's programs and inputs, y, cR, LRinv.  Row s of the trace is stored BEFORE y_s is used: a sample of p(x_s | y_{0:s-1}).
// Time convention: ModelRollout's -- row t holds x_t, u_t, xi_t and y_t = g(x_t, u_t, xi_t).
//
// Per origin row s in [0, T) and lead l = 0 .. min(H, T - s) - 1 (target row tau = s + l, horizon h = l + 1); particle i < N has the Philox
// particle index pi(l, i) = ((uint64)l << 32) | i.  In this order:
//   1. cloud     l = 0: the state registers take x[k, s, i]; nothing is propagated.  l >= 1: mr_advance<false>(t = s + l - 1, particle =
//                pi(l, i)): process noise on PGAS_STREAM_M_STATE at time s + l with the lead in the high word of the particle counter --
//                disjoint from the filter's own counters (l = 0) and from every other (target row, lead, particle).  Then, at every lead,
//                mr_intvars(t = s + l, particle = pi(l, i)) and mr_run(g).  At l = 0, pi = i: xi_s and g are the ones slot i of the filter
//                formed at row s (with interface-variable noise the filter's own normals are reused), so the cloud at h = 1 is the
//                filter's.  mr_intvars, mr_run, mr_advance and mr_normals are called unchanged; no new stream id.  The noise depends on
//                (target row, lead, particle) alone: not on H, not on TB, not on which draws share a launch.
//   2. channels  x_j (j < nx), then g_j (j < ny), read from the register file after g has run: k_model_filter's step 4
//   3. moments   sum[k, l, tau, :] = sum_i v, sumsq = sum_i (v * v) (product rounded, then added) in k_model_filter's order: lane-local
//                ascending r from +0.0, wave_sum_tree, (w0 + w1) + (w2 + w3).  At l = 0 the operation sequence of its pred_sum / pred_sumsq.
//   4. log score (optional) l_i = cR - 0.5 sum_j e_j^2, e_j = sum_l (y_tau,l - g_l) * LRinv[j,l] from 0.0, every product and sum rounded
//                on its own: the statements of k_model_filter's step 3.  m = max l (fmax: a NaN takes no part); S = sum_i pgas_exp(l_i - m)
//                in the order of 3 (a NaN l adds +0.0); lpd[k, l, tau] = (m + pgas_log(S)) - pgas_log((double)N); -inf when S = 0; NaN
//                when y_tau holds a NaN (set explicitly)
//   5. the entries without an origin row (tau < l) are NaN in every output: written by the draw's chunk 0
//   6. optional clouds: cloud_x (K, H, T, N, nx), cloud_y (K, H, T, N, ny) hold the values of 2 per particle at [k, l, tau, i, :]
// Every defined entry (l, tau) belongs to origin tau - l alone, so it has one writer; no flag, counter, atomic or barrier crosses a
// workgroup, so K x chunks may exceed what the GPU holds.
//
// Register files: k_model_filter's.  Every 64 consecutive particles own one LDS file (file r * 4 + wave: rl[reg * 64], then nz park rows,
// stride 64); there are ceil(N / 64) files, the draw's coefficient rows follow the last one and are read by broadcast.  Lanes past N in the
// last file repeat particle N - 1, add +0.0 / -inf and store nothing.  After g has run, park row 0 of a file carries the particle's l
// until the thread has read it back (before the barrier of the same step).
//   dynamic LDS = ceil(N / 64) (nreg + nz) 512 B + 8 sum n_i M_i B,  nz = the filter's max(nx, max n_i, ny, nx + sum n_i);
//   static LDS  = the reduction slots, 2 x 4 x 34 doubles = 2176 B
//
// Barriers.  The origin range [s_lo, s_hi) and the lead-loop bound min(H, T - s) are workgroup-uniform (blockIdx and kernel arguments
// only), and a wave or row without particles skips the model only (wave-uniformly, no barrier inside), so every wave reaches every
// barrier: the one way this kernel could hang.  The steps of a workgroup (all leads of all its origins) are numbered n = 0, 1, ...;
// there is ONE barrier per step and one more after the last.
//
// LDS hazards (B0 the barrier after staging; slot set n & 1 of red; barrier n the one of step n; "own" = written and read by the same
// thread only):
//   coefficient rows         written before B0 by the whole workgroup, read-only afterwards
//   constants                own, written before B0
//   state, input, interface  own: no thread ever touches another thread's column (no scan, no search, no gather)
//   temporaries, park rows   own (mr_intvars, mr_run, mr_advance of the owning wave; l parked and read back by the same thread)
//   moment slots, max slot   written before barrier n, read after it (wave 0 the moments, every wave the maximum); next written before
//                            barrier n + 2, that is after barrier n + 1, which no wave passes before every wave has read step n
//   exp-sum slot             needs the maximum: written after barrier n, read after barrier n + 1 (by the thread that stores lpd of step
//                            n, whose maximum, target and NaN flag it kept in registers); next written after barrier n + 2
// The outputs leave through st_stream stores that nothing waits for.
#pragma once

#include "pgas_marginal_filter.hip.h"

#define PG_MFC_MAX (2 * PG_MF_NV)         // slot of the wave's maximum
#define PG_MFC_SLOTS (2 * PG_MF_NV + 2)   // S1, S2 of each value channel, the maximum, the exp sum

struct MfcArgs {   // by value: what the forecast needs beside MrArgs; nullable outputs as documented in include/pgas_marginal.h
    const double* x;     // (K, T, N, nx): pgas_m_filter's trace
    const double* y;     // (T, ny); read only when lpd != NULL
    double* sum;         // (K, H, T, nx + ny)
    double* sumsq;
    double* lpd;         // (K, H, T) or NULL
    double* cloud_x;     // (K, H, T, N, nx) or NULL
    double* cloud_y;     // (K, H, T, N, ny) or NULL
    int32_t H, TB;
    double cR;
    double LRinv[PG_EX_MAXOUT * PG_EX_MAXOUT];   // row-major ny x ny
};

template <int NR>
__global__ __launch_bounds__(PG_BLK) void k_model_forecast(MrArgs a, MfcArgs s) {
    __shared__ double red[2][PG_BLK / 64][PG_MFC_SLOTS];   // [step parity][wave][slot]
    extern __shared__ __attribute__((aligned(16))) double pg_mfc_lds[];
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, N = a.P, nx = a.nx, ny = a.ny, nv = nx + ny, Hz = s.H;
    const int s_lo = (int)blockIdx.y * s.TB, s_hi = s_lo + s.TB < T ? s_lo + s.TB : T;   // workgroup-uniform
    const int fstride = (a.nreg + a.nz) * 64, park = a.nreg * 64;   // doubles per file; where its park rows start
    double* __restrict__ Al = pg_mfc_lds + (size_t)((N + 63) >> 6) * fstride;
    const uint64_t seed = a.seeds != nullptr ? ld_const(a.seeds + draw) : 0ull;
    const bool score = s.lpd != nullptr;
    const double ninf = -__builtin_inf(), qnan = __builtin_nan("");
    const double* __restrict__ x_trace = s.x + draw * (size_t)T * N * nx;
    double* __restrict__ sum_out = s.sum + draw * (size_t)Hz * T * nv;       // (H, T, nv)
    double* __restrict__ sumsq_out = s.sumsq + draw * (size_t)Hz * T * nv;
    double* __restrict__ lpd_out = score ? s.lpd + draw * (size_t)Hz * T : nullptr;                    // (H, T)
    double* __restrict__ cx_out = s.cloud_x ? s.cloud_x + draw * (size_t)Hz * T * N * nx : nullptr;    // (H, T, N, nx)
    double* __restrict__ cy_out = s.cloud_y ? s.cloud_y + draw * (size_t)Hz * T * N * ny : nullptr;    // (H, T, N, ny)

    // ---- once: the draw's coefficient rows (the whole workgroup), then per file the constant pool
    mr_stage_coeffs(a, draw, tid, Al);
#pragma unroll 1
    for (int r = 0; r < NR; ++r) {
        if (r * PG_BLK + wave * 64 >= N) continue;   // wave-uniform: no file
        double* __restrict__ rl = pg_mfc_lds + (size_t)(r * 4 + wave) * fstride + lane;
        for (int j = 0; j < a.nconst; ++j) rl[(a.n_in + j) * 64] = ld_const(a.consts + j);
    }
    lds_barrier();   // B0

    // ---- 5. the entries no origin row reaches: rows tau = 0 .. l - 1 of horizon index l are contiguous in every output
    if (blockIdx.y == 0) {
        for (int l = 1; l < Hz; ++l) {
            for (int e = tid; e < l * nv; e += PG_BLK) {
                st_stream(&sum_out[(size_t)l * T * nv + e], qnan);
                st_stream(&sumsq_out[(size_t)l * T * nv + e], qnan);
            }
            if (score)
                for (int e = tid; e < l; e += PG_BLK) st_stream(&lpd_out[(size_t)l * T + e], qnan);
            if (cx_out)
                for (size_t e = tid; e < (size_t)l * N * nx; e += PG_BLK) st_stream(&cx_out[(size_t)l * T * N * nx + e], qnan);
            if (cy_out)
                for (size_t e = tid; e < (size_t)l * N * ny; e += PG_BLK) st_stream(&cy_out[(size_t)l * T * N * ny + e], qnan);
        }
    }

    int n = 0;                 // the workgroup's step counter: the slot set's parity
    double m_prev = ninf;      // step n - 1: its maximum, where its lpd goes, whether its observation row holds a NaN
    size_t lpd_prev = 0;
    bool ynan_prev = false;

    for (int so = s_lo; so < s_hi; ++so) {
        // ---- the origin's cloud: row so of the trace into the state registers
#pragma unroll 1
        for (int r = 0; r < NR; ++r) {
            if (r * PG_BLK + wave * 64 >= N) continue;
            const int i = r * PG_BLK + tid, pc = i < N ? i : N - 1;
            double* __restrict__ rl = pg_mfc_lds + (size_t)(r * 4 + wave) * fstride + lane;
            for (int k = 0; k < nx; ++k) rl[k * 64] = x_trace[((size_t)so * N + pc) * nx + k];
        }
        const int L = Hz < T - so ? Hz : T - so;   // workgroup-uniform
        for (int l = 0; l < L; ++l, ++n) {
            const int par = n & 1, t = so + l;
            const size_t row = (size_t)l * T + t;   // (horizon index, target row)
            const double* __restrict__ yt = score ? s.y + (size_t)t * ny : nullptr;

            // ---- 1., 6. per row: the propagation, the interface variables, g; the particle's log-likelihood into park row 0
#pragma unroll 1
            for (int r = 0; r < NR; ++r) {
                if (r * PG_BLK + wave * 64 >= N) continue;
                const int i = r * PG_BLK + tid;
                const bool live = i < N;
                const uint64_t particle = ((uint64_t)l << 32) | (uint64_t)(live ? i : N - 1);
                double* __restrict__ rl = pg_mfc_lds + (size_t)(r * 4 + wave) * fstride + lane;
                double* __restrict__ zl = rl + park;
                if (l > 0) mr_advance<false>(a, seed, particle, t - 1, rl, zl, nullptr, false);
                mr_intvars(a, draw, seed, particle, t, rl, zl, Al);
                mr_run(rl, a.gcode, a.g_ninstr);
                if (cx_out && live)
                    for (int k = 0; k < nx; ++k) st_stream(&cx_out[(row * N + i) * nx + k], rl[k * 64]);
                if (cy_out && live)
                    for (int j = 0; j < ny; ++j) st_stream(&cy_out[(row * N + i) * ny + j], rl[a.g_out[j] * 64]);
                if (score) {
                    double q = 0.0;
                    for (int j = 0; j < ny; ++j) {
                        double e = 0.0;
                        for (int c = 0; c < ny; ++c) e += (ld_const(yt + c) - rl[a.g_out[c] * 64]) * s.LRinv[j * ny + c];
                        q += e * e;
                    }
                    zl[0] = live ? s.cR - 0.5 * q : ninf;
                }
            }

            // ---- 2., 3. the channels, one at a time: lane-local sums in ascending r, the wave's tree, lane 0 of the wave to LDS
            for (int c = 0; c < nv; ++c) {
                const int reg = c < nx ? c : a.g_out[c - nx];
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    if (r * PG_BLK + wave * 64 < N) {
                        const bool has = r * PG_BLK + tid < N;
                        const double v = pg_mfc_lds[(size_t)(r * 4 + wave) * fstride + reg * 64 + lane], vv = v * v;
                        s1 = has ? s1 + v : s1;
                        s2 = has ? s2 + vv : s2;
                    }
                }
                s1 = wave_sum_tree(s1);
                s2 = wave_sum_tree(s2);
                if (lane == 0) {
                    red[par][wave][c] = s1;
                    red[par][wave][PG_MF_NV + c] = s2;
                }
            }

            // ---- 4. log score: the wave's maximum before the barrier
            double lcur[NR];
            bool ynan = false;
            if (score) {
                for (int j = 0; j < ny; ++j) {
                    const double v = ld_const(yt + j);
                    ynan = ynan || v != v;
                }
                double m = ninf;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    lcur[r] = ninf;
                    if (r * PG_BLK + wave * 64 < N) lcur[r] = pg_mfc_lds[(size_t)(r * 4 + wave) * fstride + park + lane];
                    m = __builtin_fmax(m, lcur[r]);   // NaN takes no part
                }
                m = wave_max(m);
                if (lane == 0) red[par][wave][PG_MFC_MAX] = m;
            }
            lds_barrier();   // barrier n

            // ---- after the barrier: wave 0 sends the step's moments on their way; every wave needs the maximum
            if (tid < 2 * nv) {
                const int c = tid < nv ? tid : tid - nv, slot = tid < nv ? c : PG_MF_NV + c;
                double* __restrict__ dst = (tid < nv ? sum_out : sumsq_out) + row * nv + c;
                st_stream(dst, (red[par][0][slot] + red[par][1][slot]) + (red[par][2][slot] + red[par][3][slot]));
            }
            if (score) {
                if (n > 0 && tid == 2 * nv) {   // lpd of step n - 1: its exp sums were written after barrier n - 1
                    const int q = par ^ 1, slot = PG_MFC_MAX + 1;
                    const double S = (red[q][0][slot] + red[q][1][slot]) + (red[q][2][slot] + red[q][3][slot]);
                    const double v = S == 0.0 ? ninf : (m_prev + pgas_log(S)) - pgas_log((double)N);
                    st_stream(&lpd_out[lpd_prev], ynan_prev ? qnan : v);
                }
                const int slot = PG_MFC_MAX;
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
                if (lane == 0) red[par][wave][PG_MFC_MAX + 1] = sx;
                m_prev = mb;
                lpd_prev = row;
                ynan_prev = ynan;
            }
        }
    }
    if (score) {   // the last step's lpd (every workgroup has at least one step: s_lo < T and L >= 1)
        lds_barrier();
        if (tid == 2 * nv) {
            const int q = (n - 1) & 1, slot = PG_MFC_MAX + 1;
            const double S = (red[q][0][slot] + red[q][1][slot]) + (red[q][2][slot] + red[q][3][slot]);
            const double v = S == 0.0 ? ninf : (m_prev + pgas_log(S)) - pgas_log((double)N);
            st_stream(&lpd_out[lpd_prev], ynan_prev ? qnan : v);
        }
    }
}
