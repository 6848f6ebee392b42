// pgas_marginal_filter.hip.h -- a bootstrap particle filter per coefficient draw of a GREY-BOX model (traced physics f / g, learned
// xi_i = A_k,i phi_i) on a held-out record, K draws in ONE launch: the one-step-ahead predictive density
// p(y_t | y_{0:t-1}, A_k), its sum over t (the log marginal likelihood of the record) and the filtered state.
//
//   k_model_filter<NR>   one workgroup of 256 per draw (blockIdx.x = draw); particle i = r * 256 + tid, r < NR (small_scan's geometry)
//
// Per step t = 0 .. T-1 (ModelRollout's time convention: row t holds x_t, u_t, xi_t, y_t = g(x_t, u_t, xi_t)), in this order:
//   1. state     t = 0: x_0 by mr_begin's four x0 modes with P := N; t >= 1: the result of 9 at t - 1.  Row t of the trace x leaves here.
//   2. mr_intvars(t), mr_run(g): k_model_rollout_stats' two calls; trace yhat = g
//   3. l_i = cR - 0.5 |LRinv (y_t - g)|^2 with the operations of k_model_rollout_stats' log score; -inf for a slot without a particle
//   4. predictive channels (the unweighted cloud, before y_t is used): x_j, then g_j; S1 = sum v, S2 = sum (v * v) in k_filter's order --
//      lane-local ascending r from +0.0, wave_sum_tree, (w0 + w1) + (w2 + w3)
//   5. small_scan<1, NR>: k = pgas_seg_ref(max l), numerators q_i, integer cumsum c, S = s 2^-51; valid = 0 < S < inf
//   6. ell[t] = filter_ell(k, S, N); -inf when S == 0; NaN when y_t holds a NaN
//   7. filtered channels: w_i = q_i 2^-51; filt_sum_j = sum_i (w_i x_ij), wtot = S, ess = (S S) / sum_i (w_i w_i), 0 when not valid
//   8. a_t[i] = min(#{j : c_j 2^-51 < U_i S}, N - 1), U_i = slot_U(u, i), u = pgas_rng_uniform(seed_k, PGAS_STREAM_M_RESAMPLE, t);
//      identity when not valid (a NaN observation row is a pure prediction step)
//   9. (t < T - 1) slot i takes (x_t, xi_t) of particle a_t[i] -- xi_t is GATHERED, its noise is the ancestor's -- then
//      mr_advance<false>(t) with slot i's own normals (PGAS_STREAM_M_STATE, t + 1, particle i)
//  10. loglik = sum_t ell[t], ascending t from +0.0 over the rows whose y_t holds no NaN
// filter_ref, filter_increment, filter_weights and sum4 of 5 - 7 are k_filter's own code (pgas_filter.hip.h); the sums over w x stay here,
// their operands come from the LDS register files, and so do the three stores of 7 and the ancestor search of 8.
//
// Register files.  Every wave and row with a particle (i.e. every 64 consecutive particles) owns one register file laid out as
// k_model_rollout's: rl[reg * 64], then nz = max(nx, max n_i, ny, nx + sum n_i) park rows, stride 64.  There are ceil(N / 64) files,
// file (r * 4 + wave) for particle row r of a wave; the draw's coefficient rows follow the last file and are read by broadcast.  So
// mr_intvars, mr_run and mr_advance are called unchanged, once per row, wave-uniformly skipped for a row without particles.  Lanes past
// N inside the last file repeat particle N - 1 (as in k_model_rollout); they hold +0.0 in every sum, -inf as weight, the identity as
// ancestor, and store nothing.
//   dynamic LDS = ceil(N / 64) (nreg + nz) 512 B + 8 sum n_i M_i B;   static: SmallSmem and the reduction slots (about 41.5 KB)
//
// The gather.  The resampled particle reaches its new owner through LDS: (A) every slot reads the nx + sum n_i state and interface
// registers of its ancestor's column and writes them to its OWN park rows; one barrier; (B) every slot copies its park rows into its
// own registers.  No private array has a run-time index.
//
// LDS hazards (B0 the barrier after staging; B1..B3 the barriers of small_scan, B4 the one between the two phases of the gather;
// "own" = written and read by the same thread only):
//   coefficient rows          written before B0, read-only afterwards
//   constants                 own, written before B0
//   temporaries, input row    own (mr_intvars, mr_run, mr_advance of the owning wave)
//   state, interface regs     written by the owner after B4 of step t - 1 (phase B, mr_advance) and before B1 of step t (mr_intvars);
//                             read by ANY thread between B3 and B4 of step t (phase A); the owner reads them at any time
//   park rows                 own: normals before B1, the gathered pair between B3 and B4, read back and reused for normals after B4
//   sm.la                     own: l_i written before B1, read before B1 and after B3
//   red[][pred slots]         written before B1 of step t, read by wave 0 after B3; next written after B4
//   sm.red[0][]               written before B1, read (the maximum, for k and q_i) after B3; next written after B4
//   sm.num[0]                 written before B3, searched between B3 and B4; next written after B4 (and after B1, B2 of step t + 1)
//   red[][filt slots]         written between B3 and B4, read after B4; next written after B3 of step t + 1
// Every wave reaches every barrier: a wave or row without particles skips the model only.  Draws never wait for each other: no flag,
// counter or barrier crosses a workgroup, so K may exceed what the GPU holds.
#pragma once

#include "pgas_filter.hip.h"
#include "pgas_marginal_rollout.hip.h"

#define PG_MF_NV (2 * PG_EX_MAXOUT)                     // value channels: x (<= 8), yhat (<= 8)
#define PG_MF_PRED (2 * PG_MF_NV)                       // S1, S2 of each
#define PG_MF_SLOTS (PG_MF_PRED + PG_EX_MAXOUT + 1)     // + sum w x_j (<= 8), sum w w

struct MfArgs {   // by value: what the filter needs beside MrArgs; nullable outputs as documented in include/pgas_marginal.h
    const double* y;    // (T, ny)
    double cR;
    double LRinv[PG_EX_MAXOUT * PG_EX_MAXOUT];   // row-major ny x ny
    double* ell;        // (K, T)
    double* loglik;     // (K)
    double* ess;        // (K, T) or NULL
    double* pred_sum;   // (K, T, nx + ny) or NULL
    double* pred_sumsq; // with pred_sum
    double* filt_sum;   // (K, T, nx) or NULL
    double* wtot;       // with filt_sum
    double* x;          // (K, T, N, nx) or NULL
    int32_t* anc;       // (K, T, N) or NULL
    double* lw;         // (K, T, N) or NULL
    double* yhat;       // (K, T, N, ny) or NULL
};

template <int NR>
__global__ __launch_bounds__(PG_BLK) void k_model_filter(MrArgs a, MfArgs s) {
    __shared__ SmallSmem sm;
    __shared__ double red[PG_BLK / 64][PG_MF_SLOTS];
    extern __shared__ __attribute__((aligned(16))) double pg_mf_lds[];
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, N = a.P, nx = a.nx, nu = a.nu, ny = a.ny, nv = nx + ny, niv = a.n_in - nx - nu, ng = nx + niv;
    const int fstride = (a.nreg + a.nz) * 64, park = a.nreg * 64;   // doubles per file; where its park rows start
    double* __restrict__ Al = pg_mf_lds + (size_t)((N + 63) >> 6) * fstride;
    const uint64_t seed = ld_const(a.seeds + draw);
    const bool pow2 = (N & (N - 1)) == 0;
    const double invN = 1.0 / (double)N, ninf = -__builtin_inf();
    double* __restrict__ ell_out = s.ell + draw * (size_t)T;
    double* __restrict__ x_trace = s.x ? s.x + draw * (size_t)T * N * nx : nullptr;
    double* __restrict__ y_trace = s.yhat ? s.yhat + draw * (size_t)T * N * ny : nullptr;
    double* __restrict__ l_trace = s.lw ? s.lw + draw * (size_t)T * N : nullptr;
    int32_t* __restrict__ anc_trace = s.anc ? s.anc + draw * (size_t)T * N : nullptr;
    const bool want_pred = s.pred_sum != nullptr, want_filt = s.filt_sum != nullptr, want_w = want_filt || s.ess != nullptr;

    // ---- once: the draw's coefficient rows (the whole workgroup), then per file the constant pool and x_0 (mr_begin's statements)
    mr_stage_coeffs(a, draw, tid, Al);
#pragma unroll 1
    for (int r = 0; r < NR; ++r) {
        if (r * PG_BLK + wave * 64 >= N) continue;   // wave-uniform: no file
        const int i = r * PG_BLK + tid, pc = i < N ? i : N - 1;
        double* __restrict__ rl = pg_mf_lds + (size_t)(r * 4 + wave) * fstride + lane;
        double* __restrict__ zl = rl + park;
        for (int j = 0; j < a.nconst; ++j) rl[(a.n_in + j) * 64] = ld_const(a.consts + j);
        if (a.x0_mode == PG_MR_X0_DRAWN) {
            mr_normals(zl, seed, PGAS_STREAM_M_INIT_STATE, 0u, (uint64_t)pc, nx);
            for (int k = 0; k < nx; ++k) {
                double v = ld_const(a.m0L0 + k);
                for (int l = 0; l < nx; ++l) v += zl[l * 64] * ld_const(a.m0L0 + nx + k * nx + l);
                rl[k * 64] = v;
            }
        } else {
            const size_t off = a.x0_mode == PG_MR_X0_ONE ? 0 : a.x0_mode == PG_MR_X0_DRAW ? draw * nx : (draw * (size_t)N + pc) * nx;
            for (int k = 0; k < nx; ++k) rl[k * 64] = a.x0[off + k];
        }
    }
    lds_barrier();   // B0
    double total = 0.0;

    for (int t = 0; t < T; ++t) {
        const double* __restrict__ yt = s.y + (size_t)t * ny;
        const double u1 = pgas_rng_uniform(seed, PGAS_STREAM_M_RESAMPLE, (uint32_t)t);

        // ---- 1 - 3. per row: trace x_t, the interface variables, g, the particle's log-likelihood
#pragma unroll 1
        for (int r = 0; r < NR; ++r) {
            const int i = r * PG_BLK + tid;
            if (r * PG_BLK + wave * 64 >= N) {
                sm.la[i] = ninf;
                continue;
            }
            const bool live = i < N;
            const uint64_t particle = (uint64_t)(live ? i : N - 1);
            double* __restrict__ rl = pg_mf_lds + (size_t)(r * 4 + wave) * fstride + lane;
            double* __restrict__ zl = rl + park;
            if (x_trace && live)
                for (int k = 0; k < nx; ++k) st_stream(&x_trace[((size_t)t * N + i) * nx + k], rl[k * 64]);
            mr_intvars(a, draw, seed, particle, t, rl, zl, Al);
            mr_run(rl, a.gcode, a.g_ninstr);
            if (y_trace && live)
                for (int j = 0; j < ny; ++j) st_stream(&y_trace[((size_t)t * N + i) * ny + j], rl[a.g_out[j] * 64]);
            double q = 0.0;
            for (int j = 0; j < ny; ++j) {
                double e = 0.0;
                for (int l = 0; l < ny; ++l) e += (ld_const(yt + l) - rl[a.g_out[l] * 64]) * s.LRinv[j * ny + l];
                q += e * e;
            }
            const double ll = live ? s.cR - 0.5 * q : ninf;
            if (l_trace && live) st_stream(&l_trace[(size_t)t * N + i], ll);
            sm.la[i] = ll;
        }
        double lw[1][NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) lw[0][r] = sm.la[r * PG_BLK + tid];

        // ---- 4. predictive channels: lane-local sums in ascending r, the wave's tree, lane 0 of the wave to LDS
        if (want_pred) {
            for (int c = 0; c < nv; ++c) {
                const int reg = c < nx ? c : a.g_out[c - nx];
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    if (r * PG_BLK + wave * 64 < N) {
                        const bool has = r * PG_BLK + tid < N;
                        const double v = pg_mf_lds[(size_t)(r * 4 + wave) * fstride + reg * 64 + lane], vv = v * v;
                        s1 = has ? s1 + v : s1;
                        s2 = has ? s2 + vv : s2;
                    }
                }
                s1 = wave_sum_tree(s1);
                s2 = wave_sum_tree(s2);
                if (lane == 0) {
                    red[wave][c] = s1;
                    red[wave][PG_MF_NV + c] = s2;
                }
            }
        }

        // ---- 5. fixed-point scan (ends with a barrier: sm.num, sm.red and the predictive slots are visible)
        double S[1];
        small_scan<1, NR>(sm, lw, N, S);
        const bool valid = (S[0] > 0.0) && (S[0] < __builtin_inf());
        const double kref = filter_ref(sm);
        if (want_pred && tid < 2 * nv) {
            const int c = tid < nv ? tid : tid - nv, slot = tid < nv ? c : PG_MF_NV + c;
            double* __restrict__ dst = (tid < nv ? s.pred_sum : s.pred_sumsq) + (draw * T + t) * (size_t)nv + c;
            st_stream(dst, sum4(red, slot));
        }

        // ---- 6. evidence increment
        if (tid == 0) {
            bool ynan = false;
            for (int j = 0; j < ny; ++j) {
                const double v = ld_const(yt + j);
                ynan = ynan || v != v;
            }
            const double e = filter_increment(ynan, kref, S[0], N);
            st_stream(&ell_out[t], e);
            if (!ynan) total = total + e;
        }

        // ---- 7. filtered channels
        if (want_w) {
            double w[NR];
            filter_weights<NR>(lw[0], kref, w);
            double sw = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const double ww = w[r] * w[r];
                sw = r * PG_BLK + tid < N ? sw + ww : sw;
            }
            sw = wave_sum_tree(sw);
            if (lane == 0) red[wave][PG_MF_PRED + PG_EX_MAXOUT] = sw;
            for (int k = 0; k < nx; ++k) {
                double sx = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    if (r * PG_BLK + wave * 64 < N) {
                        const double wx = w[r] * pg_mf_lds[(size_t)(r * 4 + wave) * fstride + k * 64 + lane];
                        sx = r * PG_BLK + tid < N ? sx + wx : sx;
                    }
                }
                sx = wave_sum_tree(sx);
                if (lane == 0) red[wave][PG_MF_PRED + k] = sx;
            }
        }

        // ---- 8, 9A. systematic resampling at every step; the ancestor's (x_t, xi_t) into the slot's own park rows
#pragma unroll 1
        for (int r = 0; r < NR; ++r) {
            const int i = r * PG_BLK + tid;
            if (r * PG_BLK + wave * 64 >= N) continue;
            int an = i;   // no positive weight, or no particle: identity
            if (valid && i < N) {
                const int p = small_lower_bound<NR * PG_BLK>(sm.num[0], slot_U(u1, i, N, invN, pow2) * S[0]);
                an = p > N - 1 ? N - 1 : p;
            }
            if (anc_trace && i < N) st_stream(&anc_trace[(size_t)t * N + i], (int32_t)an);
            if (t < T - 1) {
                const double* __restrict__ src = pg_mf_lds + (size_t)(an >> 6) * fstride + (an & 63);   // an < N or an == i: a column of a file
                double* __restrict__ zl = pg_mf_lds + (size_t)(r * 4 + wave) * fstride + park + lane;
                for (int j = 0; j < ng; ++j) zl[j * 64] = src[(j < nx ? j : nu + j) * 64];
            }
        }
        lds_barrier();   // B4: every ancestor's registers have been read; the filtered slots are visible; sm.num / sm.red are free
        if (want_w) {
            const double f = sum4(red, PG_MF_PRED + (tid < nx ? tid : PG_EX_MAXOUT));
            if (want_filt && tid < nx) st_stream(&s.filt_sum[(draw * T + t) * (size_t)nx + tid], f);
            if (want_filt && tid == nx) st_stream(&s.wtot[draw * T + t], S[0]);
            if (s.ess && tid == nx + 1) st_stream(&s.ess[draw * T + t], valid ? (S[0] * S[0]) / f : 0.0);
        }
        if (t == T - 1) break;

        // ---- 9B. the gathered pair into the slot's registers, then x_t+1 = f(x_t, u_t, xi_t) [+ Qc z] with the slot's own normals
#pragma unroll 1
        for (int r = 0; r < NR; ++r) {
            const int i = r * PG_BLK + tid;
            if (r * PG_BLK + wave * 64 >= N) continue;
            double* __restrict__ rl = pg_mf_lds + (size_t)(r * 4 + wave) * fstride + lane;
            double* __restrict__ zl = rl + park;
            for (int j = 0; j < ng; ++j) rl[(j < nx ? j : nu + j) * 64] = zl[j * 64];
            mr_advance<false>(a, seed, (uint64_t)(i < N ? i : N - 1), t, rl, zl, nullptr, false);
        }
    }
    if (tid == 0) st_stream(&s.loglik[draw], total);
}
