// pgas_marginal_smooth.hip.h -- the smoothing distribution of a GREY-BOX model, p(x_{0:T-1}, xi_{0:T-1} | y_{0:T-1}, A_k), by backward
// simulation (FFBSi) over the particle trace pgas_m_filter stored: B trajectories of each of K draws in ONE launch.
//
//   k_model_smooth<NR, NX>   one workgroup of 256 per draw (blockIdx.x = draw); the rows are walked from t = T - 1 down to 0
//
// The filter's particle is the pair (x_t, xi_t) and x_{t+1} = f(x_t, u_t, xi_t) + Qc z, so the backward kernel over the pair needs
// N(xt_{t+1}; f(x_t^i, u_t, xi_t^i), Q) alone: p(xi_{t+1} | x_{t+1}) is the same for every candidate i.  xi_t^i is a function of
// (x[k,t,i], u_t, A_k, Lrow_k, seed_k, i, t) -- what step 2 of the filter computed -- and is recomputed here, not stored.
//
// Per row t, in this order:
//   A. every particle once, by the whole workgroup, on the filter's register files: x[k,t,i] into the state registers, mr_intvars(t)
//      with the particle's own Philox index (t < T - 1, or when an interface output is asked for), mr_run(f) (t < T - 1; no noise, no
//      mr_advance), l_i = lw[k,t,i] (+0.0 when y_t holds a NaN) into LDS.  The traces fmean = f and xi leave here.
//   B. every trajectory g = b0 + b, inside ONE wave (b = wave, wave + 4, ...), no workgroup barrier:
//        v_i = l_i (t = T - 1), l_i + h_i (t < T - 1), h_i = cQ - 0.5 q, q = sum_j e_j e_j, e_j = sum_l (xt_{t+1,l} - f_{i,l}) LQinv[j,l],
//        ascending from 0.0, every product and sum rounded on its own (pgas_m_expr_eval mode 2's operations)
//        k = pgas_seg_ref(max v), q_i = dev_exp_q51_n(pgas_seg_arg(v_i, k)), integer inclusive cumsum c_i, total s, S = s 2^-51
//        u = pgas_u52 of words 0, 1 of pgas_rng_block(seed_k, PGAS_STREAM_M_SMOOTH, 0, t, particle = g); tau = u S (the wave's uniforms
//        of the row are formed before BA, one Philox block per lane, and read by readlane)
//        j_t = min(#{i < N : c_i 2^-51 < tau}, N - 1); when S is not in (0, inf): g mod N (t = T - 1), anc[k, t, j_{t+1}] (t < T - 1)
//        xt_t = x[k, t, j_t] and xit_t = xi_t^{j_t}: the chosen column's state and interface registers, read before the next row's A
//      k_smooth's sequence (pgas_smooth.hip.h).  The sums are integers, so no bit depends on the layout.
//   C. moments over the call's trajectories: channels xt_j, yhat[k, t, j_t]_j, and on their own xit_j; sum and sum of squares in
//      k_smooth's order: value b at position b of the 256-position tree (thread b holds trajectory b), positions >= B hold +0.0
//
// Layout.  F = ceil(N / 64) register files as k_model_filter's (same stride, park rows and coefficient rows: mr_prepare's sizes), but
// particle i = L F + r sits in file r, column L: lane L owns the F consecutive particles L F .. L F + F - 1, so B needs one wave scan of
// the lane totals per trajectory and reads f_i from its own column of every file.  mr_intvars takes the particle index as an argument, so
// the mapping costs nothing.  In A wave w of pass p owns file 4 p + w.  Columns past N repeat particle N - 1, weigh -inf and store nothing.
//
// LDS hazards (B0 the barrier after staging; BA the barrier after A, BM the one after B, BR the one after the wave partials of C;
// without moments BM alone):
//   coefficient rows, constants   written before B0, read-only afterwards
//   files (state, xi, f), lws     written by the owning wave before BA of row t; read by any wave between BA and BM (B) and by thread
//                                 b between BM and BR (C: the xi of its column); next written after BM (and BR) of row t
//   xt[b], jt[b]                  read (row t + 1) and then written (row t) by the ONE wave that owns b, between BA and BM; read by thread
//                                 b after BM; next written after BA of row t - 1, which no wave passes before thread b has read
//   red                           written after BM, read by waves 0 and 1 after BR; next written after BM of row t - 1, which both reach
//                                 after their reads
// Every wave reaches every barrier: a wave without a file skips the model only, and the trip counts of the trajectory loop differ between
// waves, but the barriers stand outside both.  The outputs leave through st_stream stores that nothing waits for.  No private array is
// indexed at run time: LQinv comes from the kernel arguments (padded to 8 x 8; with NX > 0 into registers, once), xt_{t+1} and f from LDS.
#pragma once

#include "pgas_smooth.hip.h"
#include "pgas_marginal_filter.hip.h"

#define PG_MS_MAXXI 16                              // interface components an interface output can have
#define PG_MS_NV (PG_MF_NV + PG_MS_MAXXI)           // value channels: x (<= 8), yhat (<= 8), xi (<= 16)

struct MsArgs {   // by value: what the smoother needs beside MrArgs; nullable outputs as documented in include/pgas_marginal.h
    const double* x;      // (K, T, N, nx): pgas_m_filter's traces
    const int32_t* anc;   // (K, T, N)
    const double* lw;     // (K, T, N)
    const double* yhat;   // (K, T, N, ny)
    const double* y;      // (T, ny)
    double cQ;
    double LQinv[PG_EX_MAXOUT * PG_EX_MAXOUT];   // row j at [j * 8], zero beyond nx
    int32_t B, nxi;
    int64_t b0;
    int32_t* idx;         // (K, B, T) or NULL
    double* xs;           // (K, B, T, nx) or NULL
    double* xis;          // (K, B, T, nxi) or NULL
    double* sum;          // (K, T, nx + ny) or NULL
    double* sumsq;        // with sum
    double* xi_sum;       // (K, T, nxi) or NULL
    double* xi_sumsq;     // with xi_sum
    double* fmean;        // (K, T, N, nx) or NULL; rows 0 .. T - 2
    double* xi;           // (K, T, N, nxi) or NULL
};

// NX: the state dimension as a constant (1 .. 4: LQinv and the result registers of f sit in registers, the chains of B have no guards), or 0:
// any nx <= 8, read at run time.  The operations and their order are the same.
template <int NR, int NX>
__global__ __launch_bounds__(PG_BLK) void k_model_smooth(MrArgs a, MsArgs s) {
    constexpr int R = 4 * NR;                      // particles per lane in B, at most
    constexpr int NXB = NX ? NX : PG_EX_MAXOUT;    // the bound of the unrolled loops over state components
    __shared__ double lws[NR * PG_BLK];            // l by position: file r, column L at r 64 + L
    __shared__ double xt[PG_BLK][PG_EX_MAXOUT];    // the trajectories' states of the row last drawn
    __shared__ int jt[PG_BLK];                     // ... and their indices
    __shared__ double red[PG_BLK / 64][2 * PG_MS_NV];
    extern __shared__ __attribute__((aligned(16))) double pg_ms_lds[];
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, N = a.P, nx = NX ? NX : a.nx, nu = a.nu, ny = a.ny, nv = nx + ny, nxi = s.nxi, B = s.B;
    const int F = (N + 63) >> 6;                   // register files: lane L owns particles L F .. L F + F - 1
    const int fstride = (a.nreg + a.nz) * 64, park = a.nreg * 64;   // doubles per file; where its park rows start
    double* __restrict__ Al = pg_ms_lds + (size_t)F * fstride;
    const uint64_t seed = ld_const(a.seeds + draw);
    const int64_t b0 = s.b0;
    const double ninf = -__builtin_inf(), cQ = s.cQ;
    const double* __restrict__ x_trace = s.x + draw * (size_t)T * N * nx;
    const int32_t* __restrict__ anc_trace = s.anc + draw * (size_t)T * N;
    const double* __restrict__ l_trace = s.lw + draw * (size_t)T * N;
    const double* __restrict__ y_trace = s.yhat + draw * (size_t)T * N * ny;
    int32_t* __restrict__ idx_out = s.idx ? s.idx + draw * (size_t)B * T : nullptr;
    double* __restrict__ xs_out = s.xs ? s.xs + draw * (size_t)B * T * nx : nullptr;
    double* __restrict__ xis_out = s.xis ? s.xis + draw * (size_t)B * T * nxi : nullptr;
    double* __restrict__ f_out = s.fmean ? s.fmean + draw * (size_t)T * N * nx : nullptr;
    double* __restrict__ xi_out = s.xi ? s.xi + draw * (size_t)T * N * nxi : nullptr;
    const bool want_sum = s.sum != nullptr, want_xisum = s.xi_sum != nullptr;
    const bool want_xi = xis_out != nullptr || want_xisum || xi_out != nullptr;

    // ---- once: the draw's coefficient rows (the whole workgroup), then per file the constant pool
    for (int i = 0; i < a.L; ++i) {
        const int cnt = a.lat[i].n * a.lat[i].M;
        const double* __restrict__ src = a.lat[i].A + draw * (size_t)cnt;
        for (int e = tid; e < cnt; e += PG_BLK) Al[a.lat[i].a_off + e] = src[e];
    }
#pragma unroll 1
    for (int p = 0; p < NR; ++p) {
        if (p * 4 + wave >= F) continue;   // wave-uniform: no file
        double* __restrict__ rl = pg_ms_lds + (size_t)(p * 4 + wave) * fstride + lane;
        for (int j = 0; j < a.nconst; ++j) rl[(a.n_in + j) * 64] = ld_const(a.consts + j);
    }
    lds_barrier();   // B0
    double LQ[NXB * NXB];                          // NX > 0: LQinv and f's result registers, once; NX = 0: not used
    int fo[NXB];
    if constexpr (NX > 0) {
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            fo[j] = a.f_out[j] * 64;
#pragma unroll
            for (int c = 0; c < NX; ++c) LQ[j * NX + c] = s.LQinv[j * PG_EX_MAXOUT + c];
        }
    }

    for (int t = T - 1; t >= 0; --t) {
        const bool last = t == T - 1;
        // ---- A. x_t, xi_t, f and l_i of every particle, once
        const double* __restrict__ yt = s.y + (size_t)t * ny;
        bool ynan = false;
        for (int j = 0; j < ny; ++j) {
            const double v = ld_const(yt + j);
            ynan = ynan || v != v;
        }
#pragma unroll 1
        for (int p = 0; p < NR; ++p) {
            const int f = p * 4 + wave;
            if (f >= F) continue;   // wave-uniform: no file
            const int i = lane * F + f;
            const bool live = i < N;
            const int pc = live ? i : N - 1;
            double* __restrict__ rl = pg_ms_lds + (size_t)f * fstride + lane;
            double* __restrict__ zl = rl + park;
            for (int k = 0; k < nx; ++k) rl[k * 64] = x_trace[((size_t)t * N + pc) * nx + k];
            lws[f * 64 + lane] = ynan ? 0.0 : l_trace[(size_t)t * N + pc];
            if (!last || want_xi) {
                mr_intvars(a, draw, seed, (uint64_t)pc, t, rl, zl, Al);
                if (xi_out && live)
                    for (int j = 0; j < nxi; ++j) st_stream(&xi_out[((size_t)t * N + i) * nxi + j], rl[(nx + nu + j) * 64]);
            }
            if (!last) {
                mr_run(rl, a.fcode, a.f_ninstr);
                if (f_out && live)
                    for (int k = 0; k < nx; ++k) st_stream(&f_out[((size_t)t * N + i) * nx + k], rl[a.f_out[k] * 64]);
            }
        }
        // the row's uniforms of this wave's trajectories, one Philox block per lane: lane L forms the one of b = wave + 4 L (<= 64 per wave)
        double ulane;
        {
            const pgas_u32x4 wd = pgas_rng_block(seed, PGAS_STREAM_M_SMOOTH, 0u, (uint32_t)t, (uint64_t)(b0 + wave + (PG_BLK / 64) * lane));
            ulane = pgas_u52(wd.v[0], wd.v[1]);
        }
        lds_barrier();   // BA

        // ---- B. the trajectories of this wave
        for (int b = wave; b < B; b += PG_BLK / 64) {
            const int64_t g = b0 + b;
            double xn[NXB];
#pragma unroll
            for (int l = 0; l < NXB; ++l) xn[l] = (!last && l < nx) ? xt[b][l] : 0.0;
            double v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double val = ninf;
                if (r < F) {   // uniform: file r exists
                    const double* __restrict__ fl = pg_ms_lds + (size_t)r * fstride + lane;
                    const bool has = lane * F + r < N;
                    const double l = lws[r * 64 + lane];
                    if (last) {
                        val = has ? l : ninf;
                    } else {
                        double d[NXB];
#pragma unroll
                        for (int c = 0; c < NXB; ++c) d[c] = c < nx ? xn[c] - fl[NX ? fo[c] : a.f_out[c] * 64] : 0.0;
                        double q = 0.0;
#pragma unroll
                        for (int j = 0; j < NXB; ++j) {
                            if (j < nx) {
                                double e = 0.0;
#pragma unroll
                                for (int c = 0; c < NXB; ++c)
                                    if (c < nx) e += d[c] * (NX ? LQ[j * NXB + c] : s.LQinv[j * PG_EX_MAXOUT + c]);
                                q += e * e;
                            }
                        }
                        const double h = cQ - 0.5 * q;
                        val = has ? l + h : ninf;
                    }
                }
                v[r] = val;
            }
            double m = ninf;
#pragma unroll
            for (int r = 0; r < R; ++r) m = __builtin_fmax(m, v[r]);
            m = wave_max(m);
            const double kref = pgas_seg_ref(m);
            double arg[R];
            uint64_t q[R];
#pragma unroll
            for (int r = 0; r < R; ++r) arg[r] = pgas_seg_arg(v[r], kref);
            dev_exp_q51_n<R>(arg, q);
            uint64_t run = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                run += q[r];
                q[r] = run;   // the lane's inclusive cumsum
            }
            const uint64_t incl = wave_incl_scan_u64(run);
            const uint64_t base = incl - run;
            const uint64_t tot = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(incl >> 32), 63) << 32) |
                                 (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)incl, 63);
            const double S = pgas_u64_to_double(tot) * PGAS_FIX_INV;
            const bool valid = (S > 0.0) && (S < __builtin_inf());
            const double tau = readlane_f64(ulane, (b - wave) / (PG_BLK / 64)) * S;
            int cnt = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) cnt += (r < F && lane * F + r < N && pgas_u64_to_double(base + q[r]) * PGAS_FIX_INV < tau) ? 1 : 0;
            int j = wave_sum_i(cnt);
            j = j > N - 1 ? N - 1 : j;
            if (!valid) j = last ? (int)(g % (int64_t)N) : (int)anc_trace[(size_t)t * N + jt[b]];   // jt[b] < N: an index this wave drew at row t + 1
            j = j < 0 ? 0 : (j > N - 1 ? N - 1 : j);   // a trace that is not the filter's must not lead outside row t
            j = __builtin_amdgcn_readfirstlane(j);
            // the chosen column: file j mod F, column j / F (< 64, since j < N <= 64 F); lane c < nx takes x_c, lane nx + c takes xi_c
            const double* __restrict__ col = pg_ms_lds + (size_t)(j % F) * fstride + j / F;
            if (lane < nx) {
                const double val = col[lane * 64];
                xt[b][lane] = val;
                if (xs_out) st_stream(&xs_out[((size_t)b * T + t) * nx + lane], val);
            } else if (xis_out && lane < nx + nxi) {
                st_stream(&xis_out[((size_t)b * T + t) * nxi + (lane - nx)], col[(nu + lane) * 64]);
            }
            if (lane == 0) {
                jt[b] = j;
                if (idx_out) st_stream(&idx_out[(size_t)b * T + t], (int32_t)j);
            }
        }
        lds_barrier();   // BM

        // ---- C. moments over the trajectories: thread b holds trajectory b
        if (want_sum || want_xisum) {
            const bool has = tid < B;
            const int jb = has ? jt[tid] : 0;
            if (want_sum) {
                for (int c = 0; c < nv; ++c) {
                    double s1 = 0.0, s2 = 0.0;
                    const double val = !has ? 0.0 : c < nx ? xt[tid][c] : y_trace[((size_t)t * N + jb) * ny + (c - nx)], vv = val * val;
                    s1 = has ? s1 + val : s1;
                    s2 = has ? s2 + vv : s2;
                    s1 = wave_sum_tree(s1);
                    s2 = wave_sum_tree(s2);
                    if (lane == 0) {
                        red[wave][c] = s1;
                        red[wave][PG_MS_NV + c] = s2;
                    }
                }
            }
            if (want_xisum) {
                const double* __restrict__ col = pg_ms_lds + (size_t)(jb % F) * fstride + jb / F;
                for (int c = 0; c < nxi; ++c) {
                    double s1 = 0.0, s2 = 0.0;
                    const double val = has ? col[(nx + nu + c) * 64] : 0.0, vv = val * val;
                    s1 = has ? s1 + val : s1;
                    s2 = has ? s2 + vv : s2;
                    s1 = wave_sum_tree(s1);
                    s2 = wave_sum_tree(s2);
                    if (lane == 0) {
                        red[wave][PG_MF_NV + c] = s1;
                        red[wave][PG_MS_NV + PG_MF_NV + c] = s2;
                    }
                }
            }
            lds_barrier();   // BR
            if (want_sum && tid < 2 * nv) {
                const int c = tid < nv ? tid : tid - nv, slot = tid < nv ? c : PG_MS_NV + c;
                double* __restrict__ dst = (tid < nv ? s.sum : s.sumsq) + (draw * T + t) * (size_t)nv + c;
                st_stream(dst, sum4(red, slot));
            }
            if (want_xisum && tid >= 64 && tid < 64 + 2 * nxi) {
                const int e = tid - 64, c = e < nxi ? e : e - nxi, slot = (e < nxi ? 0 : PG_MS_NV) + PG_MF_NV + c;
                double* __restrict__ dst = (e < nxi ? s.xi_sum : s.xi_sumsq) + (draw * T + t) * (size_t)nxi + c;
                st_stream(dst, sum4(red, slot));
            }
        }
    }
}
