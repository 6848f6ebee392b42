// pgas_smooth.hip.h -- the smoothing distribution p(x_{0:T-1} | y_{0:T-1}, A_k, S_k) by backward simulation (FFBSi, Godsill, Doucet and
// West 2004) over the particle trace pgas_filter stored, B trajectories of each of K draws in ONE launch.
//
//   k_smooth   one workgroup of 256 per draw (blockIdx.x = draw); the rows are walked from t = T - 1 down to 0
//
// Per row t, in this order:
//   A. every particle once, by the whole workgroup: l_i = loglik<NX>(y_t, x[k,t,i]) (+0.0 when y_t holds a NaN: the filter made that row
//      a pure prediction step) and, for t < T - 1, mu_i = eval_mean(x[k,t,i], u_{t+1}) -- k_filter's instantiation on the coefficient
//      tensor in LDS, the input row of the propagation x_{t+1} = A phi(x_t, u_{t+1}) + LS z.  Both go to LDS; all trajectories share them
//   B. every trajectory g = b0 + b, inside ONE wave (b = wave, wave + 4, ...), no workgroup barrier:
//        v_i = l_i (t = T - 1), l_i + h_i (t < T - 1), h_i = fma(-0.5, quad, cS) with propagate_particles' chain against xt_{t+1}
//        k = pgas_seg_ref(max v), q_i = dev_exp_q51_n(pgas_seg_arg(v_i, k)), integer inclusive cumsum c_i, total s, S = s 2^-51
//        u = pgas_u52 of words 0, 1 of pgas_rng_block(seed_k, PGAS_STREAM_SMOOTH, 0, t, particle = g); tau = u S (the wave's uniforms
//        of the row are formed before BA, one Philox block per lane, and read by readlane)
//        j_t = min(#{i < N : c_i 2^-51 < tau}, N - 1); when S is not in (0, inf): g mod N (t = T - 1), anc[k, t, j_{t+1}] (t < T - 1)
//        xt_t = x[k, t, j_t]
//      The sums are integers, so no bit depends on the layout: here lane L owns the R = ceil(N / 64) rounded up to 4, 8 or 16
//      consecutive particles L R .. L R + R - 1 (one wave scan of the lane totals, the count is a sum of lane-local counts)
//   C. moments over the call's trajectories: channels xt_j, then yhat_j = sum_k H[j,k] xt_k (fma chain from +0.0); sum and sum of
//      squares in the order of pgas_rollout_stats.hip.h levels 1-2 with one register row: value b at position b of the 256-position
//      tree (thread b reads trajectory b from LDS, whichever wave computed it), positions >= B hold +0.0
//
// LDS layout: particle i = L R + r sits at position r 64 + L of mu / lw, so that the lanes of a wave read consecutive words in B; in A
// thread tid of pass p owns position p 256 + tid (r = 4 p + wave, L = lane), so its writes are consecutive too.
//
// LDS hazards (BA the barrier after A, BM the one after B, BR the one after the wave partials of C; without sums BM alone):
//   mu, lw        written before BA of row t, read between BA and BM; next written after BM (and BR) of row t, before BA of row t - 1
//   xt[b], jt[b]  read (row t + 1) and then written (row t) by the ONE wave that owns b, between BA and BM; read by thread b after BM;
//                 next written after BA of row t - 1, which no wave passes before thread b has read
//   red           written after BM, read by wave 0 after BR; next written after BM of row t - 1, which wave 0 reaches after its reads
// Every wave reaches every barrier: the trip counts of the trajectory loop differ between waves, the barriers stand outside it.
// Row t - 1 of x is fetched into registers before B of row t.  The outputs leave through st_stream stores that nothing waits for.
#pragma once

#include "pgas_filter.hip.h"

struct SmoothOut {   // by value: the outputs of pgas_smooth, per draw k slice k of each; nullable as documented in include/pgas_hip.h
    int32_t* idx;    // (K, B, T) or NULL
    double* xs;      // (K, B, T, nx) or NULL
    double* sum;     // (K, T, nx + ny) or NULL
    double* sumsq;   // with sum
};

template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_smooth(DevModel md, const TransParams* __restrict__ tp_all, const double* __restrict__ G_all, int64_t gstride,
                                                   const uint64_t* __restrict__ seeds, const double* __restrict__ x_all, const int32_t* __restrict__ anc_all,
                                                   int B, int64_t b0, SmoothOut out) {
    constexpr int R = 4 * NR;                      // particles per lane in B
    __shared__ double mu[NX][NR * PG_BLK];         // transition means by position
    __shared__ double lw[NR * PG_BLK];             // observation log-densities by position
    __shared__ double xt[PG_BLK][NX];              // the trajectories' states of the row last drawn
    __shared__ int jt[PG_BLK];                     // ... and their indices
    __shared__ double red[PG_BLK / 64][2 * PG_RS_NV];
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_smooth[];   // the draw's coefficient tensor
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, N = md.N, T = md.T, ny = md.ny, nv = NX + ny;
    const double* __restrict__ G_arg = G_all + draw * (size_t)gstride;
    {
        int gtot = NX;
#pragma unroll
        for (int d = 0; d < D; ++d) gtot *= (d == D - 1 && D > 1) ? JIN : md.J[d];
        for (int i = tid; i < gtot; i += PG_BLK) pg_g_lds_smooth[i] = G_arg[i];
        lds_barrier();
    }
    const double* Guse = pg_g_lds_smooth;
    const uint64_t seed = ld_const(seeds + draw);
    double LSinv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) LSinv[q] = ld_const(&tp_all[draw].LSinv[q]);
    const double cS = ld_const(&tp_all[draw].cS);
    const double ninf = -__builtin_inf();
    const size_t row = (size_t)N * NX;
    const double* __restrict__ x_trace = x_all + draw * (size_t)T * row;
    const int32_t* __restrict__ anc_trace = anc_all + draw * (size_t)T * N;
    int32_t* __restrict__ idx_out = out.idx ? out.idx + draw * (size_t)B * T : nullptr;
    double* __restrict__ xs_out = out.xs ? out.xs + draw * (size_t)B * T * NX : nullptr;
    const bool want_sum = out.sum != nullptr;

    // A's particles of this thread: pass p owns position p 256 + tid, that is particle lane R + 4 p + wave (clamped for the loads)
    double xrow[NR][NX];
#pragma unroll
    for (int p = 0; p < NR; ++p) {
        const int i = lane * R + 4 * p + wave, ic = i < N ? i : N - 1;
#pragma unroll
        for (int k = 0; k < NX; ++k) xrow[p][k] = x_trace[(size_t)(T - 1) * row + (size_t)ic * NX + k];
    }

    for (int t = T - 1; t >= 0; --t) {
        const bool last = t == T - 1;
        // ---- A. l_i and mu_i of every particle, once
        const double* __restrict__ yt = md.y + (size_t)t * ny;
        bool ynan = false;
#pragma unroll
        for (int j = 0; j < PGAS_MAX_NY; ++j) ynan = ynan || (j < ny && yt[j] != yt[j]);
        const double* __restrict__ un = md.u + (size_t)(last ? t : t + 1) * md.nu;
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            if (4 * p + wave < N) {   // wave-uniform: lane 0's particle; a pass past N holds no particle
                const int pos = p * PG_BLK + tid;
                lw[pos] = ynan ? 0.0 : loglik<NX>(md, yt, xrow[p]);
                if (!last) {
                    double xin[1][NX], aux[1][NX];
#pragma unroll
                    for (int k = 0; k < NX; ++k) xin[0][k] = xrow[p][k];
                    eval_mean<NX, D, JIN, 1, J0T, true>(md, Guse, un, xin, aux);
#pragma unroll
                    for (int k = 0; k < NX; ++k) mu[k][pos] = aux[0][k];
                }
            }
        }
        // row t - 1 on its way while B runs
        if (t > 0) {
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                const int i = lane * R + 4 * p + wave, ic = i < N ? i : N - 1;
#pragma unroll
                for (int k = 0; k < NX; ++k) xrow[p][k] = x_trace[(size_t)(t - 1) * row + (size_t)ic * NX + k];
            }
        }
        // the row's uniforms of this wave's trajectories, one Philox block per lane: lane L forms the one of b = wave + 4 L (<= 64 per wave)
        double ulane;
        {
            const pgas_u32x4 wd = pgas_rng_block(seed, PGAS_STREAM_SMOOTH, 0u, (uint32_t)t, (uint64_t)(b0 + wave + (PG_BLK / 64) * lane));
            ulane = pgas_u52(wd.v[0], wd.v[1]);
        }
        lds_barrier();   // BA

        // ---- B. the trajectories of this wave
        {
            int bprev = -1;        // the trajectory whose state is still on its way from memory
            double pend[NX];
#pragma unroll
            for (int k = 0; k < NX; ++k) pend[k] = 0.0;
            for (int b = wave; b < B; b += PG_BLK / 64) {
                const int64_t g = b0 + b;
                double v[R];
                if (last) {
#pragma unroll
                    for (int r = 0; r < R; ++r) v[r] = (r < N && lane * R + r < N) ? lw[r * 64 + lane] : ninf;
                } else {
                    double xn[NX];
#pragma unroll
                    for (int k = 0; k < NX; ++k) xn[k] = xt[b][k];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        double val = ninf;
                        if (r < N) {   // uniform: position row r holds a particle (lane 0's)
                            double quad = 0.0;
#pragma unroll
                            for (int k = 0; k < NX; ++k) {
                                double w = 0.0;
#pragma unroll
                                for (int l = 0; l <= k; ++l) w = PGAS_FMA(LSinv[k * NX + l], xn[l] - mu[l][r * 64 + lane], w);
                                quad = PGAS_FMA(w, w, quad);
                            }
                            const double h = PGAS_FMA(-0.5, quad, cS);
                            val = lane * R + r < N ? lw[r * 64 + lane] + h : ninf;
                        }
                        v[r] = val;
                    }
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
                const uint64_t s = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(incl >> 32), 63) << 32) |
                                   (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)incl, 63);
                const double S = pgas_u64_to_double(s) * PGAS_FIX_INV;
                const bool valid = (S > 0.0) && (S < __builtin_inf());
                const double tau = readlane_f64(ulane, (b - wave) / (PG_BLK / 64)) * S;
                int cnt = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) cnt += (lane * R + r < N && pgas_u64_to_double(base + q[r]) * PGAS_FIX_INV < tau) ? 1 : 0;
                int j = wave_sum_i(cnt);
                j = j > N - 1 ? N - 1 : j;
                if (!valid) j = last ? (int)(g % (int64_t)N) : (int)anc_trace[(size_t)t * N + jt[b]];   // jt[b] < N: an index this wave drew at row t + 1
                j = j < 0 ? 0 : (j > N - 1 ? N - 1 : j);   // a trace that is not the filter's must not lead outside row t
                j = __builtin_amdgcn_readfirstlane(j);
                // the state drawn one trajectory ago has arrived by now
                if (bprev >= 0 && lane == 0) {
#pragma unroll
                    for (int k = 0; k < NX; ++k) xt[bprev][k] = pend[k];
                    if (xs_out) {
#pragma unroll
                        for (int k = 0; k < NX; ++k) st_stream(&xs_out[((size_t)bprev * T + t) * NX + k], pend[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < NX; ++k) pend[k] = x_trace[(size_t)t * row + (size_t)j * NX + k];   // 0 <= j < N
                if (lane == 0) {
                    jt[b] = j;
                    if (idx_out) st_stream(&idx_out[(size_t)b * T + t], (int32_t)j);
                }
                bprev = b;
            }
            if (bprev >= 0 && lane == 0) {
#pragma unroll
                for (int k = 0; k < NX; ++k) xt[bprev][k] = pend[k];
                if (xs_out) {
#pragma unroll
                    for (int k = 0; k < NX; ++k) st_stream(&xs_out[((size_t)bprev * T + t) * NX + k], pend[k]);
                }
            }
        }
        lds_barrier();   // BM

        // ---- C. moments over the trajectories: thread b holds trajectory b
        if (want_sum) {
            const bool has = tid < B;
            double xv[NX];
#pragma unroll
            for (int k = 0; k < NX; ++k) xv[k] = has ? xt[tid][k] : 0.0;
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                double s1 = 0.0, s2 = 0.0;
                const double val = xv[k], vv = val * val;
                s1 = has ? s1 + val : s1;
                s2 = has ? s2 + vv : s2;
                s1 = wave_sum_tree(s1);
                s2 = wave_sum_tree(s2);
                if (lane == 0) {
                    red[wave][k] = s1;
                    red[wave][PG_RS_NV + k] = s2;
                }
            }
#pragma unroll
            for (int j = 0; j < PGAS_MAX_NY; ++j) {
                if (j < ny) {
                    double s1 = 0.0, s2 = 0.0, acc = 0.0;
#pragma unroll
                    for (int k = 0; k < NX; ++k) acc = PGAS_FMA(md.H[j * NX + k], xv[k], acc);
                    const double vv = acc * acc;
                    s1 = has ? s1 + acc : s1;
                    s2 = has ? s2 + vv : s2;
                    s1 = wave_sum_tree(s1);
                    s2 = wave_sum_tree(s2);
                    if (lane == 0) {
                        red[wave][NX + j] = s1;
                        red[wave][PG_RS_NV + NX + j] = s2;
                    }
                }
            }
            lds_barrier();   // BR
            if (tid < 2 * nv) {
                const int c = tid < nv ? tid : tid - nv, slot = tid < nv ? c : PG_RS_NV + c;
                double* __restrict__ dst = (tid < nv ? out.sum : out.sumsq) + (draw * T + t) * (size_t)nv + c;
                st_stream(dst, sum4(red, slot));
            }
        }
    }
}
