// pgas_marginal_chains.hip.h -- what is per CHAIN in C marginalised Particle-Gibbs chains run as one batch (src/Algorithm3.py, src/Algorithm2.py;
// pgas_amd/marginal_chains.py).  The particle axis is C N long, chain c at [c N, (c + 1) N); the per-particle kernels of
// pgas_marginal.hip.h serve it with global ancestor indices, the random numbers, the resampler and the weighted reduction are those of
// pgas_marginal_runs.hip.h.  The solve kernels and k_lbm_diff take a run length (per-run reference statistics); here are
//
//   k_runs_categorical   one categorical draw per run from softmax(logw[run]): the ancestor of the reference particle (src/Algorithm3.py:117-127)
//                        and the final index (:293-294), one workgroup per run, N <= 1024
//   k_runs_backtrace     reconstruct_trajectory (src/Filtering.py:40-55) of every run from traces (T, R, N, w): k_backtrace_idx with the run as
//                        the grid dimension and the final index read from device memory
//
// Runs never wait for each other: no flag, counter or barrier crosses a workgroup.
#pragma once

#include "pgas_marginal_runs.hip.h"

#define PG_CAT_THREADS 256
#define PG_CAT_PER 4   // consecutive particles per thread: 256 x 4 = 1024

// idx[run] = min(#{i < N : c_i < u S}, N - 1) with c the inclusive cumulative sum of e_i = pgas_exp(logw_i - max logw) and S = c_N-1, in this
// DEFINED order (tests/runs_categorical_numpy.py restates it):
//   thread t holds particles 4 t .. 4 t + 3 (e = +0.0 at i >= N); l_0 = e_4t, l_j = l_j-1 + e_4t+j, its total l_3;
//   the 256 totals are scanned inclusively by Kogge-Stone: for d = 1, 2, 4, ..., 128: v_t = v_t + v_t-d for t >= d (all t at once);
//   c_4t+j = l_j for t = 0 and v_t-1 + l_j beyond;  S = v_255;  the threshold is the ONE product u * S.
// A row that holds a NaN, or whose maximum is -inf or +inf (no softmax exists), gives N - 1: the reference particle keeps its own ancestor,
// as for a deterministic model (quirk Q15).  anc_local / anc_global (nullable, (R, N) int32): slot N - 1 of row `run` receives idx and
// run N + idx; no other slot is touched.
__global__ __launch_bounds__(PG_CAT_THREADS) void k_runs_categorical(int N, const double* __restrict__ logw_all, const double* __restrict__ u_all,
                                                                     int32_t* __restrict__ idx_out, int32_t* __restrict__ anc_local,
                                                                     int32_t* __restrict__ anc_global) {
    __shared__ double sv[2][PG_CAT_THREADS];
    __shared__ double smax[PG_CAT_THREADS / 64];
    __shared__ int scnt[PG_CAT_THREADS / 64];
    const size_t run = blockIdx.x, base = run * (size_t)N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double lw[PG_CAT_PER];
    double m = -__builtin_inf();
    int nan = 0;
#pragma unroll
    for (int j = 0; j < PG_CAT_PER; ++j) {
        const int i = PG_CAT_PER * tid + j;
        lw[j] = i < N ? logw_all[base + i] : -__builtin_inf();
        nan |= lw[j] != lw[j];
        m = lw[j] > m ? lw[j] : m;   // a NaN never replaces m; the row is refused below
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double other = __shfl_xor(m, o);
        m = other > m ? other : m;
    }
    if (lane == 0) smax[wave] = m;
    const int any_nan = __syncthreads_or(nan);   // also the barrier that publishes smax
    m = smax[0];
#pragma unroll
    for (int w = 1; w < PG_CAT_THREADS / 64; ++w) m = smax[w] > m ? smax[w] : m;
    int32_t pick = N - 1;
    if (!any_nan && m > -__builtin_inf() && m < __builtin_inf()) {   // block-uniform
        double l[PG_CAT_PER];
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < PG_CAT_PER; ++j) {
            const int i = PG_CAT_PER * tid + j;
            const double e = i < N ? pgas_exp(lw[j] - m) : 0.0;
            acc = j == 0 ? e : acc + e;
            l[j] = acc;
        }
        int cur = 0;
        sv[0][tid] = acc;
        __syncthreads();
#pragma unroll
        for (int d = 1; d < PG_CAT_THREADS; d <<= 1) {
            const double v = sv[cur][tid];
            sv[cur ^ 1][tid] = tid >= d ? v + sv[cur][tid - d] : v;
            cur ^= 1;
            __syncthreads();
        }
        const double S = sv[cur][PG_CAT_THREADS - 1];
        const double thr = u_all[run] * S;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < PG_CAT_PER; ++j) {
            const int i = PG_CAT_PER * tid + j;
            const double c = tid == 0 ? l[j] : sv[cur][tid - 1] + l[j];
            cnt += (i < N && c < thr) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) scnt[wave] = cnt;
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int w = 0; w < PG_CAT_THREADS / 64; ++w) total += scnt[w];
        pick = total < N - 1 ? total : N - 1;
    }
    if (tid == 0) {
        idx_out[run] = pick;
        if (anc_local) anc_local[base + (size_t)(N - 1)] = pick;
        if (anc_global) anc_global[base + (size_t)(N - 1)] = (int32_t)(base + (size_t)pick);
    }
}

// Run blockIdx.x: traj[run] (T, w) = the trajectory that ends in particle idx[run] of the last row, from x_trace (T, R, N, w) and anc_trace
// (T-1, R, N) holding every run's OWN indices: the two phases of k_backtrace (index chase into LDS, then a gather by all threads).  An index
// outside [0, N) -- only a caller's mistake can produce one -- is clamped, so that no load leaves the run's rows.
__global__ __launch_bounds__(PG_BT_THREADS) void k_runs_backtrace(int R, int N, int T, int w, const double* __restrict__ x_trace,
                                                                  const int32_t* __restrict__ anc_trace, const int32_t* __restrict__ idx,
                                                                  double* __restrict__ traj_all) {
    __shared__ int32_t rec[PG_BT_CHUNK];
    const size_t run = blockIdx.x;
    const pg_gi32p anc = (pg_gi32p)anc_trace;
    const pg_gf64p x = (pg_gf64p)x_trace;
    double* __restrict__ traj = traj_all + run * (size_t)T * w;
    const bool vec2 = w == 2 && (((uintptr_t)traj_all | (uintptr_t)x_trace) & 15) == 0;
    int32_t b = idx[run];
    b = b < 0 ? 0 : (b > N - 1 ? N - 1 : b);
    auto anc_row = [&](int i) { return anc + ((size_t)i * R + run) * N; };
    bt_passes(T, w, (uint32_t)b, rec, traj, vec2,
              [&](int hi, int lo, uint32_t bb, int32_t* rc) { return bt_chase_rows(hi, lo, bb, rc, anc_row); },
              [&](int i, uint32_t bb) { return x + (((size_t)i * R + run) * N + bb) * w; });
}
