// pgas_marginal_runs.hip.h -- R independent RUNS of the marginalised filter (src/Algorithm1.py) in the launches of one.
// The per-particle kernels of pgas_marginal.hip.h batch over runs as they are: the particle axis is R N long and the ancestor indices are
// global.  What is per RUN has its batched form here:
//
//   k_runs_rng_normal / _student_t / _uniform   the Philox streams of run r are keyed by keys[r]; particle i of run r draws from the counters of
//                                               particle i (k_rng_normal / k_rng_student_t / k_rng_uniform_dev with seed keys[r] and p0 = 0)
//   k_runs_systematic                           systematic resampling (src/Filtering.py:6-37) of R weight vectors, one workgroup per run
//                                               (blockIdx.x = run), N <= 1024: the one-segment CDF of the small sweeps
//   k_runs_weighted_stats_partial / _final      the weighted reduction of the statistics (pgas_marginal.hip.h: ws_column) with the run as a grid
//                                               dimension: chunks start at each run's first particle; pgas_m_weighted_stats_n is R = 1
//
// Runs never wait for each other: no flag, counter or barrier crosses a workgroup, so the results do not depend on dispatch order or on
// how many workgroups are resident at once (R may exceed what the GPU holds).  Run r's arrays are slice r of (R, N, ...) arrays.
#pragma once

#include "pgas_marginal.hip.h"
#include "pgas_resample.hip.h"

// keys (R) u64; out (R, N, ncol).  q = flat index over (run, particle): 64-bit, R N may pass 2^31
__global__ __launch_bounds__(256) void k_runs_rng_normal(const uint64_t* __restrict__ keys, uint32_t stream, uint32_t t, const uint32_t* __restrict__ t_dev,
                                                          int64_t total, int64_t N, int ncol, double* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    if (t_dev) t = *t_dev;
    const int64_t run = q / N, p = q - run * N;
    double z[8];
    pgas_rng_normals(keys[run], stream, t, (uint64_t)p, ncol, z);
    for (int k = 0; k < ncol; ++k) out[q * ncol + k] = z[k];
}

// nu (R, N) read at q, or -- nu_anc given -- nu0 + nu_scale * nu[nu_anc[q]] with nu_anc a GLOBAL index into the R N axis (k_rng_student_t's
// expression: df = P3 + lambda T3[a], BI:45)
__global__ __launch_bounds__(256) void k_runs_rng_student_t(const uint64_t* __restrict__ keys, uint32_t stream, uint32_t t, const uint32_t* __restrict__ t_dev,
                                                             int64_t total, int64_t N, const double* __restrict__ nu, double* __restrict__ out,
                                                             const int32_t* __restrict__ nu_anc, double nu0, double nu_scale) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    if (t_dev) t = *t_dev;
    const int64_t run = q / N, p = q - run * N;
    const double v = nu_anc ? nu0 + nu_scale * nu[nu_anc[q]] : nu[q];
    out[q] = pgas_rng_student_t(keys[run], stream, t, (uint64_t)p, v);
}

// out[r] = the uniform of (keys[r], stream, t): the u of run r's systematic resampling
__global__ __launch_bounds__(256) void k_runs_rng_uniform(const uint64_t* __restrict__ keys, uint32_t stream, uint32_t t, const uint32_t* __restrict__ t_dev,
                                                           int R, double* __restrict__ out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    out[r] = pgas_rng_uniform(keys[r], stream, t_dev ? *t_dev : t);
}

// Run blockIdx.x: idx_local[i] = #{k : num_k < (u + i) / N * S} min'ed with N - 1 against the fixed-point CDF of softmax(logw[run]) (one segment:
// num_k = c_k 2^-51, S = s 2^-51 -- small_scan, the arithmetic of the general search bit for bit); a run without a positive finite weight
// sum keeps the identity (src/Filtering.py:25).  idx_global (nullable) = run N + idx_local: what the gather kernels over the R N axis take.
// A threshold of exactly 0 (slot 0 under u = 0, which no Philox uniform is: they are odd multiples of 2^-53) gives N - 1: the general search
// (resample_search) settles a slot only where the carry in front of its source segment is strictly below the threshold and leaves the
// others at N - 1, and row r here is pgas_systematic_resample_dev's row for every u, that one included.
template <int NR>
__global__ __launch_bounds__(PG_BLK) void k_runs_systematic(int N, const double* __restrict__ u_all, const double* __restrict__ logw_all,
                                                            int32_t* __restrict__ idx_local, int32_t* __restrict__ idx_global) {
    __shared__ SmallSmem sm;
    const size_t run = blockIdx.x, base = run * (size_t)N;
    const int tid = threadIdx.x;   // particle i = r * 256 + tid, r < NR
    const bool pow2 = (N & (N - 1)) == 0;
    const double invN = 1.0 / (double)N;
    const double u1 = u_all[run];
    double lw[1][NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int i = r * PG_BLK + tid;
        lw[0][r] = i < N ? logw_all[base + i] : -__builtin_inf();
    }
    double S[1];
    small_scan<1, NR>(sm, lw, N, S);   // ends with a barrier: sm.num is visible
    const bool valid = (S[0] > 0.0) && (S[0] < __builtin_inf());
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int i = r * PG_BLK + tid;
        if (i < N) {
            int a = i;
            if (valid) {
                const double tau = slot_U(u1, i, N, invN, pow2) * S[0];
                const int p = small_lower_bound<NR * PG_BLK>(sm.num[0], tau);
                a = p > N - 1 ? N - 1 : p;
                if (!(0.0 < tau)) a = N - 1;   // u = 0: see above
            }
            idx_local[base + i] = (int32_t)a;
            if (idx_global) idx_global[base + i] = (int32_t)(base + (size_t)a);
        }
    }
}

// run blockIdx.z: particles [run n, (run + 1) n), chunk blockIdx.y of THAT range; partial (R, nchunk, ncol)
__global__ __launch_bounds__(256) void k_runs_weighted_stats_partial(int64_t n, int M, int nv, const double* __restrict__ w, const double* __restrict__ T0,
                                                                      const double* __restrict__ T1, const double* __restrict__ T2,
                                                                      const double* __restrict__ T3, double* __restrict__ partial) {
    const int ncol = M * M + M * nv + nv * nv + 1;
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int64_t first = (int64_t)blockIdx.z * n;
    const int64_t p0 = first + (int64_t)blockIdx.y * PG_WS_CHUNK;
    const int64_t p1 = p0 + PG_WS_CHUNK < first + n ? p0 + PG_WS_CHUNK : first + n;
    if (col >= ncol) return;
    double acc0 = 0.0, acc1 = 0.0;  // two chains: the loads of consecutive particles overlap
    int64_t p = p0;
    for (; p + 1 < p1; p += 2) {
        acc0 = PGAS_FMA(w[p], ws_column(col, M, nv, p, T0, T1, T2, T3), acc0);
        acc1 = PGAS_FMA(w[p + 1], ws_column(col, M, nv, p + 1, T0, T1, T2, T3), acc1);
    }
    if (p < p1) acc0 = PGAS_FMA(w[p], ws_column(col, M, nv, p, T0, T1, T2, T3), acc0);
    partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * ncol + col] = acc0 + acc1;
}

// run blockIdx.y: the chunks' partial sums added in index order -> S0 (R, M, nv), S1 (R, M, M), S2 (R, nv, nv), S3 (R)
__global__ __launch_bounds__(256) void k_runs_weighted_stats_final(int nchunk, int M, int nv, const double* __restrict__ partial_all, double* __restrict__ S0,
                                                                    double* __restrict__ S1, double* __restrict__ S2, double* __restrict__ S3) {
    const int mm = M * M, m0 = M * nv, m2 = nv * nv, ncol = mm + m0 + m2 + 1;
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= ncol) return;
    const size_t run = blockIdx.y;
    const double* __restrict__ partial = partial_all + run * (size_t)nchunk * ncol;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;   // four chains in a fixed interleaving: deterministic, and the loads overlap
    int c = 0;
    for (; c + 3 < nchunk; c += 4) {
        a0 += partial[(size_t)c * ncol + col];
        a1 += partial[(size_t)(c + 1) * ncol + col];
        a2 += partial[(size_t)(c + 2) * ncol + col];
        a3 += partial[(size_t)(c + 3) * ncol + col];
    }
    for (; c < nchunk; ++c) a0 += partial[(size_t)c * ncol + col];
    const double acc = (a0 + a1) + (a2 + a3);
    if (col < mm) S1[run * mm + col] = acc;
    else if (col < mm + m0) S0[run * m0 + (col - mm)] = acc;
    else if (col < mm + m0 + m2) S2[run * m2 + (col - mm - m0)] = acc;
    else S3[run] = acc;
}
