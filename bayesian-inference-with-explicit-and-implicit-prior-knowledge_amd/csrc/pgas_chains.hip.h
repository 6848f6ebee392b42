// pgas_chains.hip.h -- C independent PGAS chains of ONE model (one pgas_ctx) in batched launches: every launch below covers all
// chains, so a Gibbs iteration of C chains is a fixed number of launches whatever C is.
//
//   k_sweep_chains   the whole sweep of a chain in ONE workgroup (blockIdx.x = chain); the single-chain sweep of pgas_sweep under
//                    PGAS_OPT_SMALL_SWEEP = 2 is this kernel at C = 1 on the context's own buffers (contexts without a log-weight trace)
//   k_chains_pack    per chain: A (nx, M) -> coefficient tensor G, S (nx, nx) -> (LS, LS^-1, cS) -- k_pack's arithmetic
//   k_chains_begin   per chain: k_sweep_begin with the chain's seed read from device memory
//   k_chains_noise   the propagation noise of every (chain, t, particle), ahead of the sweep (pgas_sweep's small paths: C = 1)
//   k_chains_keys    the key handling of PGAS.__call__ (src/PGAS.py:356, :365, :377) and PGAS.param_draws per chain
//   k_chains_draws   the random numbers of PGAS.param_draws per chain: chi^2(df - i) (k_rng_chi2), (nx, nx) and (nx, M) normals (k_rng_normal)
// The sufficient statistics take the chain as grid dimension z of k_traj_basis / k_syrk_lds / k_syrk_reduce (pgas_suffstats.hip.h).
//
// Chains never wait for each other: no flag, counter or barrier crosses a workgroup, so the results do not depend on dispatch order or
// on how many workgroups are resident at once (C may exceed what the GPU holds).  Chain c's arrays are slice c of (C, ...) arrays.
#pragma once

#include "pgas_resample.hip.h"

#define PG_STREAM_SPLIT 16u          // pgas_amd/random.py: STREAM_SPLIT (key derivation: counter (i, 0, 0, STREAM_SPLIT))
#define PG_STREAM_PARAM_NORMAL 17u   //                     STREAM_PARAM_NORMAL
#define PG_STREAM_PARAM_UNIFORM 18u  //                     STREAM_PARAM_UNIFORM

// The WHOLE sweep (src/PGAS.py:176-228) of a chain with at most one segment of particles -- x_0, T - 1 steps, final index, back-trace --
// in ONE launch, one workgroup per chain; the one-segment arithmetic and the helpers are in pgas_resample.hip.h.
// per chain c: tpp[c], G + c gstride, swp[c], u_res / u_anc (C, T + 1), ref / traj (C, T, nx), x_trace (C, T, N, nx),
// anc_trace (C, max(T - 1, 1), N), logw_last (C, N), hdr[c], znoise (C, T, N, 2).  No log-weight trace: a context that keeps one
// (keep_logw_trace) sweeps with k_sweep_duo whatever PGAS_OPT_SMALL_SWEEP says -- the extra pointer cost the batched sweep 2 % at M = 729
// (profiles/one_small_sweep_ab.txt).
template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_sweep_chains(DevModel md, const TransParams* __restrict__ tp_all, const double* __restrict__ G_all,
                                                         int64_t gstride, const SweepParams* __restrict__ sp_all, const double* __restrict__ ures_all,
                                                         const double* __restrict__ uanc_all, const double* __restrict__ m0L0,
                                                         const double* __restrict__ ref_all, double* __restrict__ x_all, int32_t* __restrict__ anc_all,
                                                         double* __restrict__ logw_all, UpperHdr* __restrict__ hdr_all, double* __restrict__ traj_all,
                                                         const double* __restrict__ znoise_all) {
    __shared__ SmallSmem sm;
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_small[];   // the chain's coefficient tensor
    // chain blockIdx.x's slices
    const size_t chain = blockIdx.x, Nc = (size_t)md.N, Tc = (size_t)md.T, anc_rows = Tc > 1 ? Tc - 1 : 1;
    const TransParams* __restrict__ tpp = tp_all + chain;
    const double* __restrict__ G_arg = G_all + chain * (size_t)gstride;
    const SweepParams* __restrict__ swp = sp_all + chain;
    const double* __restrict__ u_res = ures_all + chain * (Tc + 1);
    const double* __restrict__ u_anc = uanc_all + chain * (Tc + 1);
    const double* __restrict__ ref = ref_all + chain * Tc * NX;
    double* __restrict__ x_trace = x_all + chain * Tc * Nc * NX;
    int32_t* __restrict__ anc_trace = anc_all + chain * anc_rows * Nc;
    double* __restrict__ logw_last = logw_all + chain * Nc;
    UpperHdr* __restrict__ hdr = hdr_all + chain;
    double* __restrict__ traj = traj_all + chain * Tc * NX;
    const double* __restrict__ znoise = znoise_all + chain * Tc * Nc * 2;
    // the sweep on these slices: the text k_sweep_records (pgas_records.hip.h) shares
#include "pgas_sweep_workgroup.inc"
}

// one thread per (chain, coefficient): G_c[pos[m]][k] = A_c[k][m] * nrm (the caller zeroes G first); the chain's first thread factors S_c
__global__ void k_chains_pack(int C, const double* __restrict__ A, const int32_t* __restrict__ pos, int M, int nx, double nrm, double* __restrict__ G,
                              int64_t gstride, const double* __restrict__ S, TransParams* __restrict__ tp_out) {
    const int64_t per = (int64_t)M * nx;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)C * per) return;
    const int64_t c = i / per, r = i % per;
    const int m = (int)(r / nx), k = (int)(r % nx);
    double* __restrict__ Gc = G + c * gstride;
    Gc[(int64_t)pos[m] * nx + k] = A[c * per + (int64_t)k * M + m] * nrm;
    if (r == 0) {
        TransParams tp{};
        tp_from_cov(nx, S + c * nx * nx, tp);
        tp.G = Gc;
        tp_out[c] = tp;
    }
}

// grid (ceil((T + 1) / 256), C)
__global__ void k_chains_begin(const uint64_t* __restrict__ seeds, int T, SweepParams* __restrict__ sp, double* __restrict__ u_res,
                               double* __restrict__ u_anc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t c = blockIdx.y;
    const uint64_t seed = seeds[c];
    if (t <= T) {
        u_res[c * (T + 1) + t] = pgas_rng_uniform(seed, PGAS_STREAM_RESAMPLE, (uint32_t)t);
        u_anc[c * (T + 1) + t] = pgas_rng_uniform(seed, PGAS_STREAM_ANCESTOR, (uint32_t)t);
    }
    if (t == 0) {
        sp[c].seed = seed;
        sp[c].epoch = 0;
        sp[c].pad = 0;
        sp[c].u_final = pgas_rng_uniform(seed, PGAS_STREAM_FINAL, 0u);
    }
}

// The propagation noise of whole sweeps (src/PGAS.py:72-75), one Philox block + Box-Muller pair per (chain, t, particle), written by a
// grid-wide launch BEFORE the one- and two-workgroup sweeps: generated by the lane that owns the particle, in sequence with everything
// else, it is two thirds of the step's latency chain at one wave per SIMD (6 700 of 10 200 cycles, measured); generated ahead by
// noise waves inside the workgroup, the waves got in each other's way (14.5 ms per sweep).  T x N x 16 bytes: 6.4 MB at N = 200.
// grid (ceil(N (T - 1) / 256), C)
__global__ __launch_bounds__(256) void k_chains_noise(const SweepParams* __restrict__ swp, int N, int T, double* __restrict__ znoise) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)N * (T - 1)) return;
    const size_t c = blockIdx.y;
    const int t = 1 + (int)(q / N), i = (int)(q % N);
    double z0, z1;
    pgas_normal_pair(pgas_rng_block(ld_const(&swp[c].seed), PGAS_STREAM_PROP, 0u, (uint32_t)t, (uint64_t)i), &z0, &z1);
    double* __restrict__ zc = znoise + c * (size_t)T * N * 2;
    zc[((size_t)t * N + i) * 2] = z0;
    zc[((size_t)t * N + i) * 2 + 1] = z1;
}

// child i of key k: pgas_amd.random.split(k, n)[i]
__device__ __forceinline__ uint64_t key_child(uint64_t k, uint32_t i) {
    const pgas_u32x4 w = pgas_philox4x32_10(i, 0u, 0u, PG_STREAM_SPLIT, (uint32_t)k, (uint32_t)(k >> 32));
    return (uint64_t)w.v[0] | ((uint64_t)w.v[1] << 32);
}

// out (6, C): next key, step key, parameter key, then the parameter key's (key_A, key_chi, key_norm) of PGAS.param_draws.
// first = 1: the start of PGAS.__call__, key, key_para = split(key) (:356; no step key: 0); first = 0: one Gibbs iteration,
// key, key_step = split(key) (:365), key, key_para = split(key) (:377).  out may alias keys.
__global__ void k_chains_keys(int C, const uint64_t* keys, int first, uint64_t* out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    uint64_t k = keys[c], ks = 0;
    if (!first) {
        ks = key_child(k, 1u);
        k = key_child(k, 0u);
    }
    const uint64_t kp = key_child(k, 1u);
    k = key_child(k, 0u);
    const uint64_t kS = key_child(kp, 1u);
    out[c] = k;
    out[(size_t)C + c] = ks;
    out[2 * (size_t)C + c] = kp;
    out[3 * (size_t)C + c] = key_child(kp, 0u);
    out[4 * (size_t)C + c] = key_child(kS, 0u);
    out[5 * (size_t)C + c] = key_child(kS, 1u);
}

// one thread per (chain, variate): slots j < nx chi^2(df - j) of key_chi, then nx * nx normals of key_norm, then nx * M normals of key_A --
// the counters, streams and arithmetic of k_rng_chi2 / k_rng_normal as PGAS.param_draws launches them
__global__ __launch_bounds__(256) void k_chains_draws(int C, int nx, int M, double df, const uint64_t* __restrict__ keys6, double* __restrict__ chi2,
                                                      double* __restrict__ normals_T, double* __restrict__ normals_A) {
    const int64_t per = (int64_t)nx + (int64_t)nx * nx + (int64_t)nx * M;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)C * per) return;
    const int64_t c = i / per, j = i % per;
    double z[2];
    if (j < nx) {
        const double nu = df - (double)j;
        chi2[c * nx + j] = 2.0 * pgas_rng_gamma(keys6[4 * (int64_t)C + c], PG_STREAM_PARAM_UNIFORM, 0u, (uint64_t)j, 0.5 * nu);
    } else if (j < nx + (int64_t)nx * nx) {
        const int64_t p = j - nx;
        pgas_rng_normals(keys6[5 * (int64_t)C + c], PG_STREAM_PARAM_NORMAL, 0u, (uint64_t)p, 1, z);
        normals_T[c * nx * nx + p] = z[0];
    } else {
        const int64_t p = j - nx - (int64_t)nx * nx;
        pgas_rng_normals(keys6[3 * (int64_t)C + c], PG_STREAM_PARAM_NORMAL, 0u, (uint64_t)p, 1, z);
        normals_A[c * nx * M + p] = z[0];
    }
}
