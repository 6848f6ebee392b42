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
    const int tid = threadIdx.x;
    const int N = md.N, T = md.T;   // particle i = r * 256 + tid, r < NR
    const size_t row = (size_t)N * NX;
    TransParams tp;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        tp.LS[q] = ld_const(&tpp->LS[q]);
        tp.LSinv[q] = ld_const(&tpp->LSinv[q]);
    }
    tp.cS = ld_const(&tpp->cS);
    tp.G = G_arg;
    const uint64_t seed = ld_const(&swp->seed);
    {
        int gtot = NX;
#pragma unroll
        for (int d = 0; d < D; ++d) gtot *= (d == D - 1 && D > 1) ? JIN : md.J[d];
        for (int i = tid; i < gtot; i += PG_BLK) pg_g_lds_small[i] = G_arg[i];
        lds_barrier();
    }
    const double* Guse = pg_g_lds_small;
    const bool pow2 = (N & (N - 1)) == 0;
    const double invN = 1.0 / (double)N;

    // ---- x_0 ~ N(m0, P0), conditioned particle = ref_0 (src/PGAS.py:155-174,194)
    double x[NR][NX], logw[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int i = r * PG_BLK + tid;
        logw[r] = 0.0;
        double z[2];
        pgas_rng_normals(seed, PGAS_STREAM_INIT, 0u, (uint64_t)(i < N ? i : N - 1), NX, z);
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            double v = m0L0[k];
#pragma unroll
            for (int l = 0; l <= k; ++l) v = PGAS_FMA(m0L0[NX + k * NX + l], z[l], v);
            x[r][k] = (i == N - 1) ? ref[k] : v;
        }
        if (i < N) {
#pragma unroll
            for (int k = 0; k < NX; ++k) x_trace[(size_t)i * NX + k] = x[r][k];
        }
    }

    // ---- the time loop (src/PGAS.py:199-221).  y_t, ref_t, the uniforms and the particles' noise are fetched one step ahead.
    double yn[PGAS_MAX_NY], rn[NX], u1n = 0.0, u2n = 0.0;
    double2 zn[NR];
    auto fetch = [&](int t) {
#pragma unroll
        for (int k = 0; k < PGAS_MAX_NY; ++k) yn[k] = k < md.ny ? md.y[(size_t)t * md.ny + k] : 0.0;
#pragma unroll
        for (int k = 0; k < NX; ++k) rn[k] = ref[(size_t)t * NX + k];
        u1n = u_res[t];
        u2n = u_anc[t];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int i = r * PG_BLK + tid;
            zn[r] = reinterpret_cast<const double2*>(znoise)[(size_t)t * N + (i < N ? i : N - 1)];
        }
    };
    if (T > 1) fetch(1);
    for (int t = 1; t < T; ++t) {
        const double* __restrict__ ut = md.u + (size_t)t * md.nu;
        double yt[PGAS_MAX_NY], rf[NX];
#pragma unroll
        for (int k = 0; k < PGAS_MAX_NY; ++k) yt[k] = yn[k];
#pragma unroll
        for (int k = 0; k < NX; ++k) rf[k] = rn[k];
        const double u1 = u1n, u2 = u2n;
        double2 zc[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) zc[r] = zn[r];
        fetch(t + 1 < T ? t + 1 : t);
        double lw[2][NR], ln[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int i = r * PG_BLK + tid;
            double xin[1][NX], xt[NX], la1, h1, ln1;
#pragma unroll
            for (int k = 0; k < NX; ++k) xin[0][k] = x[r][k];
            const double z[2] = {zc[r].x, zc[r].y};
            small_particle_step<NX, D, JIN, J0T>(md, tp, Guse, ut, yt, rf, md.p0 + i == md.Ng - 1, xin, z, xt, la1, h1, ln1);
            lw[0][r] = -__builtin_inf();
            lw[1][r] = -__builtin_inf();
            ln[r] = ln1;
            if (i < N) {
#pragma unroll
                for (int k = 0; k < NX; ++k) {
                    x[r][k] = xt[k];
                    st_stream(&x_trace[(size_t)t * row + (size_t)i * NX + k], xt[k]);
                }
                const double l1 = la1 + logw[r];   // src/PGAS.py:101-102
                lw[0][r] = l1;
                lw[1][r] = l1 + h1;                // :117-118
            }
            sm.la[i] = la1;
        }
        double S[2];
        small_scan<2, NR>(sm, lw, N, S);   // ends with a barrier: sm.num and sm.la are visible
        // ---- systematic resampling (src/Filtering.py:28-35) and the ancestor of the conditioned particle (src/PGAS.py:121-127)
        const bool valid1 = (S[0] > 0.0) && (S[0] < __builtin_inf()), valid2 = (S[1] > 0.0) && (S[1] < __builtin_inf());
        const int cnt2 = small_count<NR>(sm, sm.num[1], u2 * S[1]);
        const int ref_idx = valid2 ? (cnt2 > N - 1 ? N - 1 : cnt2) : N - 1;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int i = r * PG_BLK + tid;
            if (i < N) {
                int a = i;   // no positive weight: identity (src/Filtering.py:25)
                if (valid1) {
                    const int p = small_lower_bound<NR * PG_BLK>(sm.num[0], slot_U(u1, i, N, invN, pow2) * S[0]);
                    a = p > N - 1 ? N - 1 : p;
                }
                if (i == N - 1) a = ref_idx;
                anc_trace[(size_t)(t - 1) * N + i] = (int32_t)a;   // plain store: the back-trace of this very launch reads it (L2)
                logw[r] = ln[r] - sm.la[a];   // src/PGAS.py:137-147
            }
        }
        lds_barrier();   // sm.la / sm.num are rewritten by the next step
    }

    // ---- final index (src/PGAS.py:224-225) and back-trace (src/Filtering.py:40-55)
    double lwf[1][NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int i = r * PG_BLK + tid;
        lwf[0][r] = i < N ? logw[r] : -__builtin_inf();
        if (i < N) logw_last[i] = logw[r];
    }
    double Sf[1];
    small_scan<1, NR>(sm, lwf, N, Sf);
    const bool validf = (Sf[0] > 0.0) && (Sf[0] < __builtin_inf());
    const int cf = small_count<NR>(sm, sm.num[0], ld_const(&swp->u_final) * Sf[0]);
    const int fidx = validf ? (cf > N - 1 ? N - 1 : cf) : N - 1;
    // the traces were written by every wave of this workgroup: make them visible to the one lane that chases
    __threadfence();
    lds_barrier();
    if (tid == 0) {
        hdr->final_idx = fidx;
        int b = fidx;
        for (int i = T - 1; i >= 0; --i) {
#pragma unroll
            for (int k = 0; k < NX; ++k) traj[(size_t)i * NX + k] = __hip_atomic_load(&x_trace[(size_t)i * row + (size_t)b * NX + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (i > 0) b = __hip_atomic_load(&anc_trace[(size_t)(i - 1) * N + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
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
