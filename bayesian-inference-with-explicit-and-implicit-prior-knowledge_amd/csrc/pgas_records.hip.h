// pgas_records.hip.h -- ONE model learned from E records (experiments) that share (A, S): the context's y / u are the concatenation of
// the records, Tsum = sum T_e rows, and a record table (pgas_records_set) says where each record starts.
//
//   k_sweep_records   grid (E, C): the whole conditional-SMC sweep of record e under chain c's parameters in ONE workgroup -- the text of
//                     k_sweep_chains (pgas_sweep_workgroup.inc) on record e's rows
//   k_records_begin   the uniforms and per-sweep scalars of every (chain, record), k_chains_begin with LOCAL time
//   k_records_noise   the propagation noise of every (chain, row, particle), k_chains_noise with LOCAL time
//   k_records_seeds   seeds[c, 0] = step key c, seeds[c, e] = child e of step key c
// The statistics take k_traj_basis_seams (pgas_suffstats.hip.h): rows whose successor belongs to the next record are zeros.
//
// Time inside a record is local (row - row0[e]): Philox counters, uniforms and noise are those of a single-record context built on
// record e alone, so workgroup (c, e) computes bit for bit what that context computes from seeds[c, e].  Records never wait for each
// other: no flag, counter or barrier crosses a workgroup (the rule of pgas_chains.hip.h), so ragged lengths cost tail idle time only
// and E x C may exceed what the GPU holds at once.
//
// Layouts, Tsum rows each with record e's rows at row0[e]: ref / traj (C, Tsum, nx), x_trace (C, Tsum, N, nx), znoise (C, Tsum, N, 2),
// anc_trace (C, Tsum, N) (record e uses T_e - 1 rows; its last row is unused), u_res / u_anc (C, Tsum); per (chain, record):
// swp / hdr (C, E), logw_last (C, E, N), seeds (C, E).  Per record: row0 (E + 1), m0L0 (E, nx + nx nx).  Per chain: tp, G (the buffers
// pgas_chains_set_params_dev packs).
#pragma once

#include "pgas_chains.hip.h"

template <int NX, int D, int JIN, int J0T, int NR>
__global__ __launch_bounds__(PG_BLK) void k_sweep_records(DevModel mdc, const int32_t* __restrict__ row0, const TransParams* __restrict__ tp_all,
                                                          const double* __restrict__ G_all, int64_t gstride, const SweepParams* __restrict__ sp_all,
                                                          const double* __restrict__ ures_all, const double* __restrict__ uanc_all,
                                                          const double* __restrict__ m0L0_all, const double* __restrict__ ref_all,
                                                          double* __restrict__ x_all, int32_t* __restrict__ anc_all, double* __restrict__ logw_all,
                                                          UpperHdr* __restrict__ hdr_all, double* __restrict__ traj_all,
                                                          const double* __restrict__ znoise_all) {
    __shared__ SmallSmem sm;
    extern __shared__ __attribute__((aligned(16))) double pg_g_lds_small[];   // the chain's coefficient tensor
    // record blockIdx.x under chain blockIdx.y: rows r0 .. r0 + T_e - 1 of chain c's (Tsum, ...) arrays, as a model of T_e rows
    const size_t e = blockIdx.x, chain = blockIdx.y, E = gridDim.x, Nc = (size_t)mdc.N;
    const int r0i = ld_const(&row0[e]);
    const size_t r0 = (size_t)r0i, crow = chain * (size_t)mdc.T + r0, ce = chain * E + e;
    DevModel md = mdc;
    md.T = ld_const(&row0[e + 1]) - r0i;
    md.y = mdc.y + r0 * mdc.ny;
    md.u = mdc.u + r0 * mdc.nu;
    const TransParams* __restrict__ tpp = tp_all + chain;
    const double* __restrict__ G_arg = G_all + chain * (size_t)gstride;
    const SweepParams* __restrict__ swp = sp_all + ce;
    const double* __restrict__ u_res = ures_all + crow;
    const double* __restrict__ u_anc = uanc_all + crow;
    const double* __restrict__ m0L0 = m0L0_all + e * (NX + NX * NX);
    const double* __restrict__ ref = ref_all + crow * NX;
    double* __restrict__ x_trace = x_all + crow * Nc * NX;
    int32_t* __restrict__ anc_trace = anc_all + crow * Nc;
    double* __restrict__ logw_last = logw_all + ce * Nc;
    UpperHdr* __restrict__ hdr = hdr_all + ce;
    double* __restrict__ traj = traj_all + crow * NX;
    const double* __restrict__ znoise = znoise_all + crow * Nc * 2;
#include "pgas_sweep_workgroup.inc"
}

// grid (ceil(Tsum / 256), C); rec[r] = record of row r
__global__ void k_records_begin(const uint64_t* __restrict__ seeds, const int32_t* __restrict__ rec, const int32_t* __restrict__ row0, int Tsum, int E,
                                SweepParams* __restrict__ sp, double* __restrict__ u_res, double* __restrict__ u_anc) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= Tsum) return;
    const size_t c = blockIdx.y;
    const int e = rec[r], t = r - row0[e];
    const uint64_t seed = seeds[c * E + e];
    u_res[c * Tsum + r] = pgas_rng_uniform(seed, PGAS_STREAM_RESAMPLE, (uint32_t)t);
    u_anc[c * Tsum + r] = pgas_rng_uniform(seed, PGAS_STREAM_ANCESTOR, (uint32_t)t);
    if (t == 0) {
        SweepParams* __restrict__ s = sp + c * E + e;
        s->seed = seed;
        s->epoch = 0;
        s->pad = 0;
        s->u_final = pgas_rng_uniform(seed, PGAS_STREAM_FINAL, 0u);
    }
}

// grid (ceil(N Tsum / 256), C): a record's first row (local t = 0) takes no propagation noise
__global__ __launch_bounds__(256) void k_records_noise(const uint64_t* __restrict__ seeds, const int32_t* __restrict__ rec, const int32_t* __restrict__ row0,
                                                       int N, int Tsum, int E, double* __restrict__ znoise) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)N * Tsum) return;
    const size_t c = blockIdx.y;
    const int r = (int)(q / N), i = (int)(q % N);
    const int e = rec[r], t = r - row0[e];
    if (t == 0) return;
    double z0, z1;
    pgas_normal_pair(pgas_rng_block(seeds[c * E + e], PGAS_STREAM_PROP, 0u, (uint32_t)t, (uint64_t)i), &z0, &z1);
    double* __restrict__ zc = znoise + c * (size_t)Tsum * N * 2;
    zc[((size_t)r * N + i) * 2] = z0;
    zc[((size_t)r * N + i) * 2 + 1] = z1;
}

// one thread per (chain, record)
__global__ void k_records_seeds(int C, int E, const uint64_t* __restrict__ step_keys, uint64_t* __restrict__ seeds) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)C * E) return;
    const uint64_t k = step_keys[i / E];
    const uint32_t e = (uint32_t)(i % E);
    seeds[i] = e == 0 ? k : key_child(k, e);
}
