// pgas_marginal_rollout_cdf.hip.h -- the empirical predictive CDF of the grey-box rollout of pgas_marginal_rollout.hip.h at given
// thresholds, counted over the replicates inside the kernel:
// count[k, t, c, j] = #{replicates p < P : v_c <= thr[t, c, j]}, an int32.
//
//   k_model_rollout_cdf   one wave per workgroup, grid (B = ceil(P / 64), K); lane = replicate p = 64 b + lane (k_model_rollout_stats'
//                         geometry); B = 1 stores the counts, B > 1 adds them with integer atomics onto an output the host zeroed on the
//                         same stream
//
// The propagation is k_model_rollout's own code (mr_begin, mr_intvars, mr_run(g), mr_advance<false>), so replicate p0 + p carries exactly
// the x_t and y_t = g(x_t, u_t, xi_t) that pgas_m_rollout stores for it.  All T rows are counted, row 0 and the last row included.  The
// value channels are k_model_rollout_stats', read from the LDS register file one at a time AFTER g has run:
//   x_j      j < nx
//   yhat_j   j < ny: g_j, continued with acc = fma(LR[j,l], e_l, acc), l = 0 .. j ascending, when observation noise is asked for; e =
//            mr_normals on PGAS_STREAM_M_ROLLOUT_OBS at time t, particle p0 + p, parked in the normals rows -- the values
//            k_model_rollout_stats draws, so the counts and its moments describe one cloud
// Lanes past P run the propagation on a copy of the last replicate, as in k_model_rollout, and are masked out of every ballot.
//
// The counting stage is pgas_rollout_cdf.hip.h's with one register row: slot i = c J + j < (nx + ny) J <= 64 sits in lane i; lane i holds
// thr[t, i] in a register, fetched one step ahead; cdf_count_channel<1> leaves the wave's count of slot i in lane i.  One wave per
// workgroup: no LDS beyond k_model_rollout_stats' (the counts never pass through LDS) and no barrier beyond mr_begin's.  Integer addition
// is exact: no result bit depends on the block split, on p0 chunking or on which draws share a launch.
// The counts leave through st_stream stores (B = 1) or atomicAdd on int32 (B > 1) that nothing waits for.  No flag, counter or barrier
// crosses a workgroup: K and P are not bounded by residency.
#pragma once

#include "pgas_marginal_rollout.hip.h"
#include "pgas_rollout_cdf.hip.h"

struct MrCdfArgs {   // by value: what the counts need beside MrArgs
    const double* thr;   // (T, nx + ny, J)
    int32_t* count;      // (K, T, nx + ny, J)
    int32_t J;
    int32_t noise;       // 1: yhat = g + LR e
    double LR[PG_EX_MAXOUT * PG_EX_MAXOUT];   // lower Cholesky factor of R, row-major ny x ny
};

__global__ __launch_bounds__(64) void k_model_rollout_cdf(MrArgs a, MrCdfArgs s) {
    extern __shared__ __attribute__((aligned(16))) double pg_mrc_lds[];
    const int lane = threadIdx.x, T = a.T, P = a.P, nx = a.nx, ny = a.ny, J = s.J;
    const size_t draw = blockIdx.y;
    const int pbase = (int)blockIdx.x * 64, p = pbase + lane, pc = p < P ? p : P - 1;
    const int nrem = P - pbase, nslots = (nx + ny) * J;
    const bool add = gridDim.x > 1;
    double* __restrict__ rl = pg_mrc_lds + lane;
    double* __restrict__ zl = pg_mrc_lds + (size_t)a.nreg * 64 + lane;
    double* __restrict__ Al = pg_mrc_lds + (size_t)(a.nreg + a.nz) * 64;
    const uint64_t seed = a.seeds != nullptr ? ld_const(a.seeds + draw) : 0ull;
    const uint64_t particle = (uint64_t)(a.p0 + pc);
    int32_t* __restrict__ count = s.count + draw * (size_t)T * nslots;

    double thnext = cdf_fetch_thresholds(s.thr, lane, nslots);   // row 0
    mr_begin(a, draw, lane, pc, seed, particle, rl, zl, Al);
    for (int t = 0; t < T; ++t) {
        const double thv = thnext;
        if (t + 1 < T) thnext = cdf_fetch_thresholds(s.thr + (size_t)(t + 1) * nslots, lane, nslots);   // one step ahead
        mr_intvars(a, draw, seed, particle, t, rl, zl, Al);
        mr_run(rl, a.gcode, a.g_ninstr);
        int mine = 0;   // the wave's count of slot `lane`
        for (int k = 0; k < nx; ++k) {
            const double v[1] = {rl[k * 64]};
            mine = cdf_count_channel<1>(v, lane, nrem, thv, k * J, J, mine);
        }
        if (s.noise) mr_normals(zl, seed, PGAS_STREAM_M_ROLLOUT_OBS, (uint32_t)t, particle, ny);
        for (int j = 0; j < ny; ++j) {
            double acc = rl[a.g_out[j] * 64];
            if (s.noise)
                for (int l = 0; l <= j; ++l) acc = PGAS_FMA(s.LR[j * ny + l], zl[l * 64], acc);
            const double v[1] = {acc};
            mine = cdf_count_channel<1>(v, lane, nrem, thv, (nx + j) * J, J, mine);
        }
        if (lane < nslots) {
            int32_t* dst = &count[(size_t)t * nslots + lane];
            if (add) atomicAdd(dst, mine);
            else st_stream(dst, (int32_t)mine);
        }
        if (t == T - 1) break;
        mr_advance<false>(a, seed, particle, t, rl, zl, nullptr, false);
    }
}
