// pgas_marginal_rollout_stats.hip.h -- the posterior predictive of the grey-box rollout of pgas_marginal_rollout.hip.h, reduced over the
// replicates inside the kernel ("Predictive moments and log score"): nothing per replicate is written to memory.
//
//   k_model_rollout_stats   one wave per workgroup, grid (B = ceil(P / 64), K); lane = replicate p = 64 b + lane; per step the block's
//                           partial sums go to part (K, B, T, C), C = 2 (nx + ny) + 2
//   k_rollout_stats_finish  (pgas_rollout_stats.hip.h, unchanged: part has its layout) one thread per (k, t, channel): the blocks'
//                           partials in ascending b from +0.0; the log predictive density.  It runs for B = 1 too.
//
// The propagation is k_model_rollout's own code (mr_begin, mr_intvars, mr_advance), so replicate p0 + p carries exactly the x_t and
// y_t = g(x_t, u_t, xi_t) that pgas_m_rollout stores for it.  Per step t = 0 .. T-1 (row 0 and the last row included; g runs on every row)
// and replicate, the value channels are read from the LDS register file one at a time AFTER g has run -- no accumulator is live across
// the basis loop:
//   x_j      j < nx
//   yhat_j   j < ny: g_j, continued with acc = fma(LR[j,l], e_l, acc), l = 0 .. j ascending, when observation noise is asked for; e =
//            pgas_rng_normals' pairing on PGAS_STREAM_M_ROLLOUT_OBS at time t, particle p0 + p, parked in the normals rows
//   l        (log score only) the Gaussian log-density of observation row y_t at the NOISE-FREE g, with k_expr mode 2's operations:
//            e_j = sum_l (y_l - g_l) * LRinv[j,l] from 0.0 over all l < ny ascending, product and sum rounded separately;
//            q = sum_j e_j * e_j from 0.0; l = cR - 0.5 * q
// Every value channel v is reduced to S1 = sum v and S2 = sum (v * v) (product rounded, then added).  The summation order is section 13's
// with a block of 64 replicates and one replicate per lane:
//   1. inside a block   wave_sum_tree: the balanced adjacent-pair tree v <- v[0::2] + v[1::2], six times; lanes with p >= P hold +0.0
//   2. across blocks    ascending b from +0.0 (k_rollout_stats_finish)
// Lanes past P run the propagation on a copy of the last replicate, as in k_model_rollout; they contribute +0.0 to the sums and -inf to
// the maximum, never their values.  Log score per block: m_b = max l (fmax: a NaN takes no part), s_b = sum pgas_exp(l - m_b) in the order
// of 1 (a NaN l adds +0.0; a block without a finite l has m_b = -inf, s_b = 0).
//
// One wave per workgroup: the reduction needs no barrier and no LDS beyond k_model_rollout's, whose normals rows grow to
// max(nx, n_i, ny) for e:   LDS = (nreg + max(nx, max_i n_i, ny)) * 512 B + 8 sum_i n_i M_i B.
// Lane c holds channel c of the step, so the block's C values leave in ONE coalesced store that nothing waits for.  No flag, counter,
// atomic or barrier crosses a workgroup: K and P are not bounded by residency.
#pragma once

#include "pgas_marginal_rollout.hip.h"
#include "pgas_rollout_stats.hip.h"

struct MrStatsArgs {   // by value: what the reductions need beside MrArgs
    const double* y;   // (T, ny) observation rows; read only when score != 0
    double* part;      // (K, B, T, C)
    double cR;
    int32_t noise;     // 1: yhat = g + LR e
    int32_t score;     // 1: the log score channels are formed
    double LR[PG_EX_MAXOUT * PG_EX_MAXOUT];      // lower Cholesky factor of R, row-major ny x ny
    double LRinv[PG_EX_MAXOUT * PG_EX_MAXOUT];   // its inverse
};

__global__ __launch_bounds__(64) void k_model_rollout_stats(MrArgs a, MrStatsArgs s) {
    extern __shared__ __attribute__((aligned(16))) double pg_mrs_lds[];
    const int lane = threadIdx.x, T = a.T, P = a.P, nx = a.nx, ny = a.ny;
    const size_t draw = blockIdx.y;
    const int p = blockIdx.x * 64 + lane, pc = p < P ? p : P - 1;
    const bool live = p < P;
    double* __restrict__ rl = pg_mrs_lds + lane;
    double* __restrict__ zl = pg_mrs_lds + (size_t)a.nreg * 64 + lane;
    double* __restrict__ Al = pg_mrs_lds + (size_t)(a.nreg + a.nz) * 64;
    const uint64_t seed = a.seeds != nullptr ? ld_const(a.seeds + draw) : 0ull;
    const uint64_t particle = (uint64_t)(a.p0 + pc);
    const int nv = nx + ny, C = rollout_stats_channels(nx, ny), nstore = s.score ? C : 2 * nv;
    double* __restrict__ part = s.part + (draw * gridDim.x + blockIdx.x) * (size_t)T * C;
    const double ninf = -__builtin_inf();

    mr_begin(a, draw, lane, pc, seed, particle, rl, zl, Al);
    for (int t = 0; t < T; ++t) {
        mr_intvars(a, draw, seed, particle, t, rl, zl, Al);
        mr_run(rl, a.gcode, a.g_ninstr);
        double mine = 0.0;   // channel `lane` of this step
        for (int k = 0; k < nx; ++k) {
            const double v = rl[k * 64], vv = v * v;
            const double s1 = wave_sum_tree(live ? v : 0.0), s2 = wave_sum_tree(live ? vv : 0.0);
            mine = lane == k ? s1 : lane == nv + k ? s2 : mine;
        }
        if (s.noise) mr_normals(zl, seed, PGAS_STREAM_M_ROLLOUT_OBS, (uint32_t)t, particle, ny);
        for (int j = 0; j < ny; ++j) {
            double acc = rl[a.g_out[j] * 64];
            if (s.noise)
                for (int l = 0; l <= j; ++l) acc = PGAS_FMA(s.LR[j * ny + l], zl[l * 64], acc);
            const double vv = acc * acc;
            const double s1 = wave_sum_tree(live ? acc : 0.0), s2 = wave_sum_tree(live ? vv : 0.0);
            mine = lane == nx + j ? s1 : lane == nv + nx + j ? s2 : mine;
        }
        if (s.score) {
            double q = 0.0;
            for (int j = 0; j < ny; ++j) {
                double e = 0.0;
                for (int l = 0; l < ny; ++l) e += (ld_const(s.y + (size_t)t * ny + l) - rl[a.g_out[l] * 64]) * s.LRinv[j * ny + l];
                q += e * e;
            }
            const double ll = live ? s.cR - 0.5 * q : ninf;
            const double mb = wave_max(__builtin_fmax(ninf, ll));   // NaN takes no part
            const double ex = pgas_exp(ll - mb);
            const double sb = wave_sum_tree((ll == ll) && mb != ninf && live ? ex : 0.0);
            mine = lane == 2 * nv ? mb : lane == 2 * nv + 1 ? sb : mine;
        }
        if (lane < nstore) st_stream(&part[(size_t)t * C + lane], mine);
        if (t == T - 1) break;
        mr_advance<false>(a, seed, particle, t, rl, zl, nullptr, false);
    }
}
