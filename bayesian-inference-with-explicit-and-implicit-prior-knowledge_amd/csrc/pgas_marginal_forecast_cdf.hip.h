// pgas_marginal_forecast_cdf.hip.h -- the empirical CDF of the h-step-ahead clouds of pgas_marginal_forecast.hip.h at given thresholds,
// every origin row of every draw in ONE launch:
// count[k, h - 1, tau, c, j] = #{particles i < N : v_c <= thr[tau, c, j]}, an int32.
//
//   k_model_forecast_cdf<NR>   grid (K, ceil(T / TB)): blockIdx.x = draw, blockIdx.y = chunk of TB origin rows; one workgroup of 256;
//                              particle i = 256 r + tid, r < NR (k_model_forecast's geometry and register files)
//
// The clouds are k_model_forecast's, bit for bit: per origin row s and lead l = 0 .. min(H, T - s) - 1 (target row tau = s + l, horizon
// h = l + 1), particle i < N with the Philox particle index pi(l, i) = ((uint64)l << 32) | i:
//   1. cloud     l = 0: the state registers take x[k, s, i]; l >= 1: mr_advance<false>(t = tau - 1, particle = pi(l, i)).  Then, at every
//                lead, mr_intvars(t = tau, particle = pi(l, i)) and mr_run(g): called unchanged
//   2. channels  x_j (j < nx), then yhat_j (j < ny) = g_j read from the register file after g has run, continued with
//                acc = fma(LR[j,q], e_q, acc), q = 0 .. j ascending, when observation noise is asked for: e = mr_normals on
//                PGAS_STREAM_M_ROLLOUT_OBS at time tau, particle ((uint64)(l + 1) << 32) | i, parked in the file's park rows (free once g
//                has run: there is no log score here).  The high word is never 0, so no counter is shared with the open loop's noise
//                (pgas_marginal_rollout_cdf.hip.h and pgas_marginal_rollout_stats.hip.h, particle = p0 + p < 2^32)
//   3. counts    the counting stage of pgas_rollout_cdf.hip.h against the thresholds of the TARGET row, thr[tau]: one threshold set
//                serves every horizon.  v[r] of a channel is read from file r * 4 + wave where r * 256 + wave * 64 < N
//   4. the entries without an origin row (tau < l) are -1: written by the draw's chunk 0
// Every defined entry (l, tau) belongs to origin tau - l alone, so it has one writer and plain stores do; no flag, counter, atomic or
// barrier crosses a workgroup, so K x chunks may exceed what the GPU holds.
//
// LDS: the dynamic part is k_model_forecast's (ceil(N / 64) register files of (nreg + nz) 512 B with the filter's nz, then the draw's
// coefficient rows); the static part is the count slots, 2 x 4 x 64 int32 = 2048 B <= k_model_forecast's 2176 B: what the forecast holds
// this kernel holds.
//
// Barriers.  The origin range [s_lo, s_hi) and the lead-loop bound min(H, T - s) are workgroup-uniform (blockIdx and kernel arguments
// only), and a wave or row without particles skips the model only (wave-uniformly, no barrier inside), so every wave reaches every
// barrier: the one way this kernel could hang.  The steps of a workgroup (all leads of all its origins) are numbered n = 0, 1, ...;
// there is ONE barrier per step.
//
// LDS hazards (B0 the barrier after staging; slot set n & 1 of cnt; barrier n the one of step n; "own" = written and read by the same
// thread only):
//   coefficient rows            written before B0 by the whole workgroup, read-only afterwards
//   constants                   own, written before B0
//   state, input, interface     own: no thread ever touches another thread's column
//   temporaries, park rows      own (mr_intvars, mr_run, mr_advance, mr_normals of the owning wave; e parked and read back by the same
//                               thread within the step)
//   cnt[n & 1][wave][0 .. 63]   written by every wave before barrier n, read by wave 0 after it; next written before barrier n + 2, that
//                               is after barrier n + 1, which no wave passes before wave 0 has read step n (lds_barrier waits for its
//                               LDS reads)
// The thresholds of step n + 1 (target row t + 1 within an origin, s + 1 at the next origin's lead 0) are fetched during step n.  The
// counts leave through st_stream stores of wave 0 that nothing waits for.
#pragma once

#include "pgas_marginal_forecast.hip.h"
#include "pgas_rollout_cdf.hip.h"

struct MfcCdfArgs {   // by value: what the counts need beside MrArgs
    const double* x;     // (K, T, N, nx): pgas_m_filter's trace
    const double* thr;   // (T, nx + ny, J)
    int32_t* count;      // (K, H, T, nx + ny, J)
    int32_t H, TB, J;
    int32_t noise;       // 1: yhat = g + LR e
    double LR[PG_EX_MAXOUT * PG_EX_MAXOUT];   // lower Cholesky factor of R, row-major ny x ny
};

template <int NR>
__global__ __launch_bounds__(PG_BLK) void k_model_forecast_cdf(MrArgs a, MfcCdfArgs s) {
    __shared__ int cnt[2][PG_BLK / 64][PG_CDF_SLOTS];   // [step parity][wave][slot]
    extern __shared__ __attribute__((aligned(16))) double pg_mfcc_lds[];
    const size_t draw = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, N = a.P, nx = a.nx, ny = a.ny, nv = nx + ny, Hz = s.H, J = s.J, nslots = nv * J;
    const int s_lo = (int)blockIdx.y * s.TB, s_hi = s_lo + s.TB < T ? s_lo + s.TB : T;   // workgroup-uniform
    const int fstride = (a.nreg + a.nz) * 64, park = a.nreg * 64;   // doubles per file; where its park rows start
    double* __restrict__ Al = pg_mfcc_lds + (size_t)((N + 63) >> 6) * fstride;
    const uint64_t seed = a.seeds != nullptr ? ld_const(a.seeds + draw) : 0ull;
    const double* __restrict__ x_trace = s.x + draw * (size_t)T * N * nx;
    int32_t* __restrict__ count = s.count + draw * (size_t)Hz * T * nslots;   // (H, T, nv, J)

    // ---- once: the draw's coefficient rows (the whole workgroup), then per file the constant pool
    mr_stage_coeffs(a, draw, tid, Al);
#pragma unroll 1
    for (int r = 0; r < NR; ++r) {
        if (r * PG_BLK + wave * 64 >= N) continue;   // wave-uniform: no file
        double* __restrict__ rl = pg_mfcc_lds + (size_t)(r * 4 + wave) * fstride + lane;
        for (int j = 0; j < a.nconst; ++j) rl[(a.n_in + j) * 64] = ld_const(a.consts + j);
    }
    lds_barrier();   // B0

    // ---- 4. the entries no origin row reaches: rows tau = 0 .. l - 1 of horizon index l are contiguous
    if (blockIdx.y == 0) {
        for (int l = 1; l < Hz; ++l)
            for (int e = tid; e < l * nslots; e += PG_BLK) st_stream(&count[(size_t)l * T * nslots + e], (int32_t)-1);
    }

    int n = 0;   // the workgroup's step counter: the slot set's parity
    double thnext = cdf_fetch_thresholds(s.thr + (size_t)s_lo * nslots, lane, nslots);   // step 0: target row s_lo

    for (int so = s_lo; so < s_hi; ++so) {
        // ---- the origin's cloud: row so of the trace into the state registers
#pragma unroll 1
        for (int r = 0; r < NR; ++r) {
            if (r * PG_BLK + wave * 64 >= N) continue;
            const int i = r * PG_BLK + tid, pc = i < N ? i : N - 1;
            double* __restrict__ rl = pg_mfcc_lds + (size_t)(r * 4 + wave) * fstride + lane;
            for (int k = 0; k < nx; ++k) rl[k * 64] = x_trace[((size_t)so * N + pc) * nx + k];
        }
        const int L = Hz < T - so ? Hz : T - so;   // workgroup-uniform
        for (int l = 0; l < L; ++l, ++n) {
            const int par = n & 1, t = so + l;
            const double thv = thnext;
            {
                const int tn = l + 1 < L ? t + 1 : so + 1;   // the next step's target row; so + 1 >= s_hi fetches a row nobody uses
                if (tn < T) thnext = cdf_fetch_thresholds(s.thr + (size_t)tn * nslots, lane, nslots);
            }

            // ---- 1. per row: the propagation, the interface variables, g; then the observation noise's normals into the park rows
#pragma unroll 1
            for (int r = 0; r < NR; ++r) {
                if (r * PG_BLK + wave * 64 >= N) continue;
                const int i = r * PG_BLK + tid;
                const uint64_t ic = (uint64_t)(i < N ? i : N - 1);
                const uint64_t particle = ((uint64_t)l << 32) | ic;
                double* __restrict__ rl = pg_mfcc_lds + (size_t)(r * 4 + wave) * fstride + lane;
                double* __restrict__ zl = rl + park;
                if (l > 0) mr_advance<false>(a, seed, particle, t - 1, rl, zl, nullptr, false);
                mr_intvars(a, draw, seed, particle, t, rl, zl, Al);
                mr_run(rl, a.gcode, a.g_ninstr);
                if (s.noise) mr_normals(zl, seed, PGAS_STREAM_M_ROLLOUT_OBS, (uint32_t)t, ((uint64_t)(l + 1) << 32) | ic, ny);
            }

            // ---- 2., 3. the channels, one at a time, against the target row's thresholds: the wave's counts gather in `mine`
            int mine = 0;
            for (int c = 0; c < nv; ++c) {
                const int j = c - nx, reg = c < nx ? c : a.g_out[j];
                double v[NR];
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    v[r] = 0.0;
                    if (r * PG_BLK + wave * 64 < N) {
                        const double* __restrict__ rl = pg_mfcc_lds + (size_t)(r * 4 + wave) * fstride + lane;
                        double acc = rl[reg * 64];
                        if (s.noise && c >= nx)
                            for (int q = 0; q <= j; ++q) acc = PGAS_FMA(s.LR[j * ny + q], rl[park + q * 64], acc);
                        v[r] = acc;
                    }
                }
                mine = cdf_count_channel<NR>(v, tid, N, thv, c * J, J, mine);
            }
            cnt[par][wave][lane] = mine;
            lds_barrier();   // barrier n

            // ---- after the barrier: wave 0 sends the step's counts on their way
            if (tid < nslots) st_stream(&count[((size_t)l * T + t) * nslots + tid], (int32_t)cdf_block_total(cnt[par], tid));
        }
    }
}
