// pgas_marginal_rollout.hip.h -- open-loop simulation of a GREY-BOX model under K coefficient draws in ONE launch:
// known physics f / g as traced register programs (k_expr's opcodes), L latent functions xi_i = A_k,i phi_i(feature_i(x_t, u_t)) plugged in
// as interface variables, P replicates per draw, the time loop inside the kernel.
//
//   k_model_rollout   one wave per workgroup, grid (ceil(P / 64), K); lane = replicate
//
// For t = 0 .. T-1, in Algorithm1's time convention (step t -> t+1 reads input row t, Algorithm1.py:184-250, :363-365):
//   v_i   = concat(x_t, u_t)[sel]  or the result of a traced feature program        (basis argument, D_i <= PG_HB_MAXD)
//   phi_i = the expression of k_hilbert_batch on v_i, same operation order
//   xi_i  = A_k,i phi_i [+ Lrow_k,i e]      ascending-m fma chain from 0; e ~ N(0, I) on PGAS_STREAM_M_ROLLOUT_INTVAR + i at time t
//   y_t   = g(x_t, u_t, xi)                                                         -> out_y[k, t, p, :]   (optional)
//   x_t+1 = f(x_t, u_t, xi) [+ Qc z]        k_expr's mode-1 tail; z on PGAS_STREAM_M_STATE at time t + 1, as Algorithm1._draw_states
//
// All programs share one register numbering (the host relocates them): [0, nx) state, [nx, nx + nu) input, then the interface variables'
// components, then ONE pool of constants, then temporaries.  No program writes below the temporaries, so the state, the input row, the
// interface variables and the constants live in the register file itself: the file is the replicate's on-chip state for all T steps.  It
// sits in LDS as r[reg][lane] (lane-contiguous: conflict-free, no run-time-indexed private array, no scratch), followed by the rows the
// normals are parked in and by the draw's coefficient rows A_k,i, which every lane reads at the same address (broadcast).
// Replicates never talk to each other and no flag, counter or barrier crosses a workgroup: K and P are unbounded by residency.
#pragma once

#include "pgas_marginal.hip.h"

#define PG_MR_MAXN 8            // components of one interface variable
#define PG_MR_X0_DRAWN 0        // x_0 = m0 + L0 z on PGAS_STREAM_M_INIT_STATE, as Algorithm1._init_algorithm
#define PG_MR_X0_ONE 1          // x0 (nx)
#define PG_MR_X0_DRAW 2         // x0 (K, nx)
#define PG_MR_X0_EACH 3         // x0 (K, P, nx)

struct MrLatent {
    int32_t M, D, n, feat, sel[PG_HB_MAXD];
    double div[PG_HB_MAXD], center[PG_HB_MAXD], L[PG_HB_MAXD], size[PG_HB_MAXD], amp[PG_HB_MAXD];
    const int32_t* idx; const double* A; const double* Lrow; const int32_t* fcode;
    int32_t f_ninstr, a_off;    // a_off: where this function's coefficient rows start in the LDS copy
};
struct MrArgs {
    int32_t T, P, L, nx, nu, ny, n_in, nconst, nreg, nz, x0_mode, f_ninstr, g_ninstr;
    int32_t f_out[PG_EX_MAXOUT], g_out[PG_EX_MAXOUT];
    int64_t p0;
    const double* consts; const int32_t* fcode; const int32_t* gcode; const double* u; const uint64_t* seeds; const double* Qc;
    const double* x0; const double* m0L0; double* out_x; double* out_y;
    MrLatent lat[PG_EX_MAXIV];
};

// one program on the LDS register file: the switch of k_expr, operands and result in r[reg][lane]
__device__ __forceinline__ void mr_run(double* __restrict__ rl, const int32_t* __restrict__ code, int ninstr) {
    for (int i = 0; i < ninstr; ++i) {   // uniform control flow: the program words are scalar loads
        const int op = ld_const(code + 4 * i), d = ld_const(code + 4 * i + 1);
        const double x = rl[ld_const(code + 4 * i + 2) * 64], y = rl[ld_const(code + 4 * i + 3) * 64];
        double v;
        switch (op) {
            case 1: v = x + y; break;
            case 2: v = x - y; break;
            case 3: v = x * y; break;
            case 4: v = x / y; break;
            case 5: v = -x; break;
            case 6: v = cos(x); break;
            case 7: v = sin(x); break;
            case 8: v = tan(x); break;
            case 9: v = tanh(x); break;
            case 10: v = atan(x); break;
            case 11: v = sqrt(x); break;
            case 12: v = exp(x); break;
            case 13: v = (double)((x > 0.0) - (x < 0.0)); break;
            default: v = x; break;
        }
        rl[d * 64] = v;
    }
}

// normals z[0 .. n) of (seed, stream, t, particle) parked in zl[j * 64] (pgas_rng_normals' pairing: draw d yields z[2d], z[2d + 1])
__device__ __forceinline__ void mr_normals(double* __restrict__ zl, uint64_t seed, uint32_t stream, uint32_t t, uint64_t particle, int n) {
    for (int d = 0; 2 * d < n; ++d) {
        double a, b;
        pgas_normal_pair(pgas_rng_block(seed, stream, (uint32_t)d, t, particle), &a, &b);
        zl[(2 * d) * 64] = a;
        if (2 * d + 1 < n) zl[(2 * d + 1) * 64] = b;
    }
}

// ---- the propagation in three pieces, shared word for word with k_model_rollout_stats (pgas_marginal_rollout_stats.hip.h) ----------------
// once per workgroup: the draw's coefficient rows, the constant pool, row 0; ends in the barrier that orders the staged rows
__device__ __forceinline__ void mr_begin(const MrArgs& a, size_t draw, int lane, int pc, uint64_t seed, uint64_t particle, double* __restrict__ rl,
                                         double* __restrict__ zl, double* __restrict__ Al) {
    const int nx = a.nx;
    for (int i = 0; i < a.L; ++i) {
        const int cnt = a.lat[i].n * a.lat[i].M;
        const double* __restrict__ src = a.lat[i].A + draw * (size_t)cnt;
        for (int e = lane; e < cnt; e += 64) Al[a.lat[i].a_off + e] = src[e];
    }
    for (int j = 0; j < a.nconst; ++j) rl[(a.n_in + j) * 64] = ld_const(a.consts + j);
    if (a.x0_mode == PG_MR_X0_DRAWN) {
        mr_normals(zl, seed, PGAS_STREAM_M_INIT_STATE, 0u, particle, nx);
        for (int k = 0; k < nx; ++k) {
            double v = ld_const(a.m0L0 + k);
            for (int l = 0; l < nx; ++l) v += zl[l * 64] * ld_const(a.m0L0 + nx + k * nx + l);
            rl[k * 64] = v;
        }
    } else {
        const size_t off = a.x0_mode == PG_MR_X0_ONE ? 0 : a.x0_mode == PG_MR_X0_DRAW ? draw * nx : (draw * (size_t)a.P + pc) * nx;
        for (int k = 0; k < nx; ++k) rl[k * 64] = a.x0[off + k];
    }
    __syncthreads();   // one wave: orders the staged coefficient rows against the broadcast reads below
}

// once per workgroup of PG_BLK (the filter's, the forecasts' and the smoother's): the draw's coefficient rows into Al; the caller's barrier orders them
__device__ __forceinline__ void mr_stage_coeffs(const MrArgs& a, size_t draw, int tid, double* __restrict__ Al) {
    for (int i = 0; i < a.L; ++i) {
        const int cnt = a.lat[i].n * a.lat[i].M;
        const double* __restrict__ src = a.lat[i].A + draw * (size_t)cnt;
        for (int e = tid; e < cnt; e += PG_BLK) Al[a.lat[i].a_off + e] = src[e];
    }
}

// step t: the input row, then the interface variables xi_i = A_k,i phi_i(v_i) [+ Lrow e] into their registers
__device__ __forceinline__ void mr_intvars(const MrArgs& a, size_t draw, uint64_t seed, uint64_t particle, int t, double* __restrict__ rl,
                                           double* __restrict__ zl, const double* __restrict__ Al) {
    const int nx = a.nx, nu = a.nu;
    for (int j = 0; j < nu; ++j) rl[(nx + j) * 64] = ld_const(a.u + (size_t)t * nu + j);
    int ivreg = nx + nu;
    for (int i = 0; i < a.L; ++i) {
        const MrLatent& h = a.lat[i];
        if (h.feat) mr_run(rl, h.fcode, h.f_ninstr);
        double w[PG_HB_MAXD];
#pragma unroll
        for (int d = 0; d < PG_HB_MAXD; ++d)
            w[d] = d < h.D ? (rl[h.sel[d] * 64] / h.div[d] - h.center[d] + h.L[d]) / h.size[d] : 0.0;
        double acc[PG_MR_MAXN];
#pragma unroll
        for (int j = 0; j < PG_MR_MAXN; ++j) acc[j] = 0.0;
        const double* __restrict__ Ai = Al + h.a_off;
        for (int m = 0; m < h.M; ++m) {
            double prod = 1.0;
#pragma unroll
            for (int d = 0; d < PG_HB_MAXD; ++d) {
                if (d < h.D) {
                    const double ang = PGAS_PI_D * (double)ld_const(h.idx + m * h.D + d) * w[d];
                    const double f = h.amp[d] * sin(ang);
                    prod = d == 0 ? f : prod * f;
                }
            }
#pragma unroll
            for (int j = 0; j < PG_MR_MAXN; ++j)
                if (j < h.n) acc[j] = PGAS_FMA(Ai[j * h.M + m], prod, acc[j]);
        }
        if (h.Lrow) {
            mr_normals(zl, seed, PGAS_STREAM_M_ROLLOUT_INTVAR + (uint32_t)i, (uint32_t)t, particle, h.n);
            const double* __restrict__ Lr = h.Lrow + draw * (size_t)(h.n * h.n);
#pragma unroll
            for (int j = 0; j < PG_MR_MAXN; ++j)
                if (j < h.n)
                    for (int l = 0; l <= j; ++l) acc[j] = PGAS_FMA(ld_const(Lr + j * h.n + l), zl[l * 64], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < PG_MR_MAXN; ++j)
            if (j < h.n) rl[(ivreg + j) * 64] = acc[j];
        ivreg += h.n;
    }
}

// x_t+1 = f(x_t, u_t, xi) [+ Qc z]: the tail of k_expr's mode 1, z of time t + 1.  STORE: live lanes also write row t + 1 to ox.
template <bool STORE>
__device__ __forceinline__ void mr_advance(const MrArgs& a, uint64_t seed, uint64_t particle, int t, double* __restrict__ rl, double* __restrict__ zl,
                                           double* __restrict__ ox, bool live) {
    const int nx = a.nx;
    mr_run(rl, a.fcode, a.f_ninstr);
    if (a.Qc) mr_normals(zl, seed, PGAS_STREAM_M_STATE, (uint32_t)(t + 1), particle, nx);
    for (int j = 0; j < nx; ++j) {   // the results sit in temporaries (never in [0, nx)), so row t + 1 can replace row t in place
        double v = rl[a.f_out[j] * 64];
        if (a.Qc)
            for (int l = 0; l < nx; ++l) v += zl[l * 64] * ld_const(a.Qc + j * nx + l);
        rl[j * 64] = v;
        if (STORE && live) st_stream(&ox[(size_t)(t + 1) * a.P * nx + j], v);
    }
}

__global__ __launch_bounds__(64) void k_model_rollout(MrArgs a) {
    extern __shared__ __attribute__((aligned(16))) double pg_mr_lds[];
    const int lane = threadIdx.x, T = a.T, P = a.P, nx = a.nx;
    const size_t draw = blockIdx.y;
    const int p = blockIdx.x * 64 + lane, pc = p < P ? p : P - 1;   // lanes past P repeat the last replicate and store nothing
    const bool live = p < P;
    double* __restrict__ rl = pg_mr_lds + lane;                      // register j of this lane: rl[j * 64]
    double* __restrict__ zl = pg_mr_lds + (size_t)a.nreg * 64 + lane;
    double* __restrict__ Al = pg_mr_lds + (size_t)(a.nreg + a.nz) * 64;
    const uint64_t seed = a.seeds != nullptr ? ld_const(a.seeds + draw) : 0ull;
    const uint64_t particle = (uint64_t)(a.p0 + pc);

    mr_begin(a, draw, lane, pc, seed, particle, rl, zl, Al);
    double* __restrict__ ox = a.out_x + draw * (size_t)T * P * nx + (size_t)pc * nx;
    double* __restrict__ oy = a.out_y ? a.out_y + draw * (size_t)T * P * a.ny + (size_t)pc * a.ny : nullptr;
    if (live)
        for (int k = 0; k < nx; ++k) ox[k] = rl[k * 64];

    for (int t = 0; t < T; ++t) {
        if (t == T - 1 && !oy) break;   // the last row only has an output to compute
        mr_intvars(a, draw, seed, particle, t, rl, zl, Al);
        // ---- y_t = g(x_t, u_t, xi)
        if (oy) {
            mr_run(rl, a.gcode, a.g_ninstr);
            if (live)
                for (int j = 0; j < a.ny; ++j) st_stream(&oy[(size_t)t * P * a.ny + j], rl[a.g_out[j] * 64]);
        }
        if (t == T - 1) break;
        mr_advance<true>(a, seed, particle, t, rl, zl, ox, live);
    }
}
