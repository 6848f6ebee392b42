// pgas_sweep_workgroup.inc -- the one-workgroup conditional-SMC sweep (src/PGAS.py:176-228) on ONE workgroup's slices: x_0, T - 1 steps,
// final index, back-trace.  Program text shared by k_sweep_chains (pgas_chains.hip.h: a chain per workgroup) and k_sweep_records
// (pgas_records.hip.h: a (record, chain) per workgroup), which differ only in how they form the slices; it is included, not called, so
// that each kernel compiles exactly as if the text stood in it (as a __forceinline__ function of the slices it changed k_sweep_chains'
// register allocation at every instantiation).
// In scope at the point of inclusion: template parameters NX, D, JIN, J0T, NR; `sm` (SmallSmem) and `pg_g_lds_small` (dynamic LDS);
// DevModel md with md.T rows at md.y / md.u; and the workgroup's tpp, G_arg, swp, u_res, u_anc, m0L0, ref, x_trace, anc_trace,
// logw_last, hdr, traj, znoise -- T rows each (anc_trace T - 1; u_res[t] / u_anc[t] for t < T), time counted from the first row.
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
