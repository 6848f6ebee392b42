/* pgas_marginal.h -- C ABI of the device primitives behind the MARGINALISED family (reference src/Algorithm1.py,
 * src/Algorithm3.py, src/Algorithm2.py).  Same conventions as pgas_hip.h: return 0 = ok, error
 * text through pgas_last_error(ctx), device pointers of fp64 / int32 arrays, work enqueued on the caller's stream.  `ctx` is
 * any context of the target device (the host mirror uses the utility context of pgas_amd/_lib.py); it supplies the device and
 * the error channel only.
 *
 * The reference maps per-particle functions with jax.vmap; these entry points are the batched bodies of
 *   jax.random.normal / jax.random.t                                    src/StateSpaceModel.py:67, src/BayesianInferrence.py:104
 *   BI.prior_mniw_mean + einsum            (auxiliary interface variable) src/Algorithm1.py:211-231
 *   BI.prior_mniw_2naturalPara_inv + BI.prior_mniw_Predictive            src/Algorithm1.py:251-262, BI:35-45, :64-89
 *   BI.prior_mniw_log_base_measure                                       src/Algorithm3.py:95-108, BI:111-124
 *   forgetting, ancestor gather and BI.prior_mniw_calcStatistics update  src/Algorithm1.py:317-320, :358-377
 * for a scalar interface variable (n = 1: every instantiation in the reference). */
#ifndef PGAS_MARGINAL_H
#define PGAS_MARGINAL_H

#include "pgas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The scalar uniform of (seed, stream, t): host value, identical to what the device kernels would draw (pgas_canon.h). */
double pgas_m_rng_uniform(uint64_t seed, uint32_t stream, uint32_t t);

/* out (n, ncol): normals of particles p0 .. p0+n at (stream, t); ncol <= 8. */
int pgas_m_rng_normal(pgas_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t t, int64_t p0, int64_t n, int32_t ncol,
                      double* out_dev, void* stream_handle);

/* out (n): Student-t(nu[p]) variates (z / sqrt(chi2_nu / nu), Marsaglia-Tsang gamma sampler on the same Philox streams). */
/* Device-resident time index.  With t_dev != NULL every later pgas_m_rng_normal / _student_t / _uniform_dev call of this context takes
 * the time index of its Philox counters from *t_dev at execution time (the `t` argument is ignored): a filter step captured once in a HIP
 * graph can then be replayed for every t (reference loop src/Algorithm1.py:418-457).  NULL restores the argument.  t_dev must stay valid. */
int pgas_m_set_time_source(pgas_ctx* ctx, const uint32_t* t_dev);
/* out_dev[0] = the uniform pgas_m_rng_uniform(seed, stream, t) returns on the host, written on the device (t from the time source if set) */
int pgas_m_rng_uniform_dev(pgas_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t t, double* out_dev, void* stream_handle);

int pgas_m_rng_student_t(pgas_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t t, int64_t p0, int64_t n, const double* nu_dev,
                         double* out_dev, void* stream_handle);
/* The same Student-t variates computed on the HOST by the library's own arithmetic (no context, no device; bit-identical to the
 * kernel's): for host-side helpers such as prior_mniw_drawPred (BI:92-108), so that one key never means two samplers. */
int pgas_m_rng_student_t_host(uint64_t seed, uint32_t stream, uint32_t t, int64_t p0, int64_t n, const double* nu_host, double* out_host);

/* chi^2(nu_p) variates, out[p] = 2 Gamma(nu_p / 2) on the counters of particle p0 + p (pgas_rng_gamma, include/pgas_canon.h): the
 * diagonal of the Bartlett factor in PGAS.sample_params (reference src/PGAS.py:323-327, jax.random.chisquare there). */
int pgas_m_rng_chi2(pgas_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t t, int64_t p0, int64_t n, const double* nu_dev, double* out_dev,
                    void* stream_handle);

/* Per particle p, with s = anc[p] (anc NULL: s = p): eta0 = P0 + scale T0[s] (+ R0), eta1 = P1 + scale T1[s] (+ R1)
 * (M <= 126, eta1 symmetric positive definite; M <= 62: one matrix row per lane, the trailing update on the f64 matrix cores; 63 ... 126: two rows
 * per lane, the triangle updated in place in LDS -- a generality path);
 *   m[p] = eta0^T eta1^-1 phi[p],  c[p] = phi[p]^T eta1^-1 phi[p],  q[p] = eta0^T eta1^-1 eta0,  logdet[p] = log det eta1.
 * R0/R1 (the reference trajectory's statistics, src/Algorithm3.py:96-101), phi and every output may be NULL.
 * Lfac_dev (n, (M+2)(M+3)/2), optional, receives the packed Cholesky factor for pgas_m_mniw_trisolve: rows of L with 1/L_kk on the
 * diagonal, followed by the two right-hand-side rows the kernel eliminates along with the matrix (row M = L^-1 phi, row M+1 =
 * w = L^-1 eta0).  The children of a resampled particle share its matrix (src/Algorithm1.py:358-361), so it is factorised once
 * per step, before resampling, not once more per child.
 * Asynchronous; a matrix that is not positive definite is counted on the device and reported by pgas_m_check. */
int pgas_m_mniw_solve(pgas_ctx* ctx, int64_t n, int32_t M, double scale, const int32_t* anc_dev, const double* P0_dev, const double* P1_dev,
                      const double* T0_dev, const double* T1_dev, const double* R0_dev, const double* R1_dev, const double* phi_dev,
                      double* m_dev, double* c_dev, double* q_dev, double* logdet_dev, double* Lfac_dev, void* stream_handle);

/* With the factor stored by pgas_m_mniw_solve: m[p] = w[s] . v, c[p] = v . v, v = L[s]^-1 phi[p], s = anc[p] (NULL: p). */
int pgas_m_mniw_trisolve(pgas_ctx* ctx, int64_t n, int32_t M, const int32_t* anc_dev, const double* Lfac_dev, const double* phi_dev,
                         double* m_dev, double* c_dev, void* stream_handle);

/* Synchronises the stream; PGAS_E_STATE if any pgas_m_mniw_solve since the last check met a matrix that was not positive
 * definite (its outputs are NaN). */
int pgas_m_check(pgas_ctx* ctx, void* stream_handle);

/* T_out[p] = scale * T_in[anc[p]] + (phi[p] xi[p], phi[p] phi[p]^T, xi[p]^2, 1); anc may be NULL (identity).  In and out must
 * not alias. */
int pgas_m_stats_gather_update(pgas_ctx* ctx, int64_t n, int32_t M, double scale, const int32_t* anc_dev, const double* T0_in,
                               const double* T1_in, const double* T2_in, const double* T3_in, const double* phi_dev,
                               const double* xi_dev, double* T0_out, double* T1_out, double* T2_out, double* T3_out,
                               void* stream_handle);

/* S = sum_p w[p] (T0[p], T1[p], T2[p], T3[p]): the weighted statistics trace of src/Algorithm1.py:166-170, :445-457
 * (S0 (M), S1 (M,M), S2 (1), S3 (1)).  Streaming reduction in two deterministic passes. */
int pgas_m_weighted_stats(pgas_ctx* ctx, int64_t n, int32_t M, const double* w_dev, const double* T0_dev, const double* T1_dev,
                          const double* T2_dev, const double* T3_dev, double* S0_dev, double* S1_dev, double* S2_dev, double* S3_dev,
                          void* stream_handle);

/* Three small fusions of the filter step's per-particle glue (each replaces a handful of elementwise launches):
 *   pgas_m_rng_student_t_df  Student-t variates with nu[p] = nu0 + nu_scale * src[anc[p]] formed in the kernel (df = P3 + lambda T3[a], BI:45);
 *   pgas_m_mniw_draw         xi[p] = m[p] + sqrt((P2 + scale T2[a] - q[a]) / (P3 + scale T3[a])) t[p] sqrt(c[p] + 1), a = anc[p]  (BI:64-108, n = 1);
 *   pgas_m_hilbert_basis     phi (n, M) = prod_d sqrt(1/L_d) sin(pi j[m][d] (v_d / div_d - center_d + L_d) / size_d), v = concat(state[p], input)[sel]
 *                            (src/BasisFunctions.py:77-80 under the vmap of src/Algorithm1.py:220-225): sel / div / center / L / size host (D <= 4),
 *                            idx_dev (M, D) int32 on the device. */
int pgas_m_rng_student_t_df(pgas_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t t, int64_t p0, int64_t n, const int32_t* anc_dev, const double* src_dev,
                            double nu0, double nu_scale, double* out_dev, void* stream_handle);
int pgas_m_mniw_draw(pgas_ctx* ctx, int64_t n, double scale, const int32_t* anc_dev, const double* m_dev, const double* c_dev, const double* q_dev,
                     const double* T2_dev, const double* T3_dev, double P2, double P3, const double* t_dev, double* out_dev, void* stream_handle);
/* g[p] = lbm(P + T[p]) - lbm(P + T[p] + R) with lbm(nu, Psi, logdet) = -M/2 log 2pi + logdet/2 - nu/2 log 2 - lgamma(nu/2) + nu/2 log Psi: the
 * base-measure term of the conditional filter's ancestor weights (src/Algorithm3.py:93-108, BI:111-124, n = 1) from the q / logdet of the two
 * pgas_m_mniw_solve calls; r2_dev / r3_dev: the reference statistics' T2 / T3 (one double each, on the device). */
int pgas_m_lbm_diff(pgas_ctx* ctx, int64_t n, int32_t M, const double* T2_dev, const double* T3_dev, const double* q1_dev, const double* logdet1_dev,
                    const double* q2_dev, const double* logdet2_dev, double P2, double P3, const double* r2_dev, const double* r3_dev, double* out_dev,
                    void* stream_handle);
int pgas_m_hilbert_basis(pgas_ctx* ctx, int64_t n, int32_t M, int32_t D, const double* state_dev, int32_t nx, const double* input_dev, int32_t nu,
                         const int32_t* sel, const double* div, const double* center, const double* L, const double* size, const int32_t* idx_dev,
                         double* out_dev, void* stream_handle);

/* A model callable as data (src/StateSpaceModel.py:32-87: transition_mdl / output_mdl / draw_state / log_likelihood, which the reference
 * evaluates per particle under jax.vmap): `code_dev` (ninstr, 4) int32 = (opcode, destination, source a, source b) over `nreg` <= 96 registers
 * per particle; registers [0, n_in) are preloaded with the state's nx columns, the nu input components and the interface variables'
 * components (in that order), [n_in, n_in + nconst) with `consts_dev`; opcodes 1..14 = add sub mul div neg cos sin tan tanh atan sqrt exp
 * sign mov (pgas_amd/exprs.py traces a model written against an array namespace into this form).  The registers `out_regs` (host, nout <= 8)
 * hold the result v; mode 0: out (n, nout) = v; mode 1: out = v + aux (n, nout) mat^T (draw_state: aux standard normals, mat = chol Q);
 * mode 2: out (n) = cR - |mat (aux (nout) - v)|^2 / 2 (log_likelihood: aux = y_t, mat = chol(R)^-1).  anc_dev (nullable): particle p reads
 * the state and interface variables of particle anc[p].  iv_dev / iv_widths: host arrays of n_iv <= 4 device pointers / widths. */
int pgas_m_expr_eval(pgas_ctx* ctx, int64_t n, const int32_t* code_dev, int32_t ninstr, const double* consts_dev, int32_t nconst, int32_t n_in,
                     int32_t nreg, const int32_t* out_regs, int32_t nout, const double* state_dev, int32_t nx, const int32_t* anc_dev,
                     const double* input_dev, int32_t nu, const double* const* iv_dev, const int32_t* iv_widths, int32_t n_iv, int32_t mode,
                     const double* aux_dev, const double* mat_dev, double cR, double* out_dev, void* stream_handle);

/* The same four operations for an interface variable with nvar > 1 components (the reference's formulas are general in n: eta0 (M, n),
 * eta2 (n, n), BI:18-50, 53-61, 64-108; no configuration of the reference uses n > 1).  Layouts: P0 / R0 (M, nvar), T0 (n, M, nvar),
 * T2 (n, nvar, nvar), xi (n, nvar), all row-major; results m (n, nvar) = eta0^T eta1^-1 phi (BI:81), q (n, nvar, nvar) = eta0^T eta1^-1 eta0
 * (row_scale = eta2 - q, BI:42), c and logdet as above; Lfac (n, (M+1+nvar)(M+2+nvar)/2) carries nvar right-hand-side rows behind the
 * factor.  M + 1 + nvar <= 128, nvar <= 8.  nvar = 1 is exactly the scalar entry point (which forwards here). */
int pgas_m_mniw_solve_n(pgas_ctx* ctx, int64_t n, int32_t M, int32_t nvar, double scale, const int32_t* anc_dev, const double* P0_dev,
                        const double* P1_dev, const double* T0_dev, const double* T1_dev, const double* R0_dev, const double* R1_dev,
                        const double* phi_dev, double* m_dev, double* c_dev, double* q_dev, double* logdet_dev, double* Lfac_dev,
                        void* stream_handle);
int pgas_m_mniw_trisolve_n(pgas_ctx* ctx, int64_t n, int32_t M, int32_t nvar, const int32_t* anc_dev, const double* Lfac_dev,
                           const double* phi_dev, double* m_dev, double* c_dev, void* stream_handle);
int pgas_m_stats_gather_update_n(pgas_ctx* ctx, int64_t n, int32_t M, int32_t nvar, double scale, const int32_t* anc_dev, const double* T0_in,
                                 const double* T1_in, const double* T2_in, const double* T3_in, const double* phi_dev,
                                 const double* xi_dev, double* T0_out, double* T1_out, double* T2_out, double* T3_out,
                                 void* stream_handle);
int pgas_m_weighted_stats_n(pgas_ctx* ctx, int64_t n, int32_t M, int32_t nvar, const double* w_dev, const double* T0_dev,
                            const double* T1_dev, const double* T2_dev, const double* T3_dev, double* S0_dev, double* S1_dev,
                            double* S2_dev, double* S3_dev, void* stream_handle);

/* R independent RUNS of the marginalised filter in the launches of one (pgas_amd/runs.py).  Arrays are (R, N, ...)
 * row-major with run r at slice r; the per-particle entry points above serve R N particles unchanged when their ancestor indices are
 * GLOBAL (r N + i).  What is per run has its batched form here.  keys_dev (R) u64: the root key of every run.  Work is enqueued on the
 * caller's stream, without host synchronisation; the one scratch buffer (weighted statistics) is sized at first use.
 *
 * Random numbers: element (r, i) is exactly what the single-seed entry point returns for seed keys[r], p0 = 0 and particle i -- same
 * stream, time and counter layout, and the same device-resident time index (pgas_m_set_time_source).
 *   _normal        out (R, N, ncol), ncol <= 8
 *   _student_t     out (R, N) with nu_dev (R, N)
 *   _student_t_df  nu = nu0 + nu_scale * src[anc[p]], anc a global index into the R N axis
 *   _uniform       out (R): the value pgas_m_rng_uniform_dev writes for keys[r] */
int pgas_m_runs_rng_normal(pgas_ctx* ctx, const uint64_t* keys_dev, int32_t R, int64_t N, uint32_t stream, uint32_t t, int32_t ncol, double* out_dev,
                           void* stream_handle);
int pgas_m_runs_rng_student_t(pgas_ctx* ctx, const uint64_t* keys_dev, int32_t R, int64_t N, uint32_t stream, uint32_t t, const double* nu_dev,
                              double* out_dev, void* stream_handle);
int pgas_m_runs_rng_student_t_df(pgas_ctx* ctx, const uint64_t* keys_dev, int32_t R, int64_t N, uint32_t stream, uint32_t t, const int32_t* anc_dev,
                                 const double* src_dev, double nu0, double nu_scale, double* out_dev, void* stream_handle);
int pgas_m_runs_rng_uniform(pgas_ctx* ctx, const uint64_t* keys_dev, int32_t R, uint32_t stream, uint32_t t, double* out_dev, void* stream_handle);

/* systematic_SISR (src/Filtering.py:6-37) of R weight vectors, one workgroup per run, N <= 1024 (PGAS_E_ARG beyond): u_dev (R) the uniform of
 * every run, logw_dev (R, N).  idx_local_dev (R, N) int32: row r is element for element what pgas_systematic_resample_dev returns for
 * (u[r], logw[r]) on a context of N particles (a row without a positive finite weight gives the identity); idx_global_dev (R, N) int32 or
 * NULL receives r N + idx_local.  Runs do not communicate: R may exceed what the device holds at once. */
int pgas_m_runs_systematic(pgas_ctx* ctx, int32_t R, int32_t N, const double* u_dev, const double* logw_dev, int32_t* idx_local_dev,
                           int32_t* idx_global_dev, void* stream_handle);

/* pgas_m_weighted_stats_n per run: w (R, N), T0 (R, N, M, nvar), T1 (R, N, M, M), T2 (R, N, nvar, nvar), T3 (R, N) -> S0 (R, M, nvar),
 * S1 (R, M, M), S2 (R, nvar, nvar), S3 (R); slice r is bit-identical to pgas_m_weighted_stats_n on run r's slices (the chunks of the
 * two-pass reduction start at each run's first particle).  R <= 65535. */
int pgas_m_runs_weighted_stats(pgas_ctx* ctx, int32_t R, int64_t N, int32_t M, int32_t nvar, const double* w_dev, const double* T0_dev,
                               const double* T1_dev, const double* T2_dev, const double* T3_dev, double* S0_dev, double* S1_dev, double* S2_dev,
                               double* S3_dev, void* stream_handle);

/* R marginalised Particle-Gibbs CHAINS (src/Algorithm3.py under src/Algorithm2.py) in the launches of one (pgas_amd/marginal_chains.py,
 * DESIGN.md section 23): the layout and the conventions of the pgas_m_runs_* entry points above -- arrays (R, N, ...) with run r at slice r,
 * global ancestor indices for the per-particle kernels -- plus what the conditional filter has per run.  Asynchronous on the caller's
 * stream, no host synchronisation, no allocation beyond pgas_m_mniw_solve_n's own failure counter (first solve of a context).
 *
 * pgas_m_runs_mniw_solve_n: pgas_m_mniw_solve_n over the R N particles with per-run reference statistics R0 (R, M, nvar), R1 (R, M, M);
 *   particle p adds the slice of run p / N.  Slice r of every output, Lfac included, is bit-identical to pgas_m_mniw_solve_n on run r's
 *   slices with R0[r], R1[r] (the same kernels; their run length 0 is the shared R0 / R1 of the single-run entry point).
 * pgas_m_runs_lbm_diff: pgas_m_lbm_diff with r2_dev (R), r3_dev (R), one pair per run; slice r bit-identical to the single-run call.
 * pgas_m_runs_categorical: one categorical draw per run, idx[r] = min(searchsorted(cumsum(softmax(logw[r])), u[r]), N - 1)
 *   (src/Algorithm3.py:117-127 and :293-294), logw (R, N), u (R), idx (R) int32, N <= 1024 (PGAS_E_ARG beyond), one workgroup per run; R may
 *   exceed what is resident.  Defined arithmetic: e_i = pgas_exp(logw_i - max logw); thread t of 256 sums its four
 *   consecutive particles 4 t .. 4 t + 3 in ascending order; the 256 totals are scanned by Kogge-Stone (distances 1, 2, ..., 128);
 *   c_i = (scanned total of thread t - 1) + (the thread's running sum); S = the last scanned total; idx = min(#{i < N : c_i < u S}, N - 1).
 *   A row that holds a NaN, or whose maximum is -inf or +inf, gives N - 1.  anc_local_dev / anc_global_dev (R, N) int32, nullable: slot
 *   N - 1 of row r receives idx[r] and r N + idx[r] (the reference particle's ancestor); no other slot is written.
 * pgas_m_runs_backtrace: pgas_reconstruct_trajectory for every run: trace (T, R, N, w), anc (T-1, R, N) int32 holding each run's OWN
 *   indices (NULL allowed when T = 1), idx (R) int32 on the device -> out (R, T, w); row r is bit-identical to pgas_reconstruct_trajectory
 *   on run r's slices.  An idx outside [0, N) is clamped into it. */
int pgas_m_runs_mniw_solve_n(pgas_ctx* ctx, int32_t R, int64_t N, int32_t M, int32_t nvar, double scale, const int32_t* anc_dev, const double* P0_dev,
                             const double* P1_dev, const double* T0_dev, const double* T1_dev, const double* R0_dev, const double* R1_dev,
                             const double* phi_dev, double* m_dev, double* c_dev, double* q_dev, double* logdet_dev, double* Lfac_dev,
                             void* stream_handle);
int pgas_m_runs_lbm_diff(pgas_ctx* ctx, int32_t R, int64_t N, int32_t M, const double* T2_dev, const double* T3_dev, const double* q1_dev,
                         const double* logdet1_dev, const double* q2_dev, const double* logdet2_dev, double P2, double P3, const double* r2_dev,
                         const double* r3_dev, double* out_dev, void* stream_handle);
int pgas_m_runs_categorical(pgas_ctx* ctx, int32_t R, int32_t N, const double* logw_dev, const double* u_dev, int32_t* idx_dev,
                            int32_t* anc_local_dev, int32_t* anc_global_dev, void* stream_handle);
int pgas_m_runs_backtrace(pgas_ctx* ctx, int32_t R, int32_t N, int32_t T, int32_t w, const double* trace_dev, const int32_t* anc_dev,
                          const int32_t* idx_dev, double* out_dev, void* stream_handle);

/* Open-loop simulation of a grey-box model under K coefficient draws in ONE launch (pgas_amd/model_rollout.py): the
 * model's transition f and output g as register programs (the opcodes of pgas_m_expr_eval), L latent functions
 * xi_i = A_k,i phi_i(v_i) [+ Lrow_k,i e] as its interface variables, P replicates per draw, the time loop inside the kernel.  For t = 0 .. T-1
 *   y_t = g(x_t, u_t, xi(x_t, u_t))  -> out_y (K, T, P, ny)   (optional),     x_t+1 = f(x_t, u_t, xi(x_t, u_t)) [+ Qc z]  -> out_x (K, T, P, nx),
 * row 0 of out_x being x_0.  Step t -> t+1 reads input row t (the convention of Algorithm1 and of the reference's validation loop, NOT
 * the shifted one of pgas_rollout).
 *
 * Programs: f, g and the feature programs share ONE register numbering over nreg <= 96 registers: [0, nx) the state, [nx, nx + nu) the
 * input row, then the interface variables' components (n_in = nx + nu + sum n_i registers in all), then [n_in, n_in + nconst) one pool of
 * constants (consts_dev), then temporaries.  No instruction may write below n_in + nconst, and the result registers f_out / g_out lie at
 * or above it.  Every program is given twice, (ninstr, 4) int32 words on the device and the same words on the host, where they are checked.
 * Latent function i: v_d = register sel[d] -- a state / input register (feat = 0: the pick of pgas_m_hilbert_basis) or, with feat = 1, a
 * result register of the feature program fcode_dev run first; phi = the Hilbert basis of pgas_m_hilbert_basis at v (D <= 4, idx_dev (M, D));
 * xi_i = A_dev[k] (n, M) phi as an ascending-m fma chain from 0, plus Lrow_dev[k] (n, n; lower triangle read) times standard normals when
 * Lrow_dev is not NULL.
 * Random numbers (seeds_dev (K) u64; NULL: none may be asked for): process noise z = row p0 + p of pgas_m_rng_normal(seed_k,
 * PGAS_STREAM_M_STATE, t + 1, ...) (nx columns) for the step that produces x_t+1, as Algorithm1 draws it; the interface variable's normals
 * on PGAS_STREAM_M_ROLLOUT_INTVAR + i at time t (n_i columns); x0_mode 0: x_0 = m0 + L0 z on PGAS_STREAM_M_INIT_STATE at time 0
 * (m0L0_dev: m0 (nx) then L0 (nx, nx)); x0_mode 1 / 2 / 3: x0_dev (nx) / (K, nx) / (K, P, nx).
 * Asynchronous on the caller's stream, no host synchronisation, no allocation; the device arrays must stay valid until the kernel has run.
 * PGAS_E_ARG (with a message, the context stays usable): K < 1, P < 1, T < 1, L outside [1, 4], more than 96 registers or a register number
 * out of range, nx + nu + sum n_i != n_in, D > 4, n_i > 8, noise without seeds, or an LDS need ((nreg + max(nx, n_i)) * 512 B + 8 sum n_i M_i
 * B) above what a workgroup of the device can have. */
#define PGAS_STREAM_M_ROLLOUT_INTVAR 192u /* + i: normals of the rollout's interface-variable noise (none of the filter's streams) */
#define PGAS_M_ROLLOUT_MAXIV 4
typedef struct pgas_m_rollout_latent {
    int32_t M, D, n, feat;
    int32_t sel[4];
    double div[4], center[4], L[4], size[4];
    const int32_t* idx_dev;
    const double* A_dev;
    const double* Lrow_dev;
    const int32_t* fcode_dev;
    const int32_t* fcode_host;
    int32_t f_ninstr, reserved;
} pgas_m_rollout_latent;
typedef struct pgas_m_rollout_desc {
    int32_t K, T, P, L, nx, nu, ny, n_in, nconst, nreg, x0_mode, f_ninstr, g_ninstr, reserved;
    int32_t f_out[8], g_out[8];
    int64_t p0;
    const double* consts_dev;
    const int32_t* fcode_dev;
    const int32_t* gcode_dev; /* with out_y_dev, or both NULL */
    const int32_t* fcode_host; /* the same program words on the host: every register number is checked before the launch */
    const int32_t* gcode_host;
    const double* inputs_dev; /* (T, nu); may be NULL when nu = 0 */
    const uint64_t* seeds_dev;
    const double* Qc_dev;     /* (nx, nx) factor of the process noise, or NULL */
    const double* x0_dev;
    const double* m0L0_dev;
    double* out_x_dev;
    double* out_y_dev;
    pgas_m_rollout_latent lat[PGAS_M_ROLLOUT_MAXIV];
} pgas_m_rollout_desc;
int pgas_m_rollout(pgas_ctx* ctx, const pgas_m_rollout_desc* desc, void* stream_handle);

/* The same rollout reduced over its replicates inside the kernel ("Predictive moments and log score"): the clouds
 * (K, T, P, nx) and (K, T, P, ny) are never stored.  `desc` is pgas_m_rollout's descriptor; out_x_dev / out_y_dev are ignored and may be
 * NULL, the output program (gcode_dev, gcode_host, ny >= 1) is mandatory.  Replicate p carries exactly the x_t and y_t = g(x_t, u_t, xi_t)
 * that pgas_m_rollout stores for it.  Per draw k and step t = 0 .. T-1, over the replicates p < P:
 *   sum_dev / sumsq_dev (K, T, nx + ny): sum v and sum (v * v) of the channels x_0 .. x_nx-1, yhat_0 .. yhat_ny-1, where yhat = g, or with
 *     noise != 0 yhat_j = g_j + sum_{l <= j} LR[j,l] e_l (ascending fma chain) with e = row p0 + p of pgas_m_rng_normal(seed_k,
 *     PGAS_STREAM_M_ROLLOUT_OBS, t, ...) (ny columns);
 *   lpd_dev (K, T) or NULL (then no log-density is evaluated): log (1/P) sum_p N(y_t; g(x_t^p, ...), R) from y_dev (T, ny), with
 *     l = cR - |LRinv (y_t - g)|^2 / 2 formed by pgas_m_expr_eval mode 2's operations; -inf when every replicate's density underflows,
 *     NaN where row t of y holds a NaN.
 * LR / LRinv: row-major ny x ny (lower Cholesky factor of the output noise and its inverse), by value.  The summation order is defined
 * (a balanced adjacent-pair tree over each block of 64 replicates, then the B = ceil(P / 64) blocks in ascending order from +0.0) and
 * does not depend on K.  part_dev: the caller's scratch of at least K B T (2 (nx + ny) + 2) doubles; its content afterwards is unspecified.
 * Asynchronous on the caller's stream, no host synchronisation, no allocation.  PGAS_E_ARG (with a message, the context stays usable):
 * everything pgas_m_rollout refuses, and P > 2^20, ny < 1 or no output program, lpd_dev without y_dev, noise without seeds, NULL sums,
 * part_dev NULL or part_bytes too small, or an LDS need ((nreg + max(nx, n_i, ny)) * 512 B + 8 sum n_i M_i B) above the device's. */
#define PGAS_STREAM_M_ROLLOUT_OBS 200u /* normals of the predicted observations' noise: clear of the filter's ids (< 160) and of 192 + i */
#define PGAS_M_ROLLOUT_STATS_MAX_P (1 << 20)
typedef struct pgas_m_rollout_stats_desc {
    const double* y_dev;
    double* sum_dev;
    double* sumsq_dev;
    double* lpd_dev;
    double* part_dev;
    uint64_t part_bytes;
    double cR;
    int32_t noise, reserved;
    double LR[64], LRinv[64];
} pgas_m_rollout_stats_desc;
int pgas_m_rollout_stats(pgas_ctx* ctx, const pgas_m_rollout_desc* desc, const pgas_m_rollout_stats_desc* st, void* stream_handle);

/* A bootstrap particle filter per coefficient draw of the same grey-box model on a held-out record, K draws in ONE launch (DESIGN.md
 * section 16): one workgroup per draw, N = desc->P particles (1 .. 1024, and what the model's LDS need allows), resampling at every step.
 * `desc` is pgas_m_rollout's descriptor: p0 must be 0 (the Philox particle index of slot i is i), out_x_dev / out_y_dev are ignored, the
 * output program is mandatory, seeds_dev is mandatory.  Per draw k and step t = 0 .. T-1 (row t holds x_t, u_t, xi_t, y_t = g(x_t, u_t, xi_t)):
 *   x_0 by x0_mode (with P := N), x_t+1 = f(x_t, u_t, xi_t)[a_t[i]] [+ Qc z], z = row i of pgas_m_rng_normal(seed_k, PGAS_STREAM_M_STATE,
 *     t + 1, ...): the pair (x_t, xi_t) is the RESAMPLED particle's -- xi_t is gathered with the noise of its ancestor, not recomputed;
 *   l_i = cR - |LRinv (y_t - g_i)|^2 / 2 (pgas_m_expr_eval mode 2's operations) from y_dev (T, ny);
 *   ell_dev (K, T): log (1/N) sum_i exp l_i from the exact fixed-point sum; -inf when every density underflows, NaN where row t of y holds
 *     a NaN (such a row is a pure prediction step: no weights, identity ancestors);  loglik_dev (K): sum_t ell over the rows without a NaN;
 *   a_t = systematic resampling with u = pgas_m_rng_uniform(seed_k, PGAS_STREAM_M_RESAMPLE, t), the identity when no weight is positive.
 * Nullable outputs: ess_dev (K, T) = (sum w)^2 / sum w^2; pred_sum_dev / pred_sumsq_dev (K, T, nx + ny), both or neither: sum v and
 * sum (v * v) over the unweighted cloud of the channels x_0 .. x_nx-1, g_0 .. g_ny-1 before y_t is used; filt_sum_dev (K, T, nx) / wtot_dev
 * (K, T), both or neither: sum_i w_i x_i and sum_i w_i (the filtered mean is their quotient); the traces x_dev (K, T, N, nx), anc_dev
 * (K, T, N) int32, lw_dev (K, T, N) = l, yhat_dev (K, T, N, ny) = g.  The summation order is defined (ascending particle row per lane, a
 * balanced adjacent-pair tree over the 256 lanes) and does not depend on K.
 * Asynchronous on the caller's stream, no host synchronisation, no allocation.  PGAS_E_ARG (with a message, the context stays usable):
 * everything pgas_m_rollout_stats refuses of `desc`, and N < 1 or N > 1024, p0 != 0, NULL y / ell / loglik, half of a pair, no seeds,
 * K > 65535, or an LDS need (ceil(N / 64) (nreg + nz) 512 B + 8 sum n_i M_i B with nz = max(nx, n_i, ny, nx + sum n_i), plus the kernel's
 * static LDS) above the device's; that message names the largest N that fits. */
typedef struct pgas_m_filter_desc {
    const double* y_dev;
    double* ell_dev;
    double* loglik_dev;
    double* ess_dev;
    double* pred_sum_dev;
    double* pred_sumsq_dev;
    double* filt_sum_dev;
    double* wtot_dev;
    double* x_dev;
    int32_t* anc_dev;
    double* lw_dev;
    double* yhat_dev;
    double cR;
    double LRinv[64];
} pgas_m_filter_desc;
int pgas_m_filter(pgas_ctx* ctx, const pgas_m_rollout_desc* desc, const pgas_m_filter_desc* fl, void* stream_handle);

/* h-step-ahead predictions of the same grey-box model from the filter's particle trace, every origin row of every draw in ONE launch
 * (DESIGN.md section 18): a workgroup per (draw, chunk of origin rows).  `desc` is pgas_m_rollout's descriptor as pgas_m_filter takes it:
 * P = N, p0 must be 0, x0_* and out_* are ignored, the output program is mandatory, seeds_dev is mandatory when there is any noise.
 * x_dev (K, T, N, nx) is pgas_m_filter's trace: row s was stored before y_s was used, a sample of p(x_s | y_{0:s-1}).  Per draw k, origin
 * row s and lead l = 0 .. min(H, T - s) - 1 (target row tau = s + l, horizon h = l + 1):
 *   l = 0: the cloud is x[k, s]; l >= 1: x_tau = f(x_tau-1, u_tau-1, xi_tau-1) [+ Qc z], z = row i of pgas_m_rng_normal(seed_k,
 *     PGAS_STREAM_M_STATE, tau, p0 = l << 32, ...): the lead sits in the high word of the Philox particle index, so the noise names (target
 *     row, lead, particle) alone -- not H, not the chunking, not the draws of the launch; the interface variables xi_tau use the same particle
 *     index on PGAS_STREAM_M_ROLLOUT_INTVAR + i at time tau (at l = 0 the filter's own normals);
 *   sum_dev / sumsq_dev (K, H, T, nx + ny) at [k, l, tau]: sum v and sum (v * v) over the N particles of the channels x_0 .. x_nx-1,
 *     g_0 .. g_ny-1 in pgas_m_filter's summation order (at l = 0 its pred_sum / pred_sumsq bit for bit);
 *   lpd_dev (K, H, T) or NULL (then no log-density is evaluated and y_dev may be NULL): log (1/N) sum_i N(y_tau; g_i, R) with
 *     l_i = cR - |LRinv (y_tau - g_i)|^2 / 2 (pgas_m_expr_eval mode 2's operations) as (m + pgas_log(sum_i pgas_exp(l_i - m))) - pgas_log(N),
 *     m = max l; -inf when every density underflows, NaN where row tau of y holds a NaN;
 *   cloud_x_dev (K, H, T, N, nx) / cloud_y_dev (K, H, T, N, ny) or NULL, each on its own: the channels per particle.
 * Entries with tau < l (no origin row) are NaN in every output.
 * Asynchronous on the caller's stream, no host synchronisation, no allocation.  PGAS_E_ARG (with a message, the context stays usable):
 * everything pgas_m_rollout_stats refuses of `desc`, and N < 1 or N > 1024, p0 != 0, H < 1 or H > T, NULL x / sum / sumsq, lpd_dev without
 * y_dev, K > 65535, more than 65535 chunks of pgas_m_forecast_origins_per_block() origin rows, or an LDS need (ceil(N / 64) (nreg + nz)
 * 512 B + 8 sum n_i M_i B with the filter's nz, plus the kernel's static LDS) above the device's. */
typedef struct pgas_m_forecast_desc {
    const double* x_dev;
    const double* y_dev;
    double* sum_dev;
    double* sumsq_dev;
    double* lpd_dev;
    double* cloud_x_dev;
    double* cloud_y_dev;
    int32_t H, reserved;
    double cR;
    double LRinv[64];
} pgas_m_forecast_desc;
int pgas_m_forecast(pgas_ctx* ctx, const pgas_m_rollout_desc* desc, const pgas_m_forecast_desc* fc, void* stream_handle);
/* Origin rows per workgroup of pgas_m_forecast: a built-in constant, or the environment variable PGAS_M_FORECAST_TB (measurements only).
 * No result bit depends on it. */
int pgas_m_forecast_origins_per_block(void);

/* The empirical predictive CDF of the grey-box model at given thresholds, counted inside the kernels: the twins of
 * pgas_rollout_cdf / pgas_forecast_cdf (pgas_hip.h).  Value channels per replicate or particle, in pgas_m_rollout_stats' order: x_j
 * (j < nx), then yhat_j (j < ny) = g_j, or with noise != 0 yhat_j = g_j + sum_{l <= j} LR[j,l] e_l (ascending fma chain).  thr_dev
 * (T, nx + ny, J) fp64, 1 <= J <= PGAS_CDF_MAX_J and (nx + ny) J <= 64 (one wave lane per (channel, threshold) slot, so
 * J_max = min(16, 64 / (nx + ny))).  The comparison is IEEE's v <= thr: a NaN on either side counts nothing, +inf counts every finite
 * value, -inf counts none.  Counts are exact integers: no result bit depends on the wave layout, the block split, p0 chunking, H, the
 * origin chunking or on which draws share a launch.
 *
 * pgas_m_rollout_cdf: the open loop.  `desc` as pgas_m_rollout_stats takes it (out_x_dev / out_y_dev ignored, the output program
 *   mandatory); replicate p0 + p carries exactly the x_t, y_t that pgas_m_rollout stores for it and e = row p0 + p of
 *   pgas_m_rng_normal(seed_k, PGAS_STREAM_M_ROLLOUT_OBS, t, ...): the values pgas_m_rollout_stats draws.
 *   count_dev (K, T, nx + ny, J) int32: count[k, t, c, j] = #{p < P : v_c <= thr[t, c, j]}, every row t = 0 .. T-1.  With P > 64 the
 *   output is zeroed on the stream (hipMemsetAsync) and the blocks of 64 replicates add to it with integer atomics.
 * pgas_m_forecast_cdf: horizons 1 .. H from pgas_m_filter's trace x_dev (K, T, N, nx).  `desc` as pgas_m_forecast takes it; the clouds are
 *   pgas_m_forecast's, bit for bit (lead l = h - 1 uses the Philox particle index l << 32 | i); e = row i of pgas_m_rng_normal(seed_k,
 *   PGAS_STREAM_M_ROLLOUT_OBS, tau, p0 = (l + 1) << 32, ...): the high word is never 0, so no counter is shared with the open loop.
 *   count_dev (K, H, T, nx + ny, J) int32 at [k, h - 1, tau] against the thresholds of the TARGET row, thr[tau]; entries with tau < h - 1
 *   (no origin row) are -1.
 * Both: asynchronous on the caller's stream, no host synchronisation, no allocation.  PGAS_E_ARG (with a message, the context stays
 * usable): everything pgas_m_rollout_stats (rollout) / pgas_m_forecast (forecast) refuses of `desc`, P > 2^20 (rollout), J < 1,
 * J > PGAS_CDF_MAX_J, (nx + ny) J > 64 (the message names J_max), NULL thr_dev / count_dev / x_dev, noise without seeds, H < 1 or H > T. */
typedef struct pgas_m_rollout_cdf_desc {
    const double* thr_dev;
    int32_t* count_dev;
    int32_t J, noise;
    double LR[64];
} pgas_m_rollout_cdf_desc;
typedef struct pgas_m_forecast_cdf_desc {
    const double* x_dev;
    const double* thr_dev;
    int32_t* count_dev;
    int32_t H, J, noise, reserved;
    double LR[64];
} pgas_m_forecast_cdf_desc;
int pgas_m_rollout_cdf(pgas_ctx* ctx, const pgas_m_rollout_desc* desc, const pgas_m_rollout_cdf_desc* cd, void* stream_handle);
int pgas_m_forecast_cdf(pgas_ctx* ctx, const pgas_m_rollout_desc* desc, const pgas_m_forecast_cdf_desc* fc, void* stream_handle);

/* The smoothing distribution of the same grey-box model by backward simulation (FFBSi) over pgas_m_filter's particle trace, B
 * trajectories of each of K draws in ONE launch: one workgroup per draw.  `desc` is pgas_m_rollout's descriptor as
 * pgas_m_filter took it: P = N, p0 must be 0, x0_* and out_* are ignored, seeds_dev and Qc_dev (a model with process noise) are mandatory.
 * x_dev (K, T, N, nx), anc_dev (K, T, N) int32, lw_dev (K, T, N), yhat_dev (K, T, N, ny) are the traces of a pgas_m_filter call with the
 * same descriptor, y_dev (T, ny) its observations.  LQinv: row-major nx x nx, the inverse of chol(Q); cQ = -nx/2 log 2pi - sum log diag
 * chol(Q).  The filter's particle is the pair (x_t, xi_t) and xi_t+1 depends on x_t+1 alone, so the backward kernel needs only
 * N(xt_t+1; f(x_t^i, u_t, xi_t^i), Q); xi_t^i = the interface variables of (x[k,t,i], u_t) with the Philox particle index i at time t --
 * what the filter computed -- is recomputed, and f_i = the transition program on (x[k,t,i], u_t, xi_t^i), without noise.
 * Per draw k, trajectory g = b0 + b (b < B) and row t from T - 1 down, with u = pgas_u52 of words 0, 1 of pgas_rng_block(seed_k,
 * PGAS_STREAM_M_SMOOTH, 0, t, particle = g):
 *   l_i = lw[k,t,i], or +0.0 for every i when y_t holds a NaN; v_i = l_i on row T - 1, below it v_i = l_i + h_i, h_i = cQ - 0.5 q,
 *     q = sum_j e_j e_j, e_j = sum_l (xt_t+1,l - f_i,l) LQinv[j,l], ascending from 0.0, every product and sum rounded on its own
 *     (pgas_m_expr_eval mode 2's operations);
 *   k = pgas_seg_ref(max v), q_i = the fixed-point exp of pgas_seg_arg(v_i, k), c the integer inclusive cumsum, S = c_N-1 2^-51;
 *   j_t = min(#{i < N : c_i 2^-51 < u S}, N - 1); when S is not in (0, inf): g mod N on row T - 1, anc[k,t,j_t+1] clamped into [0, N) below;
 *   xt_t = x[k,t,j_t], xit_t = xi_t^{j_t}, yhat_t = yhat[k,t,j_t].
 * Outputs, each nullable (not all of them): idx_dev (K, B, T) int32 = j; xs_dev (K, B, T, nx) = xt; xis_dev (K, B, T, nxi) = xit with
 * nxi = sum n_i; sum_dev / sumsq_dev (K, T, nx + ny), both or neither: sum v and sum (v * v) over the call's trajectories of the channels
 * xt_j then yhat_j; xi_sum_dev / xi_sumsq_dev (K, T, nxi), both or neither, of xit_j -- value b at position b of a balanced adjacent-pair
 * tree over 256 positions, +0.0 at positions >= B; and the traces fmean_dev (K, T, N, nx) = f_i (rows 0 .. T - 2 are written) and xi_dev
 * (K, T, N, nxi) = xi_t^i.  Row T - 1 evaluates the interface variables only when xis, xi_sum or xi is asked for.  Trajectory g depends on
 * (seed_k, t, g) and the trace alone: not on B, b0 or the draws that share the launch.
 * Asynchronous on the caller's stream, no host synchronisation, no allocation.  PGAS_E_ARG (with a message, the context stays usable):
 * everything pgas_m_rollout_stats refuses of `desc`, and B outside 1 .. PGAS_M_SMOOTH_MAX_B, b0 < 0, N < 1 or N > 1024, p0 != 0, a NULL
 * trace, y, seeds or Qc, half of a pair, an interface output with nxi > PGAS_M_SMOOTH_MAX_XI, K > 65535, a non-finite LQinv or cQ, no
 * output at all, or an LDS need (pgas_m_filter's dynamic need plus this kernel's static LDS) above the device's.
 * The kernel has instances with the state dimension as a constant (nx <= 4) and one that reads it at run time (nx = 5 .. 8); the
 * environment variable PGAS_M_SMOOTH_RUNTIME_NX=1 (tests and measurements only) selects the latter for every nx.  No result bit depends on it. */
#define PGAS_STREAM_M_SMOOTH 201u /* the backward draw's uniforms: clear of the filter's ids (< 160), of 192 + i and of 200 */
#define PGAS_M_SMOOTH_MAX_B 256
#define PGAS_M_SMOOTH_MAX_XI 16
typedef struct pgas_m_smooth_desc {
    const double* x_dev;
    const int32_t* anc_dev;
    const double* lw_dev;
    const double* yhat_dev;
    const double* y_dev;
    int32_t* idx_dev;
    double* xs_dev;
    double* xis_dev;
    double* sum_dev;
    double* sumsq_dev;
    double* xi_sum_dev;
    double* xi_sumsq_dev;
    double* fmean_dev;
    double* xi_dev;
    int64_t b0;
    int32_t B, reserved;
    double cQ;
    double LQinv[64];
} pgas_m_smooth_desc;
int pgas_m_smooth(pgas_ctx* ctx, const pgas_m_rollout_desc* desc, const pgas_m_smooth_desc* sm, void* stream_handle);

#ifdef __cplusplus
}
#endif
#endif /* PGAS_MARGINAL_H */
