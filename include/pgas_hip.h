/*
 * pgas_hip.h -- C ABI of libpgas_hip.so, the MI355X (gfx950) engine for the conditional-SMC /
 * PGAS hot path of VolkmannB/bayesian-inference-with-explicit-and-implicit-prior-knowledge.
 *
 * The reference has no FFI: its boundary is the Python call surface of src/PGAS.py.  Each entry
 * point below names the reference interface it stands under (paths relative to the reference
 * root); INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C, no C++ types, no torch types; every function returns 0 on success or a negative
 *     PGAS_E_* code, and pgas_last_error(ctx) gives the message.  No exceptions cross the ABI.
 *   - "dev" pointers are device (HBM) pointers on ctx's device, "host" pointers are ordinary
 *     host memory read during the call.  The caller owns every buffer it passes; the library
 *     owns only the context (model tables, traces, scan scratch).
 *   - all work is enqueued on the caller's stream (`stream` = hipStream_t, e.g.
 *     torch.cuda.current_stream().cuda_stream); calls return without synchronising unless noted.
 *   - one context per device; a context is not thread-safe, distinct contexts are independent.
 *   - arithmetic is fp64 throughout (reference src/__init__.py:4) in the canonical order of
 *     DESIGN.md section 4; ancestor indices are int32.
 *   - particle arrays are row-major (N, nx) exactly as the reference's state_trace[t]
 *     (src/PGAS.py:160-162).
 */
#ifndef PGAS_HIP_H
#define PGAS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGAS_OK 0
#define PGAS_E_ARG (-1)      /* bad argument / unsupported model shape */
#define PGAS_E_HIP (-2)      /* a HIP runtime call failed */
#define PGAS_E_STATE (-3)    /* call sequence error (e.g. sweep before set_params) */
#define PGAS_E_NOMEM (-4)    /* device allocation failed */

typedef struct pgas_ctx pgas_ctx;

/*
 * Declarative model description.  The reference passes Python callables that JAX traces
 * (basis_fcn, likelihood_fcn: src/PGAS.py:20-21,31-32); a HIP kernel cannot, so the two families
 * the reference actually instantiates are described by tables:
 *
 *   basis_fcn(state, input)  = Hilbert-space GP basis of src/BasisFunctions.py:8-80 evaluated at
 *        v[sel[d]] with v = concat(state, input):   phi_m = nrm * prod_d sin(pi * idx[m][d] * r_d),
 *        r_d = v[sel[d]] * alpha[d] + beta[d]
 *        (alpha_d = 1/(div_d * 2 L_d), beta_d = (L_d - center_d)/(2 L_d), nrm = prod_d L_d^-1/2;
 *         covers src/Toy_Example.py:146, src/EMPS.py:110-113, src/SingleMassOscillator.py:151).
 *   likelihood_fcn(obs, state, input) = log N(obs; H state, R)
 *        (src/Toy_Example.py:142-144, src/EMPS.py:250-252), given as H, LRinv = chol(R)^-1 and
 *        cR = -ny/2 log(2 pi) - sum(log diag chol(R)).
 */
typedef struct pgas_model_desc {
    int32_t N;            /* particles            (N_samples,   src/PGAS.py:26)  */
    int32_t T;            /* time steps           (observations.shape[0], :159)  */
    int32_t nx, ny, nu;   /* state / observation / input dimensions (nx<=2, ny<=2, nu<=4) */
    int32_t M, D;         /* basis functions, basis input dimension (D<=3) */
    const int32_t* idx;   /* host (M,D): frequency j of basis m in dimension d, reference order */
    const int32_t* sel;   /* host (D)  */
    const double* alpha;  /* host (D)  */
    const double* beta;   /* host (D)  */
    double nrm;
    const double* H;      /* host (ny,nx) */
    const double* LRinv;  /* host (ny,ny) lower triangular */
    double cR;
    const double* m0;     /* host (nx)      init_state_mean (src/PGAS.py:29) */
    const double* L0;     /* host (nx,nx)   chol(init_state_cov) lower (src/PGAS.py:30) */
    const double* y;      /* host (T,ny)    observations */
    const double* u;      /* host (T,nu)    inputs; may be NULL when nu == 0 */
    int32_t device;       /* HIP device ordinal */
    int32_t keep_logw_trace; /* 1: keep the (T,N) log-weight trace like src/PGAS.py:163 (costs 8 B/particle-step) */
    int32_t no_fast_variant; /* test knob: 1 = never use the k_propagate instantiations specialised for the reference's model shapes */
} pgas_model_desc;

/* Replaces condSequentialMonteCarlo.__init__ (src/PGAS.py:24-43) / PGAS.__init__ (:237-260):
 * copies the model tables to the device.  Traces are allocated lazily by the first sweep. */
int pgas_create(const pgas_model_desc* desc, pgas_ctx** out);
void pgas_destroy(pgas_ctx* ctx);
/* message of the last failing call on ctx (or of the last failing pgas_create when ctx == NULL) */
const char* pgas_last_error(const pgas_ctx* ctx);

/* Canonical-arithmetic constants the build was made with (segment length, fixed-point bits). */
int32_t pgas_segment_size(void);

/* Parameters of the transition x_t ~ N(A phi(x_{t-1},u_t), S) for the following step/sweep calls
 * (coeff_mat, error_cov of src/PGAS.py:85-86,180-181).  A_dev: device (nx,M) row-major.
 * LS_host = chol(S) lower (nx,nx), LSinv_host = LS^-1, cS = -nx/2 log(2 pi) - sum(log diag LS). */
int pgas_set_params(pgas_ctx* ctx, const double* A_dev, const double* LS_host, const double* LSinv_host,
                    double cS, void* stream);

/* The same with error_cov on the DEVICE: S_dev (nx,nx) row-major, symmetric positive definite.  Its Cholesky factor, the factor's
 * inverse and the constant are formed by the pack kernel (IEEE sqrt, /, *, - and the shared logarithm, in a fixed order), so a Gibbs
 * iteration -- PGAS.sample_params -> sweep, src/PGAS.py:366-378 -- needs no host round trip.  pgas_get_params reads back the factor,
 * its inverse and the constant the kernels use (synchronises the stream; for tests and for replaying a chain with the oracle). */
int pgas_set_params_dev(pgas_ctx* ctx, const double* A_dev, const double* S_dev, void* stream);
int pgas_get_params(pgas_ctx* ctx, double* LS_host, double* LSinv_host, double* cS, void* stream);

/* Test hook: phi (np,M) = basis_fcn(x[p], inputs[t]) in reference order
 * (vmap(basis_fcn) of src/PGAS.py:52-54). x_dev (np,nx). */
int pgas_basis_eval(pgas_ctx* ctx, const double* x_dev, int64_t np, int32_t t, double* phi_dev, void* stream);

/* Test hook: aux (N,nx) = _generate_auxiliary_states (src/PGAS.py:45-57). */
int pgas_aux_states(pgas_ctx* ctx, const double* x_dev, int32_t t, double* aux_dev, void* stream);

/* condSequentialMonteCarlo._init_algorithm + the conditioning of :194: x0 (N,nx) ~ N(m0,P0),
 * x0[N-1] = ref0 (host, nx). */
int pgas_init_state(pgas_ctx* ctx, uint64_t seed, const double* ref0_host, double* x0_dev, void* stream);

/* condSequentialMonteCarlo.step (src/PGAS.py:79-153): one conditional-SMC step at `time` = t.
 * logw_dev (N) may be NULL (= zeros, the t = 1 case of :163); ref_t_host (nx).
 * Outputs: logw_new_dev (N), x_new_dev (N,nx), anc_dev (N int32 = a_indices). */
int pgas_step(pgas_ctx* ctx, int32_t t, uint64_t seed, const double* logw_dev, const double* x_dev,
              const double* ref_t_host, double* logw_new_dev, double* x_new_dev, int32_t* anc_dev, void* stream);

/* condSequentialMonteCarlo.__call__ (src/PGAS.py:176-228): the whole sweep incl. the final index
 * draw (:224-225) and the back-trace (src/Filtering.py:40-55), all on the device.
 * ref_dev (T,nx) in, traj_dev (T,nx) out. */
int pgas_sweep(pgas_ctx* ctx, uint64_t seed, const double* ref_dev, double* traj_dev, void* stream);

/* Device pointers of the traces of the last sweep: x_trace (T,N,nx), anc_trace (T-1,N) int32,
 * logw_last (N) = log_weights_trace[T-1], logw_trace (T,N) or NULL.  Valid until the next sweep.
 * x_trace / anc_trace are single arrays on an unsharded context (state_trace / ancestor_trace of src/PGAS.py:160-164).  A sharded
 * context (and any context after PGAS_OPT_TRACE_BLOCK_BYTES) keeps them as ROW BLOCKS -- consecutive time rows in allocations of at
 * most 1 GiB, so that each can cross process boundaries as one HIP IPC handle -- and refuses x_trace / anc_trace here (PGAS_E_STATE):
 * pgas_trace_layout gives the blocking, pgas_trace_row the device pointer of one time row. */
int pgas_get_traces(pgas_ctx* ctx, double** x_trace, int32_t** anc_trace, double** logw_last, double** logw_trace);
#define PGAS_TRACE_X 0    /* T rows of (N, nx) f64: state_trace[t] */
#define PGAS_TRACE_LA 1   /* T rows of nseg*1024 f64: log p(y_t | aux_t)      (hand-off rows between the two pipelines) */
#define PGAS_TRACE_H 2    /* T rows: log N(ref_t; aux_t, S) */
#define PGAS_TRACE_LN 3   /* T rows: log p(y_t | x_t) */
#define PGAS_TRACE_ANC 4  /* T-1 rows of N int32: ancestor_trace[t] */
/* info4 = {rows, rows per block (a power of two; = rows when the trace is one array), blocks, bytes per row} */
int pgas_trace_layout(pgas_ctx* ctx, int32_t kind, int64_t* info4);
int pgas_trace_row(pgas_ctx* ctx, int32_t kind, int32_t t, void** row_dev);

/* Index drawn by the last sweep at src/PGAS.py:225 (synchronises the stream). */
int pgas_last_final_index(pgas_ctx* ctx, int64_t* idx, void* stream);
/* PGAS_OPT_TAIL_GROUPS: *gave_up = 1 when a scanner wave of k_step ever ran out of its (bounded) wait for the segment partials on
 * this context, 0 otherwise (synchronises the stream).  Such a sweep's results are not valid; pgas_last_final_index then fails
 * with PGAS_E_STATE.  The state is never cleared: destroy the context. */
int pgas_scan_status(pgas_ctx* ctx, int32_t* gave_up, void* stream);

/* Measurement aid (bench.py): when on, pgas_sweep launches its two per-step kernels -- k_step (resampling
 * search + softmax scans) and k_propagate (all particles through a chunk of time steps) -- with start/stop HIP events
 * attached to the dispatch (hipExtLaunchKernelGGL), which carry the kernel's own begin/end timestamps on the stream it
 * runs on.  pgas_get_profile synchronises and returns, for the last sweep, the counts and summed durations of the launches
 * that were timed: every 16th by default (on = 1), every n-th for on = n > 1, every launch for on < 0 (timing every launch
 * slows the sweep it measures by ~8 %: timed dispatches serialise with their neighbours on the stream).
 * No reference counterpart (the reference has no timing code). */
int pgas_set_profiling(pgas_ctx* ctx, int32_t on);
int pgas_get_profile(pgas_ctx* ctx, int64_t* resample_launches, double* resample_ms, int64_t* propagate_launches,
                     double* propagate_ms, void* stream);
/* What the last sweep launched: info4 = {time steps per k_propagate launch, group-scan placement (0: k_groups launches between the
 * steps, 1: k_step<LOCAL> scans all groups in every workgroup, 2: inside k_step by polling scanner waves, 3: no group
 * scans at all -- the one-launch small sweep (k_sweep_duo / k_sweep_chains) ran; + 16 when
 * the last sweep replayed the captured HIP graph; + 32 when k_propagate ran its matrix-core form, PGAS_OPT_MFMA_PROPAGATE;
 * + 64 when k_step ran its whole-segment instance, + 128 when k_propagate ran its own, see PGAS_OPT_STEP_GENERIC),
 * padded innermost basis extent JP, particles per basis pass P} -- bench.py labels its kernels from this. */
int pgas_get_launch_info(pgas_ctx* ctx, int32_t* info4);

/* Tuning / test knobs.  PGAS_OPT_PROPAGATE_CHUNK: time steps per k_propagate launch (0 = the whole sweep in one launch). */
#define PGAS_OPT_PROPAGATE_CHUNK 1
#define PGAS_OPT_PROPAGATE_LDS 4 /* bytes of LDS reserved per k_propagate workgroup while overlapping (occupancy cap) */
#define PGAS_OPT_OVERLAP 3 /* 1 (default): weight recursion on an internal stream, concurrent with k_propagate */
#define PGAS_OPT_FORCE_SLOW_RESAMPLE 2 /* 1: never take k_step<LOCAL> (overrides PGAS_OPT_LOCAL_GROUPS; kept for the tests) */
/* 1: CORRECTED mode, not the reference's behaviour.  src/PGAS.py:131-133 propagates every particle from its own previous
 * state (`state`, not `state[a_indices]`) although the ancestors are recorded and used for the weights and the
 * back-trace.  With this option pgas_step / pgas_sweep draw x_t[i] ~ N(A phi(x_{t-1}[a_i]), S) as a particle filter should
 * (and as src/Algorithm1.py:286-292 does).  Same random numbers, same weight formula; the step becomes a serial chain of
 * three launches.  Default 0 = reproduce the reference. */
#define PGAS_OPT_RESAMPLE_BEFORE_PROPAGATE 5
#define PGAS_OPT_LOCAL_GROUPS 7 /* 1: on a single device with <= 1024 segments every k_step workgroup scans all groups itself (k_step<LOCAL>, no k_groups launch between the steps); default 0, the k_groups path is faster */
#define PGAS_OPT_MAX_LEAD 11 /* sweep: k_propagate may run at most this many event groups (PGAS_OPT_EVENT_STRIDE steps each) ahead of the weight recursion; 0 = unbounded */
#define PGAS_OPT_SYRK_SPLITS 10 /* pgas_suffstats: number of row splits of the Z^T Z product (partial slabs summed in split order); 0 = automatic (about two workgroups per CU) */
#define PGAS_OPT_TAIL_GROUPS 9 /* 1: single device only: the group scans run inside k_step, by scanner waves that poll for the segment partials the segment workgroups hand over as tagged 8-byte granules, instead of k_groups launches between the steps; bit-identical, measured neutral, default 0.  pgas_scan_status reports a scanner that gave up its bounded wait */
#define PGAS_OPT_EVENT_STRIDE 8 /* k_propagate launches per event that gates the weight recursion's stream (default 8) */
#define PGAS_OPT_SMALL_SWEEP 14 /* 1 (default): a context of at most one segment of particles (N <= 1024 -- the reference's own operating point is N = 200) runs the whole sweep, x_0 to back-trace, as ONE launch instead of ~3 dependent launches per time step: two workgroups (k_sweep_duo), one propagating every step ahead into a ring in device memory, the other running the weight recursion behind it with both fixed-point CDFs, the auxiliary log-likelihoods and the scan scratch in LDS; the propagation noise comes from one grid-wide launch in front of it.  2: the same work on one workgroup, all waves in lock step (k_sweep_chains, the kernel of pgas_chains_sweep, with one chain on this context's own buffers; that kernel keeps no log-weight trace, so a context created with keep_logw_trace runs k_sweep_duo under 2 as under 1: same results, same pgas_get_launch_info); 0: the general multi-launch path at every size.  Bit-identical results */
#define PGAS_OPT_MFMA_PROPAGATE 15 /* 1: models with a 3-D basis, n_x = 2 and the 729-function index ball of the 11 x 11 x 11 grid (EMPS / Vehicle, src/EMPS.py:101-113) run the innermost sum of k_propagate's contraction A phi(x) (src/PGAS.py:52-55) on v_mfma_f64_16x16x4_f64, whose four-term accumulation is the canonical ascending fma chain: bit-identical to the vector-ALU form.  Default 0: on MI355X the f64 MFMA occupies the SIMD's vector pipeline (no overlap with vector fp64 work, tools/probes/mfma_valu_overlap_probe.hip) and the padded tiles carry 1.5x the flops: 126 against 114 us per step */
#define PGAS_OPT_GRAPH 13 /* 1: pgas_sweep captures its launches (k_init ... k_backtrace, both streams) once in a HIP graph and replays it per sweep on an internal stream -- seed, uniforms, transition parameters, reference trajectory and result all live in device memory the graph's kernels read at execution time; same kernels, same order: identical results.  0: enqueue every launch (what profiled sweeps, the corrected mode and sharded sweeps always do).  Default: off -- on the HIP 7.0 runtime bundled with PyTorch 2.10 the replay measured slower than enqueueing at every size */
#define PGAS_OPT_TRACE_BLOCK_BYTES 12 /* before the first sweep / pgas_shard_setup: keep the traces in row blocks of at most this many bytes (0 = default: one array per trace on an unsharded context, 1 GiB blocks on a shard); small values are a test knob that puts block boundaries inside short sweeps */
#define PGAS_OPT_STEP_GENERIC 16 /* 1: k_step runs its general instance also where the whole-segment one applies (one unsharded device, N a multiple of 1024: an instance of k_step without the guards for ragged segments and ranks, bit-identical by construction; pgas_get_launch_info reports which ran), and so does k_propagate (its whole-segment instance exists for the SingleMassOscillator shape with ny = 1 and 16-byte aligned rows).  Default 0.  The A/B switch of that instance, and a test knob (the Python binding sets it on every context it creates when the environment variable PGAS_STEP_GENERIC is 1) */
#define PGAS_OPT_MNIW_VALU 6 /* 1: pgas_m_mniw_solve factorises column by column on the VALU instead of in MFMA-blocked panels; 2: the two-rows-per-lane kernels of 63 <= M <= 126 at every M (test knobs) */
int pgas_set_option(pgas_ctx* ctx, int32_t option, int64_t value);

/* Free functions of src/Filtering.py on the device.  systematic_SISR(key, w) (:6-37): u = the uniform the reference draws
 * from `key` (:19); weights are passed as log-weights (log 0 = -inf allowed, negative weights have no logarithm: the
 * reference's clip at :23 is the caller's clamp).  reconstruct_trajectory(Particles, ancestry, idx) (:40-55). */
int pgas_systematic_resample(pgas_ctx* ctx, double u, const double* logw_dev, int32_t* idx_dev, void* stream);
/* The same with the uniform u read from device memory at execution time (graph-captured filter steps, include/pgas_marginal.h). */
int pgas_systematic_resample_dev(pgas_ctx* ctx, const double* u_dev, const double* logw_dev, int32_t* idx_dev, void* stream);
int pgas_reconstruct_trajectory(pgas_ctx* ctx, const double* x_dev, const int32_t* anc_dev, int32_t T, int32_t nx, int64_t idx,
                                double* traj_dev, void* stream);

/* ---- particle-sharded sweep.  The reference is single-process; these entry points have no
 * counterpart there.  One context per rank holds N_local = N_global / world particles (N_local a multiple of the
 * segment size).  Per time step there is ONE collective between STEP(t) and GROUPS(t): an all-gather of the segment
 * partials (pgas_shard_buffers: segk_w/segs_w -> segk_g/segs_g); every rank then computes the same group records.
 * Ancestors that live on another rank are read through peer mappings (pgas_shard_set_peer; pgas_ipc_export / pgas_ipc_open
 * carry the mappings between processes).  Results do not depend on `world`. */
#define PGAS_SHARD_INIT 0        /* x_0                      (ref_dev)                         */
#define PGAS_SHARD_PROPAGATE 1   /* time steps [t, t_aux)    (ref_dev)                         */
#define PGAS_SHARD_STEP 2        /* launch t in [1,T]: resample step t-1 (t>1), scan step t (t<T) */
#define PGAS_SHARD_GROUPS 3      /* group records of step t, after the all-gather               */
#define PGAS_SHARD_FINAL_SCAN 4  /* softmax scan of logw_{T-1}; all-gather follows              */
#define PGAS_SHARD_FINAL 5       /* group records + final index (src/PGAS.py:224-225)           */
#define PGAS_SHARD_BACKTRACE 6   /* trajectory (traj_dev), every rank computes the same one     */
int pgas_shard_setup(pgas_ctx* ctx, int32_t rank, int32_t world);
int pgas_shard_buffers(pgas_ctx* ctx, void** out17, int64_t* sizes3);
/* The seven buffers a rank's peers read -- which = 0, 1: the segment cumsums of the two scan buffers; 2..6: the la, h, ln, x and
 * ancestor traces -- block by block: pgas_shard_layout -> info2 = {blocks, rows per block}; pgas_shard_block -> this rank's block;
 * pgas_shard_set_peer_block installs rank `peer`'s block as addressable from this process (every rank, the own one included, must be
 * installed before the first sweep).  All ranks have the same layout (equal N_local and T). */
int pgas_shard_layout(pgas_ctx* ctx, int32_t which, int64_t* info2);
int pgas_shard_block(pgas_ctx* ctx, int32_t which, int32_t blk, void** ptr_dev, int64_t* bytes);
int pgas_shard_set_peer_block(pgas_ctx* ctx, int32_t peer, int32_t which, int32_t blk, const void* ptr_dev);
int pgas_shard_run(pgas_ctx* ctx, int32_t phase, int32_t t, int32_t t_aux, uint64_t seed, const double* ref_dev, double* traj_dev,
                   void* stream);
/* The whole sharded sweep inside the library: pgas_shard_unique_id on one rank (128 bytes, to be broadcast by the host),
 * pgas_shard_comm_init on every rank (ncclCommInitRank with the rank / world of pgas_shard_setup), then pgas_shard_sweep runs
 * the phases above with the per-step all-gather issued as an RCCL call on the same stream -- no host round trip per step.
 * RCCL is bound with dlopen at first use (PGAS_E_STATE if it cannot be loaded).
 * pgas_shard_set_collective replaces the RCCL calls of that loop by a host callback (same loop, same launches): it is how
 * the multi-rank loop is exercised where RCCL is not usable (several ranks sharing one device in the tests).  The callback
 * gets the scan-buffer parity whose segk_w/segs_w must be gathered into segk_g/segs_g (parity < 0: end-of-sweep barrier)
 * and the stream the loop runs on; it must leave the gathered arrays visible to work enqueued on that stream afterwards. */
typedef int (*pgas_allgather_fn)(void* user, int32_t parity, void* stream);
int pgas_shard_unique_id(void* id128);
int pgas_shard_comm_init(pgas_ctx* ctx, const void* id128);
int pgas_shard_set_collective(pgas_ctx* ctx, pgas_allgather_fn fn, void* user);
int pgas_shard_sweep(pgas_ctx* ctx, uint64_t seed, const double* ref_dev, double* traj_dev, int32_t propagate_chunk, void* stream);
/* Measurement aid: issue the step's RCCL all-gather `reps` times on `stream` (between sweeps only). */
int pgas_shard_probe_collective(pgas_ctx* ctx, int32_t reps, void* stream);
/* Version of the HIP runtime this library is bound to in the running process (hipRuntimeGetVersion: 7.2.x = 702xxxxx), -1 on failure
 * (recorded by bench.py; the HIP 7.0 runtime bundled with PyTorch 2.10+rocm7.0 never returns from hipIpcOpenMemHandle for an
 * allocation of 2 GiB or more, which is why a shard's traces are row blocks of at most 1 GiB). */
int32_t pgas_hip_runtime_version(void);

/* HIP IPC plumbing for peers in OTHER processes: a 64-byte handle of block `blk` of this rank's buffer `which` (as in
 * pgas_shard_layout), and the mapping of a peer's handle into this process (xGMI peer access is enabled on first use). */
int pgas_ipc_export(pgas_ctx* ctx, int32_t which, int32_t blk, void* handle64);
int pgas_ipc_open(pgas_ctx* ctx, const void* handle64, void** ptr);

/* Test hook: the arithmetic primitives shared with the CPU oracle (include/pgas_detmath.h, include/pgas_canon.h) evaluated ON THE
 * DEVICE, element by element, so that the shared header is checked on gfx950 directly and not only through whole-step parity:
 * which = 0 exp(x), 1 log(x), 2 sin(pi x) -> out0 / cos(pi x) -> out1, 3 Philox4x32-10 (w: 6 words per element = counter[4], key[2];
 * outw: 4 words), 4 pgas_seg_ref(x), 5 pgas_seg_arg(x, y), 6 pgas_lvl_scale(x, y), 7 the Box-Muller pair of the Philox block of w,
 * 8 the segment scans' quantised softmax numerator rint(exp(x) 2^51) (device-only shortcut, x <= 0.25) as a double, 9 the device-only
 * Box-Muller chain of the SingleMassOscillator k_propagate on a GIVEN Philox output block (w: 6 words per element, the first four are
 * the block) -> out0, out1, 10 the device-only guarded sin(pi x) -> out0 / cos(pi x) -> out1. */
int pgas_detmath_eval(int32_t device, int32_t which, const double* x_dev, const double* y_dev, const uint32_t* w_dev, int64_t n,
                      double* out0_dev, double* out1_dev, uint32_t* outw_dev, void* stream);

/* Sufficient statistics of PGAS.sample_params (src/PGAS.py:294-303, BI:53-61) without the prior:
 * traj_dev (T,nx) -> T0 (M,nx), T1 (M,M) [fp64 MFMA SYRK], T2 (nx,nx); T3 = T-1.
 * Pairs traj[:-1] with inputs[:-1] (quirk Q3). */
int pgas_suffstats(pgas_ctx* ctx, const double* traj_dev, double* T0_dev, double* T1_dev, double* T2_dev, void* stream);

/* ---- C independent chains of this context's model on its one device.  Chain c has its own key, reference,
 * (A, S) and traces and computes exactly what the single-chain entry points compute with them; the launches cover all chains at once,
 * one workgroup per chain for the sweep, so a Gibbs iteration of C chains is a fixed number of launches whatever C is.  Every array is
 * (C, ...) with chain c's slice at offset c.  C = 1 .. 65535.  Per-chain buffers are allocated on first use and grown (not shrunk) to
 * the largest C seen: T N (16 nx / 2 + 16 + 4) bytes of traces and noise per chain plus small tables (14.4 MB at N = 200, T = 2000,
 * nx = 2); PGAS_E_NOMEM when they do not fit.  Refused with PGAS_E_ARG, the context staying usable: N > 1024 (the sweep is the
 * one-workgroup sweep), the corrected mode, keep_logw_trace, a sharded context, a coefficient tensor that does not fit the LDS of a
 * workgroup beside the kernel's own.  The single-chain entry points are unaffected. */

/* coeff_mat / error_cov of every chain: A_dev (C, nx, M), S_dev (C, nx, nx) on the device, factored as pgas_set_params_dev does
 * (bit for bit).  Sets the number of chains the next pgas_chains_sweep runs. */
int pgas_chains_set_params_dev(pgas_ctx* ctx, int32_t C, const double* A_dev, const double* S_dev, void* stream);
/* condSequentialMonteCarlo.__call__ for every chain: seeds_dev (C) u64 keys, ref_dev (C, T, nx) in, traj_dev (C, T, nx) out. */
int pgas_chains_sweep(pgas_ctx* ctx, int32_t C, const uint64_t* seeds_dev, const double* ref_dev, double* traj_dev, void* stream);
/* Device pointers of the last batched sweep's traces: x_trace (C, T, N, nx), anc_trace (C, max(T-1, 1), N) int32, logw_last (C, N).
 * Valid until the next pgas_chains_* call that grows the buffers or sweeps. */
int pgas_chains_get_traces(pgas_ctx* ctx, double** x_trace, int32_t** anc_trace, double** logw_last);
/* Final indices (src/PGAS.py:225) of the C chains of the last batched sweep into idx_host (C) (synchronises the stream). */
int pgas_chains_final_index(pgas_ctx* ctx, int32_t C, int64_t* idx_host, void* stream);
/* Key handling of PGAS.__call__ per chain, keys_dev (C) u64 -> out_dev (6, C) u64: next key, step key, parameter key and the parameter
 * key's (key_A, key_chi, key_norm) of PGAS.param_draws.  first = 1: the start of the chain, key, key_para = split(key) (src/PGAS.py:356;
 * step key 0); first = 0: one Gibbs iteration, key, key_step = split(key), key, key_para = split(key) (:365, :377).  split(k)[i] is
 * Philox4x32-10 of counter (i, 0, 0, 16) under key k (pgas_amd.random.split).  out_dev may be keys_dev. */
int pgas_chains_keys(pgas_ctx* ctx, int32_t C, const uint64_t* keys_dev, int32_t first, uint64_t* out_dev, void* stream);
/* The random numbers PGAS.param_draws consumes (src/PGAS.py:323-338), per chain from rows 3..5 of a pgas_chains_keys block keys6_dev
 * (6, C): chi2_dev (C, nx) = chi^2(df - i), normals_T_dev (C, nx, nx), normals_A_dev (C, nx, M) -- the streams and arithmetic of
 * pgas_m_rng_chi2 / pgas_m_rng_normal, bit for bit. */
int pgas_chains_param_draws(pgas_ctx* ctx, int32_t C, const uint64_t* keys6_dev, double df, double* chi2_dev, double* normals_T_dev,
                            double* normals_A_dev, void* stream);
/* pgas_suffstats of C trajectories: traj_dev (C, T, nx) -> T0 (C, M, nx), T1 (C, M, M), T2 (C, nx, nx) in one set of launches. */
int pgas_chains_suffstats(pgas_ctx* ctx, int32_t C, const double* traj_dev, double* T0_dev, double* T1_dev, double* T2_dev, void* stream);

/* ---- one model learned from E records (experiments) that share (A, S).  The context is created as usual on
 * the CONCATENATION of the records, T = sum T_e rows of y and u, and pgas_records_set declares where each record starts.  The sweep
 * then runs one workgroup per (record, chain): nothing propagates across a seam, and workgroup (c, e) computes bit for bit what a
 * context created on record e alone computes from seeds[c, e], record e's reference rows and chain c's (A, S) -- time inside a record
 * is local (Philox counters, uniforms, noise).  Records never wait for each other, so ragged lengths cost tail idle time only.  The
 * parameters are the chains': set them with pgas_chains_set_params_dev for the same C.  Every (C, T, ...) array below holds record e's
 * rows at row0[e].  The limits are those of pgas_chains_*: N <= 1024, no corrected mode, no keep_logw_trace, no shard, a coefficient
 * tensor that fits the LDS of a workgroup; C, E = 1 .. 65535.  The state traces and the noise live in the chains' buffers: a record
 * sweep and a chain sweep each invalidate the other's traces.  Every other entry point of the context, the single-record ones and
 * pgas_chains_* included, keeps treating it as ONE record of T rows. */

/* E records: rows row0[e] .. row0[e+1]-1 of the context's y / u (row0[0] = 0, row0[E] = T, strictly increasing, every T_e >= 2).
 * m0_host (E, nx) / P0_host (E, nx, nx): per-record initial state, or NULL for the context's own on every record.
 * PGAS_E_ARG on a bad table, on N > 1024, on a sharded / corrected / keep_logw_trace context (the limits of pgas_chains_*).
 * Replaces an earlier table (synchronises the device). */
int pgas_records_set(pgas_ctx* ctx, int32_t E, const int32_t* row0_host, const double* m0_host, const double* P0_host);
/* seeds_dev (C, E) from C step keys: seeds[c, 0] = step_keys[c]; seeds[c, e] = child e of step_keys[c] (pgas_amd.random.split(k, n)[e])
 * for e >= 1, so that E = 1 is exactly pgas_chains_sweep. */
int pgas_records_seeds(pgas_ctx* ctx, int32_t C, const uint64_t* step_keys_dev, uint64_t* seeds_dev, void* stream);
/* One conditional-SMC sweep per (chain, record) in one launch: seeds_dev (C, E) u64, ref_dev (C, T, nx) in, traj_dev (C, T, nx) out.
 * PGAS_E_STATE when no record table is set or the parameters are set for a different C.  Asynchronous on `stream`. */
int pgas_records_sweep(pgas_ctx* ctx, int32_t C, const uint64_t* seeds_dev, const double* ref_dev, double* traj_dev, void* stream);
/* Device pointers of the last record sweep's traces: x_trace (C, T, N, nx), anc_trace (C, T, N) int32 (record e's T_e - 1 rows start
 * at row0[e]; the last row of each record is unused), logw_last (C, E, N).  Valid until the next sweep or parameter call. */
int pgas_records_get_traces(pgas_ctx* ctx, double** x_trace, int32_t** anc_trace, double** logw_last);
/* Final indices of the last record sweep into idx_host (C, E) (synchronises the stream). */
int pgas_records_final_index(pgas_ctx* ctx, int32_t C, int64_t* idx_host, void* stream);
/* pgas_chains_suffstats over the T - 1 rows with the seams taken out: a row whose successor is the first row of a record enters as
 * zeros, so (T0, T1, T2) is the sum over the records of each record's own statistics; T3 = sum (T_e - 1). */
int pgas_records_suffstats(pgas_ctx* ctx, int32_t C, const double* traj_dev, double* T0_dev, double* T1_dev, double* T2_dev, void* stream);

/* ---- open-loop simulation of the learned transition model under K parameter draws (the reference's
 * EMPS_Validation_Simulation, src/EMPS.py:129-151, for one parameter matrix).  Draw k rolls P replicates forward over the context's
 * input rows, x_t = A_k phi(x_{t-1}, u_t) + LS_k z_t for t = 1 .. T - 1, in one launch of one workgroup per draw; out_dev (K, T, P, nx).
 * The step is the propagation of pgas_sweep -- the same input row, arithmetic and Philox counters (seed_k, PGAS_STREAM_PROP, t, particle
 * p0 + p) -- so replicate p0 + p of draw k equals particle p0 + p (below the conditioned one) of a sweep with seeds[k], A_k, S_k bit for
 * bit, and calls with p0 = 0, P, 2 P, ... are the replicates of one larger rollout.  seeds_dev = S_dev = NULL: no process noise.
 * Row 0: x0_mode 0 draws x_0 ~ N(m0, P0) as the sweep does (PGAS_STREAM_INIT, particle p0 + p; needs seeds); 1: x0_dev (nx) for every
 * draw and replicate; 2: (K, nx) per draw; 3: (K, P, nx) per draw and replicate.  S_k is factored on the device as
 * pgas_chains_set_params_dev does.  The packed parameters live in buffers of the rollout's own (grown to the largest K seen:
 * 8 nx prod(J) + 80 + 8 nx nx bytes per draw), so the parameters and traces of the single-chain and pgas_chains_* entry points are
 * untouched.  Asynchronous on `stream`, no host synchronisation.  PGAS_E_ARG: K < 1, P < 1, P > 1024, a context of more than 1024
 * particles (it has no one-workgroup variant), seeds without S or S without seeds, x0_mode 0 without seeds, x0_mode 1..3 without
 * x0_dev; PGAS_E_NOMEM when the draws' parameters do not fit (nothing is kept).  The context stays usable after either. */
int pgas_rollout(pgas_ctx* ctx, int32_t K, int32_t P, int64_t p0, const uint64_t* seeds_dev, const double* A_dev, const double* S_dev,
                 const double* x0_dev, int32_t x0_mode, double* out_dev, void* stream);
/* The same rollout reduced over its replicates inside the kernel ("Predictive moments and log score"): nothing per
 * replicate is stored.  Arguments as pgas_rollout, but 1 <= P <= 2^20 in one call (grid (K, ceil(P / 1024)); x0_mode 3 indexes x0_dev
 * (K, P, nx) by the replicate).  Value channels per step t (row 0 included) and replicate: the state x_j, j < nx, then the predicted
 * observation yhat_j = sum_k H[j,k] x_k, j < ny (ascending fma chain from +0.0); with LR (HOST pointer, ny ny doubles, the lower Cholesky
 * factor of R; needs seeds) the chain goes on with LR[j,l] e_l, l = 0 .. j, e = normals of (seed_k, PGAS_STREAM_OBS, t, p0 + p).
 * sum_dev / sumsq_dev (K, T, nx + ny) receive sum_p v and sum_p (v v) in a defined order: per lane ascending register row, the balanced
 * adjacent-pair tree over the 256 lanes, ascending block.  lpd_dev (K, T), or NULL for no log score (no likelihood is evaluated):
 * log (1/P) sum_p p(y_t | x_t^p) under the context's observations and likelihood, = (M + log S) - log P from the blocks' (max, sum exp);
 * -inf when every density underflows, NaN when y_t holds a NaN.  The blocks' partial sums live in a buffer of the context
 * (K ceil(P / 1024) T (2 (nx + ny) + 2) doubles, grown, not shrunk); the packed parameters are pgas_rollout's.  Asynchronous on `stream`,
 * no host synchronisation.  PGAS_E_ARG as pgas_rollout (P > 2^20 instead of P > 1024), and LR without seeds; PGAS_E_NOMEM keeps nothing;
 * the context stays usable after either. */
int pgas_rollout_stats(pgas_ctx* ctx, int32_t K, int32_t P, int64_t p0, const uint64_t* seeds_dev, const double* A_dev, const double* S_dev,
                       const double* x0_dev, int32_t x0_mode, const double* LR, double* sum_dev, double* sumsq_dev, double* lpd_dev, void* stream);

/* ---- a bootstrap particle filter per parameter draw on the context's observations: the one-step-ahead
 * predictive density of every observation row, its sum (the log marginal likelihood of the record under (A_k, S_k)) and the filtered
 * state, for K draws in one launch of one workgroup per draw, with the context's N <= 1024 particles, observations, inputs and
 * likelihood.  Per draw k and step t: x_0 as pgas_rollout's x0_mode says (0: drawn on PGAS_STREAM_INIT for every particle; 1: x0_dev
 * (nx); 2: (K, nx); 3: (K, N, nx)), x_t[i] = A_k phi(x_{t-1}[a_{t-1}[i]], u_t) + LS_k z with z on (seeds[k], PGAS_STREAM_PROP, t, i) --
 * propagated from the RESAMPLED state; l_i = log p(y_t | x_t[i]); the fixed-point scan of the one-workgroup sweep gives the reference
 * k = ceil(max l log2 e), the numerators q_i and S = (sum q_i) 2^-51; systematic resampling at every step with the uniform of
 * (seeds[k], PGAS_STREAM_RESAMPLE, t), the identity map when S is not in (0, inf).
 *   ell_dev (K, T)      log (1/N) sum_i p(y_t | x_t[i]) = fma(k, ln2_lo, fma(k, ln2_hi, log S)) - log N; -inf when S = 0; NaN when y_t
 *                       holds a NaN (such a row is a pure prediction step: identity ancestors)
 *   loglik_dev (K)      sum_t ell[k, t], ascending t from +0.0, over the rows whose y_t holds no NaN
 *   ess_dev (K, T)      or NULL: (S S) / sum_i (w_i w_i), w_i = q_i 2^-51; 0 when S is not in (0, inf)
 *   pred_sum_dev, pred_sumsq_dev (K, T, nx + ny)   or both NULL: sum_i v and sum_i (v v) over the unweighted cloud BEFORE y_t is used, of
 *                       the state x_j and the predicted observation yhat_j = sum_k H[j,k] x_k, in pgas_rollout_stats' order
 *   filt_sum_dev (K, T, nx), wtot_dev (K, T)   or both NULL: sum_i (w_i x_ij) in the same order, and S: the filtered mean is their ratio
 *   x_dev (K, T, N, nx), anc_dev (K, T, N) int32   or NULL, each: the particle and ancestor traces (a_t resamples step t's cloud)
 * S_k is factored on the device as pgas_chains_set_params_dev does; the packed parameters live in buffers of the filter's own (grown to
 * the largest K seen, not shrunk), so the single-chain, pgas_chains_* and pgas_rollout* buffers are untouched.  Asynchronous on
 * `stream`, no host synchronisation.  PGAS_E_ARG: K < 1, a context of more than 1024 particles, missing seeds or S, a bad x0_mode or
 * x0_mode 1..3 without x0_dev, half of a both-or-neither pair, a coefficient tensor that does not fit the LDS of a workgroup beside the
 * kernel's own; PGAS_E_NOMEM keeps nothing; the context stays usable after either. */
int pgas_filter(pgas_ctx* ctx, int32_t K, const uint64_t* seeds_dev, const double* A_dev, const double* S_dev, const double* x0_dev,
                int32_t x0_mode, double* ell_dev, double* loglik_dev, double* ess_dev, double* pred_sum_dev, double* pred_sumsq_dev,
                double* filt_sum_dev, double* wtot_dev, double* x_dev, int32_t* anc_dev, void* stream);

/* ---- h-step-ahead predictions from the filter's particle trace: p(y_tau | y_{0:tau-h}, A_k, S_k) for
 * h = 1 .. H and every row tau of the context's record, for K draws in one launch of one workgroup per (draw, chunk of origin rows).
 * x_dev (K, T, N, nx) is the trace pgas_filter stored for the same seeds, A and S: row s, stored before y_s is used, is a sample of
 * p(x_s | y_{0:s-1}).  Per draw k, origin row s and lead l = 0 .. min(H, T - s) - 1 (target row tau = s + l, horizon h = l + 1): the
 * cloud is c_0[i] = x[k, s, i] and c_l[i] = A_k phi(c_{l-1}[i], u_{s+l}) + LS_k z with pgas_rollout's arithmetic and z on (seeds[k],
 * PGAS_STREAM_FORECAST, t = s + l, particle = l << 32 | i) -- the noise depends on the target row, the lead and the particle alone,
 * not on H or on the draws that share the launch.  Value channels per particle: the state c_j, j < nx, then yhat_j = sum_k H[j,k] c_k
 * (ascending fma chain from +0.0; no measurement noise).
 *   sum_dev, sumsq_dev (K, H, T, nx + ny)   sum_i v and sum_i (v v) at [k, h - 1, tau, :] in pgas_rollout_stats' order (per lane ascending
 *                       register row, the balanced adjacent-pair tree over the 256 lanes); at h = 1 they equal pgas_filter's pred_sum /
 *                       pred_sumsq bit for bit
 *   lpd_dev (K, H, T)   or NULL (no likelihood is evaluated): log (1/N) sum_i p(y_tau | c_l[i]) = (m + log s) - log N with m = max_i l_i,
 *                       s = sum_i exp(l_i - m); -inf when every density underflows; NaN when y_tau holds a NaN
 * The entries with tau < h - 1 have no origin row: the call writes NaN there, in all three outputs.  S_k is factored on the device and the
 * packed parameters go to the filter's buffers (grown to the largest K seen), so the single-chain, pgas_chains_* and pgas_rollout*
 * buffers are untouched.  Asynchronous on `stream`, no host synchronisation.  PGAS_E_ARG: K < 1, H < 1 or H > T, NULL x_dev, sum_dev or
 * sumsq_dev, missing seeds or S, a context of more than 1024 particles, a coefficient tensor that does not fit the LDS of a workgroup
 * beside the kernel's own; PGAS_E_NOMEM keeps nothing; the context stays usable after either. */
int pgas_forecast(pgas_ctx* ctx, int32_t K, int32_t H, const uint64_t* seeds_dev, const double* A_dev, const double* S_dev, const double* x_dev,
                  double* sum_dev, double* sumsq_dev, double* lpd_dev, void* stream);
/* origin rows one workgroup of pgas_forecast walks (the environment variable PGAS_FORECAST_TB overrides the built-in value, for
 * measurements); no result depends on it. */
int pgas_forecast_origins_per_block(void);

/* ---- the smoothing distribution p(x_{0:T-1} | y_{0:T-1}, A_k, S_k) by backward simulation (FFBSi) over pgas_filter's trace (DESIGN.md
 * section 21): B trajectories for each of K draws in one launch of one workgroup per draw.  x_dev (K, T, N, nx) and anc_dev (K, T, N)
 * are the traces pgas_filter stored for the same seeds, A and S.  Trajectory g = b0 + b of draw k walks t = T - 1 .. 0:
 *   v_i = l_i(t) [+ h_i for t < T - 1], l_i = loglik(y_t, x[k,t,i]) (+0.0 when y_t holds a NaN), h_i = log N(xt_{t+1}; mu_i, S_k) with
 *         mu_i = A_k phi(x[k,t,i], u_{t+1}) (the filter's transition mean) and the sweep's chain fma(-0.5, quad, cS);
 *   the fixed-point weights of the one-segment scan over i < N: k = pgas_seg_ref(max v), q_i, integer cumsum c_i, S = s 2^-51;
 *   u = pgas_u52 of words 0, 1 of pgas_rng_block(seeds[k], PGAS_STREAM_SMOOTH, 0, t, particle = g): it depends on (seed, t, g) alone;
 *   j_t = min(#{i : c_i 2^-51 < u S}, N - 1); when S is not in (0, inf): g mod N at t = T - 1, anc[k, t, j_{t+1}] below; xt_t = x[k,t,j_t].
 *   idx_dev (K, B, T) int32 or NULL          the indices j_t
 *   xs_dev (K, B, T, nx) or NULL             the trajectories xt
 *   sum_dev, sumsq_dev (K, T, nx + ny)       both or neither: sum_b v and sum_b (v v) over the call's B trajectories of the channels xt_j,
 *                       then yhat_j = sum_k H[j,k] xt_k (fma chain from +0.0), value b at position b of pgas_rollout_stats' 256-position
 *                       adjacent-pair tree, positions >= B holding +0.0
 * More than 256 trajectories go in further calls (b0 = 256, 512, ...); the caller adds the calls' sums.  The packed parameters go to the
 * filter's buffers, so the single-chain, pgas_chains_* and pgas_rollout* buffers are untouched.  Asynchronous on `stream`, no host
 * synchronisation.  PGAS_E_ARG: K < 1, B outside 1..256, b0 < 0, NULL x_dev, anc_dev, seeds or S, one of sum_dev / sumsq_dev without the
 * other, every output NULL, a context of more than 1024 particles, a coefficient tensor that does not fit the LDS of a workgroup beside
 * the kernel's own; PGAS_E_NOMEM keeps nothing; the context stays usable after either. */
int pgas_smooth(pgas_ctx* ctx, int32_t K, int32_t B, int64_t b0, const uint64_t* seeds_dev, const double* A_dev, const double* S_dev, const double* x_dev,
                const int32_t* anc_dev, int32_t* idx_dev, double* xs_dev, double* sum_dev, double* sumsq_dev, void* stream);

/* ---- calibration: the empirical predictive CDF at given thresholds, counted inside the kernels.  The posterior
 * predictive is the mixture over the draws, so its CDF is the mean of the per-draw CDFs: the per-draw counts add up exactly over draws
 * (per-draw quantiles do not combine).  Counts are integers, so no result bit depends on a summation order, the wave layout or the
 * block split. */
#define PGAS_CDF_MAX_J 16 /* thresholds per (row, channel) */
/* pgas_rollout_stats' rollout (same arguments, 1 <= P <= 2^20, grid (K, ceil(P / 1024)), the same value channels: the state x_j, j < nx,
 * then yhat_j = sum_k H[j,k] x_k, j < ny, with LR (HOST pointer or NULL) continued with LR[j,l] e_l, e on (seed_k, PGAS_STREAM_OBS, t,
 * p0 + p) -- the values pgas_rollout_stats sums), counted against thr_dev (T, nx + ny, J) fp64, 1 <= J <= PGAS_CDF_MAX_J:
 *   count_dev (K, T, nx + ny, J) int32   count[k, t, c, j] = #{p < P : v_c <= thr[t, c, j]} under the IEEE comparison: a NaN on either
 *                                        side counts nothing, +inf counts every finite value (and +inf), -inf counts none but -inf
 * Calls with p0 = 0, P, 2 P, ... add up to the counts of one larger rollout.  P > 1024: count_dev is zeroed on `stream` and the blocks
 * add their counts with integer atomics.  The packed parameters are pgas_rollout's.  Asynchronous on `stream`, no host synchronisation.
 * PGAS_E_ARG as pgas_rollout_stats, and J outside 1..PGAS_CDF_MAX_J, NULL thr_dev or count_dev; PGAS_E_NOMEM keeps nothing; the context
 * stays usable after either. */
int pgas_rollout_cdf(pgas_ctx* ctx, int32_t K, int32_t P, int64_t p0, const uint64_t* seeds_dev, const double* A_dev, const double* S_dev,
                     const double* x0_dev, int32_t x0_mode, const double* LR, const double* thr_dev, int32_t J, int32_t* count_dev, void* stream);
/* pgas_forecast's clouds (same x_dev, seeds, A, S and H; bit for bit the clouds pgas_forecast reduces), counted against the thresholds
 * of the TARGET row: thr_dev (T, nx + ny, J) serves every horizon.  Value channels as above; with LR (HOST pointer or NULL) the
 * measurement noise e is on (seed_k, PGAS_STREAM_OBS, t = tau, particle = (l + 1) << 32 | i), l = h - 1: the high word is never 0, so no
 * counter is shared with pgas_rollout_cdf's noise.
 *   count_dev (K, H, T, nx + ny, J) int32   count[k, h - 1, tau, c, j] = #{i < N : v_c <= thr[tau, c, j]}; -1 where tau < h - 1 (no
 *                                           origin row: the integer counterpart of pgas_forecast's NaN)
 * K = 64, H = 16, T = 2000, nx + ny = 3, J = 16 is 393 MB of counts; J = 1 (the PIT) is 25 MB.  The packed parameters are the filter's.
 * Asynchronous on `stream`, no host synchronisation.  PGAS_E_ARG as pgas_forecast, and J outside 1..PGAS_CDF_MAX_J, NULL thr_dev or
 * count_dev; PGAS_E_NOMEM keeps nothing; the context stays usable after either. */
int pgas_forecast_cdf(pgas_ctx* ctx, int32_t K, int32_t H, const uint64_t* seeds_dev, const double* A_dev, const double* S_dev, const double* x_dev,
                      const double* LR, const double* thr_dev, int32_t J, int32_t* count_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PGAS_HIP_H */
