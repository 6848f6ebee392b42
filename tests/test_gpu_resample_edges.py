"""The device resampling search on degenerate and multi-scale weights: every path of resample_search / window_head / cdf_count_wg
(csrc/pgas_resample.hip.h), the `no positive weight` branches of the one-launch sweeps, and the device-only quantiser dev_exp_q51_n,
against the canonical C oracle BIT FOR BIT (no tie allowance: both sides run the canonical arithmetic of DESIGN.md 4).

The log-weight vectors and the branch census (which path a workgroup is predicted to take, derived from the oracle's CDF records) come
from tests/resample_cases.py; tests/test_resample_cases.py pins the oracle itself against exact integer arithmetic on the same cases."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from common import canon, canon_model, experiments, pgas_amd
import resample_cases as rc

pytestmark = pytest.mark.gpu

SEED = 12345678
_POOL = ThreadPoolExecutor(8)   # the oracle is serial C behind ctypes (the GIL is released): slot ranges / steps are independent


def _eq(gpu, ref, what):
    g = gpu.cpu().numpy().reshape(np.shape(ref)) if isinstance(gpu, torch.Tensor) else np.asarray(gpu).reshape(np.shape(ref))
    assert np.array_equal(g, ref, equal_nan=g.dtype.kind == "f"), f"{what}: {int((g != ref).sum())} of {g.size} entries differ"


def _oracle_resample(lw, N, u):
    segk, segs, c = canon.segment_partials(lw)
    cuts = np.linspace(0, N, min(16, N) + 1).astype(np.int64)
    parts = _POOL.map(lambda k: canon.resample_range(segk, segs, c, N, u, int(cuts[k]), int(cuts[k + 1])), range(len(cuts) - 1))
    return np.concatenate(list(parts))


# ------------------------------------------------------------------------------------------ (a) direct resampling
@pytest.mark.parametrize("name", rc.NAMES)
def test_direct_resampling(name):
    """Engine.systematic_resample (k_segscan, k_groups, k_systematic) on every case, all N indices, host-u and device-u entry points."""
    from pgas_amd._lib import Engine

    lw, N, u = rc.case(name)
    exp = _oracle_resample(lw, N, u)
    eng = Engine.utility(N)
    got = eng.systematic_resample(u, lw).cpu().numpy()
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{name}: {bad.size} of {N} ancestors differ, first at slot {bad[0]} (workgroup {bad[0] // 1024}): {got[bad[0]]} != {exp[bad[0]]}"
    assert np.all(np.diff(got) >= 0) and got.min() >= 0 and got.max() < N
    ud = torch.tensor([u], dtype=torch.float64, device=eng.device)
    _eq(eng.systematic_resample(ud, lw), exp, f"{name}: device-u entry point")
    if name in rc.EMPTY_NAMES:
        assert np.array_equal(got, np.arange(N)), "no positive weight: identity"


# ------------------------------------------------------------------------------------------ (b) teacher-forced step
def _regimes(N):
    r = {
        "flat": rc.flat(N), "one_hot_last": rc.one_hot(N, N - 1), "one_hot_1024": rc.one_hot(N, 1024),
        "one_plus_tail": rc.one_plus_tail(N, (3 * N) // 4, 0.99), "all_empty": rc.all_empty(N), "nan_and_empty": rc.nan_and_empty(N),
        "with_nan": rc.with_nan(N), "huge_range": rc.huge_range(N), "stairs700": rc.stairs(N, 700),
    }
    if N >= 70000:
        r.update({f"staged_{k}": rc.staged(N, k, *rc.STAGED_AT.get(k, (50, 2))) for k in (3, 4, 7, 8, 9)})
        r["staged_flushed"] = rc.staged(N, 6, 30, 2, fill=500.0)
    return r


_STEP_PROBLEMS = {"smo": lambda: experiments.smo_pgas(T=6), "veh27": lambda: experiments.vehicle_pgas(T=6, M=27)}


@pytest.mark.parametrize("corrected", [False, True], ids=["default", "corrected"])
@pytest.mark.parametrize("name,N", [("smo", 1025), ("smo", 70000), ("smo", 200000), ("veh27", 70000)])
def test_teacher_forced_step(name, N, corrected):
    """csmc.step (k_front, k_groups, k_count, k_back / k_back_corrected) with the cases injected as log_weights: new log-weights, new
    states and ancestors against the oracle's step, NaN equal to NaN.  The particles sit within 1e-3 of one point, so the likelihood
    changes the injected weights by little and the census of the step's own CDF (from the oracle's l_aux + log_weights) shows the regime.
    A SUBSET of the cases, for run time: SMO at N = 1025 takes the regimes that need no second group (no staged ones), SMO at N = 70000
    all of _regimes, and SMO at N = 200000 and Vehicle-27 six of them; every case in full is the business of test_direct_resampling."""
    pb = _STEP_PROBLEMS[name]()
    A, S = experiments.initial_params(pb)
    cm = canon_model(pb, N)
    cm.set_corrected(corrected)
    csmc = pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn,
                                             resample_before_propagate=corrected)
    LS, LSinv, cS = cm.chol_parts(S)
    t = 2
    x = pb.X_true[t - 1] + 1e-3 * np.random.default_rng(N).standard_normal((N, pb.nx))
    regs = _regimes(N)
    if name != "smo" or N == 200000:
        regs = {k: regs[k] for k in ("one_plus_tail", "all_empty", "with_nan", "staged_8", "staged_9", "stairs700")}
    ora = dict(zip(regs, _POOL.map(lambda lw: cm.step(t, SEED, x, lw, A, LS, LSinv, cS, pb.X_true[t], debug=True), regs.values())))
    seen = set()
    for reg, lw in regs.items():
        lwo, xo, ao, dbg = ora[reg]
        seen |= rc.branches(rc.census(dbg["lw1"], dbg["u"][0]))
        lwg, xg, ag = csmc.step(SEED, t, torch.as_tensor(lw), torch.as_tensor(x), A, S, pb.X_true[t])
        _eq(ag, ao, f"{reg}: a_indices")
        _eq(xg, xo, f"{reg}: new_state")
        _eq(lwg, lwo, f"{reg}: new_log_weights")
        if reg in ("all_empty", "nan_and_empty"):
            assert np.array_equal(ao, np.arange(N)), "no positive weight: identity ancestors, reference ancestor N - 1"
    print(f"step census {name} N={N}: {sorted(seen)}")
    assert "!valid" in seen and "ns=1" in seen
    if N >= 70000:
        assert "ns>8" in seen and len([b for b in seen if b.startswith("ns=")]) >= 3


# ------------------------------------------------------------------------------------------ (c), (d) whole sweeps
def _sweep_problem(T, degenerate, nan_row=None):
    """SingleMassOscillator with (degenerate) R = 1e-6 -- one or a few of the iid particles carry a step -- and outlier observations at
    t = 1, mid-sweep and t = T - 1; the reference trajectory runs 5 standard deviations of the initial cloud beside the truth.
    nan_row: that observation and the last one are NaN.  No weight of step nan_row is positive, nor of the step after it (its weights
    start from the NaN log-weights the step left; its own are finite again), nor of the last step, nor of the final draw."""
    from pgas_amd.descriptors import GaussianLikelihood

    pb = experiments.smo_pgas(T=T)
    pb.observations = pb.observations.copy()
    ref = pb.X_true.copy()
    if degenerate:
        for t in (1, T // 2, T - 1):
            pb.observations[t] += 0.3
        pb.likelihood_fcn = GaussianLikelihood.of_component(0, 2, np.array([[1e-6]]))
        ref = ref + np.array([0.05, 0.0])
    if nan_row is not None:
        pb.observations[nan_row] = pb.observations[T - 1] = np.nan
    return pb, ref


@functools.lru_cache(maxsize=None)
def _oracle_sweep(N, T, degenerate, nan_row, corrected=False):
    """The oracle's sweep step by step (so that the log-weights every step resamples are at hand for the census), the final index and
    the back-trace: (traj, X, ANC, logw_last, the steps' branch sets, per step (largest share of one particle in the ancestor CDF of
    the conditioned particle, that particle's index))."""
    pb, ref = _sweep_problem(T, degenerate, nan_row)
    A, S = experiments.initial_params(pb)
    cm = canon_model(pb, N)
    cm.set_corrected(corrected)
    LS, LSinv, cS = cm.chol_parts(S)
    X = np.empty((T, N, pb.nx))
    ANC = np.empty((T - 1, N), np.int32)
    X[0] = cm.init_state(SEED, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), ref[0])
    lw, lw1, dom = None, [], []
    for t in range(1, T):
        lw, X[t], ANC[t - 1], dbg = cm.step(t, SEED, X[t - 1], lw, A, LS, LSinv, cS, ref[t], debug=True)
        lw1.append((dbg["lw1"], dbg["u"][0]))
        l2 = np.where(np.isfinite(dbg["lw2"]), dbg["lw2"], -np.inf)
        if np.isfinite(l2.max()):
            w = np.exp(l2 - l2.max())
            dom.append((float(1.0 / w.sum()), int(np.argmax(l2))))
        else:
            dom.append((0.0, -1))
    seen = [rc.branches(c) for c in _POOL.map(lambda a: rc.census(*a), lw1)]
    b = cm.final_index(SEED, lw)
    traj = np.empty((T, pb.nx))
    for t in range(T - 1, -1, -1):
        traj[t] = X[t, b]
        if t:
            b = ANC[t - 1, b]
    return traj, X, ANC, lw, seen, dom


def _check_sweep(csmc, N, T, degenerate, nan_row, opts, corrected=False):
    pb, ref = _sweep_problem(T, degenerate, nan_row)
    A, S = experiments.initial_params(pb)
    for k, v in opts.items():
        csmc.engine.set_option(k, v)
    traj = csmc(SEED, ref, A, S)
    trajo, Xo, ANCo, lwo, seen, _ = _oracle_sweep(N, T, degenerate, nan_row, corrected)
    X, ANC, LW, _ = csmc.engine.traces()
    _eq(ANC[: T - 1], ANCo, "ancestor_trace")
    _eq(X, Xo, "state_trace")
    _eq(LW, lwo, "log_weights_trace[-1]")
    _eq(traj, trajo, "trajectory")
    return seen


def _csmc(pb, N, **kw):
    return pgas_amd.condSequentialMonteCarlo(N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn, **kw)


@pytest.mark.parametrize("N,opts", [(70000, {}), (70000, {7: 1}), (70000, {9: 1}), (1 << 17, {}), (1 << 17, {7: 1}), (1 << 17, {9: 1}),
                                    (200, {14: 2}), (200, {}), (1024, {14: 2}), (1024, {})])
def test_degenerate_sweep(N, opts):
    """Whole sweeps of the degenerate model: k_step in its three forms (group records from k_groups, 7: every workgroup scans the groups
    itself, 9: the last-arriving workgroup scans them), k_sweep_chains with one chain (14: 2) and k_sweep_duo.  The census of the oracle's log-weights
    says what the general path met: at least one step whose workgroups take the bisection path."""
    T = 8
    pb, _ = _sweep_problem(T, True)
    csmc = _csmc(pb, N)
    seen = _check_sweep(csmc, N, T, True, None, opts)
    info = csmc.engine.launch_info()
    assert info["small"] == (N <= 1024)
    print(f"sweep census N={N}: {[sorted(s) for s in seen]}")
    if N > 1024:
        assert info["local_groups"] == (opts.get(7, 0) == 1)
        assert any("ns>8" in s for s in seen) and any(len(s & {f"ns={k}" for k in range(3, 9)}) >= 2 for s in seen), seen
    _, _, ANCo, _, _, dom = _oracle_sweep(N, T, True, None)
    assert min(len(np.unique(r)) for r in ANCo) < max(2, N // 100), "the sweep really was degenerate"
    # the reference runs beside the cloud: one particle holds the ancestor CDF of the conditioned particle, and that particle is drawn
    # (share > 0.99 in at least one step, where the draw returns the holder; a valid CDF reaches the clip at N - 1 only through rounding,
    # the fallback N - 1 of an invalid one is the business of the NaN-row sweeps below)
    held = [t for t, (share, _) in enumerate(dom) if share > 0.99]
    assert held and any(ANCo[t, N - 1] == dom[t][1] for t in held), (dom, ANCo[:, N - 1])


@pytest.mark.parametrize("N,opts,corrected", [(70000, {}, False), (70000, {7: 1}, False), (70000, {9: 1}, False), (200, {14: 2}, False), (200, {}, False),
                                              (1024, {14: 2}, False), (1024, {}, False), (1025, {}, False),
                                              (70000, {}, True), (200, {}, True)])   # corrected mode: one serial path for every size
def test_sweep_through_a_step_without_a_positive_weight(N, opts, corrected):
    """NaN observations mid-sweep and at the end: in the steps without a positive weight the ancestors are the identity and the reference
    particle's ancestor is N - 1, and so is the final index -- the `valid == false` branches of k_step, k_sweep_chains,
    k_sweep_duo and of the serial corrected path.  Nothing indexes with a threshold there: the searches are skipped and every ancestor
    is an in-range identity index.  The steps in between resample as usual."""
    T, nan_row = 8, 4
    pb, _ = _sweep_problem(T, False, nan_row)
    csmc = _csmc(pb, N, resample_before_propagate=corrected)
    _check_sweep(csmc, N, T, False, nan_row, opts, corrected)
    _, _, ANCo, lwo, _, _ = _oracle_sweep(N, T, False, nan_row, corrected)
    for t in range(1, T):
        assert np.array_equal(ANCo[t - 1], np.arange(N)) == (t in (nan_row, nan_row + 1, T - 1)), f"step {t}"
    assert np.isnan(lwo).all()
    assert csmc.engine.last_final_index() == N - 1


@pytest.mark.parametrize("N", [200, 1024])
@pytest.mark.parametrize("nan_row", [None, 4])
def test_chains_with_one_degenerate_chain(N, nan_row):
    """Three chains in one batched sweep (k_sweep_chains); only the middle one is degenerate (its error covariance is 10^4 times the others',
    so its particles scatter and one to five of them carry a step; its coefficients and its reference differ too): every chain equals the oracle's sweep with its
    own inputs, so the degenerate chain leaves its neighbours alone.  With a NaN observation row every chain takes the branch without a
    positive weight in the steps the NaN reaches."""
    from pgas_amd import chains as ch
    from pgas_amd import random as prng

    T, C = 10, 3
    pb, _ = _sweep_problem(T, False, nan_row)
    A, S = experiments.initial_params(pb)
    keys = [prng.key(77 + 13 * c) for c in range(C)]
    refs = np.stack([pb.X_true, pb.X_true + np.array([0.05, 0.0]), pb.X_true])
    As, Ss = np.stack([A, 3.0 * A, A]), np.stack([S, 1e4 * S, S])
    chs = ch.condSequentialMonteCarloChains(C, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    traj = chs(keys, refs, As, Ss).cpu().numpy()
    X, ANC, LW = (t.cpu().numpy() for t in chs.traces())
    fidx = chs.final_index()
    cm = canon_model(pb, N)
    L0 = np.linalg.cholesky(pb.init_state_cov)
    uniq = []
    for c in range(C):
        LS, LSinv, cS = cm.chol_parts_dev(Ss[c])
        trajo, Xo, ANCo, lwo = cm.sweep(keys[c], refs[c], As[c], LS, LSinv, cS, pb.init_state_mean, L0)
        _eq(ANC[c, : T - 1], ANCo, f"chain {c}: ancestor trace")
        _eq(X[c], Xo, f"chain {c}: state trace")
        _eq(LW[c], lwo, f"chain {c}: final log-weights")
        _eq(traj[c], trajo, f"chain {c}: trajectory")
        assert fidx[c] == cm.final_index(keys[c], lwo)
        uniq.append(np.median([len(np.unique(r)) for r in ANCo[: (nan_row or T) - 1]]))
        if nan_row is not None:
            for t in range(1, T):
                assert np.array_equal(ANC[c, t - 1], np.arange(N)) == (t in (nan_row, nan_row + 1, T - 1)), f"chain {c} step {t}"
            assert fidx[c] == N - 1
    print(f"median number of distinct ancestors per chain: {uniq}")
    assert uniq[1] < 0.35 * min(uniq[0], uniq[2]), uniq


def test_sharded_degenerate_sweep():
    """Four shards (four segments each) of one device on the degenerate model: every shard has steps whose ancestors live on another shard,
    and in some step a workgroup draws from five or more source segments, i.e. from more segments than its own shard holds."""
    from pgas_amd import sharded

    N, T, world = 16384, 8, 4
    pb, ref = _sweep_problem(T, True)
    A, S = experiments.initial_params(pb)
    trajo, Xo, ANCo, lwo, seen, _ = _oracle_sweep(N, T, True, None)
    grp = sharded.make_local_group(world, N, pb.observations, pb.inputs, pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    trajs = sharded.sharded_sweep(grp, SEED, ref, A, S, propagate_chunk=5)
    Nl = N // world
    for r, (s, tr) in enumerate(zip(grp.shards, trajs)):
        _eq(tr, trajo, f"trajectory on rank {r}")
        X, ANC, LW, _ = s.eng.traces()
        _eq(ANC[: T - 1], ANCo[:, r * Nl:(r + 1) * Nl], f"ancestor_trace shard {r}")
        _eq(X, Xo[:, r * Nl:(r + 1) * Nl], f"state_trace shard {r}")
        _eq(LW, lwo[r * Nl:(r + 1) * Nl], f"log_weights shard {r}")
    assert min(len(np.unique(r)) for r in ANCo) < N // 100, "the sweep really was degenerate"
    print(f"sharded sweep census: {[sorted(s) for s in seen]}")
    assert any(s & ({f"ns={k}" for k in range(5, 9)} | {"ns>8"}) for s in seen), seen
    for r in range(world):
        assert any((row[r * Nl:(r + 1) * Nl] // Nl != r).any() for row in ANCo), f"shard {r} never has a remote ancestor"


# ------------------------------------------------------------------------------------------ (e) the quantiser
def _q51_host(x):
    """The reference expression of the segment scans (oracle segment_scan, cdf_count_wg's rebuild): rint(exp(x) 2^51), 0 unless exp > 0."""
    e = canon.det_exp(x)
    with np.errstate(invalid="ignore"):
        return np.where(e > 0.0, np.rint(e * 2.0 ** 51), 0.0)


def test_device_quantiser_equals_the_reference_expression():
    """dev_exp_q51_n (csrc/pgas_kernels.hip.h), the segment scans' shortcut, against pgas_double_to_u64(rint(pgas_exp(x) 2^51)) on its
    stated domain x <= 0.25, NaN and -inf included, bit for bit; and against mpmath within 0.5 + 2^51 ulp(exp(x)) (pgas_exp is good to
    less than one ulp, the rounding to an integer adds a half)."""
    from pgas_amd import _lib

    rng = np.random.default_rng(13)
    lo = [-708.0]
    hi = [-708.0]
    for _ in range(64):
        lo.append(np.nextafter(lo[-1], -np.inf))
        hi.append(np.nextafter(hi[-1], np.inf))
    special = np.array(lo + hi[1:] + [-0.0, 0.0, 0.25, -745.2, -1e300, -np.inf, np.nan, -np.nan])
    x = np.concatenate([rng.uniform(-745.0, 0.25, 800000), rng.uniform(-40.0, -30.0, 200000), rng.uniform(-1.0, 0.25, 50000),
                        np.log(np.arange(4000) + 0.5) - 51.0 * np.log(2.0) + 1e-12 * rng.standard_normal(4000),   # q at its rounding boundaries
                        special])
    assert x.size >= 10 ** 6
    q = _lib.detmath_eval(8, x=x)[0]
    ref = _q51_host(x)
    bad = np.nonzero(q != ref)[0]
    assert bad.size == 0, f"{bad.size} arguments differ, e.g. x = {x[bad[0]]!r}: device {q[bad[0]]} != {ref[bad[0]]}"
    assert q[-3:].tolist() == [0.0, 0.0, 0.0] and q.max() < 2.0 ** 52 and np.all(q == np.floor(q))
    small = (x > -40.0) & (x < -30.0)
    assert len(np.unique(q[small])) > 200, "the dense range must resolve q = 0, 1, 2, ... (exp(-30) 2^51 = 211)"
    import mpmath as mp

    mp.mp.prec = 200
    for i in np.concatenate([rng.integers(0, 800000, 200), rng.integers(800000, 1000000, 200), np.arange(x.size - special.size, x.size - 3)]):
        ex = mp.exp(mp.mpf(float(x[i])))
        ulp = float(np.spacing(float(ex))) if ex > mp.mpf(2) ** -1000 else 0.0
        assert abs(mp.mpf(float(q[i])) - ex * 2 ** 51) <= 0.5 + 2.0 ** 51 * ulp, (x[i], q[i])
