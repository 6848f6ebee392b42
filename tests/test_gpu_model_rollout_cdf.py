"""pgas_amd.ModelRollout.cdf on the GPU (pgas_m_rollout_cdf, csrc/pgas_marginal_rollout_cdf.hip.h): the open-loop
grey-box rollout counted against thresholds inside the kernel, compared (np.array_equal: the counts are integers) with the NumPy
restatement (tests/model_rollout_cdf_numpy.py) applied to what ``ModelRollout.__call__(outputs=True)`` itself stores -- which
tests/test_gpu_model_rollout.py pins step by step to the primitives it fuses.  Replicate p of a rollout does not depend on how many
replicates the call has (its Philox particle counter is p0 + p), so ONE materialised rollout of 1000 replicates per model is the cloud of
every smaller P.  A closed form that does not pass through the restatement closes the file."""
import functools
import types

import numpy as np
import pytest
import torch

import model_cdf_cases as mc
import model_filter_cases as cases
import model_rollout_cdf_numpy as mrc
from common import experiments, pgas_amd
from pgas_amd._lib import ModelRolloutCdfDesc, PgasError
from pgas_amd.model_rollout import STREAM_ROLLOUT_OBS
from test_gpu_model_filter import Case, _case, _np

pytestmark = pytest.mark.gpu
K, T, KEYS = cases.K, cases.T, cases.KEYS
PS = [1, 63, 64, 65, 128, 129, 1000]   # one lane; the wave edge; B = 1 <-> B > 1 (store <-> memset + atomics); a ragged last block of 16
PMAX = max(PS)
NAMES = list(cases.MODELS) + ["wide"]
INF, NAN = float("inf"), float("nan")


@functools.lru_cache(maxsize=None)
def _wide():
    ops = _case("smo").ops
    ssm, sim, A, y = mc.wide_rollout(ops)
    return types.SimpleNamespace(name="wide", ops=ops, dev=ops.device, ssm=ssm, sim=sim, y=sim.observations, A=[torch.as_tensor(a, device=ops.device) for a in A])


def _get(name):
    return _wide() if name == "wide" else _case(name)


def _LR(c):
    return np.linalg.cholesky(np.asarray(c.ssm.output_noise, dtype=np.float64))


def _obs_normals(c, P, p0=0, keys=KEYS):
    """e (K, T, P, ny): rows p0 .. p0 + P of rng_normal(key_k, 200, t, ., ny)."""
    return np.stack([np.stack([_np(c.ops.eng.rng_normal(k, STREAM_ROLLOUT_OBS, t, p0 + P, c.sim.ny))[p0:] for t in range(T)]) for k in keys])


@functools.lru_cache(maxsize=None)
def _channels(name):
    """(noise-free, noisy) value channels (K, T, PMAX, nx + ny) of __call__(outputs=True) with drawn x_0 and process noise; computed
    once, never changed."""
    c = _get(name)
    ox, oy = (_np(a) for a in c.sim(c.A, KEYS, replicates=PMAX, outputs=True))
    out = (mrc.channels(ox, oy), mrc.channels(ox, oy, _LR(c), _obs_normals(c, PMAX)))
    assert np.array_equal(out[0][..., :c.sim.nx], out[1][..., :c.sim.nx]) and not np.array_equal(out[0], out[1])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _thr(name, J):
    """threshold_grid of the noise-free cloud's own pooled moments; J = 1: the mean itself."""
    v = _channels(name)[0]
    flat = np.moveaxis(v, 1, 0).reshape(T, -1, v.shape[-1])
    th = pgas_amd.threshold_grid(flat.mean(axis=1), flat.std(axis=1), J, width=2.0 if J > 1 else 0.0).numpy()
    th.setflags(write=False)
    return th


def _jmax(name):
    return 12 if name == "wide" else 16


# ---- 1. counts = the restated counts of __call__(outputs=True)'s own clouds ----------------------------------------------------------------
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("name", NAMES)
def test_counts_equal_the_restated_counts_of_the_materialised_rollout(name, P):
    c = _get(name)
    nv = c.sim.nx + c.sim.ny
    assert c.sim.max_thresholds() == _jmax(name)
    for J in (1, _jmax(name)):
        thr = _thr(name, J)
        for noise in (False, True):
            want = mrc.counts(_channels(name)[int(noise)][:, :, :P], thr)
            r = c.sim.cdf(c.A, KEYS, replicates=P, thresholds=thr, observation_noise=noise)
            got = _np(r.count)
            assert r.n == P and r.nx == c.sim.nx and not r.pit and got.dtype == np.int32 and got.shape == (K, T, nv, J)
            assert np.array_equal(_np(r.thresholds), thr)
            assert (want != 0).any() and (want != P).any(), "thresholds that count nothing or everything test nothing"
            assert np.array_equal(got, want), f"{name} P = {P} J = {J} noise = {noise}"


# ---- 2. threshold edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vehicle", "toy"])
def test_ties_count_the_next_double_below_does_not_and_nan_and_infinities(name):
    c = _get(name)
    P = 129
    for noise in (False, True):
        v = _channels(name)[int(noise)][:, :, :P]
        nv = v.shape[-1]
        thr = np.empty((T, nv, 5))
        thr[..., 0] = v[0, :, 5, :]                     # replicate 5 of draw 0: a tie
        thr[..., 1] = np.nextafter(thr[..., 0], -INF)
        thr[..., 2], thr[..., 3], thr[..., 4] = NAN, INF, -INF
        got = _np(c.sim.cdf(c.A, KEYS, replicates=P, thresholds=thr, observation_noise=noise).count)
        assert np.array_equal(got, mrc.counts(v, thr))
        ties = (v[0] == thr[:, None, :, 0]).sum(axis=1)                                     # (T, nv)
        assert (ties >= 1).all() and np.array_equal(got[0, ..., 0] - got[0, ..., 1], ties)
        assert (got[..., 2] == 0).all() and (got[..., 3] == P).all() and (got[..., 4] == 0).all()
    grid = _np(c.sim.cdf(c.A, KEYS, replicates=P, thresholds=_thr(name, 16), observation_noise=True).count)
    assert (np.diff(grid, axis=-1) >= 0).all() and (grid >= 0).all() and (grid <= P).all()


# ---- 3. invariances ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vehicle", "wide"])
def test_chunks_by_p0_add_up_to_the_one_call(name):
    c = _get(name)
    thr = _thr(name, _jmax(name))
    whole = _np(c.sim.cdf(c.A, KEYS, replicates=200, thresholds=thr, observation_noise=True).count)
    assert np.array_equal(whole, mrc.counts(_channels(name)[1][:, :, :200], thr))
    parts = [_np(c.sim.cdf(c.A, KEYS, replicates=P, thresholds=thr, observation_noise=True, p0=p0).count) for p0, P in ((0, 64), (64, 64), (128, 72))]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)
    assert np.array_equal(parts[1], mrc.counts(_channels(name)[1][:, :, 64:128], thr))


def test_equal_draws_give_equal_rows_and_a_draw_does_not_depend_on_its_launch():
    c = _get("vehicle")
    thr, P = _thr("vehicle", 16), 130
    full = _np(c.sim.cdf(c.A, KEYS, replicates=P, thresholds=thr, observation_noise=True).count)
    idx = [0, 2, 0]
    dup = _np(c.sim.cdf([a[idx].contiguous() for a in c.A], [KEYS[i] for i in idx], replicates=P, thresholds=thr, observation_noise=True).count)
    assert np.array_equal(dup[0], dup[2]) and np.array_equal(dup[0], full[0]) and np.array_equal(dup[1], full[2]) and not np.array_equal(dup[0], dup[1])
    for k in range(K):
        alone = _np(c.sim.cdf([a[k:k + 1].contiguous() for a in c.A], KEYS[k:k + 1], replicates=P, thresholds=thr, observation_noise=True).count)
        assert np.array_equal(alone[0], full[k])
    Kbig = 700                                             # more workgroups than the device holds at once: 700 x 3 blocks
    A = [torch.as_tensor(a, device=c.dev) for a in cases.coeffs(c.pb, Kbig, seed=11)]
    keys = [1000 + 7 * k for k in range(Kbig)]
    big = _np(c.sim.cdf(A, keys, replicates=P, thresholds=thr).count)
    lo = _np(c.sim.cdf([a[:300].contiguous() for a in A], keys[:300], replicates=P, thresholds=thr).count)
    assert np.array_equal(big[:300], lo) and (big >= 0).all() and (big <= P).all()


# ---- 4. modes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smo", "vehicle", "wide"])
def test_no_thresholds_means_the_observations_the_pit(name):
    c = _get(name)
    nx, P = c.sim.nx, 129
    pit = c.sim.cdf(c.A, KEYS, replicates=P, observation_noise=True)
    same = c.sim.cdf(c.A, KEYS, replicates=P, thresholds=c.y, observation_noise=True)
    assert pit.pit and not same.pit and tuple(pit.count.shape) == (K, T, nx + c.sim.ny, 1)
    assert torch.equal(pit.count, same.count) and bool((pit.count[:, :, :nx] == 0).all())
    th = _np(pit.thresholds)
    assert np.isnan(th[:, :nx]).all() and np.array_equal(th[:, nx:, 0], c.y)
    assert np.array_equal(_np(pit.count), mrc.counts(_channels(name)[1][:, :, :P], th))
    s = pgas_amd.calibration_summary(pit)                  # takes the result as it is
    assert tuple(s["pit"].shape) == (T, c.sim.ny) and bool(torch.isfinite(s["ks"]))


def test_the_four_initial_state_modes_row_cov_and_noise_free():
    c = _get("smo")
    P, thr = 130, _thr("smo", 16)
    m0 = np.asarray(c.pb.init_state_mean, dtype=np.float64)
    rng = np.random.default_rng(3)
    for x0 in (m0 + 0.01, np.stack([m0 + 0.01 * (k + 1) for k in range(K)]), m0 + 0.01 * rng.standard_normal((K, P, 2))):   # (nx), (K, nx), (K, P, nx)
        ox, oy = (_np(a) for a in c.sim(c.A, KEYS, replicates=P, init_state=x0, outputs=True))
        assert np.array_equal(_np(c.sim.cdf(c.A, KEYS, replicates=P, init_state=x0, thresholds=thr).count), mrc.rollout_counts(ox, oy, thr)), x0.shape
    x0 = m0 + 0.01 * rng.standard_normal((K, P, 2))        # noise-free: process noise off, a per-replicate x_0, no keys
    fx, fy = (_np(a) for a in c.sim(c.A, None, replicates=P, init_state=x0, process_noise=False, outputs=True))
    assert np.array_equal(_np(c.sim.cdf(c.A, None, replicates=P, init_state=x0, process_noise=False, thresholds=thr).count), mrc.rollout_counts(fx, fy, thr))
    c2 = _get("smo2")                                      # interface-variable noise
    B = rng.standard_normal((K, 2, 2))
    covs = [1e-2 * (B @ B.transpose(0, 2, 1) + np.eye(2))]
    ox, oy = (_np(a) for a in c2.sim(c2.A, KEYS, replicates=65, row_cov=covs, outputs=True))
    th2 = _thr("smo2", 16)
    got = _np(c2.sim.cdf(c2.A, KEYS, replicates=65, row_cov=covs, thresholds=th2, observation_noise=True).count)
    assert np.array_equal(got, mrc.rollout_counts(ox, oy, th2, _LR(c2), _obs_normals(c2, 65)))
    assert not np.array_equal(got, mrc.counts(_channels("smo2")[1][:, :, :65], th2))


def test_a_record_of_one_row():
    from test_gpu_model_forecast import _record

    c = _get("smo")
    sim, ssm, A, y = _record("smo", 1, c.ops)
    for P in (1, 70):
        ox, oy = (_np(a) for a in sim(A, KEYS, replicates=P, outputs=True))
        thr = np.concatenate([ox, oy], axis=-1)[0, :, 0, :, None] * np.ones(2)   # (1, 3, 2): replicate 0 of draw 0, a tie
        thr[..., 1] = INF
        got = _np(sim.cdf(A, KEYS, replicates=P, thresholds=thr).count)
        assert got.shape == (K, 1, 3, 2) and np.array_equal(got, mrc.rollout_counts(ox, oy, thr)) and (got[..., 1] == P).all() and (got[0, ..., 0] >= 1).all()


# ---- 5. safety -----------------------------------------------------------------------------------------------------------------------------
def test_cdf_makes_no_host_round_trip():
    c = _get("vehicle")
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    thr = torch.as_tensor(_thr("vehicle", 16), device=c.dev)
    thr_y = thr[:, 2:].contiguous()
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    calls = [lambda: c.sim.cdf(c.A, kd, replicates=1000, thresholds=thr, observation_noise=True),
             lambda: c.sim.cdf(c.A, kd, replicates=3, init_state=x0, thresholds=thr_y), lambda: c.sim.cdf(c.A, kd, replicates=64, observation_noise=True)]
    warm = [f() for f in calls]   # uploads of the programs, tables and observations, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [f() for f in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a.count, b.count) and bool((a.count >= 0).all()) and bool(a.count.sum() > 0)


def test_cdf_leaves_the_rollout_predict_and_algorithm1_on_the_same_context_unchanged():
    pb = experiments.emps_marginal(T=T)

    def run():
        alg = pgas_amd.Algorithm1(64, pb.observations, pb.inputs, pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel), pb.forgetting_factor,
                                  pb.init_state_mean, pb.init_state_cov, pb.init_int_var_mean, pb.init_int_var_cov, pb.GP_prior, pb.basis_fcn())
        out = alg(12345678)
        return alg, [out[0], out[1][0], out[3], out[4]]

    alg, before = run()
    c = Case("emps", ops=alg.ops)
    assert c.sim.ops is alg.ops
    plain = [a.clone() for a in c.sim(c.A, KEYS, replicates=70, outputs=True)]
    st = c.sim.predict(c.A, KEYS, replicates=70, observation_noise=True)
    pred = [t.clone() for t in (st.x_sum, st.x_sumsq, st.y_sum, st.y_sumsq, st.lpd)]
    r = c.sim.cdf(c.A, KEYS, replicates=70, observation_noise=True)
    r2 = c.sim.cdf(c.A, KEYS, replicates=200, thresholds=_thr("emps", 16))
    assert bool((r.count >= 0).all()) and bool((r2.count <= 200).all())
    again = c.sim(c.A, KEYS, replicates=70, outputs=True)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    st = c.sim.predict(c.A, KEYS, replicates=70, observation_noise=True)
    for a, b in zip(pred, (st.x_sum, st.x_sumsq, st.y_sum, st.y_sumsq, st.lpd)):
        assert torch.equal(a, b)
    _, after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_abi_refusals_leave_the_context_usable():
    c = _get("vehicle")
    sim, P, J = c.sim, 70, 16
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    thr = torch.as_tensor(_thr("vehicle", J), device=c.dev)
    good = sim.cdf(c.A, kd, replicates=P, thresholds=thr, observation_noise=True)
    count = torch.empty((K, T, 4, J), dtype=torch.int32, device=c.dev)
    LR = _LR(c)

    def descs(s=sim, A=c.A, nv=4):
        d = s._desc(K, P, 0, 0, A, None, kd, None, True, None, None)
        q = ModelRolloutCdfDesc()
        q.thr_dev, q.count_dev, q.J, q.noise = thr.data_ptr(), count.data_ptr(), J, 1
        for j in range(2):
            for l in range(2):
                q.LR[2 * j + l] = float(LR[j, l])
        return d, q

    edits = {
        "J = 0": lambda d, q: setattr(q, "J", 0),
        "J = 17": lambda d, q: setattr(q, "J", 17),
        "NULL argument (thr, count)": lambda d, q: setattr(q, "thr_dev", None),
        "(thr, count)": lambda d, q: setattr(q, "count_dev", None),
        "needs seeds": lambda d, q: setattr(d, "seeds_dev", None),
        f"P = {(1 << 20) + 1}": lambda d, q: setattr(d, "P", (1 << 20) + 1),
        "P = 0": lambda d, q: setattr(d, "P", 0),
        "output program": lambda d, q: setattr(d, "gcode_dev", None),   # what pgas_m_rollout_stats refuses of the descriptor
        "L = 0": lambda d, q: setattr(d, "L", 0),
        "K = 0": lambda d, q: setattr(d, "K", 0),
        "97 registers": lambda d, q: setattr(d, "nreg", 97),
    }
    for what, edit in edits.items():
        d, q = descs()
        edit(d, q)
        with pytest.raises(PgasError, match=r"pgas_m_rollout_cdf failed \(-1\)") as ei:   # PGAS_E_ARG, with the library's message
            sim.ops.model_rollout_cdf(d, q)
        assert "pgas_m_rollout_cdf: " in str(ei.value) and what in str(ei.value), (what, str(ei.value))
    d, q = descs()                                            # observation noise alone needs seeds too: a noise-free descriptor, noise = 1
    d.seeds_dev, d.Qc_dev, d.x0_mode = None, None, 2
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    d.x0_dev, d.m0L0_dev = x0.data_ptr(), None
    with pytest.raises(PgasError, match="observation noise needs seeds"):
        sim.ops.model_rollout_cdf(d, q)
    w = _wide()                                               # five channels: J = 13 needs 65 slots
    d, q = descs(w.sim, w.A)
    q.J = 13
    with pytest.raises(PgasError, match="J_max = 12"):
        w.sim.ops.model_rollout_cdf(d, q)
    d, q = descs()                                            # the untouched descriptors still run on the same context
    sim.ops.model_rollout_cdf(d, q)
    torch.cuda.synchronize()
    assert torch.equal(count, good.count)
    assert torch.equal(sim.cdf(c.A, kd, replicates=P, thresholds=thr, observation_noise=True).count, good.count)


# ---- 6. closed form, independent of the restatement ------------------------------------------------------------------------------------------
def test_memoryless_model_pooled_counts_are_binomial():
    """x' = xi + N(0, q), y = x with A = 0: x_t (t >= 1) is iid N(0, q) and yhat + e iid N(0, q + r) over rows, replicates and draws, so
    the count at sigma * TAUS pooled over K = 3 draws, rows 1 .. 11 and P = 4096 replicates is Binomial(n = 135168, Phi(TAUS)): |z| <= 4,
    the project's bound for every closed-form test.  (A model with memory must not be pooled over rows: its rows are correlated.)
    tests/test_model_rollout_cdf_host.py evaluates the same statistic on the CPU from the generator's normals: max |z| = 1.425 (x),
    1.643 (yhat); the device's counts are those counts when its clouds are the generator's."""
    ops = _case("toy").ops
    ssm, sim, A, y = mc.memoryless_rollout(ops)
    r = sim.cdf(A, KEYS, replicates=mc.CLOSED_P, thresholds=mc.closed_thresholds(T), observation_noise=True)
    cnt = _np(r.count)
    assert cnt.shape == (K, T, 2, len(mc.TAUS))
    tot, rows = mc.pool_rollout(cnt)
    z = mc.binomial_z(tot, rows * mc.CLOSED_P)
    print(f"open loop: n = {rows * mc.CLOSED_P}, z x = {np.round(z[0], 3).tolist()}, z yhat = {np.round(z[1], 3).tolist()}")
    assert (np.abs(z) <= 4.0).all()
