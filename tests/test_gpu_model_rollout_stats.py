"""pgas_amd.ModelRollout.predict on the GPU (pgas_m_rollout_stats, csrc/pgas_marginal_rollout_stats.hip.h): the
predictive moments and the log score reduced over the replicates inside the kernel, against the NumPy restatement of their defined order
(tests/model_rollout_stats_numpy.py) applied to what ``ModelRollout.__call__(outputs=True)`` itself stores -- which
tests/test_gpu_model_rollout.py pins step by step to the primitives it fuses.  Comparisons are np.array_equal unless stated.  Replicate p
of a rollout does not depend on how many replicates the call has (its Philox particle counter is p0 + p), so ONE materialised rollout of
257 replicates per model is the cloud of every smaller P."""
import functools

import numpy as np
import pytest
import torch

import model_rollout_stats_numpy as ms
from common import canon, experiments, pgas_amd
from pgas_amd._lib import MarginalOps, PgasError, RolloutStatsDesc
from pgas_amd.model_rollout import STREAM_ROLLOUT_OBS

pytestmark = pytest.mark.gpu
K, T = 3, 12
KEYS = [0x1234567, 0x9E3779B97F4A7C15, 42]
MODELS = {
    "smo": (experiments.smo_marginal, None),                 # 2-D basis, M = 41
    "emps": (experiments.emps_marginal, None),               # basis on x[1], M = 9
    "toy": (experiments.toy_marginal, None),                 # nx = 1, deterministic, the output IS xi
    "vehicle": (experiments.vehicle_marginal, None),         # L = 2, traced features, nu = 2, ny = 2, the output reads xi
    "smo2": (experiments.smo_two_component_marginal, [2]),   # n = 2
}
PS = [1, 63, 64, 65, 129, 257]   # one lane, one short of a wave, exactly one, one over, three and five blocks with a ragged tail
PMAX = max(PS)
NOISE_R = {"toy": np.array([[0.04]]), "vehicle": np.array([[0.09, -0.021], [-0.021, 0.0049 + 0.16]])}   # non-diagonal for ny = 2


def _np(t):
    return t.detach().cpu().numpy()


def _coeffs(pb, Kn=K, seed=5):
    """Kn coefficient sets per latent function: prior mean + 0.1 N(0, 1) sd."""
    rng = np.random.default_rng(seed)
    out = []
    for g in pb.GP_prior:
        e0, e1 = np.asarray(g[0]), np.asarray(g[1])
        M = e1.shape[0]
        mean = pgas_amd.prior_mniw_mean(e0.reshape(M, -1), e1)
        out.append(mean[None] + 0.1 * rng.standard_normal((Kn,) + mean.shape) * np.diag(np.linalg.inv(e1)))
    return out


class Case:
    """One model over T input rows on one MarginalOps: the rollout object with the model's observations, and K coefficient draws."""

    def __init__(self, name, ops=None, output_noise=None, observations=None):
        make, widths = MODELS[name]
        self.pb = pb = make(T=T)
        self.ops = ops or MarginalOps(1)
        self.dev = self.ops.device
        R = pb.output_noise if output_noise is None else output_noise
        self.ssm = pgas_amd.SymbolicStateSpaceModel(pb.process_noise, R, pb.model)
        self.ssm.bind(self.ops)
        self.y = np.asarray(pb.observations if observations is None else observations, dtype=np.float64).reshape(T, -1)
        self.sim = pgas_amd.ModelRollout(pb.inputs[:T], self.ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, int_var_widths=widths, ops=self.ops,
                                         observations=self.y)
        self.A = [torch.as_tensor(a, device=self.dev) for a in _coeffs(pb)]
        self.LR = np.linalg.cholesky(self.ssm.output_noise)


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def _noise_case(name):
    return Case(name, ops=_case(name).ops, output_noise=NOISE_R[name])


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(out_x (K, T, PMAX, nx), out_y (K, T, PMAX, ny)) of __call__ with drawn x_0 and process noise; computed once, never changed."""
    c = _case(name)
    out = tuple(_np(a) for a in c.sim(c.A, KEYS, replicates=PMAX, outputs=True))
    for a in out:
        a.setflags(write=False)
    return out


def _want_moments(ox, yh):
    """Restated (sum, sumsq) (K, T, nx + ny) of the clouds (K, T, P, nx) and (K, T, P, ny)."""
    return ms.moments(np.moveaxis(np.concatenate([ox, yh], axis=-1), 2, -1))


def _got(st):
    return np.concatenate([_np(st.x_sum), _np(st.y_sum)], axis=-1), np.concatenate([_np(st.x_sumsq), _np(st.y_sumsq)], axis=-1)


def _all(st):
    return [_np(t) for t in (st.x_sum, st.x_sumsq, st.y_sum, st.y_sumsq, st.lpd)]


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: sums"
    assert np.array_equal(got[1], want[1]), f"{what}: sums of squares"


# ---- 1. moments = the restated reduction of __call__(outputs=True)'s own clouds -------------------------------------------------------
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("name", list(MODELS))
def test_moments_equal_the_restated_reduction_of_the_materialised_rollout(name, P):
    c = _case(name)
    sim, nx, ny = c.sim, c.sim.nx, c.sim.ny
    ox, oy = (a[:, :, :P] for a in _cloud(name))
    want = _want_moments(ox, oy)
    drawn = sim.predict(c.A, KEYS, replicates=P)
    assert drawn.n == P and tuple(drawn.x_sum.shape) == (K, T, nx) and tuple(drawn.y_sumsq.shape) == (K, T, ny) and tuple(drawn.lpd.shape) == (K, T)
    _same(_got(drawn), want, "drawn x_0")
    x0 = ox[:, 0].copy()                                                            # (K, P, nx)
    _same(_got(sim.predict(c.A, KEYS, replicates=P, init_state=x0)), want, "given x_0")
    # process noise off, a per-replicate x_0: against the noise-free __call__
    fx, fy = (_np(a) for a in sim(c.A, None, replicates=P, init_state=x0, process_noise=False, outputs=True))
    assert c.ssm.is_deterministic or not np.array_equal(fx, ox)
    _same(_got(sim.predict(c.A, None, replicates=P, init_state=x0, process_noise=False)), _want_moments(fx, fy), "noise-free")


def test_shared_and_per_draw_initial_states():
    c = _case("smo")
    m0 = np.asarray(c.pb.init_state_mean, dtype=np.float64)
    for x0 in (m0 + 0.01, np.stack([m0 + 0.01 * (k + 1) for k in range(K)])):       # (nx) and (K, nx)
        ox, oy = (_np(a) for a in c.sim(c.A, KEYS, replicates=130, init_state=x0, outputs=True))
        _same(_got(c.sim.predict(c.A, KEYS, replicates=130, init_state=x0)), _want_moments(ox, oy), f"x_0 {x0.shape}")


def test_interface_variable_noise():
    c = _case("smo2")
    rng = np.random.default_rng(4)
    B = rng.standard_normal((K, 2, 2))
    covs = [1e-2 * (B @ B.transpose(0, 2, 1) + np.eye(2))]
    ox, oy = (_np(a) for a in c.sim(c.A, KEYS, replicates=65, row_cov=covs, outputs=True))
    assert not np.array_equal(ox, _cloud("smo2")[0][:, :, :65])
    _same(_got(c.sim.predict(c.A, KEYS, replicates=65, row_cov=covs)), _want_moments(ox, oy), "row_cov")


# ---- 2. observation noise ---------------------------------------------------------------------------------------------------------------
def _obs_normals(c, P, p0=0):
    """e (K, T, P, ny): rows p0 .. p0 + P of rng_normal(key_k, 200, t, ., ny)."""
    return np.stack([np.stack([_np(c.ops.eng.rng_normal(k, STREAM_ROLLOUT_OBS, t, p0 + P, c.sim.ny))[p0:] for t in range(T)]) for k in KEYS])


@pytest.mark.parametrize("P", [1, 65, 257])
@pytest.mark.parametrize("name", ["toy", "vehicle"])
def test_observation_noise_is_the_restated_fma_chain_on_its_own_stream(name, P):
    c = _noise_case(name)
    nx = c.sim.nx
    assert c.sim.ny == 1 or c.LR[1, 0] != 0.0
    ox, oy = (a[:, :, :P] for a in _cloud(name))                                    # the state does not read the output noise
    want = _want_moments(ox, ms.predicted_obs(oy, c.LR, _obs_normals(c, P)))
    st = c.sim.predict(c.A, KEYS, replicates=P, observation_noise=True, log_score=False)
    assert st.lpd is None
    got = _got(st)
    _same(got, want, "noisy observations")
    clean = _got(c.sim.predict(c.A, KEYS, replicates=P, log_score=False))
    _same(clean, _want_moments(ox, oy), "the same object without the flag")
    assert np.array_equal(clean[0][..., :nx], got[0][..., :nx]) and np.array_equal(clean[1][..., :nx], got[1][..., :nx])
    assert not np.array_equal(clean[0][..., nx:], got[0][..., nx:])


def test_a_noise_free_state_with_noisy_observations_has_distinct_replicates():
    c = _noise_case("toy")
    x0 = np.asarray(c.pb.init_state_mean, dtype=np.float64)
    P = 65
    ox, oy = (_np(a) for a in c.sim(c.A, None, init_state=x0, process_noise=False, outputs=True))          # one replicate: the others are copies
    ox, oy = np.repeat(ox, P, axis=2), np.repeat(oy, P, axis=2)
    want = _want_moments(ox, ms.predicted_obs(oy, c.LR, _obs_normals(c, P)))
    _same(_got(c.sim.predict(c.A, KEYS, replicates=P, init_state=x0, process_noise=False, observation_noise=True, log_score=False)), want, "copies + noise")


# ---- 3. log score -----------------------------------------------------------------------------------------------------------------------
def _want_lpd(c, oy, y):
    """oy (K, T, P, ny), y (T, ny) -> (K, T)."""
    ll = ms.loglik(oy, y[None, :, None, :], c.ssm._LRinv, c.ssm._cR)               # (K, T, P)
    return ms.lpd(ll, y, canon.det_exp, canon.det_log)


@pytest.mark.parametrize("P", [1, 65, 257])
@pytest.mark.parametrize("name", ["toy", "vehicle", "smo"])
def test_log_score_equals_the_restated_definition(name, P):
    c = _case(name)
    oy = _cloud(name)[1][:, :, :P]
    want = _want_lpd(c, oy, c.y)
    assert np.isfinite(want).all()
    st = c.sim.predict(c.A, KEYS, replicates=P)
    assert np.array_equal(_np(st.lpd), want)
    off = c.sim.predict(c.A, KEYS, replicates=P, log_score=False)                  # lpd_dev = NULL: no log score, the moments unchanged
    assert off.lpd is None
    for a, b in zip(_got(st), _got(off)):
        assert np.array_equal(a, b)
    noisy = c.sim.predict(c.A, KEYS, replicates=P, observation_noise=True)          # the score is taken at the NOISE-FREE output
    assert np.array_equal(_np(noisy.lpd), want) and not np.array_equal(_np(noisy.y_sum), _np(st.y_sum))


@pytest.mark.parametrize("name", ["smo", "vehicle"])
def test_restated_log_density_is_the_models_log_likelihood_of_the_stored_rows(name):
    """A cross-check of the formula, not of the rounding: within 1e-12 max(1, |l|) of SSM.log_likelihood (k_expr mode 2 on the device),
    fed the stored x_t and the interface variables of the existing primitives."""
    c = _case(name)
    P = 65
    ox, oy = (a[:, :, :P] for a in _cloud(name))
    ll = ms.loglik(oy, c.y[None, :, None, :], c.ssm._LRinv, c.ssm._cR)
    u = torch.as_tensor(np.asarray(c.pb.inputs[:T], dtype=np.float64).reshape(T, -1), device=c.dev)
    for k in range(K):
        for t in range(T):
            x = torch.as_tensor(ox[k, t].copy(), device=c.dev)
            xi = []
            for i, b in enumerate(c.pb.basis):
                phi = c.ops.hilbert_basis(b.map, b.alpha(x, u[t]).reshape(-1, 1).contiguous(), None) if hasattr(b, "feature") else c.ops.hilbert_basis(b, x, u[t])
                xi.append((phi @ c.A[i][k].T).contiguous())
            ref = _np(c.ssm.log_likelihood(c.y[t], x, u[t], *xi))
            err, bound = float(np.abs(ll[k, t] - ref).max()), 1e-12 * max(1.0, float(np.abs(ref).max()))
            assert err <= bound, f"l[{k},{t}]: max |diff| = {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", ["toy", "vehicle"])
def test_nan_and_far_observations(name):
    base_case = _case(name)
    P = 129
    y = base_case.y.copy()
    sigma = np.sqrt(np.diag(base_case.ssm.output_noise))
    y[3, -1] = np.nan                       # one component of one row
    y[5] = y[5] + 1e4 * sigma               # 10^4 sigma away
    y[7, 0] = 1e200                         # the quadratic form overflows: every density is 0
    c = Case(name, ops=base_case.ops, observations=y)
    base = _np(base_case.sim.predict(base_case.A, KEYS, replicates=P).lpd)
    got = _np(c.sim.predict(c.A, KEYS, replicates=P).lpd)
    assert np.isnan(got[:, 3]).all()
    assert np.isfinite(got[:, 5]).all()
    assert (got[:, 7] == -np.inf).all()
    rest = [t for t in range(T) if t not in (3, 5, 7)]
    assert np.array_equal(got[:, rest], base[:, rest]) and np.isfinite(base).all()
    assert np.array_equal(got, _want_lpd(c, _cloud(name)[1][:, :, :P], y), equal_nan=True)


# ---- 4. p0 ------------------------------------------------------------------------------------------------------------------------------
def test_p0_is_the_matching_slice_of_a_larger_rollout():
    c = _case("smo")
    ox, oy = (_np(a)[:, :, 64:128] for a in c.sim(c.A, KEYS, replicates=200, outputs=True))
    st = c.sim.predict(c.A, KEYS, replicates=64, p0=64)
    _same(_got(st), _want_moments(ox, oy), "p0 = 64")
    assert np.array_equal(_np(st.lpd), _want_lpd(c, oy, c.y))
    n = _noise_case("vehicle")                                                      # the observation noise follows the particle counter too
    ox, oy = (a[:, :, 64:129] for a in _cloud("vehicle"))
    want = _want_moments(ox, ms.predicted_obs(oy, n.LR, _obs_normals(n, 65, p0=64)))
    _same(_got(n.sim.predict(n.A, KEYS, replicates=65, p0=64, observation_noise=True, log_score=False)), want, "p0 = 64 with observation noise")


# ---- 5. independence across draws ---------------------------------------------------------------------------------------------------------
def test_draws_are_independent_of_their_order_and_equal_inputs_give_equal_rows():
    c = _noise_case("vehicle")
    P = 130
    fwd = _all(c.sim.predict(c.A, KEYS, replicates=P, observation_noise=True))
    rev = _all(c.sim.predict([a.flip(0).contiguous() for a in c.A], KEYS[::-1], replicates=P, observation_noise=True))
    for a, b in zip(fwd, rev):
        assert np.array_equal(a[::-1], b)
    idx = [0, 2, 0]
    dup = _all(c.sim.predict([a[idx].contiguous() for a in c.A], [KEYS[i] for i in idx], replicates=P, observation_noise=True))
    for a, d in zip(fwd, dup):
        assert np.array_equal(d[0], d[2]) and np.array_equal(d[0], a[0]) and np.array_equal(d[1], a[2]) and not np.array_equal(d[0], d[1])


def test_more_draws_than_the_device_holds_at_once():
    c = _case("vehicle")
    Kbig, P = 2000, 64
    A = [torch.as_tensor(a, device=c.dev) for a in _coeffs(c.pb, Kbig, seed=11)]
    keys = [1000 + 7 * k for k in range(Kbig)]
    got = _all(c.sim.predict(A, keys, replicates=P))
    assert got[0].shape == (Kbig, T, 2) and got[4].shape == (Kbig, T) and all(np.isfinite(g).all() for g in got)
    for k in (0, Kbig - 1):
        one = _all(c.sim.predict([a[k:k + 1].contiguous() for a in A], keys[k:k + 1], replicates=P))
        for a, b in zip(got, one):
            assert np.array_equal(a[k], b[0]), f"draw {k}"
    ox, oy = (_np(a) for a in c.sim([a[-1:].contiguous() for a in A], keys[-1:], replicates=P, outputs=True))
    want = _want_moments(ox, oy)
    assert np.array_equal(np.concatenate([got[0], got[2]], axis=-1)[-1:], want[0])


def test_draws_beyond_one_launch_run_in_chunks(monkeypatch):
    import pgas_amd.model_rollout as mr

    c = _case("smo")
    Kd, P = 5, 70
    A = [torch.as_tensor(a, device=c.dev) for a in _coeffs(c.pb, Kd, seed=3)]
    keys = [11, 12, 13, 14, 15]
    whole = _all(c.sim.predict(A, keys, replicates=P))
    launches = []
    real = c.ops.model_rollout_stats
    monkeypatch.setattr(mr, "MAX_DRAWS_PER_LAUNCH", 2)
    monkeypatch.setattr(c.ops, "model_rollout_stats", lambda d, s: (launches.append((d.K, s.part_bytes)), real(d, s))[1])
    parts = _all(c.sim.predict(A, keys, replicates=P))
    C_ = 2 * (c.sim.nx + c.sim.ny) + 2
    assert launches == [(2, 2 * 2 * T * C_ * 8), (2, 2 * 2 * T * C_ * 8), (1, 2 * 2 * T * C_ * 8)]   # one buffer of 2 draws x 2 blocks
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b)


# ---- 6. no host round trip --------------------------------------------------------------------------------------------------------------
def test_predict_makes_no_host_round_trip():
    c = _noise_case("vehicle")
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    cov = [torch.eye(1, dtype=torch.float64, device=c.dev).repeat(K, 1, 1) * 1e-4 for _ in range(2)]
    calls = [lambda: c.sim.predict(c.A, kd, replicates=130, observation_noise=True), lambda: c.sim.predict(c.A, kd, replicates=3, init_state=x0, row_cov=cov),
             lambda: c.sim.predict(c.A, None, init_state=x0, process_noise=False, log_score=False)]
    warm = [f() for f in calls]   # uploads of the programs, tables and observations, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [f() for f in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        for u, v in zip((a.x_sum, a.x_sumsq, a.y_sum, a.y_sumsq), (b.x_sum, b.x_sumsq, b.y_sum, b.y_sumsq)):
            assert torch.equal(u, v) and bool(torch.isfinite(u).all())
        assert (a.lpd is None) == (b.lpd is None) and (a.lpd is None or torch.equal(a.lpd, b.lpd))
    s = pgas_amd.predictive_summary(outs[0], y=c.y)                                 # works on the result unchanged
    assert tuple(s["y_mean_pooled"].shape) == (T, 2) and bool(torch.isfinite(s["rmse"])) and bool(torch.isfinite(s["elpd"]))


# ---- 7. no side effects -----------------------------------------------------------------------------------------------------------------
def test_predict_leaves_the_plain_rollout_and_the_filter_on_the_same_context_unchanged():
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
    assert all(np.isfinite(a).all() for a in _all(st))
    again = c.sim(c.A, KEYS, replicates=70, outputs=True)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    _same(_got(c.sim.predict(c.A, KEYS, replicates=70)), _want_moments(_np(plain[0]), _np(plain[1])), "between two __call__s")
    _, after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---- 8. refusals of the C ABI -------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable():
    c = _case("vehicle")
    sim, P = c.sim, 70
    nv, B, C_ = sim.nx + sim.ny, 2, 2 * (sim.nx + sim.ny) + 2
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    good = sim.predict(c.A, kd, replicates=P)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=c.dev)   # noqa: E731
    s1, s2, lpd, part, x0 = new(K, T, nv), new(K, T, nv), new(K, T), new(K, B, T, C_), torch.zeros(2, dtype=torch.float64, device=c.dev)
    ydev = sim._static()["y"]

    def descs(seeds=kd, mode=0, noisy_state=True):
        d = sim._desc(K, P, 0, mode, c.A, None, seeds, x0 if mode else None, noisy_state, None, None)
        s = RolloutStatsDesc()
        s.y_dev, s.sum_dev, s.sumsq_dev, s.lpd_dev, s.part_dev, s.part_bytes = ydev.data_ptr(), s1.data_ptr(), s2.data_ptr(), lpd.data_ptr(), part.data_ptr(), part.numel() * 8
        s.cR = float(c.ssm._cR)
        for j in range(2):
            for l in range(2):
                s.LR[2 * j + l], s.LRinv[2 * j + l] = float(c.LR[j, l]), float(c.ssm._LRinv[j, l])
        return d, s

    edits = {
        "P = 1048577": lambda d, s: setattr(d, "P", (1 << 20) + 1),
        "ny >= 1": lambda d, s: setattr(d, "ny", 0),
        "output program": lambda d, s: setattr(d, "gcode_dev", None),
        "needs the observations": lambda d, s: setattr(s, "y_dev", None),
        "sum, sumsq": lambda d, s: setattr(s, "sum_dev", None),
        "part has 0 B": lambda d, s: setattr(s, "part_dev", None),
        f"part has {part.numel() * 8 - 8} B": lambda d, s: setattr(s, "part_bytes", part.numel() * 8 - 8),
        "of LDS": lambda d, s: setattr(d.lat[0], "M", 1 << 20),
        "L = 0": lambda d, s: setattr(d, "L", 0),                                    # what pgas_m_rollout refuses is refused here too
        "K = 0": lambda d, s: setattr(d, "K", 0),
        "97 registers": lambda d, s: setattr(d, "nreg", 97),
        "needs seeds": lambda d, s: setattr(d, "seeds_dev", None),
    }
    for what, edit in edits.items():
        d, s = descs()
        edit(d, s)
        with pytest.raises(PgasError, match=r"pgas_m_rollout_stats failed \(-1\)") as ei:   # PGAS_E_ARG, with the library's message
            sim.ops.model_rollout_stats(d, s)
        assert "pgas_m_rollout_stats: " in str(ei.value) and what in str(ei.value), (what, str(ei.value))
    d, s = descs(seeds=None, mode=1, noisy_state=False)                             # a noise-free state: only the observation noise draws
    s.noise = 1
    with pytest.raises(PgasError, match="observation noise needs seeds"):
        sim.ops.model_rollout_stats(d, s)
    d, s = descs()                                                                  # the untouched descriptors still run on the same context
    sim.ops.model_rollout_stats(d, s)
    torch.cuda.synchronize()
    assert torch.equal(s1[..., :sim.nx], good.x_sum) and torch.equal(s2[..., sim.nx:], good.y_sumsq) and torch.equal(lpd, good.lpd)
    again = sim.predict(c.A, kd, replicates=P)
    assert torch.equal(again.y_sum, good.y_sum) and torch.equal(again.lpd, good.lpd)
