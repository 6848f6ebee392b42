"""pgas_amd.ModelRollout.forecast on the GPU (pgas_m_forecast, csrc/pgas_marginal_forecast.hip.h): the h-step-ahead
predictions of a grey-box model from the particle trace of its held-out filter, every origin row of every draw in one launch.

The checks split at the clouds.  DOWNSTREAM of them (moments, log score, the NaN triangle) everything is compared bit for bit with the
NumPy restatement (tests/model_forecast_numpy.py) fed the device's own clouds.  UPSTREAM, horizon 1 is the filter's own trace bit for bit;
every later lead is pinned TEACHER-FORCED to the per-step primitives the kernel fuses (hilbert_basis -> A phi -> expr_eval) within
1e-12 max(1, |ref|_max) (section 14's bound), with the normals of (target row, lead << 32 | particle); and without noise the clouds of an
origin are ModelRollout.__call__ from that trace row, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import model_filter_cases as cases
import model_forecast_numpy as mfc
from common import experiments, pgas_amd
from pgas_amd import _lib
from pgas_amd._lib import MarginalOps, ModelForecastDesc, PgasError
from pgas_amd.Algorithm1 import STREAM_STATE
from pgas_amd.model_rollout import STREAM_ROLLOUT_INTVAR
from test_gpu_model_filter import ALL, Case, _case, _close, _np
from test_model_forecast_host import CLOSED_FORM_KEYS, closed_form_z

pytestmark = pytest.mark.gpu
K, T, KEYS, H = cases.K, cases.T, cases.KEYS, 4
OUT = ("sum", "sumsq", "lpd", "cloud_x", "cloud_y")
FLT = ("loglik", "ell", "pred_sum", "pred_sumsq", "x", "yhat")


def _host(r):
    """A ModelForecastResult on the host: its own outputs and the filter's fields the tests use; read-only."""
    g = {f: (None if getattr(r, f) is None else _np(getattr(r, f))) for f in OUT}
    g.update({"f_" + f: _np(getattr(r.filter, f)) for f in FLT})
    for a in g.values():
        if a is not None:
            a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _drawn(name, N):
    """The forecast with drawn x_0, log score and clouds, on the host; computed once, never changed."""
    c = _case(name)
    return _host(c.sim.forecast(c.A, KEYS, N, H, clouds=True))


def _restated(g, c, y, what, Hn=H, Tn=T, draws=K):
    """Shapes, the NaN triangle, and everything downstream of the clouds against the restatement, bit for bit."""
    nx, ny, N = c.sim.nx, c.sim.ny, g["cloud_x"].shape[3]
    assert g["sum"].shape == g["sumsq"].shape == (draws, Hn, Tn, nx + ny) and g["lpd"].shape == (draws, Hn, Tn), what
    assert g["cloud_x"].shape == (draws, Hn, Tn, N, nx) and g["cloud_y"].shape == (draws, Hn, Tn, N, ny), what
    ok = mfc.defined(Hn, Tn)
    LRinv, cR = np.asarray(c.ssm._LRinv, dtype=np.float64), float(c.ssm._cR)
    for k in range(draws):
        for f in OUT:
            assert np.isnan(g[f][k][~ok]).all(), f"{what}: {f}[{k}] has a number where no origin row exists"
        assert np.isfinite(g["cloud_x"][k][ok]).all() and np.isfinite(g["cloud_y"][k][ok]).all(), what
        w = mfc.run(g["cloud_x"][k], g["cloud_y"][k], y, cR, LRinv)
        for f in ("sum", "sumsq", "lpd"):
            assert np.array_equal(g[f][k], w[f], equal_nan=True), f"{what}: {f}[{k}]"


# ---- 1. downstream of the clouds, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", ALL, ids=[f"{n}-N{N}" for n, N in ALL])
def test_everything_downstream_of_the_clouds_is_the_restatement(name, N):
    c = _case(name)
    g = _drawn(name, N)
    _restated(g, c, c.y, "drawn x_0")
    assert np.isfinite(g["lpd"][:, mfc.defined(H, T)]).all()


# ---- 2. horizon 1 is the filter -------------------------------------------------------------------------------------------------------------
def _horizon_1_is_the_filter(g, what):
    assert np.array_equal(g["cloud_x"][:, 0], g["f_x"]) and np.array_equal(g["cloud_y"][:, 0], g["f_yhat"]), what
    assert np.array_equal(g["sum"][:, 0], g["f_pred_sum"]) and np.array_equal(g["sumsq"][:, 0], g["f_pred_sumsq"]), what
    ell = g["f_ell"]
    assert np.isfinite(ell).all() and np.all(np.abs(g["lpd"][:, 0] - ell) <= 1e-12 * np.maximum(1.0, np.abs(ell))), what


@pytest.mark.parametrize("name,N", ALL, ids=[f"{n}-N{N}" for n, N in ALL])
def test_horizon_1_is_the_filter(name, N):
    c = _case(name)
    g = _drawn(name, N)
    _horizon_1_is_the_filter(g, "drawn x_0")
    alone = c.sim.filter(c.A, KEYS, N, traces=True)   # the filter inside forecast is the filter
    for f in FLT:
        assert np.array_equal(_np(getattr(alone, f)), g["f_" + f]), f


def _row_cov(c):
    rng = np.random.default_rng(4)
    covs = []
    for i, w in enumerate(c.sim.widths):
        B = rng.standard_normal((K, w, w))
        scale = float(np.abs(_np(c.xi(0, torch.as_tensor(np.asarray(c.pb.init_state_mean, dtype=np.float64)[None], device=c.dev), c.u[0])[i])).max()) + 1.0
        covs.append((1e-2 * scale) ** 2 * (B @ B.transpose(0, 2, 1) + np.eye(w)))
    return covs, [torch.as_tensor(np.linalg.cholesky(cv), device=c.dev) for cv in covs]


@functools.lru_cache(maxsize=None)
def _noisy_iv(name):
    c = _case(name)
    covs, rows = _row_cov(c)
    return _host(c.sim.forecast(c.A, KEYS, 200, H, row_cov=covs, clouds=True)), rows


@pytest.mark.parametrize("name", ["smo2", "vehicle"])
def test_horizon_1_is_the_filter_with_interface_variable_noise(name):
    """Equality with yhat shows that the particle index at lead 0 is the slot's own: xi_s is formed with the filter's normals."""
    g, _ = _noisy_iv(name)
    _horizon_1_is_the_filter(g, "row_cov")
    _restated(g, _case(name), _case(name).y, "row_cov")
    assert not np.array_equal(g["cloud_y"][:, 0], _drawn(name, 200)["cloud_y"][:, 0])


# ---- 3. the propagation, teacher-forced -----------------------------------------------------------------------------------------------------
def _normals(c, key, stream, t, lead, N, n):
    """Rows of pgas_m_rng_normal(key, stream, t, p0 = lead << 32, N, n): the lead sits in the high word of the particle index."""
    out = torch.empty((N, n), dtype=torch.float64, device=c.dev)
    eng = c.ops.eng
    eng._chk(eng.lib.pgas_m_rng_normal(eng._h, int(key), int(stream), int(t), int(lead) << 32, N, n, out.data_ptr(), eng._stream()), "pgas_m_rng_normal")
    return out


def _one_step(c, k, lead, tau, prev, N, rows=None, p0_lead=None):
    """Row tau of lead `lead` from the cloud `prev` of row tau - 1 by the per-step primitives; p0_lead: the lead the normals are taken at."""
    sim = c.sim
    pl = lead if p0_lead is None else p0_lead
    x = torch.as_tensor(prev.copy(), device=c.dev)
    xi = c.xi(k, x, c.u[tau - 1])
    if rows is not None:   # xi of row tau - 1 was formed at lead - 1
        for i in range(sim.L):
            e = _normals(c, KEYS[k], STREAM_ROLLOUT_INTVAR + i, tau - 1, lead - 1 if p0_lead is None else p0_lead, N, sim.widths[i])
            xi[i] = (xi[i] + e @ rows[i][k].T).contiguous()
    if c.ssm.is_deterministic:
        return c.ssm.transition_mdl(x, c.u[tau - 1], *xi).reshape(N, -1)
    return c.ssm.draw_state(_normals(c, KEYS[k], STREAM_STATE, tau, pl, N, sim.nx), x, c.u[tau - 1], *xi).reshape(N, -1)


def _check_propagation(c, g, N, rows=None):
    for k in range(K):
        for lead in range(1, H):
            for tau in range(lead, T):
                _close(g["cloud_x"][k, lead, tau], _one_step(c, k, lead, tau, g["cloud_x"][k, lead - 1, tau - 1], N, rows), f"cloud_x[{k},{lead},{tau}]")
        if rows is None:   # with interface-variable noise g is not a function of x alone: pinned through the next step above
            for lead in range(H):
                for tau in range(lead, T):
                    x = torch.as_tensor(g["cloud_x"][k, lead, tau].copy(), device=c.dev)
                    _close(g["cloud_y"][k, lead, tau], c.ssm.output_mdl(x, c.u[tau], *c.xi(k, x, c.u[tau])).reshape(N, -1), f"cloud_y[{k},{lead},{tau}]")


@pytest.mark.parametrize("name,N", ALL, ids=[f"{n}-N{N}" for n, N in ALL])
def test_clouds_are_the_primitives_teacher_forced(name, N):
    c = _case(name)
    g = _drawn(name, N)
    _check_propagation(c, g, N)
    if not c.ssm.is_deterministic and N >= 2:   # the same step with the filter's particle index (p0 = 0) misses
        k, lead, tau = 0, 2, 5
        wrong = _np(_one_step(c, k, lead, tau, g["cloud_x"][k, lead - 1, tau - 1], N, p0_lead=0))
        assert np.abs(wrong - g["cloud_x"][k, lead, tau]).max() > 1e-9 * max(1.0, float(np.abs(wrong).max()))
        assert not np.array_equal(g["cloud_x"][k, 1, tau], g["cloud_x"][k, 2, tau])          # each lead has its own noise


@pytest.mark.parametrize("name", ["smo2", "vehicle"])
def test_interface_variable_noise_uses_the_leads_particle_index(name):
    c = _case(name)
    g, rows = _noisy_iv(name)
    _check_propagation(c, g, 200, rows=rows)
    k, lead, tau = 0, 2, 5   # lead 2 reads xi of row 4 formed at lead 1: with the normals of lead 0 (p0 = 0) the step misses
    sim = c.sim
    x = torch.as_tensor(g["cloud_x"][k, lead - 1, tau - 1].copy(), device=c.dev)
    xi = c.xi(k, x, c.u[tau - 1])
    for i in range(sim.L):
        xi[i] = (xi[i] + _normals(c, KEYS[k], STREAM_ROLLOUT_INTVAR + i, tau - 1, 0, 200, sim.widths[i]) @ rows[i][k].T).contiguous()
    z = _normals(c, KEYS[k], STREAM_STATE, tau, lead, 200, sim.nx)
    wrong = _np(c.ssm.draw_state(z, x, c.u[tau - 1], *xi) if not c.ssm.is_deterministic else c.ssm.transition_mdl(x, c.u[tau - 1], *xi)).reshape(200, -1)
    assert np.abs(wrong - g["cloud_x"][k, lead, tau]).max() > 1e-9 * max(1.0, float(np.abs(wrong).max()))


# ---- 4. noise-free: the clouds of an origin are the rollout from that trace row ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.MODELS))
def test_noise_free_clouds_are_the_open_loop_rollout_from_the_trace_row(name):
    c = _case(name)
    N = 130
    rng = np.random.default_rng(8)
    m0 = np.asarray(c.pb.init_state_mean, dtype=np.float64)
    x0 = m0 + 0.05 * (np.abs(m0) + 1.0) * rng.standard_normal((K, N, c.sim.nx))
    r = c.sim.forecast(c.A, KEYS, N, H, init_state=x0, process_noise=False, clouds=True)
    assert np.array_equal(_np(r.filter.x[:, 0]), x0)
    _, widths, _ = cases.problem(name)
    for s in (0, 5, T - 1):
        L = min(H, T - s)
        sub = pgas_amd.ModelRollout(c.pb.inputs[s:s + L], c.ssm, c.pb.basis, int_var_widths=widths, ops=c.ops)
        ox, oy = sub(c.A, init_state=r.filter.x[:, s].contiguous(), replicates=N, process_noise=False, outputs=True)
        for lead in range(L):
            assert torch.equal(r.cloud_x[:, lead, s + lead], ox[:, lead]) and torch.equal(r.cloud_y[:, lead, s + lead], oy[:, lead]), (s, lead)


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------------------
def _record(name, Tn, ops):
    """The model over a record of Tn rows on `ops`, with K coefficient draws: (sim, ssm, A, y)."""
    make, widths = cases.MODELS[name]
    pb = make(T=Tn)
    R = pb.output_noise if cases.NOISE_R[name] is None else cases.NOISE_R[name]
    ssm = pgas_amd.SymbolicStateSpaceModel(pb.process_noise, np.atleast_2d(np.asarray(R, dtype=np.float64)), pb.model)
    y = np.asarray(pb.observations, dtype=np.float64).reshape(Tn, -1)
    sim = pgas_amd.ModelRollout(pb.inputs[:Tn], ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, int_var_widths=widths, ops=ops, observations=y)
    return sim, ssm, [torch.as_tensor(a, device=ops.device) for a in cases.coeffs(pb)], y


class _Rec:
    def __init__(self, sim, ssm):
        self.sim, self.ssm = sim, ssm


def test_record_lengths_around_the_origin_chunks_and_the_horizon_edges():
    c = _case("smo")
    TB = _lib.load().pgas_m_forecast_origins_per_block()
    assert TB >= 1
    N = 70
    for Tn in sorted({1, 2, max(TB - 1, 1), TB + 1, 2 * TB + 3}):
        sim, ssm, A, y = _record("smo", Tn, c.ops)
        for Hn in sorted({1, min(2, Tn), Tn}):
            g = _host(sim.forecast(A, KEYS, N, Hn, clouds=True))
            _restated(g, _Rec(sim, ssm), y, f"T = {Tn}, H = {Hn}", Hn, Tn)
            _horizon_1_is_the_filter(g, f"T = {Tn}, H = {Hn}")
            if Hn == Tn and Tn > 1:   # a shorter horizon is the head of a longer one
                for f in OUT:
                    assert np.array_equal(g[f][:, :1], _host(sim.forecast(A, KEYS, N, 1, clouds=True))[f], equal_nan=True), (Tn, f)


def test_horizon_4_against_horizon_2_and_the_whole_record():
    c = _case("vehicle")
    N = 200
    g = _drawn("vehicle", N)
    two = _host(c.sim.forecast(c.A, KEYS, N, 2, clouds=True))
    full = _host(c.sim.forecast(c.A, KEYS, N, T, clouds=True))
    _restated(full, c, c.y, "H = T", T, T)
    for f in OUT:
        assert np.array_equal(two[f], g[f][:, :2], equal_nan=True) and np.array_equal(full[f][:, :H], g[f], equal_nan=True), f


def test_no_result_bit_depends_on_the_origins_per_workgroup(monkeypatch):
    c = _case("smo2")
    N = 257
    g = _drawn("smo2", N)
    lib = _lib.load()
    default = lib.pgas_m_forecast_origins_per_block()
    for tb in (1, 5, T, 64):
        monkeypatch.setenv("PGAS_M_FORECAST_TB", str(tb))
        assert lib.pgas_m_forecast_origins_per_block() == tb
        h = _host(c.sim.forecast(c.A, KEYS, N, H, clouds=True))
        for f in OUT:
            assert np.array_equal(h[f], g[f], equal_nan=True), (tb, f)
    monkeypatch.delenv("PGAS_M_FORECAST_TB")
    assert lib.pgas_m_forecast_origins_per_block() == default


# ---- 6. NaN and far rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "vehicle"])
def test_nan_and_far_rows(name):
    base = _case(name)
    N = 200
    y = base.y.copy()
    y[3, -1] = np.nan          # one component of one row
    y[7, 0] = 1e200            # the quadratic form overflows: every density is 0
    c = Case(name, ops=base.ops, observations=y)
    g = _host(c.sim.forecast(c.A, KEYS, N, H, clouds=True))
    for h in range(H):
        assert np.isnan(g["lpd"][:, h, 3]).all() and (g["lpd"][:, h, 7] == -np.inf).all()
        rest = [t for t in range(h, T) if t not in (3, 7)]
        assert np.isfinite(g["lpd"][:, h, rest]).all() and np.isfinite(g["sum"][:, h, h:]).all() and np.isfinite(g["sumsq"][:, h, h:]).all()
    _restated(g, c, y, "NaN and far rows")
    assert np.array_equal(g["cloud_x"][:, 0], g["f_x"]) and np.array_equal(g["sum"][:, 0], g["f_pred_sum"])
    assert np.array_equal(g["cloud_x"][:, :, :4], _drawn(name, N)["cloud_x"][:, :, :4], equal_nan=True)   # targets up to row 3 have seen the same rows


# ---- 7. independence of the launch -----------------------------------------------------------------------------------------------------------------
def _outs(r):
    return [None if getattr(r, f) is None else _np(getattr(r, f)) for f in OUT]


def test_draws_are_independent_of_their_order_and_equal_inputs_give_equal_rows():
    c = _case("vehicle")
    N = 130
    fwd = _outs(c.sim.forecast(c.A, KEYS, N, H, clouds=True))
    rev = _outs(c.sim.forecast([a.flip(0).contiguous() for a in c.A], KEYS[::-1], N, H, clouds=True))
    for a, b in zip(fwd, rev):
        assert np.array_equal(a[::-1], b, equal_nan=True)
    idx = [0, 2, 0]
    dup = _outs(c.sim.forecast([a[idx].contiguous() for a in c.A], [KEYS[i] for i in idx], N, H, clouds=True))
    for a, d in zip(fwd, dup):
        assert np.array_equal(d[0], d[2], equal_nan=True) and np.array_equal(d[0], a[0], equal_nan=True) and np.array_equal(d[1], a[2], equal_nan=True)
        assert not np.array_equal(d[0], d[1], equal_nan=True)


def test_more_workgroups_than_the_device_holds_at_once():
    c = _case("smo")
    Kbig, N = 2000, 64
    A = [torch.as_tensor(a, device=c.dev) for a in cases.coeffs(c.pb, Kbig, seed=11)]
    keys = [1000 + 7 * k for k in range(Kbig)]
    got = _outs(c.sim.forecast(A, keys, N, H))
    assert got[0].shape == (Kbig, H, T, 3) and got[2].shape == (Kbig, H, T) and np.isfinite(got[2][:, mfc.defined(H, T)]).all()
    half = Kbig // 2
    lo = _outs(c.sim.forecast([a[:half].contiguous() for a in A], keys[:half], N, H))
    hi = _outs(c.sim.forecast([a[half:].contiguous() for a in A], keys[half:], N, H))
    for a, l, h in zip(got[:3], lo[:3], hi[:3]):
        assert np.array_equal(a[:half], l, equal_nan=True) and np.array_equal(a[half:], h, equal_nan=True)


def test_draws_beyond_one_launch_run_in_chunks(monkeypatch):
    import pgas_amd.model_rollout as mr

    c = _case("smo")
    Kd, N = 5, 70
    A = [torch.as_tensor(a, device=c.dev) for a in cases.coeffs(c.pb, Kd, seed=3)]
    keys = [11, 12, 13, 14, 15]
    whole = _outs(c.sim.forecast(A, keys, N, H, clouds=True))
    launches = []
    real = c.ops.model_forecast
    monkeypatch.setattr(mr, "MAX_DRAWS_PER_LAUNCH", 2)
    monkeypatch.setattr(c.ops, "model_forecast", lambda d, f: (launches.append((d.K, d.P, f.H)), real(d, f))[1])
    parts = _outs(c.sim.forecast(A, keys, N, H, clouds=True))
    assert launches == [(2, N, H), (2, N, H), (1, N, H)]
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 8. nullable outputs -----------------------------------------------------------------------------------------------------------------------------
def test_outputs_not_asked_for_are_none_and_change_nothing():
    c = _case("vehicle")
    N = 200
    g = _drawn("vehicle", N)
    plain = c.sim.forecast(c.A, KEYS, N, H)
    assert plain.cloud_x is None and plain.cloud_y is None
    bare = c.sim.forecast(c.A, KEYS, N, H, log_score=False)
    assert bare.lpd is None and bare.cloud_x is None and bare.cloud_y is None
    only = c.sim.forecast(c.A, KEYS, N, H, log_score=False, clouds=True)
    assert only.lpd is None
    for r in (plain, bare, only):
        assert np.array_equal(_np(r.sum), g["sum"], equal_nan=True) and np.array_equal(_np(r.sumsq), g["sumsq"], equal_nan=True)
    assert np.array_equal(_np(plain.lpd), g["lpd"], equal_nan=True)
    assert np.array_equal(_np(only.cloud_x), g["cloud_x"], equal_nan=True) and np.array_equal(_np(only.cloud_y), g["cloud_y"], equal_nan=True)
    s = pgas_amd.forecast_summary(plain, y=c.y)                                       # works on the result unchanged
    assert tuple(s["y_pred_mean"].shape) == (H, T, 2) and tuple(s["x_pred_std"].shape) == (H, T, 2)
    assert bool(torch.isfinite(s["rmse"]).all()) and bool(torch.isfinite(s["log_score"]).all())
    assert "log_score" not in pgas_amd.forecast_summary(bare)
    assert isinstance(plain, pgas_amd.ModelForecastResult) and isinstance(plain.filter, pgas_amd.ModelFilterResult) and plain.horizon == H and plain.n == N


# ---- 9. no host round trip -----------------------------------------------------------------------------------------------------------------------------
def test_forecast_makes_no_host_round_trip():
    c = _case("vehicle")
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    cov = [torch.eye(1, dtype=torch.float64, device=c.dev).repeat(K, 1, 1) * 1e-4 for _ in range(2)]
    calls = [lambda: c.sim.forecast(c.A, kd, 130, H, clouds=True), lambda: c.sim.forecast(c.A, kd, 3, 2, init_state=x0, row_cov=cov),
             lambda: c.sim.forecast(c.A, kd, 300, T, log_score=False)]
    warm = [f() for f in calls]   # uploads of the programs, tables and observations, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [f() for f in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        for f in OUT:
            u, v = getattr(a, f), getattr(b, f)
            assert (u is None) == (v is None) and (u is None or torch.equal(torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0))), f
        assert bool(torch.isfinite(a.filter.loglik).all())


# ---- 10. the context is left as it was -----------------------------------------------------------------------------------------------------------------
def test_forecast_leaves_filter_rollout_predict_and_algorithm1_on_the_same_context_unchanged():
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
    st = c.sim.predict(c.A, KEYS, replicates=70)
    pred = [t.clone() for t in (st.x_sum, st.x_sumsq, st.y_sum, st.y_sumsq, st.lpd)]
    flt = c.sim.filter(c.A, KEYS, 200, traces=True)
    r = c.sim.forecast(c.A, KEYS, 200, H, clouds=True)
    assert bool(torch.isfinite(r.filter.loglik).all())
    again = c.sim(c.A, KEYS, replicates=70, outputs=True)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    st = c.sim.predict(c.A, KEYS, replicates=70)
    for a, b in zip(pred, (st.x_sum, st.x_sumsq, st.y_sum, st.y_sumsq, st.lpd)):
        assert torch.equal(a, b)
    flt2 = c.sim.filter(c.A, KEYS, 200, traces=True)
    assert all(torch.equal(getattr(flt, f), getattr(flt2, f)) and torch.equal(getattr(flt, f), getattr(r.filter, f)) for f in flt.FIELDS)
    _, after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---- 11. the refusals of the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(monkeypatch):
    c = _case("vehicle")
    sim = c.sim
    N = 70
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    good = sim.forecast(c.A, kd, N, H)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=c.dev)   # noqa: E731
    s1, s2, lpd = new(K, H, T, 4), new(K, H, T, 4), new(K, H, T)
    ydev = sim._static()["y"]
    import pgas_amd.model_rollout as mr

    # the forecast's static LDS is smaller than the filter's, so the C ABI holds more files than ModelRollout.filter allows
    fit = 64 * ((mr.LDS_PER_WORKGROUP - mr.FORECAST_STATIC_LDS - sim.filter_lds_bytes(0)) // sim._filter_file_bytes())
    assert c.nmax < fit < 1024

    def descs():
        d = sim._desc(K, N, 0, 0, c.A, None, kd, None, True, None, None)
        f = ModelForecastDesc()
        f.x_dev, f.y_dev, f.sum_dev, f.sumsq_dev, f.lpd_dev = good.filter.x.data_ptr(), ydev.data_ptr(), s1.data_ptr(), s2.data_ptr(), lpd.data_ptr()
        f.H, f.cR = H, float(c.ssm._cR)
        for j in range(2):
            for l in range(2):
                f.LRinv[2 * j + l] = float(c.ssm._LRinv[j, l])
        return d, f

    edits = {
        "N = 0": lambda d, f: setattr(d, "P", 0),
        "N = 1025": lambda d, f: setattr(d, "P", 1025),
        "p0 = 64": lambda d, f: setattr(d, "p0", 64),
        "H = 0": lambda d, f: setattr(f, "H", 0),
        f"H = {T + 1}": lambda d, f: setattr(f, "H", T + 1),
        "NULL argument (x, sum, sumsq)": lambda d, f: setattr(f, "x_dev", None),
        "(x, sum, sumsq)": lambda d, f: setattr(f, "sum_dev", None),
        "x, sum, sumsq": lambda d, f: setattr(f, "sumsq_dev", None),
        "needs the observations y": lambda d, f: setattr(f, "y_dev", None),
        "needs seeds": lambda d, f: setattr(d, "seeds_dev", None),
        "K = 65536": lambda d, f: setattr(d, "K", 65536),
        f"the largest N that fits is {fit}": lambda d, f: setattr(d, "P", fit + 1),   # one more register file than LDS holds
        "output program": lambda d, f: setattr(d, "gcode_dev", None),              # what pgas_m_rollout_stats refuses of the descriptor
        "L = 0": lambda d, f: setattr(d, "L", 0),
        "K = 0": lambda d, f: setattr(d, "K", 0),
        "97 registers": lambda d, f: setattr(d, "nreg", 97),
    }
    for what, edit in edits.items():
        d, f = descs()
        edit(d, f)
        with pytest.raises(PgasError, match=r"pgas_m_forecast failed \(-1\)") as ei:   # PGAS_E_ARG, with the library's message
            sim.ops.model_forecast(d, f)
        assert "pgas_m_forecast: " in str(ei.value) and what in str(ei.value), (what, str(ei.value))
    d, f = descs()                                                                  # more chunks than the grid holds: T = 65536 rows, one per workgroup
    monkeypatch.setenv("PGAS_M_FORECAST_TB", "1")
    d.T = 65536
    with pytest.raises(PgasError, match="65535 chunks"):
        sim.ops.model_forecast(d, f)
    monkeypatch.delenv("PGAS_M_FORECAST_TB")
    d, f = descs()                                                                  # the untouched descriptors still run on the same context
    sim.ops.model_forecast(d, f)
    torch.cuda.synchronize()
    for got, want in ((s1, good.sum), (s2, good.sumsq), (lpd, good.lpd)):
        assert np.array_equal(_np(got), _np(want), equal_nan=True)
    d, f = descs()                                                                  # without the log score y may be NULL
    f.lpd_dev = f.y_dev = None
    s1.zero_()
    sim.ops.model_forecast(d, f)
    torch.cuda.synchronize()
    assert np.array_equal(_np(s1), _np(good.sum), equal_nan=True)
    again = sim.forecast(c.A, kd, N, H)
    assert np.array_equal(_np(again.lpd), _np(good.lpd), equal_nan=True)


# ---- 12. closed form ---------------------------------------------------------------------------------------------------------------------------------------
def test_linear_gaussian_model_against_the_kalman_h_step_predictive():
    kal = cases.KAL
    y = cases.kalman_record()
    ops = _case("toy").ops
    toy = experiments.toy_marginal(T=kal["T"])
    ssm = pgas_amd.SymbolicStateSpaceModel(np.array([[kal["q"]]]), np.array([[kal["r"]]]), cases.kalman_model)
    sim = pgas_amd.ModelRollout(np.zeros((kal["T"], 0)), ssm, toy.basis, np.array([kal["m0"]]), np.array([[kal["p0"]]]), ops=ops, observations=y)
    A = [np.zeros((kal["seeds"], 1, sim.latents[0].M))]
    assert len(CLOSED_FORM_KEYS) == kal["seeds"] == 16
    lpd = _np(sim.forecast(A, CLOSED_FORM_KEYS, kal["N"], H).lpd)
    z = closed_form_z(lpd, y, "device")
    assert (np.abs(z[2:]) <= 4.0).all()
