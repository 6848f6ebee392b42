"""pgas_amd.ModelRollout.smooth on the GPU (pgas_m_smooth, csrc/pgas_marginal_smooth.hip.h): backward simulation
over the trace of the grey-box filter, up to 256 trajectories of every draw per launch.

The checks split at the kernel's per-particle traces.  DOWNSTREAM of the filter's x, anc, lw, yhat and the smoother's fmean and xi,
every output is compared bit for bit (np.array_equal) with the NumPy restatement (tests/model_smooth_numpy.py).  UPSTREAM, fmean and xi
are pinned to ONE step of the per-step primitives the kernel fuses (hilbert_basis -> A phi [+ Lrow e] -> expr_eval) from the stored
x_t, within 1e-12 max(1, |ref|_max) (section 14's bound).  tests/test_model_smooth_host.py shows that under the process noise of
tests/model_smooth_cases.py the backward draw leaves the filter's genealogy in more than 0.3 of the steps."""
import functools

import numpy as np
import pytest
import torch

import model_filter_cases as cases
import model_smooth_cases as sc
import model_smooth_numpy as msn
from common import experiments, pgas_amd
from pgas_amd._lib import MarginalOps, ModelSmoothDesc, PgasError
from pgas_amd.model_rollout import STREAM_ROLLOUT_INTVAR
from test_smooth_host import check_marginals

pytestmark = pytest.mark.gpu
K, T, KEYS = sc.K, sc.T, sc.KEYS
FIELDS = ("idx", "xs", "xis", "sum", "sumsq", "xi_sum", "xi_sumsq")
TRACES = ("x", "anc", "lw", "yhat")


def _np(t):
    return t.detach().cpu().numpy()


class Case:
    """One model over its first Tn rows on one MarginalOps, under the smoother tests' process noise, with K coefficient draws."""

    def __init__(self, name, ops, Tn=T, observations=None):
        self.name, self.ops, self.dev, self.T = name, ops, ops.device, Tn
        self.pb, self.ssm, self.sim = sc.rollout(name, ops=ops, observations=observations, Tn=Tn)
        self.ssm.bind(ops)
        self.y = self.sim.observations
        self.u = torch.as_tensor(np.asarray(self.pb.inputs[:Tn], dtype=np.float64).reshape(Tn, -1), device=self.dev)
        self.A = [torch.as_tensor(a, device=self.dev) for a in sc.coeffs(name, self.pb)]

    def xi(self, k, x, u):
        """The interface variables of draw k at states x by the existing primitives."""
        out = []
        for i, b in enumerate(self.pb.basis):
            phi = self.ops.hilbert_basis(b.map, b.alpha(x, u).reshape(-1, 1).contiguous(), None) if hasattr(b, "feature") else self.ops.hilbert_basis(b, x.contiguous(), u)
            out.append((phi @ self.A[i][k].T).contiguous())
        return out


@functools.lru_cache(maxsize=None)
def _ops():
    return MarginalOps(1)


@functools.lru_cache(maxsize=None)
def _case(name, Tn=T):
    return Case(name, _ops(), Tn)


def _smooth(sim, A, keys, N, B, traces=True, trajectories=True, indices=True, interface=True, **kw):
    """``smooth`` with the kernel's per-particle traces: the public method's own two steps."""
    Kn, _, mode, noisy_state, _, Bn = sim.check_smooth(A, keys, N, B, kw.get("init_state"), kw.get("row_cov"), interface)
    flt = sim.filter(A, keys, N, kw.get("init_state"), kw.get("row_cov"), True, moments=True, traces=True)
    return sim._smooth_from(flt, Kn, N, mode, noisy_state, Bn, trajectories, indices, interface, traces=traces)


def _host(r):
    g = {f: (None if getattr(r, f) is None else _np(getattr(r, f))) for f in FIELDS + ("fmean", "xi")}
    g.update({f: _np(getattr(r.filter, f)) for f in TRACES})
    for a in g.values():
        if a is not None:
            a.setflags(write=False)
    return g


def _restate(sim, g, keys, y, n_traj, b0=None):
    """Everything downstream of the traces, per draw: the chunked call of the Python layer (b0 None) or one launch at b0."""
    LQinv, cQ = sim.transition_constants()
    out = []
    for k in range(len(keys)):
        args = (keys[k], g["x"][k], g["anc"][k], g["lw"][k], g["yhat"][k], g["fmean"][k], g["xi"][k], y, LQinv, cQ, n_traj)
        out.append(msn.run_chunks(*args) if b0 is None else msn.run(*args, b0))
    return out


def _assert_equal(g, want, what, fields=FIELDS):
    for k, w in enumerate(want):
        for f in fields:
            assert g[f][k].shape == w[f].shape and np.array_equal(g[f][k], w[f]), f"{what}: {f}[{k}]"


def _close(got, ref, what):
    ref = _np(ref) if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert np.all(np.isfinite(got)), what
    bound = 1e-12 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= bound, f"{what}: max |diff| = {err:.3e} > {bound:.3e}"


def _sizes(name, m):
    """(N, B, T) paired, not crossed: cases.NS clipped by max_particles() (N = 1024 on the toy model), B and T cycling along."""
    nmax = sc.rollout(name)[2].max_particles()
    ns = [n for n in (sc.NS if name in sc.MODELS else [1, 65, 200, 257, 513]) if n <= nmax] + ([1024] if name == "toy" else [])
    return [(name, N, sc.BS[(i + m) % len(sc.BS)], (12, 2, 1)[(i + 2 * m) % 3]) for i, N in enumerate(ns)]


NAMES = list(sc.MODELS) + list(sc.LINEAR)   # the linear models run the kernel's instances for nx = 3, 4 (constants) and nx = 5 (run time)
ALL = [c for m, name in enumerate(NAMES) for c in _sizes(name, m)]
assert ("toy", 1024) in [c[:2] for c in ALL] and {c[2] for c in ALL} == set(sc.BS) and {c[3] for c in ALL} == {1, 2, 12}
assert all({c[3] for c in ALL if c[0] == n} == {1, 2, 12} for n in NAMES) and ("lin3", 513) in [c[:2] for c in ALL] and ("lin5", 513) in [c[:2] for c in ALL]


# ---- 1. downstream of the traces, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,B,Tn", ALL, ids=[f"{n}-N{N}-B{B}-T{t}" for n, N, B, t in ALL])
def test_smooth_equals_the_restated_definition(name, N, B, Tn):
    c = _case(name, Tn)
    sim, nx, ny, nxi = c.sim, c.sim.nx, c.sim.ny, sum(c.sim.widths)
    g = _host(_smooth(sim, c.A, KEYS, N, B))
    assert g["idx"].shape == (K, B, Tn) and g["idx"].dtype == np.int32 and g["xs"].shape == (K, B, Tn, nx) and g["xis"].shape == (K, B, Tn, nxi)
    assert g["sum"].shape == g["sumsq"].shape == (K, Tn, nx + ny) and g["xi_sum"].shape == g["xi_sumsq"].shape == (K, Tn, nxi)
    assert g["fmean"].shape == (K, Tn, N, nx) and g["xi"].shape == (K, Tn, N, nxi)
    assert np.isnan(g["fmean"][:, Tn - 1]).all() and np.isfinite(g["fmean"][:, :Tn - 1]).all() and np.isfinite(g["xi"]).all()
    want = _restate(sim, g, KEYS, c.y, B)
    _assert_equal(g, want, f"{name}, N = {N}, B = {B}, T = {Tn}")
    if Tn > 1 and N >= 64:
        share = np.mean([sc.leaving_share(dict(anc=g["anc"][k]), dict(idx=g["idx"][k])) for k in range(K)])
        print(f"{name}, N = {N}: share of j_t != anc[t, j_t+1] on the device = {share:.3f}")


# ---- 2. fmean and xi: one step of the primitives from the stored x_t ---------------------------------------------------------------------
def _check_upstream(c, g, N, keys=KEYS, rows=None):
    sim, Tn = c.sim, c.T
    for k in range(len(keys)):
        for t in range(Tn):
            x = torch.as_tensor(g["x"][k, t].copy(), device=c.dev)
            xi = c.xi(k, x, c.u[t])
            if rows is not None:   # the noise of the particle's OWN index at time t: what step 2 of the filter drew for slot i
                for i in range(sim.L):
                    e = c.ops.eng.rng_normal(keys[k], STREAM_ROLLOUT_INTVAR + i, t, N, sim.widths[i])
                    xi[i] = (xi[i] + e @ rows[i][k].T).contiguous()
            _close(g["xi"][k, t], torch.cat([v.reshape(N, -1) for v in xi], dim=1), f"xi[{k},{t}]")
            if t < Tn - 1:
                _close(g["fmean"][k, t], c.ssm.transition_mdl(x, c.u[t], *xi).reshape(N, -1), f"fmean[{k},{t}]")


# N = 200: one pass of phase A, F = 4 files; 512, 513 and 1024: passes p >= 1 (NR = 2 and 4), where the restatement would take a wrong fmean as given
UPSTREAM = [(n, 200) for n in NAMES] + [("vehicle", 512), ("smo", 513), ("lin3", 513), ("lin4", 513), ("lin5", 513), ("toy", 1024)]


@pytest.mark.parametrize("name,N", UPSTREAM, ids=[f"{n}-N{N}" for n, N in UPSTREAM])
def test_fmean_and_xi_are_one_step_of_the_primitives(name, N):
    c = _case(name)
    g = _host(_smooth(c.sim, c.A, KEYS, N, 4))
    assert min(len(np.unique(a)) for a in g["anc"].reshape(-1, N)) <= 0.8 * N     # the rows are resampled clouds, not a rollout
    _check_upstream(c, g, N)


@pytest.mark.parametrize("name", ["smo2", "vehicle"])
def test_interface_noise_is_the_particles_own(name):
    c = _case(name)
    N, B = 130, 5
    rng = np.random.default_rng(4)
    covs = []
    for i, w in enumerate(c.sim.widths):
        Bm = rng.standard_normal((K, w, w))
        scale = float(np.abs(_np(c.xi(0, torch.as_tensor(np.asarray(c.pb.init_state_mean, dtype=np.float64)[None], device=c.dev), c.u[0])[i])).max()) + 1.0
        covs.append((1e-2 * scale) ** 2 * (Bm @ Bm.transpose(0, 2, 1) + np.eye(w)))
    rows = [torch.as_tensor(np.linalg.cholesky(cv), device=c.dev) for cv in covs]
    g = _host(_smooth(c.sim, c.A, KEYS, N, B, row_cov=covs))
    plain = _host(_smooth(c.sim, c.A, KEYS, N, B))
    assert not np.array_equal(g["xi"], plain["xi"])
    _check_upstream(c, g, N, rows=rows)
    _assert_equal(g, _restate(c.sim, g, KEYS, c.y, B), f"{name}, row_cov")


@pytest.mark.parametrize("name,N", [("toy", 200), ("smo", 200), ("vehicle", 512), ("smo2", 513), ("lin3", 200), ("lin3", 513), ("lin4", 513), ("toy", 1024)])
def test_the_run_time_nx_instance_gives_the_bits_of_the_constant_nx_instance(name, N, monkeypatch):
    """The instance that reads nx at run time (the only one a model with nx >= 5 can take) on models with nx = 1, 2, 3, 4, at NR = 1, 2, 4."""
    c = _case(name)
    B = 260 if N == 200 else 5
    const = _host(_smooth(c.sim, c.A, KEYS, N, B))
    monkeypatch.setenv("PGAS_M_SMOOTH_RUNTIME_NX", "1")
    runtime = _host(_smooth(c.sim, c.A, KEYS, N, B))
    monkeypatch.delenv("PGAS_M_SMOOTH_RUNTIME_NX")
    for f in FIELDS + ("fmean", "xi"):
        assert np.array_equal(const[f], runtime[f], equal_nan=True), f
    assert len({tuple(r) for r in const["idx"][0]}) > 1


# ---- 3. a trajectory depends on (key, g) alone ----------------------------------------------------------------------------------------------
def _launch(c, flt, N, B, b0, **out):
    """One pgas_m_smooth launch on the traces of `flt` with the outputs named in `out` (tensors)."""
    sim = c.sim
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    d = sim._desc(K, N, 0, 0, c.A, None, kd, None, True, None, None)
    sm = sim._smooth_desc()
    sm.B, sm.b0 = B, b0
    sm.x_dev, sm.anc_dev, sm.lw_dev, sm.yhat_dev = flt.x.data_ptr(), flt.anc.data_ptr(), flt.lw.data_ptr(), flt.yhat.data_ptr()
    for f, t in out.items():
        setattr(sm, f + "_dev", t.data_ptr())
    sim.ops.model_smooth(d, sm)
    torch.cuda.synchronize()
    return d, sm, kd


def test_trajectory_g_is_the_same_alone_in_a_full_launch_and_in_a_chunked_call():
    c = _case("vehicle")
    sim, N, n_traj = c.sim, 130, 300
    nx, ny, nxi = sim.nx, sim.ny, sum(sim.widths)
    r = _smooth(sim, c.A, KEYS, N, n_traj)
    g = _host(r)
    assert g["idx"].shape == (K, n_traj, T)
    _assert_equal(g, _restate(sim, g, KEYS, c.y, n_traj), "300 trajectories in two chunks")
    new = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device=c.dev)   # noqa: E731
    full = dict(idx=new(K, 256, T, dt=torch.int32), xs=new(K, 256, T, nx), xis=new(K, 256, T, nxi), sum=new(K, T, nx + ny), sumsq=new(K, T, nx + ny),
                xi_sum=new(K, T, nxi), xi_sumsq=new(K, T, nxi))
    rest = {f: (new(K, 44, T, *t.shape[3:], dt=t.dtype) if f in ("idx", "xs", "xis") else torch.empty_like(t)) for f, t in full.items()}
    _launch(c, r.filter, N, 256, 0, **full)
    _launch(c, r.filter, N, 44, 256, **rest)
    for f in ("idx", "xs", "xis"):
        assert np.array_equal(g[f], np.concatenate([_np(full[f]), _np(rest[f])], axis=1)), f
    for f in ("sum", "sumsq", "xi_sum", "xi_sumsq"):                               # the chunk sums add up as defined
        assert np.array_equal(g[f], _np(full[f]) + _np(rest[f])), f
    for gno in (0, 129, 255, 256, 299):
        one = dict(idx=new(K, 1, T, dt=torch.int32), xs=new(K, 1, T, nx), xis=new(K, 1, T, nxi))
        _launch(c, r.filter, N, 1, gno, **one)
        for f in one:
            assert np.array_equal(_np(one[f])[:, 0], g[f][:, gno]), (f, gno)


# ---- 4. fall-back rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "vehicle"])
def test_nan_row_and_outlier_rows_fall_back_to_the_filter_genealogy(name):
    base = _case(name)
    N, B = 200, 64
    y = base.y.copy()
    y[3, -1] = np.nan          # one component of one row: l = +0.0, the transition density alone decides
    y[7, 0] = 1e200            # the quadratic form overflows: every density is 0, the draw follows anc
    y[T - 1, 0] = 1e200        # ... and on the last row there is no next index: g mod N
    c = Case(name, base.ops, observations=y)
    g = _host(_smooth(c.sim, c.A, KEYS, N, B))
    assert np.isnan(g["lw"][:, 3]).all() and (g["lw"][:, 7] == -np.inf).all() and (g["lw"][:, T - 1] == -np.inf).all()
    want = _restate(c.sim, g, KEYS, y, B)
    assert all((w["S"][:, [7, T - 1]] == 0.0).all() and (np.delete(w["S"], [7, T - 1], axis=1) > 0).all() for w in want)
    _assert_equal(g, want, "NaN and far rows")
    for k in range(K):
        assert np.array_equal(g["idx"][k, :, T - 1], np.arange(B) % N)
        assert np.array_equal(g["idx"][k, :, 7], g["anc"][k, 7][g["idx"][k, :, 8]])
        assert len(np.unique(g["idx"][k, :, 3])) > 1
    shifted = _host(_smooth(c.sim, c.A, KEYS, N, 300))
    assert all(np.array_equal(shifted["idx"][k, :, T - 1], np.arange(300) % N) for k in range(K))   # b0 = 256 enters g mod N


# ---- 5. independence of the launch -------------------------------------------------------------------------------------------------------------
def test_draws_are_independent_of_their_order():
    c = _case("smo2")
    N, B = 130, 5
    fwd = _host(_smooth(c.sim, c.A, KEYS, N, B))
    rev = _host(_smooth(c.sim, [a.flip(0).contiguous() for a in c.A], KEYS[::-1], N, B))
    for f in FIELDS + ("fmean", "xi"):
        assert np.array_equal(fwd[f][::-1], rev[f], equal_nan=True), f


def test_more_draws_than_the_device_holds_at_once_and_chunks_of_draws(monkeypatch):
    import pgas_amd.model_rollout as mr

    c = _case("smo")
    Kbig, N, B = 2000, 64, 4
    A = [torch.as_tensor(a, device=c.dev) for a in cases.coeffs(c.pb, Kbig, seed=11)]
    keys = [1000 + 7 * k for k in range(Kbig)]
    got = _host(_smooth(c.sim, A, keys, N, B))
    assert got["idx"].shape == (Kbig, B, T) and np.isfinite(got["sum"]).all()
    for k in (0, 1234, Kbig - 1):
        one = _host(_smooth(c.sim, [a[k:k + 1].contiguous() for a in A], keys[k:k + 1], N, B))
        for f in FIELDS:
            assert np.array_equal(got[f][k], one[f][0]), f"draw {k}: {f}"
    sub = [a[:5].contiguous() for a in A]
    launches = []
    real = c.ops.model_smooth
    monkeypatch.setattr(mr, "MAX_DRAWS_PER_LAUNCH", 2)
    monkeypatch.setattr(c.ops, "model_smooth", lambda d, s: (launches.append((d.K, s.B, s.b0)), real(d, s))[1])
    parts = _host(_smooth(c.sim, sub, keys[:5], N, 260))
    assert launches == [(2, 256, 0), (2, 256, 0), (1, 256, 0), (2, 4, 256), (2, 4, 256), (1, 4, 256)]
    for f in ("idx", "xs", "xis"):
        assert np.array_equal(parts[f][:, :B], got[f][:5]), f


# ---- 6. the device indices are a backward simulation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kal", "toy"])
def test_marginal_of_the_device_indices_is_the_exact_smoother_marginal(name):
    N, Tn, n = 8, 6, 4096
    if name == "kal":
        ssm, sim, y = sc.kalman_rollout(_case("toy").pb.basis, _ops(), Tn)
        A, Q = [np.zeros((K, 1, sim.latents[0].M))], np.array([[sc.KAL["q"]]])
        y = y.reshape(-1, 1)
    else:
        c = _case("toy", Tn)
        sim, A, y, Q = c.sim, c.A, c.y, sc.process_noise("toy")
    g = _host(_smooth(sim, A, KEYS, N, n))
    assert g["idx"].shape == (K, n, Tn)
    w = msn.smoother_marginals(g["x"][0], g["lw"][0], g["fmean"][0], y, Q)
    assert np.allclose(w.sum(axis=1), 1.0, atol=1e-12)
    check_marginals(g["idx"][0], w, n)


# ---- 7. Kalman ---------------------------------------------------------------------------------------------------------------------------------
def test_linear_gaussian_model_against_the_rts_smoother():
    kal = sc.KAL
    ssm, sim, y = sc.kalman_rollout(_case("toy").pb.basis, _ops())
    A = [np.zeros((kal["seeds"], 1, sim.latents[0].M))]
    r = sim.smooth(A, [500 + 13 * s for s in range(kal["seeds"])], kal["N"], 256)
    mean = _np(pgas_amd.smoothing_summary(r)["x_smooth_mean_draw"])[:, :, 0]        # (seeds, T)
    want = msn.rts_smoother(kal["a"], kal["q"], kal["r"], kal["m0"], kal["p0"], y)
    se = mean.std(axis=0, ddof=1) / np.sqrt(mean.shape[0])
    z = np.abs(mean.mean(axis=0) - want) / se
    print("rows:", kal["T"], "worst |mean - RTS| / standard error:", float(z.max()))
    assert (se > 0).all() and (z <= 4).all(), f"mean {mean.mean(axis=0)}, RTS {want}, standard error {se}"
    filt = _np(r.filter.filt_sum / r.filter.wtot[..., None])[:, :, 0].mean(axis=0)
    assert np.abs(filt[:-1] - want[:-1]).max() > 4 * se[:-1].max()                  # the filtered mean is NOT the smoothed one: the test can tell
    xi = pgas_amd.interface_summary(r)
    assert float(xi["xi_smooth_mean"].abs().max()) == 0.0 and float(xi["xi_smooth_std"].abs().max()) == 0.0   # A = 0


# ---- 8. nullable outputs -------------------------------------------------------------------------------------------------------------------------
def test_nullable_outputs_change_nothing():
    c = _case("vehicle")
    N, B = 200, 64
    g = _host(_smooth(c.sim, c.A, KEYS, N, B))
    bare = c.sim.smooth(c.A, KEYS, N, B, interface=False)
    assert bare.xs is None and bare.idx is None and bare.xis is None and bare.xi_sum is None and bare.xi_sumsq is None and bare.fmean is None
    assert np.array_equal(_np(bare.sum), g["sum"]) and np.array_equal(_np(bare.sumsq), g["sumsq"])
    dflt = c.sim.smooth(c.A, KEYS, N, B)
    assert dflt.xs is None and dflt.idx is None and dflt.xis is None
    for f in ("sum", "sumsq", "xi_sum", "xi_sumsq"):
        assert np.array_equal(_np(getattr(dflt, f)), g[f]), f
    traj = c.sim.smooth(c.A, KEYS, N, B, trajectories=True, interface=False)
    assert traj.xis is None and traj.idx is None and np.array_equal(_np(traj.xs), g["xs"])
    full = c.sim.smooth(c.A, KEYS, N, B, trajectories=True, indices=True)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(full, f)), g[f]), f
    new = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device=c.dev)   # noqa: E731
    for f, t in (("idx", new(K, B, T, dt=torch.int32)), ("xis", new(K, B, T, 2)), ("fmean", new(K, T, N, 2)), ("xi", new(K, T, N, 2))):
        _launch(c, full.filter, N, B, 0, **{f: t})                                  # every output on its own
        rows = T - 1 if f == "fmean" else T                                         # row T - 1 of fmean is not written
        assert np.array_equal(_np(t)[:, :rows], g[f][:, :rows]) if f in ("fmean", "xi") else np.array_equal(_np(t), g[f]), f
    s = pgas_amd.smoothing_summary(full, y=c.y)                                     # works on the result unchanged
    assert tuple(s["y_smooth_mean"].shape) == (T, 2) and tuple(s["x_smooth_mean_draw"].shape) == (K, T, 2) and bool(torch.isfinite(s["rmse"]))
    xi = pgas_amd.interface_summary(full)
    assert tuple(xi["xi_smooth_mean"].shape) == (T, 2) and tuple(xi["xi_smooth_std_draw"].shape) == (K, T, 2)
    assert np.allclose(_np(xi["xi_smooth_mean_draw"]), g["xis"].mean(axis=1), rtol=1e-12, atol=1e-300)


# ---- 9. no host round trip -----------------------------------------------------------------------------------------------------------------------
def test_smooth_makes_no_host_round_trip():
    c = _case("vehicle")
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    cov = [torch.eye(1, dtype=torch.float64, device=c.dev).repeat(K, 1, 1) * 1e-4 for _ in range(2)]
    calls = [lambda: c.sim.smooth(c.A, kd, 130, 300, trajectories=True, indices=True), lambda: c.sim.smooth(c.A, kd, 3, 5, init_state=x0, row_cov=cov),
             lambda: c.sim.smooth(c.A, kd, 300, 64, interface=False)]
    warm = [f() for f in calls]   # uploads of the programs, tables and observations, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [f() for f in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        for f in FIELDS:
            u, v = getattr(a, f), getattr(b, f)
            assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), f
        assert bool(torch.isfinite(a.sum).all())


# ---- 10. the context is left as it was -----------------------------------------------------------------------------------------------------------
def test_smooth_leaves_the_filter_and_algorithm1_on_the_same_context_unchanged():
    pb = experiments.emps_marginal(T=T)

    def run():
        alg = pgas_amd.Algorithm1(64, pb.observations, pb.inputs, pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel), pb.forgetting_factor,
                                  pb.init_state_mean, pb.init_state_cov, pb.init_int_var_mean, pb.init_int_var_cov, pb.GP_prior, pb.basis_fcn())
        out = alg(12345678)
        return alg, [out[0], out[1][0], out[3], out[4]]

    alg, before = run()
    c = Case("emps", alg.ops)
    assert c.sim.ops is alg.ops
    r = c.sim.filter(c.A, KEYS, 200, traces=True)
    held = {f: getattr(r, f).clone() for f in r.FIELDS}
    s = c.sim.smooth(c.A, KEYS, 200, 300, trajectories=True, indices=True)
    assert bool(torch.isfinite(s.sum).all()) and bool(torch.isfinite(s.xi_sum).all())
    assert all(torch.equal(getattr(s.filter, f), held[f]) for f in held)             # smooth's own filter call is that filter
    r2 = c.sim.filter(c.A, KEYS, 200, traces=True)
    assert all(torch.equal(getattr(r2, f), held[f]) for f in held)
    s2 = c.sim.smooth(c.A, KEYS, 200, 300, trajectories=True, indices=True)
    assert all(torch.equal(getattr(s, f), getattr(s2, f)) for f in FIELDS)
    _, after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---- 11. the refusals of the C ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable():
    c = _case("vehicle")
    sim, N, B = c.sim, 70, 5
    assert sim.max_particles() == 512
    top = sim.smooth(c.A, KEYS, 512, 3)
    assert bool(torch.isfinite(top.sum).all())
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    good = sim.smooth(c.A, kd, N, B, trajectories=True, indices=True)
    flt = good.filter
    new = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device=c.dev)   # noqa: E731
    idx, s1, s2, x1, x2 = new(K, B, T, dt=torch.int32), new(K, T, 4), new(K, T, 4), new(K, T, 2), new(K, T, 2)

    def descs():
        d = sim._desc(K, N, 0, 0, c.A, None, kd, None, True, None, None)
        m = sim._smooth_desc()
        m.B, m.b0 = B, 0
        m.x_dev, m.anc_dev, m.lw_dev, m.yhat_dev = flt.x.data_ptr(), flt.anc.data_ptr(), flt.lw.data_ptr(), flt.yhat.data_ptr()
        m.idx_dev, m.sum_dev, m.sumsq_dev, m.xi_sum_dev, m.xi_sumsq_dev = idx.data_ptr(), s1.data_ptr(), s2.data_ptr(), x1.data_ptr(), x2.data_ptr()
        return d, m

    def no_output(d, m):
        for f in ("idx", "sum", "sumsq", "xi_sum", "xi_sumsq"):
            setattr(m, f + "_dev", None)

    edits = {
        "B = 0": lambda d, m: setattr(m, "B", 0),
        "B = 257": lambda d, m: setattr(m, "B", 257),
        "b0 = -1": lambda d, m: setattr(m, "b0", -1),
        "N = 0": lambda d, m: setattr(d, "P", 0),
        "N = 1025": lambda d, m: setattr(d, "P", 1025),
        "the largest N that fits is 576": lambda d, m: setattr(d, "P", 640),      # 10 files of 13824 B beside 27648 B of static LDS; the filter stops at 512
        "p0 = 64": lambda d, m: setattr(d, "p0", 64),
        "traces x, anc, lw and yhat": lambda d, m: setattr(m, "x_dev", None),
        "x, anc, lw and yhat": lambda d, m: setattr(m, "anc_dev", None),
        "anc, lw and yhat": lambda d, m: setattr(m, "lw_dev", None),
        "lw and yhat": lambda d, m: setattr(m, "yhat_dev", None),
        "NULL argument (y)": lambda d, m: setattr(m, "y_dev", None),
        "seeds are needed": lambda d, m: setattr(d, "seeds_dev", None),
        "needs process noise": lambda d, m: setattr(d, "Qc_dev", None),
        "sum and sumsq go together": lambda d, m: setattr(m, "sumsq_dev", None),
        "xi_sum and xi_sumsq go together": lambda d, m: setattr(m, "xi_sum_dev", None),
        "every output is NULL": no_output,
        "K = 65536": lambda d, m: setattr(d, "K", 65536),
        "LQinv[1,0] is not finite": lambda d, m: m.LQinv.__setitem__(2, float("nan")),
        "LQinv[0,0] is not finite": lambda d, m: m.LQinv.__setitem__(0, float("inf")),
        "cQ is not finite": lambda d, m: setattr(m, "cQ", float("-inf")),
        "output program": lambda d, m: setattr(d, "gcode_dev", None),              # what pgas_m_rollout_stats refuses of the descriptor
        "L = 0": lambda d, m: setattr(d, "L", 0),
        "97 registers": lambda d, m: setattr(d, "nreg", 97),
    }
    for what, edit in edits.items():
        d, m = descs()
        edit(d, m)
        with pytest.raises(PgasError, match=r"pgas_m_smooth failed \(-1\)") as ei:   # PGAS_E_ARG, with the library's message
            sim.ops.model_smooth(d, m)
        assert "pgas_m_smooth: " in str(ei.value) and what in str(ei.value), (what, str(ei.value))
    d, m = descs()                                                                  # the untouched descriptors still run on the same context
    sim.ops.model_smooth(d, m)
    torch.cuda.synchronize()
    assert torch.equal(idx, good.idx) and torch.equal(s1, good.sum) and torch.equal(s2, good.sumsq) and torch.equal(x1, good.xi_sum)
    again = sim.smooth(c.A, kd, N, B, trajectories=True, indices=True)
    assert all(torch.equal(getattr(again, f), getattr(good, f)) for f in FIELDS)
    assert isinstance(ModelSmoothDesc(), ModelSmoothDesc)


def test_more_than_sixteen_interface_components_are_refused_with_an_interface_output_only():
    from test_model_smooth_host import _wide_model

    sim = _wide_model()
    A = [np.zeros((K, w, h.M)) for w, h in zip(sim.widths, sim.latents)]
    with pytest.raises(ValueError, match="17 interface components"):
        sim.smooth(A, KEYS, 70, 5)
    r = sim.smooth(A, KEYS, 70, 5, trajectories=True, interface=False)
    assert r.xi_sum is None and r.xis is None and bool(torch.isfinite(r.sum).all()) and tuple(r.xs.shape) == (K, 5, T, 1)
    dev = sim.ops.device
    flt = r.filter
    kd = pgas_amd.chains.keys_tensor(KEYS, dev)
    d = sim._desc(K, 70, 0, 0, sim._keep[0], None, kd, None, True, None, None)
    m = sim._smooth_desc()
    m.B, m.b0 = 5, 0
    m.x_dev, m.anc_dev, m.lw_dev, m.yhat_dev = flt.x.data_ptr(), flt.anc.data_ptr(), flt.lw.data_ptr(), flt.yhat.data_ptr()
    xis = torch.empty((K, 5, T, 17), dtype=torch.float64, device=dev)
    m.xis_dev = xis.data_ptr()
    with pytest.raises(PgasError, match="17 interface components, an interface output takes 16"):
        sim.ops.model_smooth(d, m)
