"""pgas_amd.ModelRollout.filter on the GPU (pgas_m_filter, csrc/pgas_marginal_filter.hip.h): a bootstrap particle
filter per coefficient draw of a grey-box model, all draws in one launch.

The checks split at the particles' log-likelihoods.  DOWNSTREAM of them everything is compared bit for bit (np.array_equal) with the NumPy
restatement (tests/model_filter_numpy.py) fed the device's own traces lw, x and yhat.  UPSTREAM, the traces are pinned TEACHER-FORCED to
the per-step primitives the kernel fuses (hilbert_basis -> A phi -> expr_eval), within 1e-12 max(1, |ref|_max) (section 14's bound): yhat
and lw from the stored x_t, and every stored x_{t+1}[i] from ONE step from x_t[anc_t[i]] with the normals of (t + 1, i).
tests/test_model_filter_host.py shows that the ancestors on these records are far from the identity."""
import functools

import numpy as np
import pytest
import torch

import model_filter_cases as cases
import model_filter_numpy as mf
from common import experiments, pgas_amd
from pgas_amd._lib import MarginalOps, ModelFilterDesc, PgasError
from pgas_amd.Algorithm1 import STREAM_INIT_STATE, STREAM_STATE
from pgas_amd.model_rollout import STREAM_ROLLOUT_INTVAR

pytestmark = pytest.mark.gpu
K, T, KEYS = cases.K, cases.T, cases.KEYS
DOWNSTREAM = ("anc", "ell", "wtot", "ess", "filt_sum", "pred_sum", "pred_sumsq")


def _np(t):
    return t.detach().cpu().numpy()


class Case:
    """One model over T rows on one MarginalOps, under the filter tests' output noise, with K coefficient draws."""

    def __init__(self, name, ops=None, observations=None):
        self.name = name
        self.ops = ops or MarginalOps(1)
        self.dev = self.ops.device
        self.pb, self.ssm, self.sim = cases.rollout(name, ops=self.ops, observations=observations)
        self.ssm.bind(self.ops)
        self.y = self.sim.observations
        self.u = torch.as_tensor(np.asarray(self.pb.inputs[:T], dtype=np.float64).reshape(T, -1), device=self.dev)
        self.A = [torch.as_tensor(a, device=self.dev) for a in cases.coeffs(self.pb)]
        self.nmax = self.sim.max_particles()

    def xi(self, k, x, u):
        """The interface variables of draw k at states x by the existing primitives."""
        out = []
        for i, b in enumerate(self.pb.basis):
            phi = self.ops.hilbert_basis(b.map, b.alpha(x, u).reshape(-1, 1).contiguous(), None) if hasattr(b, "feature") else self.ops.hilbert_basis(b, x.contiguous(), u)
            out.append((phi @ self.A[i][k].T).contiguous())
        return out


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def _host(r):
    g = {f: (None if getattr(r, f) is None else _np(getattr(r, f))) for f in r.FIELDS}
    for a in g.values():
        if a is not None:
            a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _drawn(name, N):
    """The filter with drawn x_0, moments and traces, on the host; computed once, never changed."""
    c = _case(name)
    return _host(c.sim.filter(c.A, KEYS, N, traces=True))


def _particle_counts(name):
    """cases.NS clipped by the model's max_particles() (host arithmetic: no device is touched); N = 1024 runs on the toy model."""
    nmax = cases.rollout(name)[2].max_particles()
    return [n for n in cases.NS if n <= nmax] + ([1024] if name == "toy" else [])


ALL = [(n, N) for n in cases.MODELS for N in _particle_counts(n)]
assert ("toy", 1024) in ALL and ("vehicle", 512) in ALL and ("vehicle", 513) not in ALL and ("smo", 513) in ALL


def _downstream(g, y, what, keys=KEYS):
    """Everything downstream of lw, x, yhat against the restatement, bit for bit."""
    for k in range(len(keys)):
        w = mf.run(keys[k], g["lw"][k], g["x"][k], g["yhat"][k], y)
        for f in DOWNSTREAM:
            assert np.array_equal(g[f][k], w[f], equal_nan=True), f"{what}: {f}[{k}]"
        assert np.array_equal(g["loglik"][k], w["loglik"], equal_nan=True), f"{what}: loglik[{k}]"


def _close(got, ref, what):
    ref = _np(ref) if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert np.all(np.isfinite(got)), what
    bound = 1e-12 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= bound, f"{what}: max |diff| = {err:.3e} > {bound:.3e}"


# ---- 1. downstream of l, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", ALL, ids=[f"{n}-N{N}" for n, N in ALL])
def test_everything_downstream_of_the_log_likelihoods_is_the_restatement(name, N):
    c = _case(name)
    sim, nx, ny = c.sim, c.sim.nx, c.sim.ny
    g = _drawn(name, N)
    assert g["x"].shape == (K, T, N, nx) and g["yhat"].shape == (K, T, N, ny) and g["lw"].shape == g["anc"].shape == (K, T, N) and g["anc"].dtype == np.int32
    assert g["ell"].shape == g["ess"].shape == g["wtot"].shape == (K, T) and g["pred_sum"].shape == (K, T, nx + ny) and g["filt_sum"].shape == (K, T, nx)
    assert np.isfinite(g["loglik"]).all()
    _downstream(g, c.y, "drawn x_0")
    L0 = torch.as_tensor(np.linalg.cholesky(c.pb.init_state_cov), device=c.dev)
    m0 = torch.as_tensor(np.asarray(c.pb.init_state_mean, dtype=np.float64), device=c.dev)
    for k in range(K):   # row 0 as Algorithm1._init_algorithm draws it
        _close(g["x"][k, 0], m0 + c.ops.eng.rng_normal(KEYS[k], STREAM_INIT_STATE, 0, N, nx) @ L0.T, f"x0[{k}]")
    each = _host(sim.filter(c.A, KEYS, N, init_state=g["x"][:, 0].copy(), traces=True))   # (K, N, nx): the drawn cloud, given
    for f in each:
        assert np.array_equal(each[f], g[f], equal_nan=True), f"x_0 (K, N, nx): {f}"
    m0 = np.asarray(c.pb.init_state_mean, dtype=np.float64)
    for x0 in (m0 + 0.01, np.stack([m0 + 0.01 * (k + 1) for k in range(K)])):            # (nx) and (K, nx)
        if N > 1 and c.ssm.is_deterministic:
            with pytest.raises(ValueError, match="copies"):
                sim.filter(c.A, KEYS, N, init_state=x0)
            continue
        h = _host(sim.filter(c.A, KEYS, N, init_state=x0, traces=True))
        assert np.array_equal(h["x"][:, 0], np.broadcast_to(x0.reshape(-1, 1, nx), (K, N, nx)))
        _downstream(h, c.y, f"x_0 {x0.shape}")


# ---- 2, 3. l, g and the propagation through the resampling, teacher-forced ------------------------------------------------------------------
def _check_upstream(c, g, N, y, rows=None, skip_rows=()):
    """yhat and lw from the stored x_t; x_{t+1}[i] from ONE primitive step from x_t[anc_t[i]] with the state normals of (t + 1, i).  rows:
    Cholesky factors (K, n, n) of the interface-variable noise, whose normals are taken at particle index anc_t[i]."""
    sim = c.sim
    noisy = not c.ssm.is_deterministic
    for k in range(K):
        for t in range(T):
            x = torch.as_tensor(g["x"][k, t].copy(), device=c.dev)
            if rows is None:   # with interface-variable noise xi_t of the stored row is not a function of x_t alone: checked through the step below
                xi = c.xi(k, x, c.u[t])
                _close(g["yhat"][k, t], c.ssm.output_mdl(x, c.u[t], *xi).reshape(N, -1), f"yhat[{k},{t}]")
                if t not in skip_rows:
                    _close(g["lw"][k, t], c.ssm.log_likelihood(y[t], x, c.u[t], *xi), f"lw[{k},{t}]")
            if t == T - 1:
                break
            a = torch.as_tensor(g["anc"][k, t].astype(np.int64), device=c.dev)
            xa = x[a].contiguous()
            xi = c.xi(k, xa, c.u[t])
            if rows is not None:
                for i in range(sim.L):
                    e = c.ops.eng.rng_normal(KEYS[k], STREAM_ROLLOUT_INTVAR + i, t, N, sim.widths[i])
                    xi[i] = (xi[i] + e[a] @ rows[i][k].T).contiguous()
            if noisy:
                xn = c.ssm.draw_state(c.ops.eng.rng_normal(KEYS[k], STREAM_STATE, t + 1, N, sim.nx), xa, c.u[t], *xi)
            else:
                xn = c.ssm.transition_mdl(xa, c.u[t], *xi)
            _close(g["x"][k, t + 1], xn.reshape(N, -1), f"x[{k},{t + 1}]")


@pytest.mark.parametrize("name,N", ALL, ids=[f"{n}-N{N}" for n, N in ALL])
def test_traces_are_the_primitives_teacher_forced_through_the_resampling(name, N):
    c = _case(name)
    g = _drawn(name, N)
    if N >= 64:   # the check below means something: ancestors are not the identity
        assert min(len(np.unique(a)) for a in g["anc"].reshape(-1, N)) <= 0.8 * N
    _check_upstream(c, g, N, c.y)


@pytest.mark.parametrize("name", ["smo2", "vehicle"])
def test_interface_variable_noise_travels_with_the_resampled_particle(name):
    c = _case(name)
    N = 200
    rng = np.random.default_rng(4)
    covs = []
    for i, w in enumerate(c.sim.widths):
        B = rng.standard_normal((K, w, w))
        scale = float(np.abs(_np(c.xi(0, torch.as_tensor(np.asarray(c.pb.init_state_mean, dtype=np.float64)[None], device=c.dev), c.u[0])[i])).max()) + 1.0
        covs.append((1e-2 * scale) ** 2 * (B @ B.transpose(0, 2, 1) + np.eye(w)))
    rows = [torch.as_tensor(np.linalg.cholesky(cv), device=c.dev) for cv in covs]
    g = _host(c.sim.filter(c.A, KEYS, N, row_cov=covs, traces=True))
    assert not np.array_equal(g["x"][:, 1:], _drawn(name, N)["x"][:, 1:])
    distinct = [len(np.unique(a)) for a in g["anc"].reshape(-1, N)]
    assert min(distinct) <= 0.8 * N
    _downstream(g, c.y, "row_cov")
    _check_upstream(c, g, N, c.y, rows=rows)
    # the same check with xi's normals at the SLOT's index fails: the noise is large enough to tell the two apart
    k, t = 0, int(np.argmin(distinct[:T - 1]))
    x = torch.as_tensor(g["x"][k, t].copy(), device=c.dev)
    a = torch.as_tensor(g["anc"][k, t].astype(np.int64), device=c.dev)
    xa = x[a].contiguous()
    xi = c.xi(k, xa, c.u[t])
    for i in range(c.sim.L):
        xi[i] = (xi[i] + c.ops.eng.rng_normal(KEYS[k], STREAM_ROLLOUT_INTVAR + i, t, N, c.sim.widths[i]) @ rows[i][k].T).contiguous()
    wrong = _np(c.ssm.draw_state(c.ops.eng.rng_normal(KEYS[k], STREAM_STATE, t + 1, N, c.sim.nx), xa, c.u[t], *xi)).reshape(N, -1)
    assert np.abs(wrong - g["x"][k, t + 1]).max() > 1e-9 * max(1.0, float(np.abs(wrong).max()))


# ---- 4. no weights: the filter is the rollout ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nan_case(name):
    return Case(name, ops=_case(name).ops, observations=np.full((T, _case(name).sim.ny), np.nan))


@pytest.mark.parametrize("name,N", ALL, ids=[f"{n}-N{N}" for n, N in ALL])
def test_an_all_nan_record_is_the_open_loop_rollout(name, N):
    c = _nan_case(name)
    r = c.sim.filter(c.A, KEYS, N, traces=True)
    ox, oy = c.sim(c.A, KEYS, replicates=N, outputs=True)
    assert torch.equal(r.x, ox) and torch.equal(r.yhat, oy)
    assert bool(torch.isnan(r.ell).all()) and bool((r.loglik == 0).all()) and bool(torch.isnan(r.lw).all())
    assert bool((r.anc == torch.arange(N, device=c.dev, dtype=torch.int32)).all())
    assert bool((r.ess == 0).all()) and bool((r.wtot == 0).all())


# ---- 5. NaN and far rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "vehicle"])
def test_nan_and_far_rows(name):
    base = _case(name)
    N = 200
    y = base.y.copy()
    y[3, -1] = np.nan          # one component of one row
    y[7, 0] = 1e200            # the quadratic form overflows: every density is 0
    c = Case(name, ops=base.ops, observations=y)
    g = _host(c.sim.filter(c.A, KEYS, N, traces=True))
    ident = np.arange(N)
    assert np.isnan(g["ell"][:, 3]).all() and (g["ell"][:, 7] == -np.inf).all()
    assert all(np.array_equal(g["anc"][k, t], ident) for k in range(K) for t in (3, 7))
    rest = [t for t in range(T) if t not in (3, 7)]
    assert np.isfinite(g["ell"][:, rest]).all() and (g["loglik"] == -np.inf).all()
    assert np.isnan(g["lw"][:, 3]).all() and (g["lw"][:, 7] == -np.inf).all()
    assert np.array_equal(g["x"][:, :4], _drawn(name, N)["x"][:, :4])               # rows 0 .. 3 have seen the same observations
    assert min(len(np.unique(a)) for a in g["anc"][:, 8:].reshape(-1, N)) <= 0.8 * N   # later steps resample again
    _downstream(g, y, "NaN and far rows")
    _check_upstream(c, g, N, y, skip_rows=(3, 7))


# ---- 6. independence of the launch -----------------------------------------------------------------------------------------------------------
def _all(r):
    return [None if getattr(r, f) is None else _np(getattr(r, f)) for f in r.FIELDS]


def test_draws_are_independent_of_their_order_and_equal_inputs_give_equal_rows():
    c = _case("vehicle")
    N = 130
    fwd = _all(c.sim.filter(c.A, KEYS, N, traces=True))
    rev = _all(c.sim.filter([a.flip(0).contiguous() for a in c.A], KEYS[::-1], N, traces=True))
    for a, b in zip(fwd, rev):
        assert np.array_equal(a[::-1], b, equal_nan=True)
    idx = [0, 2, 0]
    dup = _all(c.sim.filter([a[idx].contiguous() for a in c.A], [KEYS[i] for i in idx], N, traces=True))
    for a, d in zip(fwd, dup):
        assert np.array_equal(d[0], d[2]) and np.array_equal(d[0], a[0]) and np.array_equal(d[1], a[2]) and not np.array_equal(d[0], d[1])


def test_more_draws_than_the_device_holds_at_once():
    c = _case("smo")
    Kbig, N = 2000, 64
    A = [torch.as_tensor(a, device=c.dev) for a in cases.coeffs(c.pb, Kbig, seed=11)]
    keys = [1000 + 7 * k for k in range(Kbig)]
    got = _all(c.sim.filter(A, keys, N))
    assert got[0].shape == (Kbig,) and got[1].shape == (Kbig, T) and np.isfinite(got[0]).all()
    for k in (0, Kbig - 1):
        one = _all(c.sim.filter([a[k:k + 1].contiguous() for a in A], keys[k:k + 1], N))
        for a, b in zip(got[:7], one[:7]):
            assert np.array_equal(a[k], b[0]), f"draw {k}"


def test_draws_beyond_one_launch_run_in_chunks(monkeypatch):
    import pgas_amd.model_rollout as mr

    c = _case("smo")
    Kd, N = 5, 70
    A = [torch.as_tensor(a, device=c.dev) for a in cases.coeffs(c.pb, Kd, seed=3)]
    keys = [11, 12, 13, 14, 15]
    whole = _all(c.sim.filter(A, keys, N, traces=True))
    launches = []
    real = c.ops.model_filter
    monkeypatch.setattr(mr, "MAX_DRAWS_PER_LAUNCH", 2)
    monkeypatch.setattr(c.ops, "model_filter", lambda d, f: (launches.append((d.K, d.P)), real(d, f))[1])
    parts = _all(c.sim.filter(A, keys, N, traces=True))
    assert launches == [(2, N), (2, N), (1, N)]
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b)


# ---- 7. Kalman ---------------------------------------------------------------------------------------------------------------------------------
def test_linear_gaussian_model_against_the_kalman_filter():
    kal = cases.KAL
    y = cases.kalman_record()
    ops = _case("toy").ops
    toy = experiments.toy_marginal(T=kal["T"])
    ssm = pgas_amd.SymbolicStateSpaceModel(np.array([[kal["q"]]]), np.array([[kal["r"]]]), cases.kalman_model)
    sim = pgas_amd.ModelRollout(np.zeros((kal["T"], 0)), ssm, toy.basis, np.array([kal["m0"]]), np.array([[kal["p0"]]]), ops=ops, observations=y)
    A = [np.zeros((kal["seeds"], 1, sim.latents[0].M))]
    ll = _np(sim.filter(A, [500 + 13 * s for s in range(kal["seeds"])], kal["N"], moments=False).loglik)
    want = mf.kalman_loglik(kal["a"], kal["q"], kal["r"], kal["m0"], kal["p0"], y)
    se = ll.std(ddof=1) / np.sqrt(len(ll))
    assert len(np.unique(ll)) == kal["seeds"]
    assert abs(ll.mean() - want) <= 4 * se, f"mean {ll.mean():.4f}, Kalman {want:.4f}, standard error {se:.4f}"


# ---- 8. nullable outputs -------------------------------------------------------------------------------------------------------------------------
def test_outputs_not_asked_for_are_none_and_change_nothing():
    c = _case("vehicle")
    N = 200
    g = _drawn("vehicle", N)
    bare = c.sim.filter(c.A, KEYS, N, moments=False)
    assert all(getattr(bare, f) is None for f in bare.FIELDS if f not in ("loglik", "ell"))
    assert np.array_equal(_np(bare.ell), g["ell"]) and np.array_equal(_np(bare.loglik), g["loglik"])
    mom = c.sim.filter(c.A, KEYS, N)
    assert all(getattr(mom, f) is None for f in ("x", "anc", "lw", "yhat"))
    for f in ("loglik", "ell", "ess", "pred_sum", "pred_sumsq", "filt_sum", "wtot"):
        assert np.array_equal(_np(getattr(mom, f)), g[f]), f
    tr = c.sim.filter(c.A, KEYS, N, moments=False, traces=True)
    assert tr.ess is None and tr.pred_sum is None and tr.filt_sum is None
    for f in ("loglik", "ell", "x", "anc", "lw", "yhat"):
        assert np.array_equal(_np(getattr(tr, f)), g[f]), f
    s = pgas_amd.evidence_summary(mom, y=c.y)                                       # works on the result unchanged
    assert tuple(s["y_pred_mean"].shape) == (T, 2) and tuple(s["x_filt_mean"].shape) == (K, T, 2) and bool(torch.isfinite(s["rmse"]))
    assert bool(torch.isfinite(s["log_evidence"])) and set(pgas_amd.evidence_summary(bare)) == {"log_evidence"}


# ---- 9. no host round trip -----------------------------------------------------------------------------------------------------------------------
def test_filter_makes_no_host_round_trip():
    c = _case("vehicle")
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    cov = [torch.eye(1, dtype=torch.float64, device=c.dev).repeat(K, 1, 1) * 1e-4 for _ in range(2)]
    calls = [lambda: c.sim.filter(c.A, kd, 130, traces=True), lambda: c.sim.filter(c.A, kd, 3, init_state=x0, row_cov=cov),
             lambda: c.sim.filter(c.A, kd, 300, moments=False)]
    warm = [f() for f in calls]   # uploads of the programs, tables and observations, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [f() for f in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        for f in a.FIELDS:
            u, v = getattr(a, f), getattr(b, f)
            assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), f
        assert bool(torch.isfinite(a.loglik).all())


# ---- 10. the context is left as it was -----------------------------------------------------------------------------------------------------------
def test_filter_leaves_the_rollout_predict_and_algorithm1_on_the_same_context_unchanged():
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
    r = c.sim.filter(c.A, KEYS, 200, traces=True)
    assert bool(torch.isfinite(r.loglik).all())
    again = c.sim(c.A, KEYS, replicates=70, outputs=True)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    st = c.sim.predict(c.A, KEYS, replicates=70)
    for a, b in zip(pred, (st.x_sum, st.x_sumsq, st.y_sum, st.y_sumsq, st.lpd)):
        assert torch.equal(a, b)
    r2 = c.sim.filter(c.A, KEYS, 200, traces=True)
    assert all(torch.equal(getattr(r, f), getattr(r2, f)) for f in r.FIELDS)
    _, after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---- 11. capacity and the refusals of the C ABI ------------------------------------------------------------------------------------------------------
def test_capacity_and_abi_refusals_leave_the_context_usable():
    c = _case("vehicle")
    sim, nmax = c.sim, c.nmax
    assert nmax == 512
    top = sim.filter(c.A, KEYS, nmax)
    assert bool(torch.isfinite(top.loglik).all())
    with pytest.raises(ValueError, match="particles"):
        sim.filter(c.A, KEYS, nmax + 1)
    N = 70
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    good = sim.filter(c.A, kd, N)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=c.dev)   # noqa: E731
    ell, ll, s1, s2, fs, wt = new(K, T), new(K), new(K, T, 4), new(K, T, 4), new(K, T, 2), new(K, T)
    ydev = sim._static()["y"]

    def descs():
        d = sim._desc(K, N, 0, 0, c.A, None, kd, None, True, None, None)
        f = ModelFilterDesc()
        f.y_dev, f.ell_dev, f.loglik_dev, f.cR = ydev.data_ptr(), ell.data_ptr(), ll.data_ptr(), float(c.ssm._cR)
        f.pred_sum_dev, f.pred_sumsq_dev, f.filt_sum_dev, f.wtot_dev = s1.data_ptr(), s2.data_ptr(), fs.data_ptr(), wt.data_ptr()
        for j in range(2):
            for l in range(2):
                f.LRinv[2 * j + l] = float(c.ssm._LRinv[j, l])
        return d, f

    edits = {
        "N = 0": lambda d, f: setattr(d, "P", 0),
        "N = 1025": lambda d, f: setattr(d, "P", 1025),
        "p0 = 64": lambda d, f: setattr(d, "p0", 64),
        "y, ell, loglik": lambda d, f: setattr(f, "y_dev", None),
        "(y, ell, loglik)": lambda d, f: setattr(f, "ell_dev", None),
        "NULL argument (y, ell, loglik)": lambda d, f: setattr(f, "loglik_dev", None),
        "pred_sum and pred_sumsq go together": lambda d, f: setattr(f, "pred_sumsq_dev", None),
        "filt_sum and wtot go together": lambda d, f: setattr(f, "filt_sum_dev", None),
        "seeds are needed": lambda d, f: setattr(d, "seeds_dev", None),
        "K = 65536": lambda d, f: setattr(d, "K", 65536),
        "the largest N that fits is 512": lambda d, f: setattr(d, "P", 576),
        "output program": lambda d, f: setattr(d, "gcode_dev", None),              # what pgas_m_rollout_stats refuses of the descriptor
        "L = 0": lambda d, f: setattr(d, "L", 0),
        "K = 0": lambda d, f: setattr(d, "K", 0),
        "97 registers": lambda d, f: setattr(d, "nreg", 97),
    }
    for what, edit in edits.items():
        d, f = descs()
        edit(d, f)
        with pytest.raises(PgasError, match=r"pgas_m_filter failed \(-1\)") as ei:   # PGAS_E_ARG, with the library's message
            sim.ops.model_filter(d, f)
        assert "pgas_m_filter: " in str(ei.value) and what in str(ei.value), (what, str(ei.value))
    d, f = descs()                                                                  # the untouched descriptors still run on the same context
    sim.ops.model_filter(d, f)
    torch.cuda.synchronize()
    assert torch.equal(ell, good.ell) and torch.equal(ll, good.loglik) and torch.equal(s1, good.pred_sum) and torch.equal(fs, good.filt_sum)
    again = sim.filter(c.A, kd, N)
    assert torch.equal(again.ell, good.ell) and torch.equal(again.ess, good.ess)
