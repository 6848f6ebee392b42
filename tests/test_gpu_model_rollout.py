"""pgas_amd.ModelRollout on the GPU: the one-launch grey-box simulation against the primitives it fuses.

The central check is TEACHER-FORCED and needs no accumulated tolerance: for every t the stored x_{t+1} is compared with ONE step of the
existing primitives (hilbert_basis -> A phi in torch -> expr_eval with the process noise of rng_normal) fed the stored x_t, and y_t with
the output program.  The stored row is the row the kernel carried, so a stale or wrong carried state shows at once.  The bound is
1e-12 max(1, |ref|_max), the one test_traced_model_programs_match_the_torch_callables uses for these programs: the only operation that is
not the same is the order of the A phi sum.  The same step is checked against the NumPy restatement (tests/model_rollout_numpy.py).
"""
import numpy as np
import pytest
import torch

from common import experiments, pgas_amd
import model_rollout_numpy as mrn
from pgas_amd._lib import MarginalOps, PgasError
from pgas_amd.Algorithm1 import STREAM_INIT_STATE, STREAM_STATE
from pgas_amd.model_rollout import STREAM_ROLLOUT_INTVAR

pytestmark = pytest.mark.gpu
K = 3
KEYS = [0x1234567, 0x9E3779B97F4A7C15, 42]
MODELS = {
    "smo": (experiments.smo_marginal, None),                 # 2-D basis, M = 41
    "emps": (experiments.emps_marginal, None),               # basis on x[1], M = 9
    "toy": (experiments.toy_marginal, None),                 # nx = 1, deterministic, the transition IS xi
    "vehicle": (experiments.vehicle_marginal, None),         # L = 2, traced features, nu = 2, ny = 2
    "smo2": (experiments.smo_two_component_marginal, [2]),   # n = 2
}


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
    """One model over T input rows on one MarginalOps: the rollout object and what the one-step references need."""

    def __init__(self, name, T, ops=None):
        make, widths = MODELS[name]
        self.pb = pb = make(T=max(T, 6))
        self.T = T
        self.ops = ops or MarginalOps(1)
        self.dev = self.ops.device
        self.ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
        self.ssm.bind(self.ops)
        self.sim = pgas_amd.ModelRollout(pb.inputs[:T], self.ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, int_var_widths=widths, ops=self.ops)
        self.u = torch.as_tensor(np.asarray(pb.inputs[:T], dtype=np.float64).reshape(T, -1), device=self.dev)
        self.A_np = _coeffs(pb)
        self.A = [torch.as_tensor(a, device=self.dev) for a in self.A_np]
        self.lat_np = [mrn.Latent(b) for b in pb.basis]
        self.model_np = pb.model(np)

    def phi(self, i, x, u):
        """The existing primitive: ops.hilbert_basis on the pick, or on the feature callable's value."""
        b = self.pb.basis[i]
        if hasattr(b, "feature"):
            return self.ops.hilbert_basis(b.map, b.alpha(x, u).reshape(-1, 1).contiguous(), None)
        return self.ops.hilbert_basis(b, x.contiguous(), u)

    def one_step(self, k, t, x, P, noisy, rows=None):
        """(y_t, x_t+1) of draw k from x = x_t (P, nx) by one step of the primitives; rows: Cholesky factors of row_cov (K, n, n) per function."""
        u = self.u[t]
        xi = []
        for i in range(self.sim.L):
            m = self.phi(i, x, u) @ self.A[i][k].T
            if rows is not None:
                m = m + self.ops.eng.rng_normal(KEYS[k], STREAM_ROLLOUT_INTVAR + i, t, P, self.sim.widths[i]) @ rows[i][k].T
            xi.append(m.contiguous())
        y = self.ssm.output_mdl(x, u, *xi).reshape(P, -1)
        if noisy:
            xn = self.ssm.draw_state(self.ops.eng.rng_normal(KEYS[k], STREAM_STATE, t + 1, P, self.sim.nx), x, u, *xi)
        else:
            xn = self.ssm.transition_mdl(x, u, *xi)
        return xi, y, xn


def _close(got, ref, what):
    got, ref = got.detach().cpu().numpy(), (ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref)
    assert np.all(np.isfinite(got)), what
    bound = 1e-12 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= bound, f"{what}: max |diff| = {err:.3e} > {bound:.3e}"


def _check_steps(c, ox, oy, P, noisy, rows=None, numpy_every=1):
    """Every stored row against one step from the row before it; the device references of a draw are compared in one go."""
    T = c.T
    Qc = None if c.ssm.is_deterministic or not noisy else c.ssm._Q_chol
    for k in range(K):
        ys, xs = [], []
        for t in range(T):
            x = ox[k, t].contiguous()
            _, y, xn = c.one_step(k, t, x, P, noisy, rows)
            ys.append(y)
            xs.append(xn)
        _close(oy[k], torch.stack(ys), f"y[{k}]")
        _close(ox[k, 1:], torch.stack(xs[:-1]), f"x[{k}]")
        for t in range(0, T, numpy_every):   # the NumPy restatement's single step from the same stored row and the same normals
            z = c.ops.eng.rng_normal(KEYS[k], STREAM_STATE, t + 1, P, c.sim.nx).cpu().numpy() if Qc is not None else None
            e = Lr = None
            if rows is not None:
                e = [c.ops.eng.rng_normal(KEYS[k], STREAM_ROLLOUT_INTVAR + i, t, P, c.sim.widths[i]).cpu().numpy() for i in range(c.sim.L)]
                Lr = [r[k].cpu().numpy() for r in rows]
            _, yn, xnn = mrn.step(c.model_np, c.lat_np, [a[k] for a in c.A_np], ox[k, t].cpu().numpy(), c.u[t].cpu().numpy(), z, Qc, e, Lr)
            _close(oy[k, t], yn, f"numpy y[{k},{t}]")
            if t < T - 1:
                _close(ox[k, t + 1], xnn, f"numpy x[{k},{t + 1}]")


CASES = [(n, 12, P) for n in MODELS for P in (1, 63, 64, 65, 257)] + [(n, 300, 65) for n in MODELS]


# ---- 1. teacher-forced step identity, noisy, x_0 drawn -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T,P", CASES, ids=[f"{n}-T{T}-P{P}" for n, T, P in CASES])
def test_every_stored_step_is_one_step_of_the_primitives(name, T, P):
    c = Case(name, T)
    ox, oy = c.sim(c.A, KEYS, replicates=P, outputs=True)
    assert ox.shape == (K, T, P, c.sim.nx) and oy.shape == (K, T, P, c.sim.ny)
    L0 = torch.as_tensor(np.linalg.cholesky(c.pb.init_state_cov), device=c.dev)
    m0 = torch.as_tensor(np.asarray(c.pb.init_state_mean, dtype=np.float64), device=c.dev)
    for k in range(K):   # row 0 as Algorithm1._init_algorithm draws it
        _close(ox[k, 0], m0 + c.ops.eng.rng_normal(KEYS[k], STREAM_INIT_STATE, 0, P, c.sim.nx) @ L0.T, f"x0[{k}]")
    _check_steps(c, ox, oy, P, noisy=True, numpy_every=1 if T <= 12 else 25)
    if not c.ssm.is_deterministic:
        assert not torch.equal(ox[0, 1:], ox[1, 1:]) and (P == 1 or not torch.equal(ox[0, 1, 0], ox[0, 1, 1]))


# ---- 2. noise-free rollout with x_0 given ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_noise_free_rollout_from_a_given_state(name):
    T, P = 12, 5
    c = Case(name, T)
    rng = np.random.default_rng(9)
    x0 = np.asarray(c.pb.init_state_mean) + 0.05 * rng.standard_normal((K, P, c.sim.nx))
    ox, oy = c.sim(c.A, None, replicates=P, init_state=x0, process_noise=False, outputs=True)
    assert np.array_equal(ox[:, 0].cpu().numpy(), x0)
    _check_steps(c, ox, oy, P, noisy=False)
    for mode_x0 in (x0[0, 0], x0[:, 0]):   # (nx) and (K, nx): the first replicate of the per-replicate run
        o1 = c.sim(c.A, None, init_state=mode_x0, process_noise=False)
        ref = ox[0:1, :, 0:1] if mode_x0.ndim == 1 else ox[:, :, 0:1]
        assert torch.equal(o1[0:1] if mode_x0.ndim == 1 else o1, ref)
    if c.ssm.is_deterministic:   # Toy: no process noise to add, with or without the flag
        a = c.sim(c.A, KEYS, replicates=P, init_state=x0, process_noise=True)
        assert torch.equal(a, ox)


# ---- 3. bit-exact invariances ------------------------------------------------------------------------------------------------------------
def test_replicates_split_over_calls_reversed_and_equal_draws():
    c = Case("smo", 12)
    sim, A = c.sim, c.A
    whole, wy = sim(A, KEYS, replicates=200, outputs=True)
    parts = [sim(A, KEYS, replicates=n, p0=p0) for p0, n in ((0, 64), (64, 64), (128, 72))]
    assert torch.equal(torch.cat(parts, dim=2), whole)
    assert torch.equal(sim(A, KEYS, replicates=200), whole)                        # outputs=True does not change out_x
    rev = sim([a.flip(0).contiguous() for a in A], KEYS[::-1], replicates=200)
    assert torch.equal(rev.flip(0), whole)
    same = sim([a[[0, 0, 1]].contiguous() for a in A], [KEYS[0], KEYS[0], KEYS[1]], replicates=70)
    assert torch.equal(same[0], same[1]) and torch.equal(same[0], whole[0, :, :70]) and torch.equal(same[2], whole[1, :, :70])
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)                                  # keys as a device tensor
    assert torch.equal(sim(A, kd, replicates=200), whole)


def test_more_draws_than_the_device_holds_at_once():
    c = Case("vehicle", 12)
    Kbig, P = 2000, 64
    A = [torch.as_tensor(a, device=c.dev) for a in _coeffs(c.pb, Kbig, seed=11)]
    keys = [1000 + 7 * k for k in range(Kbig)]
    ox, oy = c.sim(A, keys, replicates=P, outputs=True)
    for k in (0, Kbig - 1):
        ax, ay = c.sim([a[k:k + 1].contiguous() for a in A], keys[k:k + 1], replicates=P, outputs=True)
        assert torch.equal(ax[0], ox[k]) and torch.equal(ay[0], oy[k])
    assert bool(torch.isfinite(ox).all()) and bool(torch.isfinite(oy).all())


@pytest.mark.parametrize("name", ["smo2", "vehicle"])
def test_interface_variable_noise_is_rng_normal_on_its_own_stream(name):
    T, P = 12, 65
    c = Case(name, T)
    rng = np.random.default_rng(4)
    covs = []
    for w in c.sim.widths:
        B = rng.standard_normal((K, w, w))
        covs.append(1e-2 * (B @ B.transpose(0, 2, 1) + np.eye(w)))
    rows = [torch.as_tensor(np.linalg.cholesky(cv), device=c.dev) for cv in covs]
    ox, oy = c.sim(c.A, KEYS, replicates=P, row_cov=covs, outputs=True)
    _check_steps(c, ox, oy, P, noisy=True, rows=rows)
    plain = c.sim(c.A, KEYS, replicates=P)
    assert torch.equal(plain[:, 0], ox[:, 0]) and not torch.equal(plain[:, 1], ox[:, 1])
    dev_cov = c.sim(c.A, KEYS, replicates=P, row_cov=[torch.as_tensor(cv, device=c.dev) for cv in covs])   # factored on the device
    _close(dev_cov, ox, "row_cov factored on the device")


# ---- 4. no host synchronisation ----------------------------------------------------------------------------------------------------------
def test_calls_make_no_host_round_trip():
    c = Case("vehicle", 12)
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    cov = [torch.eye(1, dtype=torch.float64, device=c.dev).repeat(K, 1, 1) * 1e-4 for _ in range(2)]
    calls = [lambda: c.sim(c.A, kd, replicates=130, outputs=True)[1], lambda: c.sim(c.A, kd, replicates=3, init_state=x0, row_cov=cov),
             lambda: c.sim(c.A, None, init_state=x0, process_noise=False)]
    warm = [f() for f in calls]   # uploads of the programs and tables, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [f() for f in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---- 5. no side effects on the context ---------------------------------------------------------------------------------------------------
def test_a_rollout_leaves_the_filter_on_the_same_context_unchanged():
    pb = experiments.emps_marginal(T=10)

    def run():
        alg = pgas_amd.Algorithm1(64, pb.observations, pb.inputs, pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel), pb.forgetting_factor,
                                  pb.init_state_mean, pb.init_state_cov, pb.init_int_var_mean, pb.init_int_var_cov, pb.GP_prior, pb.basis_fcn())
        out = alg(12345678)
        return alg, [out[0], out[1][0], out[3], out[4]]

    alg, before = run()
    c = Case("emps", 10, ops=alg.ops)
    assert c.sim.ops is alg.ops
    ox = c.sim(c.A, KEYS, replicates=64)
    assert bool(torch.isfinite(ox).all())
    _, after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---- 6. refusals of the C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable():
    c = Case("vehicle", 12)
    sim, P = c.sim, 8
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    good = sim(c.A, kd, replicates=P, outputs=True)
    out_x, out_y = torch.empty_like(good[0]), torch.empty_like(good[1])

    def desc():
        return sim._desc(K, P, 0, 0, c.A, None, kd, None, True, out_x, out_y)

    bad_code = sim._fcode.copy()
    bad_code[0, 2] = 200                                                           # a source register past the file
    wild_dst = sim._gcode.copy()
    wild_dst[0, 1] = 0                                                             # a program that would overwrite the state
    edits = {
        "K = 0": lambda d: setattr(d, "K", 0),
        "P = 0": lambda d: setattr(d, "P", 0),
        "L = 0": lambda d: setattr(d, "L", 0),
        "L = 5": lambda d: setattr(d, "L", 5),
        "97 registers": lambda d: setattr(d, "nreg", 97),
        "result register out of range": lambda d: d.f_out.__setitem__(0, 96),
        "source register out of range": lambda d: setattr(d, "fcode_host", bad_code.ctypes.data),
        "destination below the temporaries": lambda d: setattr(d, "gcode_host", wild_dst.ctypes.data),
        "widths != n_in": lambda d: setattr(d, "n_in", d.n_in + 1),
        "n_i changes the sum": lambda d: setattr(d.lat[1], "n", 2),
        "D = 5": lambda d: setattr(d.lat[0], "D", 5),
        "process noise without seeds": lambda d: setattr(d, "seeds_dev", None),
        "LDS need": lambda d: setattr(d.lat[0], "M", 1 << 20),
    }
    for what, edit in edits.items():
        d = desc()
        edit(d)
        with pytest.raises(PgasError, match=r"pgas_m_rollout failed \(-1\)"):      # PGAS_E_ARG, with the library's message
            sim.ops.model_rollout(d)
        assert len(sim.ops.lib.pgas_last_error(sim.ops.eng._h)) > 20, what
    d = desc()                                                                     # iv noise without seeds
    rows = [torch.eye(1, dtype=torch.float64, device=c.dev).repeat(K, 1, 1) for _ in range(2)]
    d2 = sim._desc(K, P, 0, 1, c.A, rows, None, torch.zeros(2, dtype=torch.float64, device=c.dev), False, out_x, out_y)
    with pytest.raises(PgasError, match="needs seeds"):
        sim.ops.model_rollout(d2)
    sim.ops.model_rollout(d)                                                       # the untouched descriptor still runs on the same context
    torch.cuda.synchronize()
    assert torch.equal(out_x, good[0]) and torch.equal(out_y, good[1])
