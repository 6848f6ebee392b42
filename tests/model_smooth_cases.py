"""What tests/test_model_smooth_host.py and tests/test_gpu_model_smooth.py share: the five grey-box models of tests/model_filter_cases.py
and its linear-Gaussian model, with a process noise under which backward simulation is NOT the filter's genealogy, and a plain NumPy
filter that yields the traces the smoother's restatement (tests/model_smooth_numpy.py) works on.  No GPU, no device context.

A kernel that only followed `anc` must not pass, so the backward draw has to leave the filter's genealogy often.  Q_SCALE multiplies the
model's shipped process noise for these tests (the toy model ships deterministic, Q = 0: its entry is the variance itself); SHARE
records, for that scale, the share of (trajectory, row) pairs with j_t != anc[t, j_{t+1}] that `leaving_share` below measures with a
plain NumPy filter (draw 0, N = 200, seed 200) and the restatement's 64 trajectories (key 77) on it.  tests/test_model_smooth_host.py
recomputes every share, holds it against the record and asserts it is >= 0.3.  Measured on the way (same filter, same trajectories):
    smo      1 -> 0.399, 1e2 -> 0.396, 1e4 -> 0.653, 1e6 -> 0.959      (shipped diag Q = 5e-8, 5e-9)
    emps     1 -> 0.879, 1e2 -> 0.980, 1e4 -> 0.933, 1e6 -> 0.534      (1e-6, 1e-7; at 1e6 the filter keeps 3 distinct ancestors)
    toy      1e-4 -> 0.960, 1e-2 -> 0.717, 0.25 -> 0.703, 1 -> 0.916   (variance)
    vehicle  1e-4 -> 0.574, 1e-2 -> 0.538, 0.1 -> 0.429, 1 -> 0.318, 1e2 -> 0.179, 1e4 -> 0.286 (1e-8, 1e-8; the output noise is tight: 11 distinct
             ancestors of 200 at scale 1, a single one from 1e2 on, so a LARGER Q makes the filter, not the smoother, degenerate)
    smo2     1 -> 0.213, 1e2 -> 0.668, 1e4 -> 0.963, 1e6 -> 0.939
The linear-Gaussian model needs no scaling: a = 0.9, q = 0.25 gives 0.979.  The linear models of LINEAR (nx = 3, 4 and 5, the state
dimensions the five models do not have) give 0.925, 0.837 and 0.798 under their own full covariance."""
import numpy as np

import model_filter_cases as cases
import model_filter_numpy as mf
import model_rollout_numpy as mrn
import model_smooth_numpy as msn
from common import pgas_amd

K, T, KEYS = cases.K, cases.T, cases.KEYS
MODELS = cases.MODELS
NS = cases.NS
BS = [1, 3, 4, 5, 64, 255, 256]
KAL = cases.KAL
Q_SCALE = {"smo": 1e4, "emps": 1.0, "toy": 0.25, "vehicle": 1e-2, "smo2": 1e4}
SHARE = {"smo": 0.653, "emps": 0.879, "toy": 0.703, "vehicle": 0.538, "smo2": 0.963, "kal": 0.979, "lin3": 0.925, "lin4": 0.837, "lin5": 0.798}   # to three decimals


LINEAR = {"lin3": 3, "lin4": 4, "lin5": 5}   # state dimensions beyond the five models' 1 and 2: nx = 3, 4 (constants in the kernel) and nx = 5 (read at run time)


def linear_problem(nx, seed=9):
    """A linear model of nx states in the style of the linear-Gaussian one: x'_i = 0.8 x_i + 0.15 x_{i+1 mod nx}, x'_0 += 0.1 u + xi, y =
    (x_0, x_{nx-1}), one latent function of x_0 on the toy model's basis, a FULL process-noise covariance (so every entry of the lower
    triangle of LQinv is used), its record simulated from itself with xi = 0."""
    import types

    def model(xp):
        def f_x(state, input, *int_var):
            u, xi = input.reshape(-1)[0], int_var[0].reshape(-1)
            cols = [0.8 * state[:, i] + 0.15 * state[:, (i + 1) % nx] for i in range(nx)]
            cols[0] = cols[0] + 0.1 * u + xi
            return xp.stack(cols, 1)

        def f_y(state, input, *int_var):
            return xp.stack([state[:, 0], state[:, nx - 1]], 1)

        return f_x, f_y

    rng = np.random.default_rng(seed + nx)
    Bm = rng.standard_normal((nx, nx))
    Q = 0.05 * (Bm @ Bm.T / nx + np.eye(nx))
    R = 0.2 * np.eye(2)
    u = np.sin(0.3 * np.arange(T))
    x, y = rng.standard_normal(nx), np.empty((T, 2))
    Amat = 0.8 * np.eye(nx) + 0.15 * np.roll(np.eye(nx), 1, axis=1)
    for t in range(T):
        y[t] = x[[0, nx - 1]] + np.sqrt(0.2) * rng.standard_normal(2)
        x = Amat @ x + np.linalg.cholesky(Q) @ rng.standard_normal(nx)
        x[0] += 0.1 * u[t]
    basis = MODELS["toy"][0](T=T).basis[:1]
    return types.SimpleNamespace(model=model, inputs=u, observations=y, basis=basis, process_noise=Q, output_noise=R, init_state_mean=np.zeros(nx),
                                 init_state_cov=np.eye(nx))


def problem(name):
    """cases.problem, and the linear models of LINEAR (their own output noise, no widths)."""
    if name in LINEAR:
        pb = linear_problem(LINEAR[name])
        return pb, None, pb.output_noise
    return cases.problem(name)


def coeffs(name, pb):
    """cases.coeffs; for a linear model K coefficient sets 0.3 N(0, 1) (its latent function has no prior here)."""
    if name in LINEAR:
        b = getattr(pb.basis[0], "b", pb.basis[0])
        return [0.3 * np.random.default_rng(5).standard_normal((K, 1, int(b.basis.M)))]
    return cases.coeffs(pb)


def process_noise(name):
    """Q_SCALE times the model's process noise; the toy model's is 0 (it ships deterministic), so its entry is the variance itself."""
    if name in LINEAR:
        return linear_problem(LINEAR[name]).process_noise
    pb, _, _ = cases.problem(name)
    Q = np.atleast_2d(np.asarray(pb.process_noise, dtype=np.float64))
    return Q_SCALE[name] * (Q if np.any(Q) else np.eye(Q.shape[0]))


def rollout(name, ops=None, observations=None, Tn=T):
    """(pb, ssm, ModelRollout) of a model over its first Tn rows under the filter tests' output noise and the scaled process noise; touches no
    device."""
    pb, widths, R = problem(name)
    ssm = pgas_amd.SymbolicStateSpaceModel(process_noise(name), R, pb.model)
    y = np.asarray(pb.observations[:Tn] if observations is None else observations, dtype=np.float64).reshape(Tn, -1)
    sim = pgas_amd.ModelRollout(pb.inputs[:Tn], ssm, pb.basis, pb.init_state_mean, pb.init_state_cov, int_var_widths=widths, ops=ops, observations=y)
    return pb, ssm, sim


def kalman_rollout(basis, ops=None, T=None, observations=None):
    """(ssm, ModelRollout, y) of the linear-Gaussian model x' = a x + xi, y = x (A = 0: xi = 0) on its simulated record, cut to T rows."""
    y = cases.kalman_record() if observations is None else np.asarray(observations, dtype=np.float64)
    y = y[:T] if T is not None else y
    ssm = pgas_amd.SymbolicStateSpaceModel(np.array([[KAL["q"]]]), np.array([[KAL["r"]]]), cases.kalman_model)
    sim = pgas_amd.ModelRollout(np.zeros((len(y), 0)), ssm, basis, np.array([KAL["m0"]]), np.array([[KAL["p0"]]]), ops=ops, observations=y)
    return ssm, sim, y


def _traces(model, lat, A, u, y, R, Q, x0, rng):
    """A plain NumPy bootstrap filter (mf.bootstrap, resampling at every step) and, from its stored rows, xi_t^i and f(x_t^i, u_t, xi_t^i)
    of every particle -> dict of x, anc, lw, yhat, fmean, xi, y, Q."""
    Tn, (N, nx) = len(y), x0.shape
    Qc = np.linalg.cholesky(Q)
    res = mf.bootstrap(lambda t, x: mrn.step(model, lat, A, x, u[t], rng.standard_normal((N, nx)), Qc)[2], lambda t, x: mrn.step(model, lat, A, x, u[t])[1],
                       x0, y, R, rng.random(Tn))
    xi, fm = [], []
    for t in range(Tn):
        v, _, xn = mrn.step(model, lat, A, res["x"][t], u[t])
        xi.append(np.concatenate([np.reshape(a, (N, -1)) for a in v], axis=1))
        fm.append(np.reshape(xn, (N, nx)))
    return dict(x=res["x"], anc=res["anc"].astype(np.int32), lw=res["lw"], yhat=res["yhat"], fmean=np.array(fm), xi=np.array(xi), y=y, Q=Q)


def numpy_trace(name, k, N, seed, Tn=T):
    """Draw k of the test coefficients of model `name`, N particles, NumPy's own random numbers, the first Tn rows of the record."""
    pb, _, R = problem(name)
    lat, model = [mrn.Latent(b) for b in pb.basis], pb.model(np)
    A = [a[k] for a in coeffs(name, pb)]
    rng = np.random.default_rng(seed)
    u = np.asarray(pb.inputs[:Tn], dtype=np.float64).reshape(Tn, -1)
    y = np.asarray(pb.observations[:Tn], dtype=np.float64).reshape(Tn, -1)
    nx = len(pb.init_state_mean)
    x0 = np.asarray(pb.init_state_mean) + rng.standard_normal((N, nx)) @ np.linalg.cholesky(pb.init_state_cov).T
    return _traces(model, lat, A, u, y, R, process_noise(name), x0, rng)


def kalman_trace(N, seed, Tn=None):
    """The linear-Gaussian model with NumPy's own random numbers (xi = 0: the latent function's coefficients are 0)."""
    y = cases.kalman_record()
    y = (y[:Tn] if Tn is not None else y).reshape(-1, 1)
    rng = np.random.default_rng(seed)
    x0 = KAL["m0"] + np.sqrt(KAL["p0"]) * rng.standard_normal((N, 1))
    model = (lambda x, u, xi: KAL["a"] * x + xi.reshape(-1, 1), lambda x, u, xi: x[:, 0:1])

    class Zero:
        def phi(self, x, u):
            return np.zeros((x.shape[0], 1))

    return _traces(model, [Zero()], [np.zeros((1, 1))], np.zeros((len(y), 0)), y, np.array([[KAL["r"]]]), np.array([[KAL["q"]]]), x0, rng)


def smooth_trace(tr, key, n_traj, b0=None):
    """The restatement on a dict of traces: n_traj trajectories in chunks (b0 None), or one call of n_traj at b0."""
    LQinv, cQ = msn.transition_constants(tr["Q"])
    args = (key, tr["x"], tr["anc"], tr["lw"], tr["yhat"], tr["fmean"], tr["xi"], tr["y"], LQinv, cQ, n_traj)
    return msn.run_chunks(*args) if b0 is None else msn.run(*args, b0)


def leaving_share(tr, res):
    """The share of (trajectory, row < T - 1) pairs whose index is not the filter's ancestor of the next one."""
    idx, anc = res["idx"], tr["anc"]
    Tn = idx.shape[1]
    return float(np.mean([idx[:, t] != anc[t][idx[:, t + 1]] for t in range(Tn - 1)]))
