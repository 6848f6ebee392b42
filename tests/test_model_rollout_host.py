"""Host side of pgas_amd.ModelRollout: runs without a GPU.  The NumPy restatement of the recursion equals the
example's host loop bit for bit, every refusal of a call is raised before a device is touched, the traced Vehicle features equal the
slip-angle formulas bit for bit, and mniw_posterior_means is prior_mniw_mean draw by draw."""
import importlib.util
import os

import numpy as np
import pytest

from common import ROOT

import pgas_amd
from pgas_amd import experiments, exprs
import model_rollout_numpy as mrn


def _example():
    spec = importlib.util.spec_from_file_location("EMPS_Simulation", os.path.join(ROOT, "examples", "EMPS_Simulation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _coeffs(pb, K, seed=5):
    """K coefficient sets per latent function: prior mean + 0.1 N(0, 1) sd."""
    rng = np.random.default_rng(seed)
    out = []
    for g in pb.GP_prior:
        e0, e1 = np.asarray(g[0]), np.asarray(g[1])
        M = e1.shape[0]
        mean = pgas_amd.prior_mniw_mean(e0.reshape(M, -1), e1)                   # (n, M)
        sd = np.diag(np.linalg.inv(e1))
        out.append(mean[None] + 0.1 * rng.standard_normal((K,) + mean.shape) * sd)
    return out


def test_numpy_restatement_equals_the_examples_host_loop():
    ex = _example()
    steps = 120
    marg, pg = experiments.emps_marginal(T=8), experiments.emps_pgas(T=8, M=27)
    A = _coeffs(marg, 1)[0][0] * 50.0                                            # (1, 9): a friction curve of visible size
    # the grey-box half of validation_rmse, line for line (it returns the RMSE only), on the inputs it builds
    dt = 0.01
    tau = 45.0 * np.sign(np.sin(2 * np.pi * np.arange(steps) * dt / 1.5))
    f_np, _ = marg.model(np)
    Xa = np.zeros((steps, 2))
    for i in range(1, steps):
        F = (A @ marg.basis[0].batch(Xa[i - 1:i], None)[0])[0]
        Xa[i] = f_np(Xa[i - 1:i], np.array([tau[i - 1]]), np.array([[F]]))[0]
    ox, oy = mrn.rollout(marg.model(np), [mrn.Latent(b) for b in marg.basis], [A[None]], tau.reshape(-1, 1), np.zeros((1, 1, 2)))
    assert np.array_equal(ox[0, :, 0], Xa)
    assert np.array_equal(oy[0, :, 0, 0], Xa[:, 0])                              # f_y = position
    rmse_a, _ = ex.validation_rmse(A, np.zeros((2, 27)), marg, pg, steps=steps)
    truth = np.zeros((steps, 2))
    for i in range(1, steps):
        s, u = truth[i - 1], tau[i - 1]
        d = lambda s: np.array([s[1], (u - 203.5 * s[1] - 20.39 * np.sign(s[1]) + 3.16) / 95.11])  # noqa: E731
        k1 = d(s); k2 = d(s + dt * k1 / 2); k3 = d(s + dt * k2 / 2); k4 = d(s + dt * k3)
        truth[i] = s + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    assert rmse_a == float(np.sqrt(np.mean((ox[0, :, 0, 0] - truth[:, 0]) ** 2)))


def _sim(pb, T=6, widths=None, init=True):
    ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
    return pgas_amd.ModelRollout(pb.inputs[:T], ssm, pb.basis, pb.init_state_mean if init else None, pb.init_state_cov if init else None,
                                 int_var_widths=widths)


def test_every_refusal_is_raised_without_a_device():
    pb = experiments.smo_marginal(T=6)
    sim = _sim(pb)
    K = 3
    A = _coeffs(pb, K)
    x0 = np.zeros(2)
    keys = [1, 2, 3]
    ok = sim.check_call(A, keys, 4)
    assert ok == (3, 4, 0, True, False)
    assert sim.check_call(A, None, 1, x0, process_noise=False) == (3, 1, 1, False, False)
    bad = [
        (dict(coeffs=A[0]), "list of 1"),
        (dict(coeffs=[A[0][:, :, :5]]), r"coeffs\[0\]"),
        (dict(coeffs=[A[0][:0]], keys=[]), "K must be >= 1"),
        (dict(coeffs=A, keys=[1, 2]), "expected 3 keys"),
        (dict(coeffs=A, keys=None, init_state=x0), "needs keys"),
        (dict(coeffs=A, keys=None, init_state=x0, process_noise=False, row_cov=[np.tile(np.eye(1), (K, 1, 1))]), "needs keys"),
        (dict(coeffs=A, keys=None, process_noise=False), "draws x_0"),
        (dict(coeffs=A, keys=keys, row_cov=[np.zeros((K, 2, 2))]), r"row_cov\[0\]"),
        (dict(coeffs=A, keys=keys, replicates=0), "replicates"),
        (dict(coeffs=A, keys=keys, p0=-1), "p0"),
        (dict(coeffs=A, keys=keys, init_state=np.zeros((2, 2))), "init_state"),
        (dict(coeffs=A, keys=None, init_state=x0, process_noise=False, replicates=2), "copies"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            sim(**kw)                                                             # the full call: it must fail before it reaches a device
    with pytest.raises(ValueError, match="construct the ModelRollout with both"):
        _sim(pb, init=False)(A, keys)
    assert sim._ops is None and sim._dev_cache is None                            # nothing was created on the way
    with pytest.raises(ValueError, match=r"coeffs\[0\]: expected \(K, 2, 41\)"):
        _sim(experiments.smo_two_component_marginal(T=6), widths=[2])(A, keys)    # one-component coefficients for a two-component variable


def test_what_the_tracer_cannot_express_is_a_type_error_at_construction():
    pb = experiments.smo_marginal(T=6)
    ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel)
    with pytest.raises(TypeError, match="BasisMap"):
        pgas_amd.ModelRollout(pb.inputs, ssm, [lambda s, u: s])
    with pytest.raises(TypeError, match="SymbolicStateSpaceModel"):
        pgas_amd.ModelRollout(pb.inputs, pb.ssm(pgas_amd.StateSpaceModel, __import__("torch")), pb.basis)

    def model(xp):   # a matrix product of particles is nothing the per-particle tracer can express
        return (lambda s, u, *iv: s @ s.T), (lambda s, u, *iv: s[:, 0:1])

    odd = pgas_amd.SymbolicStateSpaceModel(pb.process_noise, pb.output_noise, model)
    with pytest.raises(TypeError):
        pgas_amd.ModelRollout(pb.inputs, odd, pb.basis)


def test_programs_share_one_register_file_and_their_results_survive_relocation():
    """The relocated programs (one constant pool, shared temporaries) compute what the separately traced ones compute."""
    for make, widths in ((experiments.smo_marginal, None), (experiments.emps_marginal, None), (experiments.toy_marginal, None),
                         (experiments.vehicle_marginal, None), (experiments.smo_two_component_marginal, [2])):
        pb = make(T=6)
        sim = _sim(pb, widths=widths)
        first_tmp = sim.n_in + len(sim._consts)
        assert sim.n_reg <= exprs.MAX_REG and sim.lds_bytes() <= 64 * 1024
        rng = np.random.default_rng(1)
        N = 5
        x = rng.standard_normal((N, sim.nx)) * 0.1
        u = np.asarray(pb.inputs[3], dtype=np.float64).reshape(-1)
        if u.size == 2:
            u = np.array([0.05, 11.0])
        ivs = [rng.standard_normal((N, w)) for w in sim.widths]
        f, g = pb.model(np)
        for code, outs, ref in ((sim._fcode, sim._fout, f(x, u, *ivs)), (sim._gcode, sim._gout, g(x, u, *ivs))):
            assert code[:, 1].min() >= first_tmp and min(outs) >= first_tmp        # nothing writes state, input, interface variables or constants
            whole = exprs.Program(code, sim._consts, sim.n_in, sim.n_reg, outs, (sim.nx, sim.nu, sim.widths))
            assert np.array_equal(exprs.run_numpy(whole, x, u, ivs), np.asarray(ref).reshape(N, -1))


def test_traced_vehicle_features_equal_the_slip_angles_bit_for_bit():
    pb = experiments.vehicle_marginal(T=6)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((64, 2)) * np.array([0.3, 1.0])
    for bf in pb.basis:
        prog = exprs.trace(lambda st, u: bf.feature(exprs.SymNamespace(st.tr))(st, u), 2, 2, ())
        for u in (np.array([0.07, 11.0]), np.array([-0.12, 7.5])):
            got = exprs.run_numpy(prog, x, u, [])
            assert got.shape == (64, 1)
            assert np.array_equal(got[:, 0], bf.alpha(x, u))
            assert np.array_equal(bf.feature(np)(x, u)[:, 0], bf.alpha(x, u))
    sim = _sim(pb)
    assert [h.code is not None for h in sim.latents] == [True, True] and sim.ny == 2 and sim.nu == 2


def test_mniw_posterior_means_is_prior_mniw_mean_draw_by_draw():
    rng = np.random.default_rng(3)
    for pb, n in ((experiments.emps_marginal(T=6), 1), (experiments.smo_two_component_marginal(T=6), 2)):
        g = pb.GP_prior[0]
        M = np.asarray(g[1]).shape[0]
        K = 4
        Phi = rng.standard_normal((K, 30, M))
        Y = rng.standard_normal((K, 30, n))
        T0 = np.einsum("ktm,ktn->kmn", Phi, Y)
        T1 = np.einsum("ktm,ktl->kml", Phi, Phi)
        got = pgas_amd.mniw_posterior_means(g, T0, T1)
        assert got.shape == (K, n, M)
        for k in range(K):
            assert np.array_equal(got[k], pgas_amd.prior_mniw_mean(np.asarray(g[0]).reshape(M, n) + T0[k], np.asarray(g[1]) + T1[k]))
    with pytest.raises(ValueError):
        pgas_amd.mniw_posterior_means(g, T0[:, :3], T1)
