"""Host side of the grey-box held-out smoother (pgas_amd.ModelRollout.smooth, pgas_m_smooth), no GPU: the NumPy
restatement (tests/model_smooth_numpy.py) on the traces of a plain NumPy filter against a plain float64 FFBSi on the same uniforms and
against the exact forward-filter / backward-smoother marginals; its transition log-density against transition_logpdf's expression; the
property the GPU tests lean on, that the backward draw leaves the filter's genealogy; the LDS inequality; every refusal of ``smooth``
before a device is touched; the C ABI binding; the stream id."""
import ctypes as C
import functools
import glob
import os
import re

import numpy as np
import pytest
import torch

import model_filter_cases as cases
import model_smooth_cases as sc
import model_smooth_numpy as msn
from common import ROOT, pgas_amd
from pgas_amd import model_rollout as mr
from test_model_rollout_stats_host import _c_struct_layout
from test_smooth_host import check_marginals

T, B = sc.T, 64
NAMES = list(sc.MODELS) + ["kal"] + list(sc.LINEAR)


@functools.lru_cache(maxsize=None)
def _trace(name, N, Tn=None, seed=None):
    seed = N if seed is None else seed
    return sc.kalman_trace(N, seed, Tn) if name == "kal" else sc.numpy_trace(name, 0, N, seed, T if Tn is None else Tn)


@functools.lru_cache(maxsize=None)
def _smoothed(name, N, n_traj=B, Tn=None, seed=None, key=77):
    tr = _trace(name, N, Tn, seed)
    return tr, sc.smooth_trace(tr, key, n_traj)


# ---- 1. the GPU tests do not pass on a kernel that follows the filter's genealogy -------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_backward_draws_leave_the_filter_genealogy(name):
    tr, res = _smoothed(name, 200, seed=200)
    share = sc.leaving_share(tr, res)
    print(f"{name}: Q scale {sc.Q_SCALE.get(name, 1.0)}, share of j_t != anc[t, j_t+1] = {share:.3f} (recorded {sc.SHARE[name]})")
    assert share >= 0.3
    assert abs(share - sc.SHARE[name]) <= 0.02                                 # the record in tests/model_smooth_cases.py is this measurement
    assert len({tuple(r) for r in res["idx"]}) > B // 2                        # and the trajectories differ from each other


# ---- 2. the restatement is a backward simulation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 65, 200])
@pytest.mark.parametrize("name", ["smo", "toy", "vehicle", "kal", "lin3", "lin4", "lin5"])
def test_restatement_agrees_with_a_float_ffbsi_on_the_same_trace_and_uniforms(name, N):
    tr, res = _smoothed(name, N)
    Tn = tr["x"].shape[0]
    assert res["idx"].shape == (B, Tn) and (res["idx"] >= 0).all() and (res["idx"] < N).all()
    assert ((res["S"] > 0) & np.isfinite(res["S"])).all()                      # no fall-back row in these cases
    rows = np.arange(Tn)
    assert np.array_equal(res["xs"], tr["x"][rows[None, :], res["idx"]]) and np.array_equal(res["xis"], tr["xi"][rows[None, :], res["idx"]])
    want = msn.float_indices(tr["lw"], tr["fmean"], tr["y"], tr["Q"], res)
    differ = int(np.count_nonzero(want != res["idx"]))
    print(f"{name}, N = {N}: {differ} of {want.size} indices differ from the float FFBSi")
    assert differ <= 0.005 * want.size
    assert np.abs(want - res["idx"]).max() <= 1                               # ... and then by one position: u S at a CDF boundary
    ch = np.concatenate([res["xs"], tr["yhat"][rows[None, :], res["idx"]]], axis=-1)
    assert np.allclose(res["sum"], ch.sum(axis=0), rtol=1e-12, atol=1e-300) and np.allclose(res["sumsq"], (ch * ch).sum(axis=0), rtol=1e-12, atol=1e-300)
    assert np.allclose(res["xi_sum"], res["xis"].sum(axis=0), rtol=1e-12, atol=1e-300)
    assert np.allclose(res["xi_sumsq"], (res["xis"] ** 2).sum(axis=0), rtol=1e-12, atol=1e-300)


def test_chunks_add_up_and_a_trajectory_does_not_depend_on_its_call():
    tr = _trace("smo", 65)
    whole = sc.smooth_trace(tr, 5, 300)
    first, second = sc.smooth_trace(tr, 5, 256, b0=0), sc.smooth_trace(tr, 5, 44, b0=256)
    assert np.array_equal(whole["idx"], np.concatenate([first["idx"], second["idx"]]))
    assert np.array_equal(whole["sum"], first["sum"] + second["sum"]) and np.array_equal(whole["xi_sumsq"], first["xi_sumsq"] + second["xi_sumsq"])
    one = sc.smooth_trace(tr, 5, 1, b0=270)
    assert np.array_equal(one["idx"][0], whole["idx"][270]) and np.array_equal(one["xis"][0], whole["xis"][270])


@pytest.mark.parametrize("name", ["kal", "toy"])
def test_marginal_of_the_drawn_indices_is_the_exact_smoother_marginal(name):
    N, Tn, n = 8, 6, 4096
    tr, res = _smoothed(name, N, n_traj=n, Tn=Tn, seed=11)
    w = msn.smoother_marginals(tr["x"], tr["lw"], tr["fmean"], tr["y"], tr["Q"])
    assert np.allclose(w.sum(axis=1), 1.0, atol=1e-12)
    assert res["idx"].shape == (n, Tn)
    check_marginals(res["idx"], w, n)


def test_restatement_fallback_rows():
    """A NaN observation row has uniform filter weights (the transition density alone decides); a row whose log-weights are all -inf has
    no weight at all and follows the filter's genealogy, g mod N on the last row."""
    tr = dict(_trace("toy", 65))
    Tn = tr["x"].shape[0]
    y, lw = tr["y"].copy(), tr["lw"].copy()
    y[5] = np.nan
    lw[5], lw[9], lw[Tn - 1] = np.nan, -np.inf, -np.inf
    tr["y"], tr["lw"] = y, lw
    res = sc.smooth_trace(tr, 3, 16, b0=60)
    assert (res["S"][:, [9, Tn - 1]] == 0.0).all() and (np.delete(res["S"], [9, Tn - 1], axis=1) > 0).all()
    assert np.array_equal(res["idx"][:, Tn - 1], (60 + np.arange(16)) % 65)
    assert np.array_equal(res["idx"][:, 9], tr["anc"][9][res["idx"][:, 10]])
    assert len(np.unique(res["idx"][:, 5])) > 1


# ---- 3. the transition log-density ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smo", "vehicle", "toy", "lin3", "lin4", "lin5"])
def test_transition_logdensity_is_the_expression_of_transition_logpdf(name):
    tr = _trace(name, 65)
    LQinv, cQ = msn.transition_constants(tr["Q"])
    xn = tr["x"][4][:7]
    h = msn.transition_logdensity(xn, tr["fmean"][3], LQinv, cQ)
    want = msn.float_transition(xn, tr["fmean"][3], tr["Q"])
    assert h.shape == (7, 65) and np.isfinite(want).all()
    assert np.all(np.abs(h - want) <= 1e-12 * np.abs(want))
    # ... and of the package's own expression: cQ - 0.5 |LQinv (target - mean)|^2 with the constants of StateSpaceModel.transition_logpdf
    Lq = np.linalg.cholesky(tr["Q"])
    e = (xn[:, None, :] - tr["fmean"][3][None]) @ np.linalg.inv(Lq).T
    ref = (-0.5 * Lq.shape[0] * np.log(2 * np.pi) - np.sum(np.log(np.diag(Lq)))) - 0.5 * (e * e).sum(axis=-1)
    assert np.all(np.abs(h - ref) <= 1e-12 * np.abs(ref))


# ---- 4. LDS: what the filter holds the smoother holds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.MODELS) + list(sc.LINEAR))
def test_the_smoother_fits_wherever_the_filter_fits(name):
    _, _, sim = sc.rollout(name)
    assert mr.SMOOTH_STATIC_LDS == 1024 * 8 + 256 * 8 * 8 + 256 * 4 + 4 * 2 * 32 * 8 == 27648 < mr.FILTER_STATIC_LDS == 42416
    nmax = sim.max_particles()
    for N in (1, 64, 65, 200, nmax):                                           # the dynamic part is the filter's own formula
        assert sim.filter_lds_bytes(N) + mr.SMOOTH_STATIC_LDS < sim.filter_lds_bytes(N) + mr.FILTER_STATIC_LDS <= mr.LDS_PER_WORKGROUP
    assert sim._ops is None


# ---- 5. every refusal of smooth is a ValueError before a device is touched ---------------------------------------------------------------
def test_every_smooth_refusal_is_raised_without_a_device():
    pb, ssm, sim = sc.rollout("smo")
    A = cases.coeffs(pb)
    keys, N = [1, 2, 3], 70
    assert sim.check_smooth(A, keys, N, 8) == (3, N, 0, True, False, 8)
    assert sim.check_smooth(A, keys, sim.max_particles(), np.int64(65536), np.zeros(2)) == (3, sim.max_particles(), 1, True, False, 65536)
    assert sim.check_smooth(A, torch.zeros(3, dtype=torch.int64), N, 1, np.zeros((3, N, 2)), [np.stack([np.eye(1)] * 3)]) == (3, N, 3, True, True, 1)
    bad = [
        (dict(particles=0), "particles"),
        (dict(particles=sim.max_particles() + 1), "particles"),
        (dict(particles=1025), "particles"),
        (dict(keys=None), "keys"),
        (dict(keys=[1, 2]), "expected 3 keys"),
        (dict(keys=torch.zeros(3, dtype=torch.int32)), "keys"),
        (dict(coeffs=A[0]), "list of 1"),
        (dict(coeffs=[A[0][:, :, :-1]]), r"coeffs\[0\]"),
        (dict(init_state=np.zeros((3, N + 1, 2))), "init_state"),
        (dict(init_state=np.zeros(3)), "init_state"),
        (dict(row_cov=[np.zeros((3, 2, 2))]), r"row_cov\[0\]"),
        (dict(n_trajectories=0), "n_trajectories"),
        (dict(n_trajectories=-4), "n_trajectories"),
        (dict(n_trajectories=65537), "n_trajectories"),
        (dict(n_trajectories=2.0), "n_trajectories"),
        (dict(n_trajectories=True), "n_trajectories"),
        (dict(n_trajectories=None), "n_trajectories"),
        (dict(n_trajectories="8"), "n_trajectories"),
    ]
    for kw, msg in bad:
        args = dict(coeffs=A, keys=keys, particles=N, n_trajectories=8)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            sim.smooth(**args)
    det = pgas_amd.ModelRollout(pb.inputs[:T], pgas_amd.SymbolicStateSpaceModel(np.zeros((2, 2)), ssm.output_noise, pb.model), pb.basis, pb.init_state_mean,
                                pb.init_state_cov, observations=pb.observations[:T])
    with pytest.raises(ValueError, match="backward simulation needs process noise"):
        det.smooth(A, keys, N, 8)
    with pytest.raises(ValueError, match="backward simulation needs process noise"):
        det.check_smooth(A, keys, N, 8, init_state=np.zeros((3, N, 2)))
    bare = pgas_amd.ModelRollout(pb.inputs[:T], ssm, pb.basis, pb.init_state_mean, pb.init_state_cov)
    with pytest.raises(ValueError, match="needs observations"):
        bare.smooth(A, keys, N, 8)
    noinit = pgas_amd.ModelRollout(pb.inputs[:T], ssm, pb.basis, observations=pb.observations[:T])
    with pytest.raises(ValueError, match="construct the ModelRollout with both"):
        noinit.smooth(A, keys, N, 8)
    # more than 16 interface components: refused with interface outputs, accepted without
    wide = _wide_model()
    Aw = [np.zeros((3, w, h.M)) for w, h in zip(wide.widths, wide.latents)]
    assert sum(wide.widths) == 17
    with pytest.raises(ValueError, match="17 interface components"):
        wide.smooth(Aw, keys, N, 8)
    assert wide.check_smooth(Aw, keys, N, 8, interface=False) == (3, N, 0, True, False, 8)
    for s in (sim, det, bare, noinit, wide):
        assert s._ops is None and s._dev_cache is None, "a refused call created the device context"


def _wide_model():
    """The linear-Gaussian model with three interface variables of 8, 8 and 1 components (their first components enter the state)."""
    def model(xp):
        def f_x(state, input, *iv):
            return sc.KAL["a"] * state + iv[0][:, 0:1] + iv[1][:, 0:1] + iv[2].reshape(-1, 1)

        return f_x, lambda state, input, *iv: state[:, 0:1]

    basis = sc.MODELS["toy"][0](T=T).basis[0]
    ssm = pgas_amd.SymbolicStateSpaceModel(np.array([[0.25]]), np.array([[0.5]]), model)
    return pgas_amd.ModelRollout(np.zeros((T, 0)), ssm, [basis] * 3, np.zeros(1), np.eye(1), int_var_widths=[8, 8, 1], observations=np.zeros(T))


def test_interface_summary_by_hand():
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    flt = pgas_amd.ModelFilterResult(4, 1, loglik=torch.zeros(2, dtype=torch.float64), ell=torch.zeros((2, 2), dtype=torch.float64))
    # K = 2 draws, 2 trajectories, T = 2, one interface component: {1, 3}, {5, 7} at t = 0 and {0, 0}, {2, 2} at t = 1
    res = pgas_amd.ModelSmoothResult(flt, 2, t([[[4.0, 4.0], [0.0, 0.0]], [[12.0, 12.0], [4.0, 4.0]]]), t([[[10.0, 10.0], [0.0, 0.0]], [[74.0, 74.0], [8.0, 8.0]]]),
                                     xi_sum=t([[[4.0], [0.0]], [[12.0], [4.0]]]), xi_sumsq=t([[[10.0], [0.0]], [[74.0], [8.0]]]))
    assert isinstance(res, pgas_amd.SmoothResult) and res.xis is None and res.xs is None and res.idx is None and res.n == 4 and res.nx == 1
    out = pgas_amd.interface_summary(res)
    assert np.array_equal(out["xi_smooth_mean"].numpy(), [[4.0], [1.0]]) and np.allclose(out["xi_smooth_std"].numpy(), [[np.sqrt(5.0)], [1.0]], rtol=1e-15)
    assert np.array_equal(out["xi_smooth_mean_draw"].numpy(), [[[2.0], [0.0]], [[6.0], [2.0]]])
    assert np.array_equal(out["xi_smooth_std_draw"].numpy(), [[[1.0], [0.0]], [[1.0], [0.0]]])
    s = pgas_amd.smoothing_summary(res, y=np.array([5.0, np.nan]))              # works on the result unchanged
    assert np.array_equal(s["x_smooth_mean"].numpy(), [[4.0], [1.0]]) and float(s["rmse"]) == 1.0
    with pytest.raises(ValueError, match="interface=True"):
        pgas_amd.interface_summary(pgas_amd.ModelSmoothResult(flt, 2, res.sum, res.sumsq))


# ---- 6. C ABI ----------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgas_marginal.h")).read(), flags=re.S)


def test_smooth_is_declared_and_bound_and_the_ctypes_struct_is_the_c_struct():
    from pgas_amd import _lib

    txt = _header()
    m = re.search(r"\bint\s+pgas_m_smooth\s*\(([^)]*)\)\s*;", txt)
    assert m, "pgas_m_smooth is not declared in include/pgas_marginal.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 4 and "pgas_m_rollout_desc" in params[1] and "pgas_m_smooth_desc" in params[2]
    fields, size = _c_struct_layout(txt, "pgas_m_smooth_desc")
    S = _lib.ModelSmoothDesc
    assert C.sizeof(S) == size == 14 * 8 + 8 + 2 * 4 + 8 + 64 * 8
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == fields
    assert [n for n, _ in S._fields_][:14] == [f + "_dev" for f in ("x", "anc", "lw", "yhat", "y", "idx", "xs", "xis", "sum", "sumsq", "xi_sum", "xi_sumsq", "fmean", "xi")]
    assert "pgas_m_smooth" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "pgas_m_smooth")
    assert L.pgas_m_smooth.restype is C.c_int and len(L.pgas_m_smooth.argtypes) == 4
    assert callable(_lib.MarginalOps.model_smooth)
    assert re.search(r"#define\s+PGAS_M_SMOOTH_MAX_B\s+256\b", txt) and mr.SMOOTH_CHUNK == 256
    assert re.search(r"#define\s+PGAS_M_SMOOTH_MAX_XI\s+16\b", txt) and mr.MAX_INTERFACE_SMOOTH == 16


def test_stream_id_201_is_the_smoothers_alone():
    ids = {}
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")) + glob.glob(os.path.join(os.path.dirname(pgas_amd.__file__), "csrc", "*")):
        for name, val in re.findall(r"#define\s+(PGAS_STREAM_\w+)\s+(\d+)u?\b", open(path, errors="replace").read()):
            ids.setdefault(int(val), set()).add(name)
    assert ids[201] == {"PGAS_STREAM_M_SMOOTH"} and msn.STREAM_M_SMOOTH == mr.STREAM_SMOOTH == 201
    assert ids[192] == {"PGAS_STREAM_M_ROLLOUT_INTVAR"} and ids[200] == {"PGAS_STREAM_M_ROLLOUT_OBS"}
    others = sorted(v for v in ids if v not in (192, 200, 201))
    assert all(v <= 160 for v in others), others                               # the filter's and the engine's ids; 192 + i (i < 4) ends at 195
    py = {}
    for path in glob.glob(os.path.join(os.path.dirname(pgas_amd.__file__), "*.py")):
        for name, val in re.findall(r"^(STREAM_\w+)\s*=\s*(\d+)\b", open(path).read(), flags=re.M):
            py.setdefault(int(val), set()).add(name)
    assert py[201] == {"STREAM_SMOOTH"}
