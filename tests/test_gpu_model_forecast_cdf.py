"""pgas_amd.ModelRollout.forecast_cdf on the GPU (pgas_m_forecast_cdf, csrc/pgas_marginal_forecast_cdf.hip.h): the
h-step-ahead clouds of the grey-box forecast counted against the thresholds of the target row inside the kernel, compared
(np.array_equal: the counts are integers) with the NumPy restatement (tests/model_rollout_cdf_numpy.py) applied to the clouds
``ModelRollout.forecast(clouds=True)`` stores for the same call arguments -- which tests/test_gpu_model_forecast.py pins to the filter's
trace and to the per-step primitives.  A closed form that does not pass through the restatement closes the file."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import model_cdf_cases as mc
import model_filter_cases as cases
import model_forecast_numpy as mfc
import model_rollout_cdf_numpy as mrc
from common import ROOT, pgas_amd
from pgas_amd import _lib
from pgas_amd._lib import ModelForecastCdfDesc, PgasError
from pgas_amd.model_rollout import STREAM_ROLLOUT_OBS
from test_gpu_model_filter import ALL, Case, _case, _np
from test_gpu_model_rollout_cdf import _LR, _get, _jmax

pytestmark = pytest.mark.gpu
K, T, KEYS, H = cases.K, cases.T, cases.KEYS, 4
INF, NAN = float("inf"), float("nan")
WIDE_NS = [1, 65, 200, 513]


def _normals(c, key, t, lead, N, n):
    """Rows of pgas_m_rng_normal(key, 200, t, p0 = lead << 32, N, n): the lead sits in the high word of the particle index."""
    out = torch.empty((N, n), dtype=torch.float64, device=c.dev)
    eng = c.ops.eng
    eng._chk(eng.lib.pgas_m_rng_normal(eng._h, int(key), STREAM_ROLLOUT_OBS, int(t), int(lead) << 32, N, n, out.data_ptr(), eng._stream()), "pgas_m_rng_normal")
    return out


def _obs_normals(c, N, Hn=H, Tn=T, keys=KEYS):
    """e (K, Hn, Tn, N, ny): horizon index l at target row tau uses particle (l + 1) << 32 | i."""
    e = torch.stack([torch.stack([torch.stack([_normals(c, k, t, l + 1, N, c.sim.ny) for t in range(Tn)]) for l in range(Hn)]) for k in keys])
    return _np(e)


@functools.lru_cache(maxsize=None)
def _clouds(name, N, Hn=H):
    """(cloud_x, cloud_y, filter x, filter yhat) of forecast(clouds=True) with drawn x_0, on the host; computed once, never changed."""
    c = _get(name)
    r = c.sim.forecast(c.A, KEYS, N, Hn, log_score=False, clouds=True)
    out = tuple(_np(a) for a in (r.cloud_x, r.cloud_y, r.filter.x, r.filter.yhat))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _thr(name, J):
    """threshold_grid of the pooled moments of the horizon-1 cloud at the largest common N; J = 1: the mean itself."""
    cx, cy = _clouds(name, 200)[:2]
    v = np.concatenate([cx[:, 0], cy[:, 0]], axis=-1)      # (K, T, N, nv)
    flat = np.moveaxis(v, 1, 0).reshape(T, -1, v.shape[-1])
    th = pgas_amd.threshold_grid(flat.mean(axis=1), flat.std(axis=1), J, width=2.0 if J > 1 else 0.0).numpy()
    th.setflags(write=False)
    return th


def _minus_one_exactly_where_no_origin_row(got, Hn=H, Tn=T):
    ok = mfc.defined(Hn, Tn)
    assert (got[:, ~ok] == -1).all() and (got[:, ok] >= 0).all()


# ---- 1. counts = the restated counts of forecast(clouds=True)'s own clouds -----------------------------------------------------------------
CASES = ALL + [("wide", N) for N in WIDE_NS]


@pytest.mark.parametrize("name,N", CASES, ids=[f"{n}-N{N}" for n, N in CASES])
def test_counts_equal_the_restated_counts_of_the_forecast_clouds(name, N):
    c = _get(name)
    cx, cy = _clouds(name, N)[:2]
    nv = c.sim.nx + c.sim.ny
    e = _obs_normals(c, N)
    for J in (1, _jmax(name)):
        thr = _thr(name, J)
        for noise in (False, True):
            want = mrc.forecast_counts(cx, cy, thr, _LR(c) if noise else None, e if noise else None)
            r = c.sim.forecast_cdf(c.A, KEYS, N, H, thresholds=thr, observation_noise=noise)
            got = _np(r.count)
            assert r.n == N and r.nx == c.sim.nx and not r.pit and got.dtype == np.int32 and got.shape == (K, H, T, nv, J)
            _minus_one_exactly_where_no_origin_row(got)
            d = got[:, mfc.defined(H, T)]
            assert N == 1 and J == 1 or ((d != 0).any() and (d != N).any()), "thresholds that count nothing or everything test nothing"
            assert np.array_equal(got, want), f"{name} N = {N} J = {J} noise = {noise}"
            if noise and N >= 63:
                assert not np.array_equal(got[..., c.sim.nx:, :], noise_free[..., c.sim.nx:, :])
            noise_free = got


@pytest.mark.parametrize("name", ["vehicle", "smo2"])
def test_horizons_one_two_and_the_whole_record(name):
    c = _get(name)
    N = 200
    thr = _thr(name, 16)
    four = _np(c.sim.forecast_cdf(c.A, KEYS, N, H, thresholds=thr).count)
    for Hn in (1, 2, T):
        got = _np(c.sim.forecast_cdf(c.A, KEYS, N, Hn, thresholds=thr).count)
        assert got.shape[1] == Hn
        _minus_one_exactly_where_no_origin_row(got, Hn)
        m = min(Hn, H)
        assert np.array_equal(got[:, :m], four[:, :m]), f"H = {Hn}: no count depends on the horizon asked for"
    cx, cy = _clouds(name, N, T)[:2]
    full = _np(c.sim.forecast_cdf(c.A, KEYS, N, T, thresholds=thr, observation_noise=False).count)
    assert np.array_equal(full, mrc.forecast_counts(cx, cy, thr))


# ---- 2. properties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smo", "vehicle", "wide"])
def test_infinite_thresholds_and_horizon_1_is_the_filters_own_trace(name):
    c = _get(name)
    N, nx = 200, c.sim.nx
    fx, fy = _clouds(name, N)[2:]
    v = np.concatenate([fx, fy], axis=-1)                  # (K, T, N, nv): the filter's own traces
    thr = np.empty((T, v.shape[-1], 4))
    thr[..., 0] = v[0, :, 7, :]                             # particle 7 of draw 0: a tie
    thr[..., 1], thr[..., 2], thr[..., 3] = INF, -INF, NAN
    got = _np(c.sim.forecast_cdf(c.A, KEYS, N, H, thresholds=thr, observation_noise=False).count)
    ok = mfc.defined(H, T)
    assert (got[:, ok][..., 1] == N).all() and (got[:, ok][..., 2] == 0).all() and (got[:, ok][..., 3] == 0).all()
    assert np.array_equal(got[:, 0], mrc.counts(v, thr)) and (got[0, 0, ..., 0] >= 1).all()
    below = thr.copy()
    below[..., 0] = np.nextafter(thr[..., 0], -INF)
    low = _np(c.sim.forecast_cdf(c.A, KEYS, N, H, thresholds=below, observation_noise=False).count)
    assert np.array_equal(got[0, 0, ..., 0] - low[0, 0, ..., 0], (v[0] == thr[:, None, :, 0]).sum(axis=1))
    grid = _np(c.sim.forecast_cdf(c.A, KEYS, N, H, thresholds=_thr(name, _jmax(name))).count)
    assert (np.diff(grid[:, ok], axis=-1) >= 0).all() and (grid <= N).all()


def test_no_thresholds_means_the_observations_and_a_nan_observation_row_counts_nothing():
    base = _get("vehicle")
    N, nx = 130, 2
    pit = base.sim.forecast_cdf(base.A, KEYS, N, H)
    same = base.sim.forecast_cdf(base.A, KEYS, N, H, thresholds=base.y)
    assert pit.pit and not same.pit and torch.equal(pit.count, same.count)
    ok = mfc.defined(H, T)
    assert (_np(pit.count)[:, ok][:, :, :nx] == 0).all()
    s = pgas_amd.calibration_summary(pit)
    assert tuple(s["pit"].shape) == (H, T, 2) and tuple(s["ks"].shape) == (H,) and bool(torch.isfinite(s["ks"]).all())
    y = base.y.copy()
    y[3, -1] = NAN
    c = Case("vehicle", ops=base.ops, observations=y)
    got = _np(c.sim.forecast_cdf(c.A, KEYS, N, H).count)
    _minus_one_exactly_where_no_origin_row(got)
    for h in range(H):
        if h <= 3:
            assert (got[:, h, 3, nx + 1] == 0).all()        # the NaN threshold counts nothing; the row is a pure prediction step of the filter
    # targets up to row 3 have seen the same observation rows: the same clouds, the same noise
    assert np.array_equal(got[:, :, :3], _np(pit.count)[:, :, :3]) and np.array_equal(got[:, :, 3, :nx + 1], _np(pit.count)[:, :, 3, :nx + 1])


def test_draws_are_independent_of_their_launch_and_equal_inputs_give_equal_rows():
    c = _get("vehicle")
    N, thr = 130, _thr("vehicle", 16)
    full = _np(c.sim.forecast_cdf(c.A, KEYS, N, H, thresholds=thr).count)
    idx = [0, 2, 0]
    dup = _np(c.sim.forecast_cdf([a[idx].contiguous() for a in c.A], [KEYS[i] for i in idx], N, H, thresholds=thr).count)
    assert np.array_equal(dup[0], dup[2]) and np.array_equal(dup[0], full[0]) and np.array_equal(dup[1], full[2]) and not np.array_equal(dup[0], dup[1])
    alone = _np(c.sim.forecast_cdf([a[1:2].contiguous() for a in c.A], KEYS[1:2], N, H, thresholds=thr).count)
    assert np.array_equal(alone[0], full[1])


def test_draws_beyond_one_launch_run_in_chunks(monkeypatch):
    import pgas_amd.model_rollout as mr

    c = _get("smo")
    Kd, N = 5, 70
    A = [torch.as_tensor(a, device=c.dev) for a in cases.coeffs(c.pb, Kd, seed=3)]
    keys = [11, 12, 13, 14, 15]
    thr = _thr("smo", 16)
    whole = _np(c.sim.forecast_cdf(A, keys, N, H, thresholds=thr).count)
    launches = []
    real = c.ops.model_forecast_cdf
    monkeypatch.setattr(mr, "MAX_DRAWS_PER_LAUNCH", 2)
    monkeypatch.setattr(c.ops, "model_forecast_cdf", lambda d, f: (launches.append((d.K, d.P, f.H, f.J)), real(d, f))[1])
    parts = _np(c.sim.forecast_cdf(A, keys, N, H, thresholds=thr).count)
    assert launches == [(2, N, H, 16), (2, N, H, 16), (1, N, H, 16)] and np.array_equal(whole, parts)


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import model_filter_cases as cases
from pgas_amd import _lib
from test_gpu_model_filter import _case
assert _lib.load().pgas_m_forecast_origins_per_block() == 1
c = _case("smo2")
thr = np.asarray(json.loads(sys.argv[3]), dtype=np.float64)
r = c.sim.forecast_cdf(c.A, cases.KEYS, 257, 4, thresholds=thr, observation_noise=True)
print("COUNTS " + json.dumps(r.count.cpu().numpy().reshape(-1).tolist()))
"""


def test_no_count_depends_on_the_origins_per_workgroup(monkeypatch):
    c = _get("smo2")
    N = 257
    thr = _thr("smo2", 16)
    want = _np(c.sim.forecast_cdf(c.A, KEYS, N, H, thresholds=thr, observation_noise=True).count)
    lib = _lib.load()
    default = lib.pgas_m_forecast_origins_per_block()
    for tb in (5, T, 64):
        monkeypatch.setenv("PGAS_M_FORECAST_TB", str(tb))
        assert lib.pgas_m_forecast_origins_per_block() == tb
        assert np.array_equal(_np(c.sim.forecast_cdf(c.A, KEYS, N, H, thresholds=thr, observation_noise=True).count), want), tb
    monkeypatch.delenv("PGAS_M_FORECAST_TB")
    assert lib.pgas_m_forecast_origins_per_block() == default
    # one origin row per workgroup, in a fresh process that has it in its environment from the start; compared by value
    env = dict(os.environ, PGAS_M_FORECAST_TB="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), json.dumps(thr.tolist())], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("COUNTS ")][-1]
    got = np.asarray(json.loads(line[len("COUNTS "):]), dtype=np.int32).reshape(want.shape)
    assert np.array_equal(got, want)


# ---- 3. safety -----------------------------------------------------------------------------------------------------------------------------
def test_forecast_cdf_makes_no_host_round_trip():
    c = _get("vehicle")
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    thr = torch.as_tensor(_thr("vehicle", 16), device=c.dev)
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    cov = [torch.eye(1, dtype=torch.float64, device=c.dev).repeat(K, 1, 1) * 1e-4 for _ in range(2)]
    calls = [lambda: c.sim.forecast_cdf(c.A, kd, 130, H, thresholds=thr), lambda: c.sim.forecast_cdf(c.A, kd, 3, 2, init_state=x0, row_cov=cov),
             lambda: c.sim.forecast_cdf(c.A, kd, 300, T, thresholds=thr[:, 2:].contiguous(), observation_noise=False)]
    warm = [f() for f in calls]   # uploads of the programs, tables and observations, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [f() for f in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(warm, outs):
        assert torch.equal(a.count, b.count) and bool((a.count >= -1).all()) and bool(a.count.sum() > 0)


def test_abi_refusals_leave_the_context_usable():
    c = _get("vehicle")
    sim, N, J = c.sim, 70, 16
    kd = pgas_amd.chains.keys_tensor(KEYS, c.dev)
    thr = torch.as_tensor(_thr("vehicle", J), device=c.dev)
    flt = sim.filter(c.A, kd, N, moments=False, traces=True)
    good = sim.forecast_cdf(c.A, kd, N, H, thresholds=thr)
    count = torch.empty((K, H, T, 4, J), dtype=torch.int32, device=c.dev)
    LR = _LR(c)
    import pgas_amd.model_rollout as mr

    fit = 64 * ((mr.LDS_PER_WORKGROUP - 2048 - sim.filter_lds_bytes(0)) // sim._filter_file_bytes())   # static LDS: 2 x 4 x 64 int32
    assert c.nmax < fit < 1024

    def descs(s=sim, A=c.A, x=flt.x):
        d = s._desc(K, N, 0, 0, A, None, kd, None, True, None, None)
        f = ModelForecastCdfDesc()
        f.x_dev, f.thr_dev, f.count_dev, f.H, f.J, f.noise = x.data_ptr(), thr.data_ptr(), count.data_ptr(), H, J, 1
        for j in range(2):
            for l in range(2):
                f.LR[2 * j + l] = float(LR[j, l])
        return d, f

    edits = {
        "J = 0": lambda d, f: setattr(f, "J", 0),
        "J = 17": lambda d, f: setattr(f, "J", 17),
        "NULL argument (x)": lambda d, f: setattr(f, "x_dev", None),
        "NULL argument (thr, count)": lambda d, f: setattr(f, "thr_dev", None),
        "(thr, count)": lambda d, f: setattr(f, "count_dev", None),
        "N = 0": lambda d, f: setattr(d, "P", 0),
        "N = 1025": lambda d, f: setattr(d, "P", 1025),
        "p0 = 64": lambda d, f: setattr(d, "p0", 64),
        "H = 0": lambda d, f: setattr(f, "H", 0),
        f"H = {T + 1}": lambda d, f: setattr(f, "H", T + 1),
        "needs seeds": lambda d, f: setattr(d, "seeds_dev", None),
        "K = 65536": lambda d, f: setattr(d, "K", 65536),
        f"the largest N that fits is {fit}": lambda d, f: setattr(d, "P", fit + 1),   # one more register file than LDS holds
        "output program": lambda d, f: setattr(d, "gcode_dev", None),
        "L = 0": lambda d, f: setattr(d, "L", 0),
        "97 registers": lambda d, f: setattr(d, "nreg", 97),
    }
    for what, edit in edits.items():
        d, f = descs()
        edit(d, f)
        with pytest.raises(PgasError, match=r"pgas_m_forecast_cdf failed \(-1\)") as ei:   # PGAS_E_ARG, with the library's message
            sim.ops.model_forecast_cdf(d, f)
        assert "pgas_m_forecast_cdf: " in str(ei.value) and what in str(ei.value), (what, str(ei.value))
    d, f = descs()                                            # observation noise alone needs seeds too
    x0 = torch.zeros((K, 2), dtype=torch.float64, device=c.dev)
    d.seeds_dev, d.Qc_dev, d.x0_mode, d.x0_dev, d.m0L0_dev = None, None, 2, x0.data_ptr(), None   # no other noise: a given x_0, no process noise
    with pytest.raises(PgasError, match="observation noise needs seeds"):
        sim.ops.model_forecast_cdf(d, f)
    w = _get("wide")                                          # five channels: J = 13 needs 65 slots
    d, f = descs(w.sim, w.A)
    f.J = 13
    with pytest.raises(PgasError, match="J_max = 12"):
        w.sim.ops.model_forecast_cdf(d, f)
    d, f = descs()                                            # the untouched descriptors still run on the same context
    sim.ops.model_forecast_cdf(d, f)
    torch.cuda.synchronize()
    assert torch.equal(count, good.count)
    assert torch.equal(sim.forecast_cdf(c.A, kd, N, H, thresholds=thr).count, good.count)
    again = sim.filter(c.A, kd, N, moments=False, traces=True)
    assert torch.equal(again.x, flt.x) and torch.equal(again.loglik, flt.loglik)


# ---- 4. closed form, independent of the restatement ------------------------------------------------------------------------------------------
def test_memoryless_model_pooled_counts_are_binomial():
    """x' = xi + N(0, q), y = x with A = 0: at every lead and whatever the ancestors are, x_tau (tau >= 1) is iid N(0, q) and yhat + e iid
    N(0, q + r) over rows, leads, particles and draws, so the count at sigma * TAUS pooled over K = 3 draws, h = 1 .. 4, rows
    tau >= max(h - 1, 1) and N = 1024 particles is Binomial(n = 125952, Phi(TAUS)): |z| <= 4, the project's bound for every closed-form
    test.  tests/test_model_rollout_cdf_host.py evaluates the same statistic on the CPU from the generator's normals: max |z| = 1.762
    (x), 1.879 (yhat)."""
    ops = _case("toy").ops
    ssm, sim, A, y = mc.memoryless_rollout(ops)
    N, Hn = mc.CLOSED_N, mc.CLOSED_H
    assert sim.max_particles() >= N
    r = sim.forecast_cdf(A, KEYS, N, Hn, thresholds=mc.closed_thresholds(T), observation_noise=True)
    cnt = _np(r.count)
    assert cnt.shape == (K, Hn, T, 2, len(mc.TAUS))
    _minus_one_exactly_where_no_origin_row(cnt, Hn)
    tot, rows = mc.pool_forecast(cnt)
    z = mc.binomial_z(tot, rows * N)
    print(f"forecasts: n = {rows * N}, z x = {np.round(z[0], 3).tolist()}, z yhat = {np.round(z[1], 3).tolist()}")
    assert (np.abs(z) <= 4.0).all()
