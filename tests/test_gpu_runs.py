"""GPU tests of R independent runs of the marginalised filter in one batched pass (pgas_amd.MultiRunAlgorithm1, pgas_m_runs_*,
DESIGN.md section 12).

Device primitives: bit for bit against the single-run entry points on every run's slice (random numbers per key, systematic resampling
per weight vector, weighted statistics per slice).  The filter: every run against Algorithm1 with that run's key on the device (ancestors,
state, interface variables, log-weights -- hence weights -- and per-particle statistics identical; the reductions over the particles to
1e-12) and, for the first and the last run, against the NumPy restatement driven by the same Philox streams.

Resampler rows: the weight vectors of tests/resample_cases.py that exist at the size -- `empty_runs` needs more than 64 segments of
1024 particles and `one_plus_tail` two particles, so neither has a row where it cannot be built."""
import math

import numpy as np
import pytest
import torch

import resample_cases as rc
from common import CanonRand, experiments, marginal_oracle, pgas_amd

pytestmark = pytest.mark.gpu
SEED = 12345678
U_LAST = math.nextafter(1.0, 0.0)


def _ops(N):
    from pgas_amd._lib import MarginalOps

    return MarginalOps(N)


def _keys(R, seed=1):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 2**64, R, dtype=np.uint64)]


def _keys_dev(keys, dev):
    from pgas_amd.chains import keys_tensor

    return keys_tensor(keys, dev)


# ------------------------------------------------------------------------------------------ 1. random numbers
@pytest.mark.parametrize("N", [1, 64, 257, 1000])
def test_runs_rng_equals_the_single_seed_calls(N):
    R = 5
    keys = _keys(R, N)
    one, all_ = _ops(N), _ops(R * N)
    dev = all_.device
    kd = _keys_dev(keys, dev)
    g = torch.Generator(device="cpu").manual_seed(N)
    nu = (torch.rand(R * N, generator=g, dtype=torch.float64) * 60 + 1.0).to(dev)
    src = (torch.rand(R * N, generator=g, dtype=torch.float64) * 40).to(dev)
    anc = torch.randint(0, R * N, (R * N,), generator=g).to(dev).to(torch.int32)

    def compare(t_batched, t_single):
        for ncol in (1, 2, 3):
            z = all_.runs_normal(kd, 17, t_batched, ncol).view(R, N, ncol)
            for r in range(R):
                assert torch.equal(z[r], one.normal(keys[r], 17, t_single, ncol)), ("normal", ncol, r)
        st = all_.runs_student_t(kd, 32, t_batched, nu).view(R, N)
        sd = all_.runs_student_t_df(kd, 33, t_batched, anc, src, 3.0, 0.999).view(R, N)
        un = all_.runs_uniform(kd, 18, t_batched)
        df = (3.0 + 0.999 * src[anc.long()]).view(R, N)
        for r in range(R):
            assert torch.equal(st[r], one.student_t(keys[r], 32, t_single, nu.view(R, N)[r])), ("student_t", r)
            assert torch.equal(sd[r], one.student_t(keys[r], 33, t_single, df[r])), ("student_t_df", r)
            assert un[r].item() == one.uniform(keys[r], 18, t_single) == one.uniform_dev(keys[r], 18, t_single).item(), ("uniform", r)

    compare(9, 9)
    if N == 257:   # the device-resident time index replaces the argument in all four kernels
        t_dev = torch.full((1,), 6, dtype=torch.int32, device=dev)
        all_.set_time_source(t_dev)
        try:
            compare(0, 6)
        finally:
            all_.set_time_source(None)


# ------------------------------------------------------------------------------------------ 2. systematic resampling
def _rows(N):
    rows = [("mild", rc.mild(N)), ("flat", rc.flat(N)), ("one_hot_first", rc.one_hot(N, 0)), ("one_hot_middle", rc.one_hot(N, N // 2)),
            ("one_hot_last", rc.one_hot(N, N - 1)), ("far_pair", rc.far_pair(N, 1e5)), ("stairs", rc.stairs(N, 700)),
            ("all_empty", rc.all_empty(N)), ("all_nan", rc.all_nan(N)), ("with_nan", rc.with_nan(N)), ("huge_range", rc.huge_range(N))]
    if N >= 2:
        rows.append(("one_plus_tail", rc.one_plus_tail(N, N // 3, 0.99)))
    return rows


def _check_resampler(N, lw, u):
    """lw (R, N), u (R,) host arrays: the batched launch against one single-vector call per row on an N-particle context."""
    from pgas_amd._lib import Engine

    R = lw.shape[0]
    eng = Engine.utility(N)
    ops = _ops(N)
    lwd, ud = torch.as_tensor(lw, device=eng.device), torch.as_tensor(u, device=eng.device)
    loc, glo = ops.runs_systematic(R, ud, lwd)
    ref = torch.stack([eng.systematic_resample(ud[r:r + 1], lwd[r]) for r in range(R)])
    bad = (loc != ref).any(dim=1).nonzero().reshape(-1).tolist()
    assert not bad, f"N = {N}: rows {bad[:10]} differ from the single-vector resampler"
    assert torch.equal(glo, ref + (torch.arange(R, device=eng.device, dtype=torch.int32) * N)[:, None])
    only_local, none = ops.runs_systematic(R, ud, lwd, want_global=False)
    assert none is None and torch.equal(only_local, ref)


@pytest.mark.parametrize("N", [1, 2, 200, 256, 257, 512, 513, 1023, 1024])
def test_runs_systematic_equals_the_single_vector_resampler(N):
    us = (0.0, rc.U_DEFAULT, U_LAST, 0.61, 0.83)
    rows = _rows(N)
    lw = np.stack([v for k in range(len(us)) for _, v in rows])               # every vector under every uniform
    u = np.array([us[k] for k in range(len(us)) for _ in rows])
    _check_resampler(N, lw, u)


@pytest.mark.parametrize("R,N", [(2000, 64), (600, 1024)])
def test_runs_systematic_with_more_runs_than_are_resident(R, N):
    lw = np.stack([rc.mild(N, seed=r) for r in range(R)])
    u = np.random.default_rng(R).uniform(0.0, 1.0, R)
    _check_resampler(N, lw, u)


def test_runs_systematic_refuses_more_than_1024_particles():
    from pgas_amd._lib import PgasError

    ops = _ops(200)
    dev = ops.device
    with pytest.raises(PgasError, match="1025"):
        ops.runs_systematic(2, torch.full((2,), 0.5, dtype=torch.float64, device=dev), torch.zeros(2, 1025, dtype=torch.float64, device=dev))
    lw = np.stack([rc.mild(200, seed=r) for r in range(3)])
    loc, _ = ops.runs_systematic(3, torch.full((3,), 0.25, dtype=torch.float64, device=dev), torch.as_tensor(lw, device=dev))
    for r in range(3):
        assert torch.equal(loc[r], ops.systematic_resample(0.25, torch.as_tensor(lw[r], device=dev)))


# ------------------------------------------------------------------------------------------ 3. weighted statistics
@pytest.mark.parametrize("R,N,M,nv", [(3, 700, 41, 1), (4, 513, 1, 1), (2, 1024, 20, 3)])
def test_runs_weighted_stats_equal_the_single_reduction_on_every_slice(R, N, M, nv):
    all_, one = _ops(R * N), _ops(N)
    dev = all_.device
    g = torch.Generator(device="cpu").manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dev)   # noqa: E731
    if nv == 1:   # the scalar layout
        T = (rnd(R * N, M), rnd(R * N, M, M), rnd(R * N), rnd(R * N))
    else:
        T = (rnd(R * N, M, nv), rnd(R * N, M, M), rnd(R * N, nv, nv), rnd(R * N))
    w = torch.softmax(rnd(R, N), dim=1).reshape(-1)
    S = all_.runs_weighted_stats(R, w, T)
    for r in range(R):
        sl = slice(r * N, (r + 1) * N)
        ref = one.weighted_stats(w[sl], tuple(t[sl] for t in T))
        for j in range(4):
            assert S[j][r].shape == ref[j].shape and torch.equal(S[j][r], ref[j]), (r, j)


# ------------------------------------------------------------------------------------------ 4. the filter, run by run
def _problem(name, T=8):
    return {"smo": experiments.smo_marginal, "toy": experiments.toy_marginal, "vehicle": experiments.vehicle_marginal,
            "emps": experiments.emps_marginal, "smo2": experiments.smo_two_component_marginal}[name.split("/")[0]](T=T)


def _args(pb, name):
    ssm = pb.ssm_symbolic(pgas_amd.SymbolicStateSpaceModel) if name.endswith("/traced") else pb.ssm(pgas_amd.StateSpaceModel, torch)
    return dict(observations=pb.observations, inputs=pb.inputs, SSM=ssm, forgetting_factor=pb.forgetting_factor, init_state_mean=pb.init_state_mean,
                init_state_cov=pb.init_state_cov, init_int_var_mean=pb.init_int_var_mean, init_int_var_cov=pb.init_int_var_cov,
                GP_prior=pb.GP_prior, basis_fcn=pb.basis_fcn())


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(np.shape(a))
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _named(out, n_int):
    """Algorithm1's 8-tuple as (name, array, kind) with kind = 'particle' (per-particle quantities and what is elementwise in them) or
    'reduced' (sums over the particles)."""
    st, iv, sst, w, anc, stats, obs, ll = out
    items = [("state_trace", st, "particle"), ("weights_trace", w, "reduced"), ("obs_trace", obs, "particle"), ("log_likelihood", ll, "particle")]
    for i in range(n_int):
        items.append((f"int_var_trace[{i}]", iv[i], "particle"))
        for j in range(4):
            items.append((f"suff_stats_trace[{i}][{j}]", sst[i][j], "reduced"))
            items.append((f"suff_stats[{i}][{j}]", stats[i][j], "particle"))
    return items


def _check_against_single_runs(name, R, N, T=8, seed=3):
    pb = _problem(name, T)
    keys = pgas_amd.random.split(SEED + seed, R)
    got = pgas_amd.MultiRunAlgorithm1(R, N, **_args(pb, name))(None, keys=keys)
    n_int = len(pb.init_int_var_mean)
    assert got[4].shape == (R, T - 1, N) and got[4].dtype == torch.int32
    problems = []
    for r in range(R):
        ref = pgas_amd.Algorithm1(N, **_args(pb, name))(keys[r])
        if not torch.equal(got[4][r], ref[4]):
            problems.append(f"run {r}: ancestor_trace differs")
        for (what, a, kind), (_, b, _) in zip(_named(got, n_int), _named(ref, n_int)):
            a = a[r]
            assert a.shape == b.shape, (what, a.shape, b.shape)
            err = _rel(a.cpu().numpy(), b.cpu().numpy())
            print(f"{name} R={R} N={N} run {r} {what}: relative difference {err:.3e}, bit-equal {torch.equal(a, b)}")
            if kind == "particle" and not torch.equal(a, b):
                problems.append(f"run {r}: {what} is not bit-equal to the single run ({err:.3e})")
            if not err <= 1e-12:
                problems.append(f"run {r}: {what} differs by {err:.3e} > 1e-12")
    assert not problems, problems
    for r in sorted({0, R - 1}):
        ref = marginal_oracle(pb, N)(CanonRand(keys[r], N))
        assert np.array_equal(got[4][r].cpu().numpy(), ref[4]), f"run {r}: ancestor_trace differs from the restatement"
        st, iv, sst, w, _, stats, obs, ll = ref
        flat_ref = [("state_trace", st), ("weights_trace", w), ("obs_trace", obs), ("log_likelihood", ll)]
        for i in range(n_int):
            flat_ref.append((f"int_var_trace[{i}]", iv[i]))
            for j in range(4):
                flat_ref += [(f"suff_stats_trace[{i}][{j}]", sst[i][j]), (f"suff_stats[{i}][{j}]", stats[i][j])]
        for (what, a, _), (what_ref, b) in zip(_named(got, n_int), flat_ref):
            assert what == what_ref
            err = _rel(np.asarray(b), a[r].cpu().numpy())
            assert err < (1e-7 if what == "log_likelihood" else 1e-8), f"run {r}: {what} differs from the restatement by {err:.3e}"


@pytest.mark.parametrize("name,R,N", [("smo", 1, 200), ("smo", 3, 200), ("smo", 7, 257), ("smo", 2, 1024), ("toy", 3, 200), ("vehicle", 3, 200),
                                      ("emps", 3, 200), ("smo/traced", 3, 200), ("smo2", 3, 200)])
def test_every_run_equals_the_single_run_filter_and_the_restatement(name, R, N):
    """torch callables, a traced model (draw_state_gather with global ancestors), two latent functions (vehicle) and an interface
    variable of two components (smo2)."""
    _check_against_single_runs(name, R, N)


# ------------------------------------------------------------------------------------------ 5. independence
def _flat(out):
    st, iv, sst, w, anc, stats, obs, ll = out
    return [st, w, anc, obs, ll] + list(iv) + [t for s in sst for t in s] + [t for s in stats for t in s]


def test_runs_are_independent_of_each_other():
    pb = _problem("smo")
    k = pgas_amd.random.split(SEED, 3)
    alg = pgas_amd.MultiRunAlgorithm1(4, 200, **_args(pb, "smo"))
    keys = [k[0], k[1], k[2], k[1]]
    fwd = _flat(alg(None, keys=keys))
    rev = _flat(alg(None, keys=keys[::-1]))
    for n, (a, b) in enumerate(zip(fwd, rev)):
        assert torch.equal(a, b.flip(0)), f"output {n}: reversing the keys does not reverse the runs"
        assert torch.equal(a[1], a[3]), f"output {n}: two runs with one key differ"
    assert not torch.equal(fwd[0][0], fwd[0][1]) and not torch.equal(fwd[2][0], fwd[2][1]), "two runs with different keys agree"
    default = _flat(alg(SEED))
    split = _flat(alg(None, keys=pgas_amd.random.split(SEED, 4)))
    assert all(torch.equal(a, b) for a, b in zip(default, split)), "the default keys are random.split(key, R)"


# ------------------------------------------------------------------------------------------ 6. graph replay
@pytest.mark.parametrize("name", ["smo", "toy", "vehicle"])
def test_runs_graph_replay_equals_eager_loop(name):
    pb = _problem(name, T=12)
    keys = pgas_amd.random.split(SEED, 3)
    eager = pgas_amd.MultiRunAlgorithm1(3, 200, **_args(pb, name))(None, keys=keys, use_graph=False)
    graphed = pgas_amd.MultiRunAlgorithm1(3, 200, **_args(pb, name))(None, keys=keys, use_graph=True)
    for k, (a, b) in enumerate(zip(_flat(eager), _flat(graphed))):
        assert a.shape == b.shape and torch.equal(a, b), f"output {k} differs between the eager loop and the graph replay"


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_device_usable():
    pb = _problem("smo")
    with pytest.raises(ValueError, match="1024"):
        pgas_amd.MultiRunAlgorithm1(2, 1025, **_args(pb, "smo"))
    with pytest.raises(ValueError, match="R must be"):
        pgas_amd.MultiRunAlgorithm1(0, 200, **_args(pb, "smo"))
    alg = pgas_amd.MultiRunAlgorithm1(3, 200, **_args(pb, "smo"))
    with pytest.raises(ValueError, match="keys"):
        alg(None, keys=[1, 2])
    with pytest.raises(ValueError, match="keys"):
        alg(None, keys=[1, 2, 3, 4])
    _check_against_single_runs("smo", 2, 200, seed=11)
