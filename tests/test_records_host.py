"""Host side of the multi-record layer (pgas_amd.records): the record table built from ragged lists, the reference forms, record
slicing, the refusals of mismatched shapes and lengths, the degrees of freedom and the seed rule.  No GPU."""
import numpy as np
import pytest
import torch

from common import experiments, pgas_amd
from pgas_amd import random as prng
from pgas_amd import records as rc


def test_record_table_from_ragged_lists():
    rng = np.random.default_rng(0)
    lengths = (2, 3, 17, 2, 9)
    ys = [rng.standard_normal(n) for n in lengths]
    us = [rng.standard_normal((n, 2)) for n in lengths]
    row0, y, u = rc.record_table(ys, us)
    assert row0.dtype == np.int64 and row0.tolist() == [0, 2, 5, 22, 24, 33]
    assert y.shape == (33,) and u.shape == (33, 2)
    for e in range(len(lengths)):
        assert np.array_equal(y[row0[e]:row0[e + 1]], ys[e]) and np.array_equal(u[row0[e]:row0[e + 1]], us[e])
    # one record, tuples, no inputs
    row0, y, u = rc.record_table((np.zeros((4, 1)),), None)
    assert row0.tolist() == [0, 4] and y.shape == (4, 1) and u.shape == (4, 0)


@pytest.mark.parametrize("ys,us,msg", [
    ([np.zeros(3), np.zeros(1)], [np.zeros(3), np.zeros(1)], "record 1: needs at least 2 rows"),
    ([np.zeros(3), np.zeros(4)], [np.zeros(3), np.zeros(5)], "record 1: 4 rows of observations"),
    ([np.zeros(3), np.zeros(4)], [np.zeros(3)], "inputs: expected a sequence of 2"),
    ([np.zeros((3, 1)), np.zeros((4, 2))], [np.zeros(3), np.zeros(4)], "record 1: row shapes"),
    ([np.zeros(3), np.zeros(4)], [np.zeros((3, 1)), np.zeros((4, 2))], "record 1: row shapes"),
    (np.zeros((2, 5)), [np.zeros(5), np.zeros(5)], "observations: expected a sequence"),
    ([], [], "no record"),
])
def test_record_table_refuses_mismatches(ys, us, msg):
    with pytest.raises(ValueError, match=msg):
        rc.record_table(ys, us)


def test_constructor_refuses_before_it_needs_a_device():
    pb = experiments.smo_pgas(T=8)
    args = (pb.init_state_mean, pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)
    with pytest.raises(ValueError, match="record 1: needs at least 2 rows"):
        pgas_amd.condSequentialMonteCarloRecords(2, 16, [pb.observations[:7], pb.observations[7:]], [pb.inputs[:7], pb.inputs[7:]], *args)
    with pytest.raises(ValueError, match="C must be >= 1"):
        pgas_amd.condSequentialMonteCarloRecords(0, 16, [pb.observations], [pb.inputs], *args)
    with pytest.raises(ValueError, match="leading dimension 3 for 2 records"):
        pgas_amd.condSequentialMonteCarloRecords(2, 16, [pb.observations[:4], pb.observations[4:]], [pb.inputs[:4], pb.inputs[4:]],
                                                 np.zeros((3, 2)), pb.init_state_cov, pb.likelihood_fcn, pb.basis_fcn)


def test_initial_states_shared_or_per_record():
    m, P = np.array([1.0, 2.0]), np.diag([3.0, 4.0])
    m0, P0, mr, Pr = rc.init_states(3, m, P)
    assert np.array_equal(m0, m) and np.array_equal(P0, P) and mr is None and Pr is None
    ms, Ps = np.arange(6.0).reshape(3, 2), np.stack([P * (e + 1) for e in range(3)])
    m0, P0, mr, Pr = rc.init_states(3, ms, Ps)
    assert np.array_equal(m0, ms[0]) and np.array_equal(P0, Ps[0]) and np.array_equal(mr, ms) and np.array_equal(Pr, Ps)
    m0, P0, mr, Pr = rc.init_states(3, ms, P)          # means per record, one covariance
    assert np.array_equal(mr, ms) and Pr.shape == (3, 2, 2) and all(np.array_equal(Pr[e], P) for e in range(3))
    m0, P0, mr, Pr = rc.init_states(3, m, Ps)          # one mean, covariances per record
    assert np.array_equal(Pr, Ps) and mr.shape == (3, 2) and all(np.array_equal(mr[e], m) for e in range(3))
    m0, P0, mr, Pr = rc.init_states(2, [0.5], [[2.0]])  # nx = 1
    assert m0.shape == (1,) and P0.shape == (1, 1)
    for bad_m, bad_P, msg in [(ms[:2], P, "leading dimension 2"), (m, Ps[:2], "init_state_cov: expected \\(3, 2, 2\\)"), (m, np.eye(3), "init_state_cov: expected \\(2, 2\\)")]:
        with pytest.raises(ValueError, match=msg):
            rc.init_states(3, bad_m, bad_P)


def test_reference_forms():
    row0 = np.array([0, 2, 5, 9])
    C, nx, Tsum = 3, 2, 9
    rng = np.random.default_rng(1)
    flat = rng.standard_normal((Tsum, nx))
    parts = [flat[0:2], flat[2:5], flat[5:9]]
    want = torch.as_tensor(flat).expand(C, Tsum, nx)
    for form in (parts, tuple(parts), [torch.as_tensor(p) for p in parts], flat, torch.as_tensor(flat), np.repeat(flat[None], C, axis=0)):
        got = rc.stack_refs(form, row0, C, nx)
        assert got.dtype == torch.float64 and got.is_contiguous() and torch.equal(got, want)
    per_chain = rng.standard_normal((C, Tsum, nx))
    assert torch.equal(rc.stack_refs(per_chain, row0, C, nx), torch.as_tensor(per_chain))
    # nx = 1: the trailing axis may be left out
    f1 = rng.standard_normal(Tsum)
    for form in ([f1[0:2], f1[2:5], f1[5:9]], f1, f1[:, None], np.repeat(f1[None], C, axis=0)):
        assert torch.equal(rc.stack_refs(form, row0, C, 1), torch.as_tensor(f1).reshape(1, Tsum, 1).expand(C, Tsum, 1))
    # equal-length records given as a list stay a list of records
    eq = np.array([0, 3, 6, 9])
    assert torch.equal(rc.stack_refs([flat[0:3], flat[3:6], flat[6:9]], eq, C, nx), want)
    for bad, msg in [([flat[0:2], flat[2:5], flat[5:8]], "ref_state\\[2\\]: expected \\(4, 2\\)"), (flat[:8], "ref_state: expected"),
                     (np.zeros((2, Tsum, nx)), "ref_state: expected"), ([flat[0:2], flat[2:9]], "ref_state: expected")]:
        with pytest.raises(ValueError, match=msg):
            rc.stack_refs(bad, row0, C, nx)


def test_record_slicing():
    row0 = np.array([0, 2, 5, 9])
    a = np.arange(3 * 9 * 4 * 2).reshape(3, 9, 4, 2)
    assert np.array_equal(rc.record_slice(row0, 1, a), a[:, 2:5])
    assert np.array_equal(rc.record_slice(row0, 2, a[0]), a[0, 5:9])
    t = torch.as_tensor(a)
    assert torch.equal(rc.record_slice(row0, 0, t), t[:, 0:2])
    v = rc.record_slice(row0, 1, a)
    v[...] = -1                                   # a view: writing a record back goes through
    assert (a[:, 2:5] == -1).all() and (a[:, :2] >= 0).all()
    sq = np.zeros((9, 9))
    with pytest.raises(ValueError, match="2 axes of length Tsum = 9"):
        rc.record_slice(row0, 0, sq)
    assert rc.record_slice(row0, 1, sq, axis=1).shape == (9, 3)
    with pytest.raises(ValueError, match="0 axes of length"):
        rc.record_slice(row0, 0, np.zeros((3, 4)))
    with pytest.raises(ValueError, match="axis 0"):
        rc.record_slice(row0, 0, a, axis=0)
    with pytest.raises(IndexError):
        rc.record_slice(row0, 3, a)


def test_degrees_of_freedom_count_transitions_not_rows():
    assert rc.records_df(3, np.array([0, 2, 5, 22, 24, 33])) == 3 + (1 + 2 + 16 + 1 + 8)
    assert rc.records_df(2.5, np.array([0, 40])) == 2.5 + 39      # one record: PGAS's P3 + (T - 1)


def test_seed_rule_against_split():
    rng = np.random.default_rng(3)
    keys = [int(v) for v in rng.integers(0, 2**64 - 1, size=50, dtype=np.uint64, endpoint=True)]
    for E in (1, 2, 5):
        seeds = rc.host_seeds(keys, E)
        assert len(seeds) == 50 and all(len(s) == E for s in seeds)
        for k, s in zip(keys, seeds):
            assert s[0] == k and s[1:] == prng.split(k, E)[1:]
    # child e does not depend on how many records there are, so adding a record leaves the earlier records' seeds alone
    assert rc.host_seeds(keys[:3], 5)[1][:3] == rc.host_seeds(keys[:3], 3)[1]
    assert rc.host_seeds([7], 1) == [[7]]
