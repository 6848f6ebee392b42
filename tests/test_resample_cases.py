"""The resampling cases of tests/resample_cases.py on the CPU: the canonical oracle against exact integer arithmetic on its own quantised
numerators, the edge contracts of DESIGN.md 4.5 for the cases without a positive weight, and the branch census -- every path of the device
search (csrc/pgas_resample.hip.h, resample_search / window_head) must be predicted for at least one workgroup of at least one case.
tests/test_gpu_resample_edges.py runs the same cases on the device."""
import bisect
from fractions import Fraction

import numpy as np
import pytest

from common import canon, canon_model, experiments
import resample_cases as rc

SEED = 12345678
TIE_CAP = 0.01   # share of slots whose index may differ from exact arithmetic, each explained by a tie (tests/test_oracle_canon.py)


def exact_cdf(lw):
    """The CDF the oracle approximates, in exact integers: particle i of segment b weighs q_i 2^kref_b, flushed to zero where the segment
    lies more than 480 binary orders below its group's reference or the group below the top reference (include/pgas_canon.h)."""
    segk, segs, c = canon.segment_partials(lw)
    nseg = len(segk)
    n1 = (nseg + rc.GRP - 1) // rc.GRP
    KG = [max(segk[g * rc.GRP:(g + 1) * rc.GRP]) for g in range(n1)]
    K = max(KG)
    shift = []
    for b in range(nseg):
        kg = KG[b // rc.GRP]
        if segk[b] == -np.inf or segk[b] - kg < -rc.FLUSH or kg - K < -rc.FLUSH:
            shift.append(None)
        else:
            shift.append(int(segk[b] - kg) + int(kg - K) + 960)
    ends, run = [], 0
    for b in range(nseg):
        run += 0 if shift[b] is None else int(segs[b]) << shift[b]
        ends.append(run)
    return c, shift, ends


def exact_count(cdf, N, u, i):
    """#{k : cum_k < (u + i) / N total} in integers."""
    c, shift, ends = cdf
    uf = Fraction(u)
    Q = N * uf.denominator
    rhs = (uf.numerator + i * uf.denominator) * ends[-1]
    b = bisect.bisect_left(ends, -(-rhs // Q))          # first segment with ends[b] Q >= rhs
    if b >= len(ends):
        return N
    before = ends[b - 1] if b else 0
    den = Q << shift[b]
    thr = -(-(rhs - before * Q) // den)                 # c_k < (rhs - before Q) / den  <=>  c_k < ceil(...)
    seg = c[b * rc.SEG:min(N, (b + 1) * rc.SEG)]
    return b * rc.SEG + int(np.searchsorted(seg, np.uint64(thr), side="left"))


def cum_share(cdf, k):
    c, shift, ends = cdf
    b = k // rc.SEG
    before = ends[b - 1] if b else 0
    return float(Fraction(before + (0 if shift[b] is None else int(c[k]) << shift[b]), ends[-1]))


def tie_share(name):
    """Share of the checked slots (first, middle and last 4096) where the oracle's index differs from exact arithmetic; asserts that every
    such slot is a tie: U_i within 1e-9 of every CDF value between the two indices (the criterion of tests/test_oracle_canon.py)."""
    lw, N, u = rc.case(name)
    segk, segs, c = canon.segment_partials(lw)
    cdf = exact_cdf(lw)
    span = min(N, 4096)
    nbad = ntot = 0
    for i0 in sorted({0, max(0, min(N // 2 - 1000, N - span)), N - span}):
        got = canon.resample_range(segk, segs, c, N, u, i0, i0 + span)
        assert np.all(np.diff(got) >= 0)
        for j in range(span):
            exp = min(exact_count(cdf, N, u, i0 + j), N - 1)
            if got[j] != exp:
                lo, hi = sorted((int(got[j]), exp))
                Ui = (u + (i0 + j)) / N
                assert abs(cum_share(cdf, lo) - Ui) < 1e-9 and abs(cum_share(cdf, hi - 1) - Ui) < 1e-9, (name, i0 + j, got[j], exp)
                nbad += 1
        ntot += span
    return nbad / ntot


VALID_NAMES = tuple(n for n in rc.NAMES if n not in rc.EMPTY_NAMES)


@pytest.mark.parametrize("name", VALID_NAMES)
def test_oracle_against_exact_arithmetic(name):
    share = tie_share(name)
    print(f"tie share {name}: {share:.5f}")
    assert share <= TIE_CAP


@pytest.mark.parametrize("name", rc.EMPTY_NAMES)
def test_edge_contracts_without_a_positive_weight(name):
    """no positive weight -> a_i = i, reference ancestor N - 1, final index N - 1."""
    lw, N, u = rc.case(name)
    segk, segs, c = canon.segment_partials(lw)
    assert np.array_equal(canon.resample_range(segk, segs, c, N, u, 0, N), np.arange(N))
    pb = experiments.smo_pgas(T=4)
    cm = canon_model(pb, N)
    assert cm.final_index(SEED, lw) == N - 1
    A, S = experiments.initial_params(pb)
    LS, LSinv, cS = cm.chol_parts(S)
    x = cm.init_state(SEED, pb.init_state_mean, np.linalg.cholesky(pb.init_state_cov), pb.X_true[0])
    for corrected in (False, True):
        cm.set_corrected(corrected)
        lwn, xn, anc = cm.step(1, SEED, x, lw, A, LS, LSinv, cS, pb.X_true[1])
        assert np.array_equal(anc, np.arange(N)) and anc[-1] == N - 1
        assert np.array_equal(xn[-1], pb.X_true[1])


@pytest.mark.parametrize("name", [n for n in rc.NAMES if n.startswith("with_nan")])
def test_nan_weights_are_ignored(name):
    """a NaN weight takes no part -- the same ancestors as with -inf in its place."""
    lw, N, u = rc.case(name)
    assert np.isnan(lw).sum() > rc.SEG
    a = canon.resample_range(*canon.segment_partials(lw), N, u, 0, N)
    b = canon.resample_range(*canon.segment_partials(np.where(np.isnan(lw), -np.inf, lw)), N, u, 0, N)
    assert np.array_equal(a, b)
    assert not np.isnan(lw[a]).any() and np.all(np.diff(a) >= 0)
    cm = canon_model(experiments.smo_pgas(T=4), N)
    assert cm.final_index(SEED, lw) == cm.final_index(SEED, np.where(np.isnan(lw), -np.inf, lw))


def test_case_sizes_and_shapes():
    sizes = {rc.case(n)[1] for n in rc.NAMES if n.startswith(("mild", "flat"))}
    assert sizes >= set(rc.SIZES)
    for n in rc.NAMES:
        lw, N, u = rc.case(n)
        assert lw.shape == (N,) and 0.0 < u < 1.0 and not np.any(lw == np.inf)
        assert np.array_equal(lw, rc.case(n)[0], equal_nan=True), "cases are deterministic"


def test_census_covers_every_branch():
    """The union of the case censuses contains every path of the device search; the cases named after a branch show that branch."""
    seen, per = set(), {}
    for n in rc.NAMES:
        lw, N, u = rc.case(n)
        cen = rc.census(lw, u)
        per[n] = cen
        b = rc.branches(cen)
        seen |= b
        print(f"census {n}: workgroups, valid, max ngw, !covered, ns = {rc.summary(cen)}")
        # ns == 0 cannot occur under a valid CDF: the segment the first threshold falls into always moved the running maximum
        assert not cen["valid"].all() or cen["ns"].min() >= 1, n
    missing = [b for b in rc.BRANCHES if b not in seen]
    assert not missing, f"no case reaches {missing}"
    for k in range(1, 10):
        assert per[f"staged_{k}@{rc.N_MID}"]["ns"][0] == k
    assert per[f"staged_ulp@{rc.N_MID}"]["ns"][0] > rc.NCAND
    # staged_flushed: five light segments, the heavy one, and one source segment that is flushed (non-empty, scale 0), staged with them
    lw, N, u = rc.case(f"staged_flushed@{rc.N_MID}")
    segk, segs, _ = canon.segment_partials(lw)
    cm = rc.upper(segk, segs)[0]
    moved = np.nonzero(cm > np.concatenate([[0.0], cm[:-1]]))[0]
    assert per[f"staged_flushed@{rc.N_MID}"]["ns"][0] == len(moved) == 7
    assert sum(1 for b in moved if segs[b] > 0 and segk[:rc.GRP].max() - segk[b] > rc.FLUSH) == 1
    for n in rc.EMPTY_NAMES:
        assert not per[n]["valid"].any()
    assert not per[f"light_prefix@{1 << 21}"]["covered"][0] and not per[f"far_pair@{(1 << 20) + 1}"]["covered"][0]
    assert per["one_plus_tail@200000"]["ns"].max() > rc.NCAND
    big = per[f"one_plus_tail@{(1 << 20) + 1}"]
    assert big["ns"].max() > rc.NCAND and 4 < big["ngw"].max() <= rc.WIN_GRP
    er = per[f"empty_runs@{rc.N_ER}"]
    assert 4 < er["ngw"].max() <= rc.WIN_GRP and er["ns"].max() <= rc.NCAND, "a window of many groups searched through staged candidates"
    # the flush boundary: segments exactly 480 (kept) and 481 (flushed) binary orders below their group, groups below the top
    lw, N, u = rc.case("stairs(700)@262000")
    segk = canon.segment_partials(lw)[0]
    assert segk[0] - segk[5] == 480 and segk[0] - segk[6] == 481
    assert segk[0] - segk[128:192].max() == 480 and segk[0] - segk[192:].max() == 481


def test_design_table_matches_the_census():
    """DESIGN.md section 6 prints the census per case; the rows there are the ones resample_cases.table_rows() generates."""
    import os

    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md"), encoding="utf-8").read()
    rows = rc.table_rows()
    assert len(rows) == len(rc.NAMES)
    missing = [r for r in rows if r not in doc]
    assert not missing, "DESIGN.md section 6 is out of date; rows to paste:\n" + "\n".join(missing)
