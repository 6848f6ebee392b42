"""The judges of tests/mniw_cases.py can fail: on two correct fp64 factorisations they stay near 1, on each planted fault they exceed the
limit that tests/test_gpu_mniw_edges.py holds the HIP kernels to.  CPU only.

The packed layout (csrc/pgas_marginal.hip.h) is restated once, in mniw_cases' docstring and unpack / pack; test_packed_layout pins it."""
import math

import numpy as np
import pytest

import mniw_cases as mc

SIZES = (1, 15, 41, 62)


def _case(name, M, seed=0, nv=1):
    eta1, phi, eta0 = mc.family(name, M, seed, nv)
    return eta1, phi, eta0, mc.augmented(eta1, phi, eta0)


def test_packed_layout():
    """Row-major lower triangle of (M + 1 + nv) rows, 1 / L_kk on the diagonal, row M = v, rows M + 1 + u = w_u, corner ignored."""
    M, nv = 3, 2
    packed = np.arange(1.0, mc.tri(M + 1 + nv) + 1)
    rows = mc.unpack(packed, M, nv)
    assert rows.shape == (6, 3)
    assert rows[:3].tolist() == [[1, 0, 0], [2, 3, 0], [4, 5, 6]]
    assert rows[3].tolist() == [7, 8, 9] and rows[4].tolist() == [11, 12, 13] and rows[5].tolist() == [16, 17, 18]   # 10, 14, 15, 19 ... : the corner
    again = mc.pack(rows, M, nv)
    keep = np.ones(packed.size, bool)
    keep[[9, 13, 14, 18, 19, 20]] = False
    assert np.array_equal(again[keep], packed[keep]) and not again[~keep].any()
    # a factor by hand: eta1 = [[4, 2], [2, 5]] = L L^T, L = [[2, 0], [1, 2]]; phi = (2, 3) -> v = (1, 1); eta0 = (4, 6) -> w = (2, 2)
    packed = np.array([0.5, 1.0, 0.5, 1.0, 1.0, 0.0, 2.0, 2.0, 0.0, 0.0])
    B = mc.augmented(np.array([[4.0, 2.0], [2.0, 5.0]]), np.array([2.0, 3.0]), np.array([4.0, 6.0]))
    assert mc.backward_ratio(B, packed, 2) == 0.0
    assert max(mc.scalar_ratios(packed, 2.0, 4.0, 8.0, 2 * math.log(4.0), 2).values()) == 0.0
    assert mc.scalar_ratios(packed, 2.0, 4.0, 8.0, 2 * math.log(4.0) * (1 + 2.0 ** -40), 2)["logdet"] > mc.SCALAR_LIMIT


def test_families_are_what_they_claim():
    for name in mc.FAMILIES:
        for M in SIZES:
            eta1, phi, eta0 = mc.family(name, M, 0)
            again = mc.family(name, M, 0)
            assert np.array_equal(eta1, eta1.T) and all(np.array_equal(a, b) for a, b in zip((eta1, phi, eta0), again))
            assert np.all(np.linalg.eigvalsh(eta1 * 2.0 ** (-200 if name == "scaled_up" else 200 if name == "scaled_down" else 0)) > 0)
    cond = {name: np.linalg.cond(mc.family(name, 62, 0)[0]) for name in mc.FAMILIES}
    assert cond["suite"] < 1e3 and 1e8 < cond["graded"] < 1e10 and 1e8 < cond["graded_rev"] < 1e10 and cond["near_singular"] > 1e11
    assert 1e3 < mc.scaled_condition(mc.family("graded", 62, 0)[0]) < 1e5
    a, phi, eta0 = mc.pivot_sweep()
    assert a.size == 4096 and np.all(a >= 2.0 ** -600) and np.all(a < 2.0 ** 601)
    m, e = np.frexp(a)
    assert np.sum(m == 0.5) >= 400 and np.sum((m == 0.5) & (e % 2 == 1)) >= 100 and np.sum((m == 0.5) & (e % 2 == 0)) >= 100   # powers of 4 and of 2
    assert np.sum(m == 0.5 + 2.0 ** -53) >= 400 and np.sum(m == 1.0 - 2.0 ** -53) >= 400                                      # and their neighbours


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", mc.FAMILIES)
def test_correct_factorisations_stay_near_one(name, M):
    """LAPACK's factor and the NumPy right-looking emulation: backward ratio <= 1.5 (1.35 measured over these families, plus slack for
    other seeds), the scalars well within their limit; the forward check within its limit where it applies."""
    eta1, phi, eta0, B = _case(name, M)
    packed, c, m, q, logdet = mc.emulate(eta1, phi, eta0)
    assert mc.backward_ratio(B, mc.lapack_packed(eta1, phi, eta0), M) <= 1.5
    assert mc.backward_ratio(B, packed, M) <= 1.5
    assert max(mc.scalar_ratios(packed, c, m, q, logdet, M).values()) <= 1.0
    if M >= 15:
        fe, kappa = mc.forward_errors(eta1, phi, eta0, c, m, q, logdet)
        if kappa <= mc.FORWARD_MAX_KAPPA:
            assert max(fe.values()) <= 0.05, fe


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", mc.FAMILIES)
def test_a_dropped_newton_step_is_seen(name, M):
    """Every reciprocal pivot off by 2^-45 (v_rsq_f64 plus ONE Newton step): ratio 256 / (j + 2) on the diagonal, 128 at the first pivot."""
    eta1, phi, eta0, B = _case(name, M)
    packed = mc.emulate(eta1, phi, eta0, rsqrt=lambda a: (1.0 / math.sqrt(a)) * (1.0 + 2.0 ** -45))[0]
    assert mc.backward_ratio(B, packed, M) > 100.0 > mc.BACKWARD_LIMIT


@pytest.mark.parametrize("M", SIZES[1:])
@pytest.mark.parametrize("name", mc.FAMILIES)
def test_planted_faults_exceed_the_backward_limit(name, M):
    eta1, phi, eta0, B = _case(name, M)
    good = mc.emulate(eta1, phi, eta0)[0]
    rows = mc.unpack(good, M)
    # one entry of the first column 8 ulp off (the one with the smallest mantissa, where 8 ulp are 16 u of it: ratio >= (16 - 2) / 2)
    i = 1 + int(np.argmin(np.frexp(np.abs(rows[1:, 0]))[0]))
    bad = rows.copy()
    for _ in range(8):
        bad[i, 0] = np.nextafter(bad[i, 0], math.inf)
    assert mc.backward_ratio(B, mc.pack(bad, M), M) > mc.BACKWARD_LIMIT
    # (the bound grows with the column: the same 8 ulp in column j are within (j + 2) u of a long sum, as they are for a correct kernel)
    # two rows of the triangle swapped (their common columns)
    bad = rows.copy()
    r = M // 2
    bad[[r, r + 1], :r] = bad[[r + 1, r], :r]
    assert mc.backward_ratio(B, mc.pack(bad, M), M) > mc.BACKWARD_LIMIT
    # w of another particle
    other = mc.emulate(*mc.family(name, M, 1))[0]
    bad = rows.copy()
    bad[M + 1] = mc.unpack(other, M)[M + 1]
    assert mc.backward_ratio(B, mc.pack(bad, M), M) > mc.BACKWARD_LIMIT
    # a non-finite factor never passes
    bad = rows.copy()
    bad[M - 1, M - 1] = math.nan
    assert mc.backward_ratio(B, mc.pack(bad, M), M) == math.inf


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", mc.FAMILIES)
def test_scalar_faults_exceed_their_limit(name, M):
    eta1, phi, eta0, _ = _case(name, M)
    packed, c, m, q, logdet = mc.emulate(eta1, phi, eta0)
    ok = mc.scalar_ratios(packed, c, m, q, logdet, M)
    assert max(ok.values()) <= 1.0
    swapped = mc.scalar_ratios(packed, m, c, q, logdet, M)                  # m and c exchanged
    assert swapped["c"] > mc.SCALAR_LIMIT and swapped["m"] > mc.SCALAR_LIMIT
    rows = mc.unpack(packed, M)
    k = int(np.argmax(np.abs(rows[M])))                                     # one term of each sum dropped
    assert mc.scalar_ratios(packed, c - rows[M, k] ** 2, m, q, logdet, M)["c"] > mc.SCALAR_LIMIT
    assert mc.scalar_ratios(packed, c, m - rows[M, k] * rows[M + 1, k], q, logdet, M)["m"] > mc.SCALAR_LIMIT or rows[M + 1, k] == 0.0
    k = int(np.argmax(np.abs(rows[M + 1])))
    assert mc.scalar_ratios(packed, c, m, q - rows[M + 1, k] ** 2, logdet, M)["q"] > mc.SCALAR_LIMIT
    k = int(np.argmax(np.abs(np.log(np.diag(rows[:M])))))
    if rows[k, k] != 1.0:
        assert mc.scalar_ratios(packed, c, m, q, logdet + 2.0 * math.log(rows[k, k]), M)["logdet"] > mc.SCALAR_LIMIT


def test_several_components():
    """nv > 1: rows M + 1 + u, m a vector, Q a matrix."""
    M, nv = 7, 3
    eta1, phi, eta0, B = _case("graded", M, nv=nv)
    packed, c, m, Q, logdet = mc.emulate(eta1, phi, eta0)
    assert mc.backward_ratio(B, packed, M, nv) <= 1.5
    assert max(mc.scalar_ratios(packed, c, m, Q, logdet, M, nv).values()) <= 1.0
    fe, kappa = mc.forward_errors(eta1, phi, eta0, c, m, Q, logdet)
    assert max(fe.values()) <= 0.5 and kappa < 1e5
    assert mc.scalar_ratios(packed, c, m[::-1].copy(), Q, logdet, M, nv)["m"] > mc.SCALAR_LIMIT
    Qt = Q.copy()
    Qt[0, 1] = Qt[1, 0] = Q[0, 2]
    assert mc.scalar_ratios(packed, c, m, Qt, logdet, M, nv)["q"] > mc.SCALAR_LIMIT


def test_general_input_form_is_exact():
    """P + scale T + R formed without rounding; the allowance is 2 u (|P| + |scale T| + |R|)."""
    M = 15
    eta1, phi, eta0, _ = _case("graded", M)
    rng = np.random.default_rng(3)
    P1 = np.diag(rng.uniform(0.5, 1.5, M))
    G = 0.1 * rng.standard_normal((M, M))
    R1 = G @ G.T
    Bx, slack = mc.exact_affine(np.tril(P1), 0.999, np.tril(eta1), np.tril(R1))
    val = np.array([[float(mc.Fraction(int(v), 1 << Bx.shift)) for v in r] for r in Bx.ints])
    fp = np.tril(P1 + 0.999 * eta1 + R1)
    assert np.all(np.abs(val - fp) <= 3 * mc.U * (np.abs(P1) + np.abs(0.999 * eta1) + np.abs(R1)))
    sl = np.array([[float(mc.Fraction(int(v), 1 << slack.shift)) for v in r] for r in slack.ints])
    assert np.allclose(sl, 2 * mc.U * np.tril(np.abs(P1) + np.abs(0.999 * eta1) + np.abs(R1)), rtol=1e-12, atol=0)
    # the matrix formed in fp64, then factorised, judged against the exact one with the allowance in the bound
    P0, R0 = rng.standard_normal(M), rng.standard_normal(M)
    packed = mc.emulate(mc.sym(fp), phi, P0 + 0.999 * eta0 + R0)[0]
    Ball, Sall = mc.augmented_affine(P1, P0, 0.999, eta1, eta0, phi, R1, R0)
    assert Ball.ints.shape == Sall.ints.shape == (M + 2, M) and not any(Sall.ints[M])
    assert mc.backward_ratio(Ball, packed, M, slack=Sall) <= 1.5
    wrong = mc.emulate(mc.sym(np.tril(P1 + eta1 + R1)), phi, P0 + 0.999 * eta0 + R0)[0]          # the forgetting factor forgotten
    assert mc.backward_ratio(Ball, wrong, M, slack=Sall) > mc.BACKWARD_LIMIT


def test_the_two_exact_routes_agree():
    """Python integers against mpmath at 400 bits: the same ratio to the last digit, with and without a fault.  A missing mpmath is an
    error here, not a skip: a judge that does not run hides failures."""
    import mpmath  # noqa: F401

    for name, M in (("graded", 15), ("near_singular", 41), ("scaled_down", 5)):
        eta1, phi, eta0, B = _case(name, M)
        for rs in (None, lambda a: (1.0 / math.sqrt(a)) * (1.0 + 2.0 ** -45)):
            packed = mc.emulate(eta1, phi, eta0, rsqrt=rs)[0]
            a, b = mc.backward_ratio(B, packed, M), mc.backward_ratio(B, packed, M, route="mpmath")
            assert a == b and a > 0.0


def test_reference_solves():
    """The >= 256-bit references against fp64 on a well-conditioned matrix, and the stored-factor bound against a perturbed solve."""
    M = 15
    eta1, phi, eta0, _ = _case("suite", M)
    c, m, Q, logs = mc.reference_solve(eta1, phi, eta0)
    L = np.linalg.cholesky(eta1)
    v, w = np.linalg.solve(L, phi), np.linalg.solve(L, eta0)
    assert abs(c - v @ v) < 1e-12 * c and abs(m[0] - w @ v) < 1e-12 * math.sqrt(c * Q[0, 0]) and abs(Q[0, 0] - w @ w) < 1e-12 * Q[0, 0]
    assert np.allclose(logs, 2 * np.log(np.diag(L)), rtol=0, atol=1e-12)
    packed = mc.emulate(eta1, phi, eta0)[0]
    phi2 = np.random.default_rng(1).standard_normal(M)
    c2, m2, v2 = mc.reference_trisolve(packed, phi2, M)
    vf = np.linalg.solve(L, phi2)
    dc, dm = mc.trisolve_bounds(packed, v2, M)
    assert np.allclose(v2, vf, rtol=1e-10, atol=1e-12) and 0 < dc < 1e-12 * c2 and 0 < dm[0] < 1e-10
    assert abs(vf @ vf - c2) < 50 * dc                           # another fp64 solve (of a factor a rounding away) is within reach of the bound
    assert abs(c2 * (1 + 1e-9) - c2) > dc                        # and an error of 1e-9 is far outside it


def test_bad_matrices_fail_exactly_where_they_say():
    """The pivot named by bad_matrix is the first non-positive one in exact elimination order (checked in fp64 on the rows before it)."""
    for M in (5, 17, 62):
        for k in sorted({0, 3, 4, 15, 16, M - 1} & set(range(M))):
            for kind in ("zero", "minus", "coupled"):
                A = mc.bad_matrix(kind, M, k)
                assert np.array_equal(A, A.T)
                if k:
                    np.linalg.cholesky(A[:k, :k])          # the leading block is positive definite
                with pytest.raises(np.linalg.LinAlgError):
                    np.linalg.cholesky(A[:k + 1, :k + 1])
            for kind in ("nan", "inf"):
                A = mc.bad_matrix(kind, M, k)
                assert np.sum(~np.isfinite(np.tril(A))) == 1
