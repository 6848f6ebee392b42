"""Inputs and exact-arithmetic judges for the MNIW solve kernels (csrc/pgas_marginal.hip.h: k_mniw_solve_mfma<NT>, k_mniw_solve<MT>,
k_mniw_solve_wide, k_mniw_trisolve, k_mniw_trisolve_wide).

Input families: seeded symmetric positive definite eta1 with the two right-hand sides phi and eta0, from the well-conditioned
construction of tests/test_gpu_marginal.py up to the graded diagonals (1e-3 ... 1e6, the Toy prior's range) and the nearly singular
matrices the filter builds at late times.

Judges: the kernels return their own packed factor, so they are judged by what that factor satisfies in EXACT arithmetic, not by a
second fp64 computation whose own error grows with the condition number.  Every double is an integer times a power of two, so sums of
products of doubles are evaluated exactly in Python integers.

The packed layout, restated once from the header comments of csrc/pgas_marginal.hip.h: the row-major lower triangle of an (R, R)
matrix, R = M + 1 + nv, element (r, c) at r (r + 1) / 2 + c.  Rows 0 ... M-1 hold the Cholesky factor L of eta1 with 1 / L_kk ON THE
DIAGONAL; row M holds v = L^-1 phi, row M + 1 + u holds w_u = L^-1 eta0[:, u] (nv = 1: row M + 1 = w).  The corner (columns >= M) is
not part of the format: one kernel leaves zeros there, the others the Schur complement; nothing reads it.

A plain module (no fixtures, no pytest hooks, NumPy only); shared by tests/test_mniw_cases.py (CPU) and tests/test_gpu_mniw_edges.py."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                       # unit roundoff of fp64
BACKWARD_LIMIT, SCALAR_LIMIT, FORWARD_LIMIT, FORWARD_MAX_KAPPA = 4.0, 2.0, 1.0, 1e5
FAMILIES = ("suite", "graded", "graded_rev", "near_singular", "scaled_up", "scaled_down")


# ------------------------------------------------------------------------------------------ input families
def sym(A):
    L = np.tril(A)
    return L + np.tril(A, -1).T


def family(name, M, seed, nv=1):
    """(eta1 (M, M) symmetric bit for bit, phi (M,), eta0 (M,) or (M, nv) when nv > 1); deterministic in (name, M, seed, nv)."""
    rng = np.random.default_rng([FAMILIES.index(name), M, seed, nv])
    B = rng.standard_normal((M, 3))
    BB = B @ B.T
    if name == "suite":                 # tests/test_gpu_marginal.py: condition number ~ 1.5e2 at M = 62
        eta1 = BB + np.diag(rng.uniform(0.5, 1.5, M))
    elif name in ("graded", "graded_rev", "scaled_up", "scaled_down"):
        d = np.logspace(-3, 6, M)       # the Toy prior's diag(P1): 2.7e-3 ... 9.9e5
        eta1 = np.diag(d[::-1] if name == "graded_rev" else d) + 0.999 ** 40 * BB
        if name == "scaled_up":
            eta1 = eta1 * 2.0 ** 200
        elif name == "scaled_down":
            eta1 = eta1 * 2.0 ** -200
    elif name == "near_singular":       # rank 3 plus 1e-10: condition number ~ 1e12
        eta1 = 1e-10 * np.diag(rng.uniform(0.5, 1.5, M)) + BB
    else:
        raise ValueError(name)
    phi = rng.standard_normal(M)
    eta0 = rng.standard_normal((M, nv) if nv > 1 else M)
    return sym(eta1), phi, eta0


def pivot_sweep(n=4096, seed=0):
    """M = 1: n pivots a = m 2^e, e in [-600, 600], m random in [1, 2) plus the exact powers of two and four with their fp64 neighbours
    (m = 1, 1 + 2^-52, 2 - 2^-52 at even and odd e); right-hand sides in [1, 2) so that every result stays a normal number."""
    rng = np.random.default_rng([seed, n])
    e = rng.integers(-600, 601, n)
    m = 1.0 + rng.random(n)
    edge = np.array([1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52])
    ee = np.append(np.arange(-600, 600, 3), 600)      # both parities, both ends of the range
    ne = min(n // 2, 3 * ee.size)
    m[:ne] = edge[np.arange(ne) % 3]
    e[:ne] = ee.repeat(3)[:ne]
    a = np.ldexp(m, e)
    return a, 1.0 + rng.random(n), 1.0 + rng.random(n)


def scaled_condition(eta1):
    """kappa_s: the fp64 2-norm condition number of D^-1/2 eta1 D^-1/2, D = diag(eta1) (powers of two rounded into D keep it finite)."""
    d = np.ldexp(1.0, -np.round(np.log2(np.diag(eta1)) / 2).astype(int))
    return float(np.linalg.cond(eta1 * d[:, None] * d[None, :]))


# ------------------------------------------------------------------------------------------ the packed layout
def tri(r):
    return r * (r + 1) // 2


def unpack(packed, M, nv=1):
    """(R, M) array: rows 0 ... M-1 the lower triangle (diagonal = 1 / L_kk, zeros above it), rows M ... R-1 the right-hand sides."""
    R = M + 1 + nv
    packed = np.asarray(packed)
    assert packed.shape == (tri(R),), (packed.shape, R)
    out = np.zeros((R, M), dtype=packed.dtype)
    for r in range(R):
        k = min(r + 1, M)
        out[r, :k] = packed[tri(r):tri(r) + k]
    return out


def pack(rows, M, nv=1):
    """Inverse of unpack (the corner is left zero)."""
    R = M + 1 + nv
    packed = np.zeros(tri(R))
    for r in range(R):
        k = min(r + 1, M)
        packed[tri(r):tri(r) + k] = rows[r, :k]
    return packed


def augmented(eta1, phi, eta0):
    """The (R, M) matrix B the kernels factorise: the lower triangle of eta1, then phi^T, then the columns of eta0 as rows."""
    M = eta1.shape[0]
    return np.vstack([np.tril(eta1), np.reshape(phi, (1, M)), np.reshape(eta0, (M, -1)).T])


# ------------------------------------------------------------------------------------------ exact arithmetic on doubles
class Exact:
    """An array of exact dyadic numbers: value = ints * 2^-shift, ints an object array of Python integers."""

    def __init__(self, ints, shift):
        self.ints, self.shift = ints, shift


def _min_exp(*arrays):
    lo = 0
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        if not np.all(np.isfinite(a)):
            raise ValueError("exact arithmetic needs finite inputs")
        nz = a[a != 0.0]
        if nz.size:
            lo = min(lo, int(np.frexp(nz)[1].min()))
    return lo


def exact(a, shift=None):
    """The doubles of a as Exact, with a common shift (default: the smallest that represents every element)."""
    a = np.asarray(a, dtype=np.float64)
    if shift is None:
        shift = 53 - _min_exp(a)
    f, e = np.frexp(a)
    mant = np.ldexp(f, 53).astype(np.int64)          # exact: |f| < 1 has 53 significant bits
    flat = [int(m) << (int(x) - 53 + shift) if m else 0 for m, x in zip(mant.ravel(), e.ravel())]   # a negative count raises
    out = np.empty(a.size, dtype=object)
    out[:] = flat
    return Exact(out.reshape(a.shape), shift)


def exact_affine(P, scale, T, R=None):
    """P + scale T (+ R) without any rounding (the general input form of the kernels), and 2 u (|P| + |scale T| + |R|), the allowance
    for the at most two roundings the kernel makes in forming it, as a second Exact of the same shift."""
    sh = 53 - _min_exp(P, T, scale, R if R is not None else 0.0)
    p, t, s = exact(P, sh), exact(T, sh), exact(scale, sh)
    one = 1 << sh
    val = p.ints * one + t.ints * s.ints.item()
    mag = abs(p.ints) * one + abs(t.ints * s.ints.item())
    if R is not None:
        r = exact(R, sh)
        val = val + r.ints * one
        mag = mag + abs(r.ints) * one
    return Exact(val, 2 * sh), Exact(mag, 2 * sh + 52)      # 2 u = 2^-52


def _stack(parts):
    sh = max(p.shift for p in parts)
    return Exact(np.vstack([np.atleast_2d(p.ints) * (1 << (sh - p.shift)) for p in parts]), sh)


def augmented_affine(P1, P0, scale, T1, T0, phi, R1=None, R0=None):
    """The exact augmented input of the general form, eta1 = P1 + scale T1 (+ R1), eta0 = P0 + scale T0 (+ R0), as (B, slack) for
    backward_ratio: the phi row is handed over as it is (no allowance), the others get 2 u (|P| + |scale T| + |R|)."""
    M = P1.shape[0]
    col = lambda a: None if a is None else np.reshape(a, (M, -1)).T          # noqa: E731
    e1, s1 = exact_affine(np.tril(P1), scale, np.tril(T1), None if R1 is None else np.tril(R1))
    e0, s0 = exact_affine(col(P0), scale, col(T0), col(R0))
    ph = exact(np.reshape(phi, (1, M)))
    return _stack([e1, ph, e0]), _stack([s1, Exact(np.zeros((1, M), dtype=object), 0), s0])


def _as_exact(B):
    return B if isinstance(B, Exact) else exact(B)


# ------------------------------------------------------------------------------------------ judge 1: componentwise backward error
def backward_ratio(B, packed, M, nv=1, slack=None, route="int"):
    """Worst ratio of the componentwise backward error of the augmented factorisation to its bound (Higham, Accuracy and Stability of
    Numerical Algorithms, Thm 10.3; the substitution rows obey the same relation): for i >= j, j < M,
        | B_ij - sum_{k<=j} L_ik L_jk |  <=  gamma_{j+2} sum_{k<=j} |L_ik L_jk|,    gamma_k = k u,
    evaluated exactly.  The packed diagonal holds d_j = 1 / L_jj, so the relation is multiplied through by d_j (by d_j^2 on the
    diagonal) and L_jj is taken to be exactly 1 / d_j:
        i > j:  | d_j (B_ij - sum_{k<j} L_ik L_jk) - L_ij |      <=  (j+2) u (d_j sum_{k<j} |L_ik L_jk| + |L_ij|)
        i = j:  | d_j^2 (B_jj - sum_{k<j} L_jk^2) - 1 |          <=  (j+2) u (d_j^2 sum_{k<j} L_jk^2 + 1).
    B is the exact (R, M) input (doubles, or Exact from exact_affine); slack, if given, is an Exact bound on what the kernel's own rounding
    of the input may add to |B_ij| (added to the right-hand side, times d_j or d_j^2).  The condition number does not enter.
    A non-finite factor returns inf.  route = "mpmath" evaluates the same expressions at 400 bits instead (a cross-check)."""
    rows = unpack(packed, M, nv)
    if not np.all(np.isfinite(rows)):
        return math.inf
    if route == "mpmath":
        return _backward_ratio_mpmath(B, rows, M, slack)
    Bx = _as_exact(B)
    Lx = exact(rows)
    L, sL, sB = Lx.ints, Lx.shift, Bx.shift
    A = abs(L)
    k = 0 if slack is None else slack.shift - sB      # ratios below are num / den with both sides times 2^(53 + k)
    assert k >= 0
    wn, wd = 0, 1                                     # the worst ratio so far, as a fraction of integers
    for j in range(M):
        d = abs(int(L[j, j]))
        below = np.arange(j, L.shape[0])
        dot = L[below, :j].dot(L[j, :j]) if j else np.zeros(below.size, dtype=object)          # scale 2 sL
        adot = A[below, :j].dot(A[j, :j]) if j else np.zeros(below.size, dtype=object)
        # rows i > j at scale sB + 3 sL: d (B_ij - dot) - L_ij  against  d adot + |L_ij|
        lhs = abs(d * ((Bx.ints[below, j] << (2 * sL)) - (dot << sB)) - (L[below, j] << (sB + 2 * sL)))
        bound = (d * adot << sB) + (A[below, j] << (sB + 2 * sL))
        ext = d * (slack.ints[below, j] << (2 * sL)) if slack is not None else None
        # row j itself (entry 0 of `below`) at scale sB + 4 sL: d^2 (B_jj - dot) - 1  against  d^2 adot + 1
        lhs[0] = abs(d * d * ((int(Bx.ints[j, j]) << (2 * sL)) - (int(dot[0]) << sB)) - (1 << (sB + 4 * sL)))
        bound[0] = (d * d * int(adot[0]) << sB) + (1 << (sB + 4 * sL))
        if slack is not None:
            ext[0] = d * d * (int(slack.ints[j, j]) << (2 * sL))
        for n_ in range(below.size):
            num = int(lhs[n_]) << (53 + k)
            if not num:
                continue
            den = (j + 2) * (int(bound[n_]) << k) + ((int(ext[n_]) << 53) if slack is not None else 0)
            if den == 0:
                return math.inf
            if num * wd > wn * den:
                wn, wd = num, den
    return float(Fraction(wn, wd))


def _backward_ratio_mpmath(B, rows, M, slack):
    import mpmath

    mp = mpmath.mp.clone()
    mp.prec = 400

    def conv(x):
        if isinstance(x, Exact):
            return [[mp.mpf(int(v)) / mp.mpf(2) ** x.shift for v in r] for r in x.ints]
        return [[mp.mpf(float(v)) for v in r] for r in np.asarray(x, dtype=np.float64)]

    Bm, L = conv(B), conv(rows)
    S = conv(slack) if slack is not None else None
    worst = mp.mpf(0)
    for j in range(M):
        d = L[j][j]
        gam = mp.mpf(j + 2) * mp.mpf(2) ** -53
        for i in range(j, len(L)):
            dot = mp.fsum(L[i][k] * L[j][k] for k in range(j))
            adot = mp.fsum(abs(L[i][k] * L[j][k]) for k in range(j))
            if i == j:
                lhs, bound, f = abs(d * d * (Bm[j][j] - dot) - 1), d * d * adot + 1, d * d
            else:
                lhs, bound, f = abs(d * (Bm[i][j] - dot) - L[i][j]), d * adot + abs(L[i][j]), d
            den = gam * bound + (f * S[i][j] if S is not None else 0)
            if lhs:
                worst = max(worst, lhs / den if den else mp.mpf(10) ** 30)
    return float(worst)


# ------------------------------------------------------------------------------------------ judge 2: the returned scalars
def _dot_ratio(got, x, y, M):
    """|got - x.y| / ((M + 2) u sum |x_k y_k|), x and y Exact integer vectors of one shift; the any-order dot-product bound."""
    got = float(got)
    if not math.isfinite(got):
        return math.inf
    s = int(x.ints.dot(y.ints))
    a = int(abs(x.ints).dot(abs(y.ints)))
    g = Fraction(got) * (1 << (2 * x.shift))
    if a == 0:
        return 0.0 if g == 0 else math.inf
    return float(abs(g - s) / (Fraction(M + 2, 1 << 53) * a))


def scalar_ratios(packed, c, m, q, logdet, M, nv=1):
    """The four returned scalars against exact sums over the factor's OWN rows: c = sum v^2, m_u = sum w_u v, Q_ut = sum w_u w_t (nv = 1:
    m and q scalars), logdet = -2 sum log(1 / L_kk); each error in units of (M + 2) u sum |terms|.  -> dict of worst ratios."""
    rows = unpack(packed, M, nv)
    if not np.all(np.isfinite(rows)):
        return {k: math.inf for k in ("c", "m", "q", "logdet")}
    X = exact(rows[M:])
    row = [Exact(X.ints[r], X.shift) for r in range(1 + nv)]
    m_, q_ = np.reshape(m, (nv,)), np.reshape(q, (nv, nv))
    out = {"c": _dot_ratio(c, row[0], row[0], M),
           "m": max(_dot_ratio(m_[u], row[1 + u], row[0], M) for u in range(nv)),
           "q": max(_dot_ratio(q_[u, t], row[1 + u], row[1 + t], M) for u in range(nv) for t in range(nv))}
    terms = [-2.0 * math.log(rows[k, k]) for k in range(M)]
    asum = math.fsum(abs(t) for t in terms)
    err = abs(float(logdet) - math.fsum(terms))
    out["logdet"] = (0.0 if err == 0.0 else math.inf) if asum == 0.0 else err / ((M + 2) * U * asum)
    if not math.isfinite(float(logdet)):
        out["logdet"] = math.inf
    return out


# ------------------------------------------------------------------------------------------ judge 3: forward errors
def reference_solve(eta1, phi, eta0, bits=512):
    """The reference of forward_errors: a fixed-point Cholesky (Python integers, `bits` fractional bits) of the exact input, scaled
    symmetrically by powers of two so that its diagonal lies in [1/2, 2] -- which leaves c, m, Q unchanged and shifts each log L_kk^2
    by a known multiple of log 2.  -> (c, m (nv,), Q (nv, nv), logs (M,)) rounded to fp64, logs[k] = log L_kk^2."""
    M = eta1.shape[0]
    nv = np.reshape(eta0, (M, -1)).shape[1]
    e = -np.round(np.log2(np.diag(eta1)) / 2).astype(int)              # d_k = 2^e_k
    B = augmented(eta1, phi, eta0)
    sc = B.copy()
    sc[:M] = np.ldexp(np.ldexp(B[:M], e[:, None]), e[None, :])
    sc[M:] = np.ldexp(B[M:], e[None, :])
    sh = 53 - _min_exp(sc)
    F = max(bits, sh)
    A = exact(sc, F).ints
    R = M + 1 + nv
    L = np.zeros((R, M), dtype=object)
    for j in range(M):
        s = (int(A[j, j]) << F) - (int(L[j, :j].dot(L[j, :j])) if j else 0)      # scale 2F
        if s <= 0:
            raise ValueError("not positive definite")
        L[j, j] = math.isqrt(s)                                                  # scale F
        for i in range(j + 1, R):
            t = (int(A[i, j]) << F) - (int(L[i, :j].dot(L[j, :j])) if j else 0)
            L[i, j] = t // int(L[j, j])

    def dot(a, b):
        return float(Fraction(int(L[a].dot(L[b])), 1 << (2 * F)))
    c = dot(M, M)
    m = np.array([dot(M + 1 + u, M) for u in range(nv)])
    Q = np.array([[dot(M + 1 + u, M + 1 + t) for t in range(nv)] for u in range(nv)])
    # log L_kk^2 of the unscaled matrix: L_kk = Ls_kk / d_k
    logs = np.array([2.0 * (math.log(float(Fraction(int(L[k, k]), 1 << F))) - int(e[k]) * math.log(2.0)) for k in range(M)])
    return c, m, Q, logs


def forward_errors(eta1, phi, eta0, c, m, q, logdet):
    """Errors of the returned scalars against reference_solve, in units of (M + 2) u kappa_s: c and q (diagonal of Q) relative to
    themselves, m_u relative to sqrt(c Q_uu), logdet relative to max(1, sum |log L_kk^2|).  -> (dict of ratios, kappa_s).  A loose
    end-to-end check, meaningful for kappa_s <= FORWARD_MAX_KAPPA only; backward_ratio is the sharp one."""
    M = eta1.shape[0]
    rc, rm, rQ, logs = reference_solve(eta1, phi, eta0)
    nv = rm.size
    kap = scaled_condition(eta1)
    unit = (M + 2) * U * kap
    m_, q_ = np.reshape(m, (nv,)), np.reshape(q, (nv, nv))
    out = {"c": abs(float(c) - rc) / (rc * unit),
           "q": max(abs(q_[u, u] - rQ[u, u]) / (rQ[u, u] * unit) for u in range(nv)),
           "m": max(abs(m_[u] - rm[u]) / (math.sqrt(rc * rQ[u, u]) * unit) for u in range(nv)),
           "logdet": abs(float(logdet) - math.fsum(logs)) / (max(1.0, math.fsum(np.abs(logs))) * unit)}
    return out, kap


# ------------------------------------------------------------------------------------------ stored-factor solve
def reference_trisolve(packed, phi, M, nv=1, bits=512):
    """v = L^-1 phi by forward substitution on the packed factor taken as exact input (L_kk = 1 / d_k exactly, so every step is a
    multiplication), results rounded to `bits` fractional bits below the smallest input; then c = v.v and m_u = w_u.v with the stored
    rows w_u.  -> (c, m (nv,), v (M,)) as fp64."""
    rows = unpack(packed, M, nv)
    sh = 53 - _min_exp(rows, phi)
    F = sh + bits
    L = exact(rows, F).ints
    b = exact(phi, F).ints
    v = np.zeros(M, dtype=object)
    for k in range(M):
        t = int(b[k]) - ((int(L[k, :k].dot(v[:k])) >> F) if k else 0)
        v[k] = (t * int(L[k, k])) >> F
    f = lambda x: float(Fraction(int(x), 1 << (2 * F)))   # noqa: E731
    c = f(v.dot(v))
    m = np.array([f(L[M + 1 + u].dot(v)) for u in range(nv)])
    return c, m, np.array([float(Fraction(int(x), 1 << F)) for x in v])


def trisolve_bounds(packed, v, M, nv=1):
    """First-order bounds on the stored-factor solve (Higham Thm 8.5), evaluated in fp64: E = gamma |L^-1| |L| |v| bounds the error of the
    computed v, |dc| <= 2 |v|.E + gamma sum v^2, |dm_u| <= |w_u|.E + gamma sum |w_uk v_k|, gamma = 2 (M + 2) u.  -> (dc, dm (nv,))."""
    rows = unpack(packed, M, nv)
    L = rows[:M].copy()
    L[np.arange(M), np.arange(M)] = 1.0 / np.diag(L)
    gam = 2 * (M + 2) * U
    av = np.abs(v)
    E = gam * (np.abs(np.linalg.inv(L)) @ (np.abs(L) @ av))
    dc = 2 * av @ E + gam * (av @ av)
    dm = np.array([np.abs(rows[M + 1 + u]) @ E + gam * (np.abs(rows[M + 1 + u]) @ av) for u in range(nv)])
    return dc, dm


# ------------------------------------------------------------------------------------------ the kernels' operation order in NumPy
def emulate(eta1, phi, eta0, rsqrt=None):
    """Right-looking elimination of the augmented matrix in fp64, column by column, as the kernels order it (individually rounded
    operations instead of FMAs; 1 / sqrt(pivot) = rsqrt(pivot), default a rounded 1 / sqrt).  -> (packed, c, m, q, logdet)."""
    M = eta1.shape[0]
    nv = np.reshape(eta0, (M, -1)).shape[1]
    R = M + 1 + nv
    A = np.zeros((R, R))
    A[:, :M] = augmented(eta1, phi, eta0)
    rs = rsqrt or (lambda a: 1.0 / math.sqrt(a))
    for k in range(M):
        inv = rs(A[k, k])
        col = A[k + 1:, k] * inv
        A[k + 1:, k] = col
        A[k, k] = inv
        A[k + 1:, k + 1:] -= np.tril(np.outer(col, col))
    packed = pack(A[:, :M], M, nv)
    c = -A[M, M]
    m = -A[M + 1:, M]
    q = -sym(A[M + 1:, M + 1:])
    logdet = -2.0 * math.fsum(math.log(A[k, k]) for k in range(M))
    return (packed, c, m[0], q[0, 0], logdet) if nv == 1 else (packed, c, m, q, logdet)


def lapack_packed(eta1, phi, eta0):
    """LAPACK's factor (numpy.linalg.cholesky) with dot-product forward substitution for the right-hand sides, in the packed layout (the
    diagonal replaced by its rounded reciprocal)."""
    M = eta1.shape[0]
    L = np.linalg.cholesky(eta1)
    rhs = np.vstack([np.reshape(phi, (1, M)), np.reshape(eta0, (M, -1)).T])
    X = np.zeros_like(rhs)
    for k in range(M):
        X[:, k] = (rhs[:, k] - X[:, :k] @ L[k, :k]) / L[k, k]
    rows = np.vstack([np.tril(L), X])
    rows[np.arange(M), np.arange(M)] = 1.0 / np.diag(L)
    return pack(rows, M, rhs.shape[0] - 1)


# ------------------------------------------------------------------------------------------ matrices that are not positive definite
def bad_matrix(kind, M, k, seed=0):
    """A symmetric (M, M) matrix whose elimination fails at pivot k EXACTLY, whatever the rounding of the steps before it:
      zero     a `graded` matrix with row and column k zeroed: every L_kj is 0 times something, the pivot is 0 - 0 = 0
      minus    the same with -1 at (k, k): the pivot is -1
      coupled  A = L L^T, L with small integers below a power-of-two diagonal (1/2 at k), A_kk lowered by 1: the pivot is 1/4 - 1 up to
               the rounding of the reciprocal pivots, so negative
      nan/inf  a `graded` matrix with a NaN / +inf at (k, k - 1) (k = 0: on the diagonal)."""
    eta1 = family("graded", M, 1000 + seed)[0]
    if kind in ("zero", "minus"):
        eta1[k, :] = 0.0
        eta1[:, k] = 0.0
        if kind == "minus":
            eta1[k, k] = -1.0
    elif kind == "coupled":
        rng = np.random.default_rng([7, M, k, seed])
        L = np.tril(rng.integers(-2, 3, (M, M)).astype(np.float64), -1)
        L[np.arange(M), np.arange(M)] = np.ldexp(1.0, rng.integers(0, 3, M))
        L[k, k] = 0.5
        eta1 = L @ L.T          # exact: small integers and quarters
        eta1[k, k] -= 1.0
    elif kind in ("nan", "inf"):
        eta1[k, max(k - 1, 0)] = eta1[max(k - 1, 0), k] = math.nan if kind == "nan" else math.inf
    else:
        raise ValueError(kind)
    return eta1
