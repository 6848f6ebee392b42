"""Named log-weight vectors that drive the device resampling search (csrc/pgas_resample.hip.h, resample_search / window_head) through
every one of its paths, with a BRANCH CENSUS per case: which path each workgroup (1024 resampling slots) is predicted to take.

The census is computed in NumPy from the canonical oracle's own per-segment records (oracle.canon.segment_partials) by restating the
hierarchical CDF of DESIGN.md 4.4 -- it is derived from the CDF, never from the device.  Per workgroup it reports
    valid    the CDF total S is positive and finite (otherwise: identity ancestors)
    ngw      number of groups of 64 segments between the group of the first and of the last threshold (the search window)
    covered  ngw <= 16: the window fits the workgroup's LDS (otherwise the slots go through the global tables one by one)
    ns       number of source segments in [segment of the first threshold, segment of the last threshold] whose running maximum of the
             CDF moves, i.e. the segments that can own a slot (<= 8: staged in passes of two; > 8: per-slot bisection)
A plain module (no fixtures, no pytest hooks); shared by tests/test_resample_cases.py (CPU) and tests/test_gpu_resample_edges.py."""
from __future__ import annotations

import math

import numpy as np

from oracle import canon

SEG, GRP, WIN_GRP, NCAND, FLUSH = 1024, 64, 16, 8, 480.0
LN2 = math.log(2.0)
BRANCHES = ("!valid",) + tuple(f"ns={k}" for k in range(1, NCAND + 1)) + ("ns>8", "ngw<=4", "4<ngw<=16", "!covered")


# ------------------------------------------------------------------------------------------ the hierarchical CDF, restated
def _ks64(v):
    """Inclusive scan of 64 lanes in the canonical order of DESIGN.md 4.4 (Kogge-Stone in rows of 16, then row totals)."""
    v = np.array(v, dtype=np.float64)
    lane = np.arange(64)
    for off in (1, 2, 4, 8):
        t = v.copy()
        sel = (lane % 16) >= off
        t[sel] = v[sel] + v[lane[sel] - off]
        v = t
    t = v.copy()
    sel = ((lane // 16) & 1) == 1
    t[sel] = v[sel] + v[(lane[sel] // 16) * 16 - 1]
    v = t
    t = v.copy()
    t[32:] = v[32:] + v[31]
    return t


def _lvl_scale(k, K):
    with np.errstate(invalid="ignore"):
        d = np.asarray(k, dtype=np.float64) - K
    ok = d >= -FLUSH                       # False for -inf and NaN (empty members, everything empty)
    return np.where(ok, np.exp2(np.where(ok, d, 0.0)), 0.0)


def upper(segk, segs):
    """Levels two and three of the CDF from the per-segment records: cm[b] = running maximum of the CDF numerator at the end of
    segment b, CM[g] the same at the end of group g, S the total, as the oracle's upper_build forms them."""
    nseg = len(segk)
    n1 = (nseg + GRP - 1) // GRP
    m = np.zeros(nseg)
    KG, TG = np.full(n1, -np.inf), np.zeros(n1)
    for g in range(n1):
        b0, nb = g * GRP, min(GRP, nseg - g * GRP)
        kg = np.max(segk[b0:b0 + nb])
        t = np.zeros(64)
        t[:nb] = _lvl_scale(segk[b0:b0 + nb], kg) * (segs[b0:b0 + nb].astype(np.float64) * 2.0 ** -51)
        inc = _ks64(t)
        e = np.concatenate([[0.0], inc[:-1]])
        m[b0:b0 + nb] = np.maximum.accumulate((e + t)[:nb])
        KG[g], TG[g] = kg, m[b0 + nb - 1]
    K = np.max(KG)
    sig = _lvl_scale(KG, K)
    n2 = (n1 + 63) // 64
    TT = np.zeros(n2 * 64)
    TT[:n1] = sig * TG
    incB = np.concatenate([_ks64(TT[64 * h:64 * h + 64]) for h in range(n2)])
    incC = np.zeros(64)
    incC[:n2] = incB[63::64]
    incC = _ks64(incC)
    E = np.array([(incC[g // 64 - 1] if g >= 64 else 0.0) + (incB[g - 1] if g % 64 else 0.0) for g in range(n1)])
    CM = np.maximum.accumulate(E + TT[:n1])
    cp = np.concatenate([[0.0], CM[:-1]])
    gi = np.arange(nseg) // GRP
    cm = np.maximum(cp[gi], E[gi] + sig[gi] * m)
    S = float(CM[-1])
    return cm, CM, S


def census(lw, u):
    """Branch census of a log-weight vector under the uniform u: dict of per-workgroup arrays valid, ngw, covered, ns."""
    lw = np.asarray(lw, dtype=np.float64)
    N = lw.size
    segk, segs, _ = canon.segment_partials(lw)
    cm, CM, S = upper(segk, segs)
    nwg, n1 = len(segk), len(CM)
    valid = bool(S > 0.0 and S < np.inf)
    out = dict(valid=np.full(nwg, valid), ngw=np.zeros(nwg, int), covered=np.zeros(nwg, bool), ns=np.zeros(nwg, int), S=S)
    if not valid:
        return out
    moved = cm > np.concatenate([[0.0], cm[:-1]])
    for w in range(nwg):
        i0, i1 = w * SEG, min(N, (w + 1) * SEG) - 1
        tf, tl = (u + float(i0)) / float(N) * S, (u + float(i1)) / float(N) * S
        g_lo, g_hi = int(np.count_nonzero(CM < tf)), min(int(np.count_nonzero(CM < tl)), n1 - 1)
        b_lo, b_hi = int(np.count_nonzero(cm < tf)), min(int(np.count_nonzero(cm < tl)), nwg - 1)
        out["ngw"][w] = g_hi - g_lo + 1
        out["covered"][w] = out["ngw"][w] <= WIN_GRP
        out["ns"][w] = int(np.count_nonzero(moved[b_lo:b_hi + 1]))
    return out


def branches(cen):
    """The set of BRANCHES a census contains."""
    if not cen["valid"].all():
        return {"!valid"}
    s = set()
    for ngw, cov, ns in zip(cen["ngw"], cen["covered"], cen["ns"]):
        if not cov:
            s.add("!covered")
            continue
        s.add("ngw<=4" if ngw <= 4 else "4<ngw<=16")
        s.add("ns>8" if ns > NCAND else f"ns={ns}")
    return s


def summary(cen):
    """One table row: (workgroups, valid, max ngw, number of !covered workgroups, sorted distinct ns of the covered workgroups)."""
    cov = cen["covered"]
    return (len(cov), bool(cen["valid"].all()), int(cen["ngw"].max()), int((~cov).sum()) if cen["valid"].all() else 0,
            sorted(set(int(x) for x in cen["ns"][cov])))


# ------------------------------------------------------------------------------------------ the cases
def _rng(*key):
    return np.random.default_rng([20240517, *key])


def _neg_inf(N):
    return np.full(N, -np.inf)


def mild(N, seed=0):
    """iid log-weights of moderate spread: the regime every other parity test runs in."""
    return 2.0 * _rng(1, N, seed).standard_normal(N)


def flat(N):
    return np.full(N, -3.25)


def one_hot(N, pos):
    lw = _neg_inf(N)
    lw[pos] = 1.5
    return lw


def one_plus_tail(N, pos, heavy):
    """One particle with `heavy` of the mass, the others share the rest (slightly uneven): runs of many source segments per workgroup
    before and after the heavy particle, one source segment for every workgroup in between."""
    lw = math.log((1.0 - heavy) / (N - 1)) + 0.05 * _rng(2, N).standard_normal(N)
    lw[pos] = math.log(heavy)
    return lw


def light_prefix(N, npre, drop):
    """The first npre particles sit `drop` below the rest: the first workgroup's thresholds run through all of the prefix's groups."""
    lw = 0.5 * _rng(3, N).standard_normal(N)
    lw[:npre] -= drop
    return lw


def far_pair(N, ratio):
    """Only the first and the last particle carry weight: the first workgroup's thresholds span every group of the device."""
    lw = _neg_inf(N)
    lw[0], lw[-1] = 0.0, math.log(ratio)
    return lw


def _at_order(k):
    """A log-weight whose segment reference ceil(lw log2 e) is exactly the integer k."""
    return (k - 0.5) * LN2


def stairs(N, spread, ascending=False):
    """Per-segment offsets running across 0 .. -spread (natural-log units), mild noise inside a segment.  Where the spread reaches that
    far, segments 5 and 6 sit exactly 480 and 481 binary orders below their group's reference (the last kept and the first flushed
    scale, PGAS_LVL_FLUSH), and groups 2 and 3 exactly 480 and 481 below the top reference."""
    nseg = (N + SEG - 1) // SEG
    r = _rng(4, N, int(spread))
    k = -np.round(spread / LN2 * np.arange(nseg) / max(nseg - 1, 1))
    if spread / LN2 >= 481 and nseg > 3 * GRP:
        k[5], k[6] = -480.0, -481.0
        k[2 * GRP:3 * GRP] = np.minimum(k[2 * GRP:3 * GRP], -480.0)
        k[2 * GRP + 7] = -480.0
        k[3 * GRP:] = np.minimum(k[3 * GRP:], -481.0)
        k[3 * GRP + 1] = -481.0
    if ascending:
        k = k[::-1].copy()
    lw = np.repeat(_at_order(k), SEG)[:N] - r.uniform(0.0, 3.0, N)
    lw[::SEG] = _at_order(k)                 # the first particle of a segment pins its reference
    return lw


def empty_runs(N):
    """Whole segments and whole groups of -inf at the start, in the middle and at the end; the few non-empty segments are in groups 1
    and 5 (three empty groups between them) and 6, some next to each other and some behind runs of empty segments inside a group."""
    nseg = (N + SEG - 1) // SEG
    lw = _neg_inf(N)
    r = _rng(5, N)
    for b, shift in ((GRP + 3, 0.0), (GRP + 4, -1.0), (GRP + 40, 0.5), (5 * GRP + 20, 0.0), (5 * GRP + 21, 1.0), (5 * GRP + 63, -0.5), (6 * GRP, 0.0)):
        assert b < nseg - GRP
        lw[b * SEG:(b + 1) * SEG] = shift + r.standard_normal(SEG)
    lw[(GRP + 40) * SEG + 100:(GRP + 41) * SEG] = -np.inf    # a segment that is empty from its 100th particle on
    return lw


def all_empty(N):
    return _neg_inf(N)


def all_nan(N):
    return np.full(N, np.nan)


def with_nan(N):
    """Scattered NaN, one whole segment of NaN, and NaN in the place of each segment's would-be maximum."""
    r = _rng(6, N)
    lw = 2.0 * r.standard_normal(N)
    lw[r.integers(0, N, N // 50)] = np.nan
    lw[7 * SEG:8 * SEG] = np.nan
    for b in range(0, (N + SEG - 1) // SEG, 3):
        seg = lw[b * SEG:(b + 1) * SEG]
        if not np.all(np.isnan(seg)):
            seg[np.nanargmax(seg)] = np.nan
    lw[0] = lw[N - 1] = np.nan
    return lw


def nan_and_empty(N):
    """NaN and -inf only: no weight is positive although not every entry is -inf."""
    lw = _neg_inf(N)
    lw[::7] = np.nan
    return lw


def huge_range(N):
    r = _rng(7, N)
    vals = np.array([-1e300, -1e5, -745.2, -700.0, -36.0, 0.0, 300.0, 690.0, 699.0, 700.0])
    lw = vals[r.integers(0, len(vals), N)] + r.uniform(-0.5, 0.0, N)
    lw[N // 3] = 700.0
    return lw


def staged(N, k, first=50, stride=2, heavy_seg=67, fill=None):
    """Workgroup 0 draws from exactly k non-empty source segments: k - 1 light segments `stride` apart (empty ones in between, the run
    crosses the group boundary at segment 64) that together hold 0.9 of the workgroup's share 1024 / N, then one heavy segment.
    fill: the segments in between are not empty but `fill` below the light ones (flushed to zero weight when that is beyond 2^-480)."""
    lw = _neg_inf(N)
    r = _rng(8, N, k)
    share = 0.9 * SEG / N
    if fill is not None:
        lw[first * SEG:heavy_seg * SEG] = math.log(share / SEG) - fill - r.uniform(0.0, 2.0, (heavy_seg - first) * SEG)
    for j in range(k - 1):
        b = first + stride * j
        assert b < heavy_seg
        w = r.uniform(0.5, 1.5, SEG)
        lw[b * SEG:(b + 1) * SEG] = np.log(w / w.sum() * share / (k - 1))
    w = r.uniform(0.5, 1.5, SEG)
    lw[heavy_seg * SEG:(heavy_seg + 1) * SEG] = np.log(w / w.sum() * (1.0 - share))
    return lw


# The prefix sums inside a group come from a scan tree, so the prefix in front of an EMPTY segment can exceed the running maximum behind
# its non-empty neighbour by an ulp; such a segment counts as a source segment (in the oracle's records and on the device alike).  With
# seven or eight light segments the placement (first, stride) decides whether that happens: these give exactly k, and the placement
# (50, 2) with seven light segments gives ten (case staged_ulp: eight real source segments, but the bisection path).  staged_flushed
# has five light segments at (30, 2) and one such extra source segment, which is not empty but FLUSHED (its weights lie 2^-721 below the
# group's): it is staged with scale 0 next to the real ones, the only way a zero scale ever meets a non-zero cumsum in the search.
STAGED_AT = {8: (48, 3), 9: (45, 3)}
SIZES = (1, 2, 1023, 1024, 1025, 65536, 65537, 200000, (1 << 20) + 1, 1 << 21)
N_MID, N_ER = 70000, 8 * 65536 + 100
U_DEFAULT = 0.37


def _table():
    t = {}
    for N in SIZES:
        t[f"mild@{N}"] = (lambda N=N: mild(N), 0.61 if N % 2 else 0.37)
    for N in (1, 2, 1025, 65537, 200000):
        t[f"flat@{N}"] = (lambda N=N: flat(N), 0.37)
    for pos in (0, N_MID - 1, 1023, 1024, 65535, 65536):
        t[f"one_hot[{pos}]@{N_MID}"] = (lambda pos=pos: one_hot(N_MID, pos), 0.83)
    t["one_hot[0]@1"] = (lambda: one_hot(1, 0), 0.5)
    t["one_plus_tail@200000"] = (lambda: one_plus_tail(200000, 150000, 0.99), 0.37)
    t[f"one_plus_tail@{(1 << 20) + 1}"] = (lambda: one_plus_tail((1 << 20) + 1, 700000, 0.998), 0.29)
    t[f"light_prefix@{1 << 21}"] = (lambda: light_prefix(1 << 21, (1 << 20) + 5000, 10.0), 0.37)
    t[f"far_pair@{(1 << 20) + 1}"] = (lambda: far_pair((1 << 20) + 1, 1e5), 0.37)
    for spread in (50, 400, 700, 1400):
        t[f"stairs({spread})@262000"] = (lambda s=spread: stairs(262000, s), 0.37)
    t["stairs_up(700)@262000"] = (lambda: stairs(262000, 700, ascending=True), 0.37)
    t[f"empty_runs@{N_ER}"] = (lambda: empty_runs(N_ER), 0.37)
    for N in (1025, N_MID):
        t[f"all_empty@{N}"] = (lambda N=N: all_empty(N), 0.37)
    t["all_nan@1025"] = (lambda: all_nan(1025), 0.37)
    t[f"nan_and_empty@{N_MID}"] = (lambda: nan_and_empty(N_MID), 0.37)
    t[f"with_nan@{N_MID}"] = (lambda: with_nan(N_MID), 0.37)
    t[f"huge_range@{N_MID}"] = (lambda: huge_range(N_MID), 0.37)
    for k in range(1, 10):
        first, stride = STAGED_AT.get(k, (50, 2))
        t[f"staged_{k}@{N_MID}"] = (lambda k=k, first=first, stride=stride: staged(N_MID, k, first, stride), 0.37)
    t[f"staged_ulp@{N_MID}"] = (lambda: staged(N_MID, 8, 50, 2), 0.37)
    t[f"staged_flushed@{N_MID}"] = (lambda: staged(N_MID, 6, 30, 2, fill=500.0), 0.37)
    return t


_TABLE = _table()
NAMES = tuple(_TABLE)
EMPTY_NAMES = tuple(n for n in NAMES if n.split("@")[0] in ("all_empty", "all_nan", "nan_and_empty"))


def table_rows():
    """The census table of DESIGN.md section 6, one markdown row per case (tests/test_resample_cases.py checks the document against it)."""
    rows = []
    for n in NAMES:
        lw, N, u = case(n)
        wg, valid, ngw, nc, ns = summary(census(lw, u))
        nstxt = f"{ns[0]}…{ns[-1]} ({len(ns)} values)" if len(ns) > 6 else ", ".join(map(str, ns))
        rows.append(f"| `{n.split('@')[0]}` | {N} | {u} | {wg} | " + (f"yes | {ngw} | {nc} | {nstxt} |" if valid else "no | – | – | – (identity) |"))
    return rows


def case(name):
    """(lw, N, u) of a named case."""
    make, u = _TABLE[name]
    lw = np.ascontiguousarray(make(), dtype=np.float64)
    return lw, lw.size, u
