"""The device-only Box-Muller chain of the SingleMassOscillator k_propagate (csrc/pgas_kernels.hip.h: dev_normal_pair_n -- uniforms
built from the 52 bits directly, log without its x > 0 select, an unscaled division and square root, sin/cos(pi r) without range and
NaN selects, Horner coefficients in scalar registers) against include/pgas_detmath.h, BIT FOR BIT.

The host side is the header itself, step by step: pgas_u52 in exact float64 arithmetic ((n + 1/2) 2^-52: n + 1/2 < 2^52 and the
scaling are exact), pgas_log and pgas_sincospi from the host build of the header (oracle.canon), the correctly rounded IEEE square
root and the two products.  The device runs the chain on GIVEN Philox output blocks (pgas_detmath_eval, which = 9), so the extreme
uniforms can be put in by hand."""
import numpy as np
import pytest

from oracle import canon

pytestmark = pytest.mark.gpu


def _dev(which, **kw):
    from pgas_amd import _lib

    return _lib.detmath_eval(which, **kw)


def _host_pair(blocks):
    b = blocks.astype(np.uint64)
    na = ((b[:, 1] << np.uint64(32)) | b[:, 0]) >> np.uint64(12)
    nb = ((b[:, 3] << np.uint64(32)) | b[:, 2]) >> np.uint64(12)
    ua = (na.astype(np.float64) + 0.5) * 2.0**-52   # n < 2^52: the conversion, the sum and the scaling are exact
    ub = (nb.astype(np.float64) + 0.5) * 2.0**-52
    lg = canon.det_log(ua)
    s, c = canon.det_sincospi(ub + ub)
    rad = np.sqrt(-2.0 * lg)
    return rad * c, rad * s


def _six(blocks):
    w = np.zeros((len(blocks), 6), dtype=np.uint32)
    w[:, :4] = blocks
    return w


def test_device_only_box_muller_equals_the_header():
    n = 1 << 20
    rng = np.random.default_rng(31)
    ctr = rng.integers(0, 2**32, (n, 6), dtype=np.uint64).astype(np.uint32)
    blocks = _dev(3, words=ctr)[2]   # 2^20 Philox4x32-10 blocks, from the device's own generator
    lo12, top = 0xFFF, 0xFFFFFFFF
    # the extreme uniforms n = 0 (u = 2^-53; f = 0 in the log) and n = 2^52 - 1 (u = 1 - 2^-53), with and without the 12 discarded low
    # bits set, in both places; mantissa of u exactly at and next to the sqrt(2) fold of the log; 2 u at and next to the quadrant edges
    edge = [[0, 0, 0, 0], [lo12, 0, lo12, 0], [top, top, top, top], [top & ~lo12, top, top & ~lo12, top], [0, 0, top, top], [top, top, 0, 0],
            [0, 0x80000000, 0, 0x80000000], [0, 0x40000000, 0, 0x40000000], [0, 0xC0000000, 0, 0xC0000000],
            [top, 0x7FFFFFFF, top, 0x3FFFFFFF], [0, 0x20000000, top, 0xBFFFFFFF], [0x1000, 0, 0x1000, 0]]
    for m in (0x6A09E667F3BCD - 1, 0x6A09E667F3BCD, 0x6A09E667F3BCD + 1):   # u in [1/2, 1): exponent -1, mantissa m after normalisation
        nn = (1 << 51) + (m >> 1)
        edge.append([(nn << 12) & top, (nn << 12) >> 32, (nn << 12) & top, (nn << 12) >> 32])
    blocks = np.concatenate([blocks, np.array(edge, dtype=np.uint32)])
    z0, z1, _ = _dev(9, words=_six(blocks))
    h0, h1 = _host_pair(blocks)
    assert np.isfinite(h0).all() and np.isfinite(h1).all()
    bad = np.nonzero((z0 != h0) | (z1 != h1))[0]
    assert bad.size == 0, f"{bad.size} of {len(blocks)} pairs differ, first at {bad[0]}: block {blocks[bad[0]]}, device {z0[bad[0]]!r} {z1[bad[0]]!r}, host {h0[bad[0]]!r} {h1[bad[0]]!r}"
    assert np.array_equal(np.signbit(z0), np.signbit(h0)) and np.array_equal(np.signbit(z1), np.signbit(h1)), "signed zeros"
    # ... and the header's own chain on the device (which = 7) from the same counters
    y0, y1, _ = _dev(7, words=ctr)
    assert np.array_equal(y0, z0[:n]) and np.array_equal(y1, z1[:n])


def test_device_only_guarded_sincospi_equals_the_header():
    """dev_sincospi_n<GUARD> (the basis calls keep the |r| < 2^30 and NaN handling: states can be non-finite)."""
    rng = np.random.default_rng(32)
    xs = np.concatenate([rng.uniform(-0.25, 0.25, 100000), rng.uniform(-64, 64, 100000), rng.uniform(-1e6, 1e6, 100000),
                         [0.0, -0.0, 0.5, 1.0, 1.5, 2.0, -1.0, 7.0, 0.25, 0.75, 2.0**30, -(2.0**30), 2.0**30 - 0.75, 0.25 - 2.0**30, 1e300, np.inf, -np.inf, np.nan]])
    # (between 2^30 - 1/4 and 2^30 the header's nearest half-integer index is 2^31, which its int32 conversion does not hold: not a
    # value the two sides are defined to agree on, and not tested)
    s, c, _ = _dev(10, x=xs)
    so, co = canon.det_sincospi(xs)
    bad = np.nonzero(~(((s == so) | (np.isnan(s) & np.isnan(so))) & ((c == co) | (np.isnan(c) & np.isnan(co)))))[0]
    assert bad.size == 0, f"{bad.size} differ, first: x = {xs[bad[0]]!r}: device {s[bad[0]]!r} {c[bad[0]]!r}, host {so[bad[0]]!r} {co[bad[0]]!r}"
    assert np.array_equal(np.signbit(s), np.signbit(so)) and np.array_equal(np.signbit(c), np.signbit(co)), "signed zeros"
