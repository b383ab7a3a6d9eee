"""CPU: the domains of the scalar-arithmetic sweep (tests/scalar_domains.py) are what they claim -- every part within the cap of one call, the listed edge
values present -- and on exactly these domains the HOST-compiled FQ_HD routines (g++, tests/host/scalar_harness.cpp) equal the references: the host libm,
numpy's conversions, numpy integer arithmetic. tests/test_gpu_scalar_arith.py runs the same arrays through the device build of the same headers, so a
mismatch there belongs to the device build and not to the domain or to the host libm."""
import numpy as np
import pytest

import scalar_domains as sd


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return sd.build_harness(tmp_path_factory.mktemp("scalar"))


def _has(arr, values):
    return bool(np.isin(sd.u32(values), arr).all())


def _has_pairs(a, b, pairs):
    key = (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
    want = [(int(x) & 0xFFFFFFFF) << 32 | (int(y) & 0xFFFFFFFF) for x, y in pairs]
    return bool(np.isin(np.asarray(want, np.uint64), key).all())


def _check_parts(name, parts, H):
    """the caps, and the host build against the reference; returns the parts' number of elements"""
    total = 0
    for label, a, b in parts:
        assert 0 < a.size <= sd.CAP and a.dtype == np.uint32 and (b is None or (b.shape == a.shape and b.dtype == np.uint32)), label
        total += a.size
        if name in sd.HOST_BUILT:
            want, got = sd.reference(name, a, b, H), sd.host_eval(H, name, a, b)
            bad = sd.mismatches(name, got, want)
            assert bad.size == 0, sd.report(label, a, b, got, want, bad, "host build")
    return total


def test_sweep_and_neighbourhoods():
    s = sd.sweep()
    assert abs(s.size - (1 << 22)) < (1 << 22) // 64 and sd.STRIDE % 2 == 1 and int(s[-1]) > 0xFFFFFFFF - sd.STRIDE
    n = sd.near(sd.bits(1.0))
    assert n.size == 2 * sd.ULPS + 1 and _has(n, [0x3F800000 - sd.ULPS, 0x3F800000 + sd.ULPS])
    z = sd.near(0x80000000)
    assert _has(z, [0x80000000, 0x80000000 + sd.ULPS, 0, sd.ULPS]) and z.size == 2 * sd.ULPS + 2
    assert _has(sd.near(0x7F800000), [0x7F800000 - sd.ULPS, 0x7F800001, 0x7F800000 + sd.ULPS])


def test_expf_domain(H):
    parts = sd.domain("expf")
    a = parts[0][1]
    assert len(parts) == 1
    for t in sd.EXPF_THRESHOLDS:
        assert _has(a, [t, t - 1 if t & 0x7FFFFFFF else t, t + 1])
    lo, hi = sd.bits(-87.0), sd.bits(-104.0)
    assert hi - lo > 2_200_000 and np.unique(a[(a >= lo) & (a <= hi)]).size == hi - lo + 1           # every float of [-104, -87]
    assert np.unique(a[a <= sd.bits(104.0)]).size > (1 << 20)
    _check_parts("expf", parts, H)


@pytest.mark.parametrize("name", ["logf", "log2f"])
def test_log_domain(H, name):
    parts = sd.domain(name)
    a = parts[0][1]
    assert len(sd.LOG_THRESHOLDS) == 11 + 48
    for t in sd.LOG_THRESHOLDS:
        assert _has(a, [t, t + 1, t + sd.ULPS])
    assert _has(a, [0x3F330000 + (j << 19) for j in range(16)] + [0x00B30000, 0x7EB30000 + (15 << 19)])
    assert np.unique(a[(a > 0) & (a < 0x00800000)]).size >= (1 << 16)
    _check_parts(name, parts, H)


def test_f2i_domain(H):
    parts = sd.domain("f2i_x86")
    a = parts[0][1]
    assert _has(a, [0x4F000000, 0x4F000000 - 1, 0x4F000000 - sd.ULPS, 0x4F000000 + sd.ULPS, 0xCF000000, 0xCF000001, 0xCF000000 + sd.ULPS, 0x7FC00000, 0x7F800000, 0xFF800000])
    _check_parts("f2i_x86", parts, H)


@pytest.mark.parametrize("piece", sd.POWF_PIECES)
def test_powf_domain(H, piece):
    total, seen = 0, False
    for label, a, b in sd.powf_domain(H, (piece,)):
        total += _check_parts("powf", [(label, a, b)], H)
        if piece == "x=2":
            assert (a == sd.bits(2.0)).all() and (np.diff(b.astype(np.int64)) == 64).all() and (b & 0x7FFFFFFF).max() <= sd.bits(64.0)
            seen |= _has(b, [sd.bits(64.0)]) or _has(b, [sd.bits(-64.0)])
        elif piece.startswith("x="):
            assert (a == sd.bits(float(piece[2:]))).all() and (np.diff(b.astype(np.int64)) == 16).all() and (b & 0x7FFFFFFF).max() <= sd.bits(4.0)
            seen |= _has(b, [sd.bits(4.0)]) or _has(b, [sd.bits(-4.0)])
        elif piece == "pairs":
            assert a.size == 1 << 22
            x, y = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
            H.scalar_powf_pairs(sd.POWF_SEED, 12345, 1, x.ctypes.data, y.ctypes.data)
            seen = (int(a[12345]), int(b[12345])) == (int(x[0]), int(y[0]))
        else:
            assert _has_pairs(a, b, [(x, y) for x in sd.POWF_SPECIAL_X for y in sd.POWF_SPECIAL_Y])
            assert ((a > 0) & (a < 0x00800000)).sum() > 10_000                                       # subnormal x
            x, y = a.view(np.float32).astype(np.float64), b.view(np.float32).astype(np.float64)
            ok = (a > 0x00800000) & (a < 0x7F800000) & (a != 0x3F800000)
            with np.errstate(all="ignore"):
                ylogx = np.where(ok, y * np.log2(np.where(ok, x, 2.0)), 0.0)
            for edge in sd.POWF_EDGES:                                                                # both sides of every branch, within 2^-20
                d = ylogx - edge
                assert ((d > 0) & (d < 2.0 ** -20)).any() and ((d < 0) & (d > -2.0 ** -20)).any(), edge
            seen = True
    assert seen and total > 0
    if piece.startswith("x="):
        assert total == 2 * ((sd.bits(64.0) // 64 + 1) if piece == "x=2" else (sd.bits(4.0) // 16 + 1))


@pytest.mark.parametrize("name", sd.NEGLIGIBLE)
def test_negligible_domain(H, name):
    parts = sd.domain(name)
    (_, a, b), = parts
    assert _has(b, [1, 1 + sd.STRIDE, 0x7F7FFFFF]) and ((b > 0) & (b < 0x00800000)).sum() > 8000 and ((b > 0) & (b < 0x7F800000)).all()
    n = a.size // 5
    assert a.size == 5 * n and (b[:n] == b[n:2 * n]).all() and (a[:n] == 0).all()
    t = a.view(np.float32).reshape(5, n)
    s = b[:n].view(np.float32)
    with np.errstate(all="ignore"):
        ulp = (np.nextafter(s.astype(np.float64), np.inf) - s.astype(np.float64)) if name == "negligible_d" else (np.nextafter(s, np.float32(np.inf)) - s).astype(np.float64)
        exact = np.isfinite(ulp) & ((0.5 * ulp).astype(np.float32).astype(np.float64) == 0.5 * ulp) & (ulp > 0)
    assert exact.sum() > n // 2 and (t[1][exact] == 0.5 * ulp[exact]).all() and (t[4][exact] == ulp[exact]).all()
    assert (t[2][exact] < t[1][exact]).all() and (t[3][exact] > t[1][exact]).all()
    want = sd.reference(name, a, b, H).reshape(5, n)
    assert want[0].all() and not want[4][exact].any() and want[2][exact].any() and not want[3][exact].any()      # the answer changes across the domain
    _check_parts(name, parts, H)


def test_f2h_domains(H):
    (_, a, _b), = sd.domain("f2h")
    for v in (0.0, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14, 65504.0, 65520.0, 65536.0, float("inf")):
        for s in (0, 0x80000000):
            t = sd.bits(v) | s
            assert _has(a, [t, t + 1, t + sd.ULPS] + ([t - 1, t - sd.ULPS] if v else []))
    assert _has(a, [0x7FC00000])
    _check_parts("f2h", sd.domain("f2h"), H)
    prod = sd.domain("f2h_product")
    assert [int(p[2][0]) for p in prod] == [int(v) for v in sd.PRODUCT_B] and len(prod) == 7
    for _, pa, pb in prod:
        assert (pb == pb[0]).all() and _has(pa, list(sd.PRODUCT_SMALL_A) + [0x80000000, sd.bits(65520.0)]) and pa.size == a.size + 4
    want = np.concatenate([sd.reference("f2h_product", pa, pb, H) for _, pa, pb in prod])
    assert (want == 0x8000).sum() > 1000 and (want == 0).sum() > 1000                                 # negative-zero and negative-underflow products
    _check_parts("f2h_product", prod, H)
    for name in ("f2h_bits", "f32_to_f16_bits", "f2h_bits_product", "f32_to_f16_bits_product"):     # no g++ build: the same arrays, caps only
        assert sum(p[1].size for p in sd.domain(name)) == sum(p[1].size for p in sd.domain("f2h" if "product" not in name else "f2h_product"))


def test_h2f_domain(H):
    for name in sd.H2F:
        (_, a, b), = sd.domain(name)
        assert b is None and (a == np.arange(65536)).all()
    _check_parts("h2f", sd.domain("h2f"), H)
    want = sd.reference("h2f", np.arange(65536, dtype=np.uint32), None, H)
    assert want[0x3C00] == 0x3F800000 and want[0x0001] == sd.bits(2.0 ** -24) and want[0xFC00] == 0xFF800000 and sd.is_nan("h2f", want[0x7E00:0x7E01]).all()


@pytest.mark.parametrize("name", sd.INTEGER)
def test_integer_domains(H, name):
    parts = sd.domain(name)
    (_, a, b), = parts
    if name in sd.DOT4:
        assert _has_pairs(a, b, [(0x80808080, 0x80808080), (0x80808080, 0x7F7F7F7F), (0x7F7F7F7F, 0x7F7F7F7F), (0x8181FF01, 0x007F80FF), (0, 0)]) and a.size == 1296 ** 2 + (1 << 20)
    elif name in sd.DOT2 or name == "pk_sub16":
        assert _has_pairs(a, b, [(0x80008000, 0x80008000), (0x80008000, 0x7FFF7FFF), (0x7FFF7FFF, 0x80008000), (0x8001FFFF, 0x00017FFF)]) and a.size == 36 ** 2 + (1 << 20)
    elif name == "pack16":
        assert _has_pairs(a, b, [(-32768, 32767), (32767, -32768), (-1, 0), (1, -32767)])
    else:
        assert _has_pairs(a, b, [(-(1 << 23), -(1 << 23)), ((1 << 23) - 1, (1 << 23) - 1), (-(1 << 23), (1 << 23) - 1)] + sd.MUL24_CALLERS)
        sa, sb = sd._fields(a, 32, 0), sd._fields(b, 32, 0)
        assert max(sa.max(), sb.max()) == (1 << 23) - 1 and min(sa.min(), sb.min()) == -(1 << 23)     # inside 24 signed bits, both ends
    _check_parts(name, parts, H)


def test_integer_reference_by_hand():
    one = lambda name, a, b: int(sd.integer_ref(name, sd.u32([a & 0xFFFFFFFF]), sd.u32([b & 0xFFFFFFFF]))[0])
    assert one("dot4", 0x80808080, 0x80808080) == 4 * 128 * 128 and one("dot4", 0x01FF7F80, 0x02030405) == (2 - 3 + 127 * 4 - 128 * 5) & 0xFFFFFFFF
    assert one("dot4_c_high", 0x7F7F7F7F, 0x7F7F7F7F) == (0x7FFFFF00 + 4 * 127 * 127) & 0xFFFFFFFF          # wraps
    assert one("dot4_c_low", 0x80808080, 0x7F7F7F7F) == (-0x7FFFFF00 - 4 * 128 * 127) & 0xFFFFFFFF
    assert one("dot2", 0x80008000, 0x80008000) == 0x80000000 and one("dot2_c_mid", 0xFFFF0002, 0x00030004) == 12345 + 8 - 3
    assert one("pack16", -2, 0x12345) == 0x2345FFFE and one("pk_sub16", 0x80000001, 0x0001FFFF) == 0x7FFF0002
    assert one("mul24", -(1 << 23), -(1 << 23)) == 0 and one("mul24", (1 << 23) - 1, -3) == (-3 * ((1 << 23) - 1)) & 0xFFFFFFFF
