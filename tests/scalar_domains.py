"""The input domains and references of the scalar-arithmetic sweep: tests/test_scalar_domains_cpu.py (the g++ build of the FQ_HD routines) and
tests/test_gpu_scalar_arith.py (ggml_hip_debug_scalar_eval: the same routines as hipcc compiles them for the device) see the same arrays.

A domain is a sequence of PARTS (label, a, b): uint32 arrays of raw bits (b None for a one-argument routine), each at most CAP elements -- one call.
The large powf slices are generated part by part. References never come from the code under test: the host libm through tests/host/scalar_harness.cpp
(scalar_libm_eval), numpy's float16 / float32 conversions and arithmetic, numpy int64 arithmetic wrapped to int32."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

import ggllm_cpp_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 24                     # elements per call
STRIDE = 1021                     # odd: the strided sweep of all 2^32 patterns takes 4 206 530 samples (about 2^22)
ULPS = 1 << 12                    # neighbourhood of a branch threshold, on both sides
THREADS = max(1, min(16, os.cpu_count() or 1))
POWF_SEED = 20240611              # test_sample_chain_cpu.py::test_powf_equals_libm_on_random_pairs' seed
FN = g.SCALAR_FN

LIBM = ("expf", "logf", "log2f", "powf", "f2i_x86")
NEGLIGIBLE = ("negligible_f", "negligible_d")
F2H_VALUE = ("f2h_bits", "f2h", "f32_to_f16_bits")
F2H_PRODUCT = ("f2h_bits_product", "f2h_product", "f32_to_f16_bits_product")
H2F = ("h2f_bits", "h2f", "f16_bits_to_f32")
DOT4 = ("dot4", "dot4_c_high", "dot4_c_low", "dot4_c_mid", "dot4z")
DOT2 = ("dot2", "dot2_c_high", "dot2_c_low", "dot2_c_mid", "dot2z")
INTEGER = DOT4 + DOT2 + ("pack16", "pk_sub16", "mul24")
ALL = LIBM + NEGLIGIBLE + F2H_VALUE + F2H_PRODUCT + H2F + INTEGER
# routines with a g++ build (f2h_bits / h2f_bits are device functions; fq_f16.h's casts need _Float16, which the hosts' g++ does not have on x86)
HOST_BUILT = tuple(n for n in ALL if n not in ("f2h_bits", "f2h_bits_product", "h2f_bits", "f32_to_f16_bits", "f32_to_f16_bits_product", "f16_bits_to_f32"))
ACC = {"_c_high": 0x7FFFFF00, "_c_low": -0x7FFFFF00, "_c_mid": 12345}


# ------------------------------------------------------------------------------------------------ the host harness
def build_harness(out_dir):
    src = os.path.join(ROOT, "tests", "host", "scalar_harness.cpp")
    out = os.path.join(str(out_dir), "libscalar_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fwrapv", "-fPIC", "-shared", "-pthread", "-I",
                           os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", out, src])
    H = C.CDLL(out)
    for f in (H.scalar_libm_eval, H.scalar_host_eval):
        f.restype, f.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
    H.scalar_powf_pairs.restype, H.scalar_powf_pairs.argtypes = None, [C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p]
    return H


def _eval(f, name, a, b):
    out = np.empty(a.shape, np.uint32)
    rc = f(FN[name], a.ctypes.data, b.ctypes.data if b is not None else None, a.size, out.ctypes.data, THREADS)
    assert rc == 0, name
    return out


def libm_eval(H, name, a, b=None):
    return _eval(H.scalar_libm_eval, name, a, b)


def host_eval(H, name, a, b=None):
    return _eval(H.scalar_host_eval, name, a, b)


# ------------------------------------------------------------------------------------------------ bits
def bits(x):
    return int(np.float32(x).view(np.uint32))


def fbits(xs):
    return np.asarray(xs, np.float32).view(np.uint32)


def u32(x):
    return np.ascontiguousarray(x, np.uint32)


def sweep():
    return np.arange(0, 1 << 32, STRIDE, dtype=np.uint64).astype(np.uint32)


def near(pattern, k=ULPS):
    """every float within k ulps of the pattern on both sides, in the order of the values (across +-0 into the other sign; past inf into the NaNs)"""
    sign, mag = pattern & 0x80000000, pattern & 0x7FFFFFFF
    same = np.arange(max(0, mag - k), min(0x7FFFFFFF, mag + k) + 1, dtype=np.uint64) | sign
    other = np.arange(0, max(0, k - mag) + 1, dtype=np.uint64) | (sign ^ 0x80000000) if mag < k else np.zeros(0, np.uint64)
    return np.concatenate([same, other]).astype(np.uint32)


def cat(*xs):
    return u32(np.concatenate([u32(x).ravel() for x in xs]))


def parts_of(label, a, b=None):
    """(label, a, b) cut into parts of at most CAP elements"""
    return [(label if a.size <= CAP else "%s[%d]" % (label, i // CAP), u32(a[i:i + CAP]), None if b is None else u32(b[i:i + CAP])) for i in range(0, a.size, CAP)]


# ------------------------------------------------------------------------------------------------ libm group
EXPF_THRESHOLDS = [0x00000000, 0x80000000, bits(88.0), bits(-88.0), bits(float.fromhex("0x1.62e42ep6")), bits(float.fromhex("-0x1.9fe368p6")),
                   0x7F800000, 0xFF800000, 0x7FC00000]


def expf_domain():
    sub = np.arange(bits(-87.0), bits(-104.0) + 1, dtype=np.uint64)                 # every float in [-104, -87]: the subnormal results
    pos = np.arange(0, bits(104.0) + 1, STRIDE, dtype=np.uint64)                   # the positive arguments typical opens
    return parts_of("expf", cat(sweep(), *[near(t) for t in EXPF_THRESHOLDS], sub, pos))


TABLE_BASES = [0x3F330000, 0x00B30000, 0x7EB30000]                                  # the 16 sub-intervals in 1.0's binade, the lowest and the highest
LOG_THRESHOLDS = ([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x80000000, 0xBF800000, 0x7FC00000, 0x7F800001]
                  + [base + (j << 19) for base in TABLE_BASES for j in range(16)])


def log_domain():
    return parts_of("log", cat(sweep(), *[near(t) for t in LOG_THRESHOLDS], np.arange(1, 0x00800000, 127, dtype=np.uint64)))      # + 66 052 subnormals


F2I_THRESHOLDS = [bits(2147483648.0), bits(-2147483648.0), 0x7FC00000, 0x7F800000, 0xFF800000]


def f2i_domain():
    return parts_of("f2i", cat(sweep(), *[near(t) for t in F2I_THRESHOLDS]))


# test_sample_chain_cpu.py::test_powf_special_cases' pairs (bits: the NaNs keep their payloads), and negative bases with integer exponents at the overflow
# and underflow branches (sign_bias)
_NAN, _INF = float("nan"), float("inf")
POWF_SPECIAL_X = cat(fbits([_NAN, -_NAN, -_INF, -3.5, -2.0, -1.0, -0.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 0.5, 1.0, 1.5, 2.0, 7.0, 65024.0, 3e38, _INF]), [0x7F800001])
POWF_SPECIAL_Y = cat(fbits([_NAN, -_INF, -1e30, -150.0, -149.5, -127.0, -3.0, -2.0, -1.0, -0.5, -1e-45, -0.0, 0.0, 1e-45, 0.5, 1.0, 2.0, 3.0, 127.0, 128.0, 1e30, _INF,
                            129.0, -129.0, -149.0, -151.0, 126.0, -126.0]), [0x7FA00000])
POWF_EDGES = [126.0, -126.0, -149.0, -150.0, float.fromhex("0x1.fffffffd1d571p+6")]


def _powf_edge_pairs():
    """(x, y) with y log2 x at the overflow / underflow branches of fq_powf: for each x the y where |y| |log2 x| crosses |edge|, found by bisection on y's
    bits, and the 64 floats on either side of it"""
    rng = np.random.default_rng(149)
    xs = cat(fbits([2.0, 3.0, 10.0, 333.0, 32000.0, 65024.0, 1.5, 1.0001, 0.9999, 0.5, 0.3, 0.001, 1e-40, 3e38]),
             rng.integers(0x00800000, 0x7F800000, 242, dtype=np.uint64))
    xa, ya = [], []
    for xb in xs:
        l = float(np.log2(np.float64(u32([xb]).view(np.float32)[0])))
        if l == 0.0:
            continue
        for edge in POWF_EDGES:
            lo, hi = 0, 0x7F800000                                                   # |y| bits: lo is below the edge, hi is not
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if float(u32([mid]).view(np.float32)[0]) * abs(l) < abs(edge):
                    lo = mid
                else:
                    hi = mid
            if hi >= 0x7F800000 - 64:
                continue
            m = np.arange(hi - 64, hi + 65, dtype=np.uint64) | (0x80000000 if (edge < 0) != (l < 0) else 0)
            xa.append(np.full(m.size, xb, np.uint64)); ya.append(m)
    return cat(*xa), cat(*ya)


POWF_PIECES = ("x=2", "x=65024", "x=32000", "x=333", "pairs", "edges")


def powf_domain(H, pieces=POWF_PIECES):
    """yields the parts of the pieces asked for; the slices of every 64th / 16th float are large and never held whole"""
    def slices(x, lim, step):
        pos = np.arange(0, bits(lim) + 1, step, dtype=np.uint64)
        for sign, tag in ((0, "+"), (0x80000000, "-")):
            yb = (pos | sign).astype(np.uint32)
            yield from parts_of("powf(%g, %sy)" % (x, tag), np.full(yb.size, bits(x), np.uint32), yb)
    if "x=2" in pieces:
        yield from slices(2.0, 64.0, 64)
    for x in (65024.0, 32000.0, 333.0):
        if "x=%g" % x in pieces:
            yield from slices(x, 4.0, 16)
    if "pairs" in pieces:
        yield powf_pairs(H)
    if "edges" in pieces:
        yield powf_edges()


def powf_pairs(H):
    n = 1 << 22
    xa, ya = np.empty(n, np.uint32), np.empty(n, np.uint32)
    H.scalar_powf_pairs(POWF_SEED, 0, n, xa.ctypes.data, ya.ctypes.data)
    return ("powf pairs", xa, ya)


def powf_edges():
    sx, sy = np.meshgrid(POWF_SPECIAL_X, POWF_SPECIAL_Y, indexing="ij")
    sub = np.arange(1, 0x00800000, 8191, dtype=np.uint64)                          # subnormal x (1 025 of them) to a few powers
    ux, uy = np.meshgrid(sub, fbits([-3.0, -2.0, -1.0, -0.5, -0.1, 0.1, 0.5, 1.0, 2.0, 3.0]), indexing="ij")
    ex, ey = _powf_edge_pairs()
    return ("powf edges", cat(sx, ux, ex), cat(sy, uy, ey))


def negligible_domain(double):
    """sum over the positive subnormal and normal floats, strided, and FLT_MAX; t at 0, half an ulp of sum, one ulp of t below and above that, and an ulp of
    sum (an ulp of the DOUBLE sum for fq_negligible_d, rounded to the f32 the entry takes)"""
    s = cat(np.arange(1, 0x7F800000, STRIDE, dtype=np.uint64), [0x7F7FFFFF]).view(np.float32)
    with np.errstate(all="ignore"):
        if double:
            sd = s.astype(np.float64)
            ulp = np.nextafter(sd, np.inf) - sd
            half, whole = (0.5 * ulp).astype(np.float32), ulp.astype(np.float32)
        else:
            ulp = np.nextafter(s, np.float32(np.inf)) - s
            half, whole = np.float32(0.5) * ulp, ulp
        ts = [np.zeros_like(s), half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(np.inf)), whole]
    return parts_of("negligible", cat(*[t.view(np.uint32) for t in ts]), np.tile(s.view(np.uint32), len(ts)))


def negligible_ref(name, a, b):
    """the same expression in numpy, in the routine's type"""
    t, s = a.view(np.float32), b.view(np.float32)
    with np.errstate(all="ignore"):
        if name == "negligible_d":
            t, s = t.astype(np.float64), s.astype(np.float64)
            return (2.0 * t < np.nextafter(s, np.inf) - s).astype(np.uint32)
        return (np.float32(2) * t < np.nextafter(s, np.float32(np.inf)) - s).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ conversions
F2H_THRESHOLDS = [t | s for s in (0, 0x80000000) for t in
                  (0, bits(2.0 ** -25), bits(2.0 ** -24), bits(2.0 ** -14), bits(65504.0), bits(65520.0), bits(65536.0), 0x7F800000, 0x7FC00000)]
PRODUCT_B = fbits([1.0, -1.0, 0.125, 1.0 / 127.0, float.fromhex("0x1.000002p0"), -0.0, 1e-30])
PRODUCT_SMALL_A = fbits([0.0, -0.0, 1e-30, -1e-30])


def f2h_value_domain():
    return parts_of("f2h", cat(sweep(), *[near(t) for t in F2H_THRESHOLDS]))


def f2h_product_domain():
    a = cat(PRODUCT_SMALL_A, f2h_value_domain()[0][1])
    return [("f2h(a * %s)" % float(u32([b]).view(np.float32)[0]).hex(), a, np.full(a.size, b, np.uint32)) for b in PRODUCT_B]


def h2f_domain():
    return parts_of("h2f", np.arange(65536, dtype=np.uint32))


def f2h_ref(a, b=None):
    x = a.view(np.float32)
    with np.errstate(all="ignore"):
        if b is not None:
            x = x * b.view(np.float32)                       # the f32 product is rounded first (no contraction)
        return x.astype(np.float16).view(np.uint16).astype(np.uint32)


def h2f_ref(a):
    return a.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ integer units
def _words(values, width):
    """every 32-bit word made of the given fields"""
    n = 32 // width
    mask = (1 << width) - 1
    return u32([sum((v & mask) << (width * i) for i, v in enumerate(c)) for c in itertools.product(values, repeat=n)])


def _pairs(w, rng):
    a, b = np.meshgrid(w, w, indexing="ij")
    r = rng.integers(0, 1 << 32, (2, 1 << 20), dtype=np.uint64)
    return cat(a, r[0]), cat(b, r[1])


def dot4_domain():
    return parts_of("dot4", *_pairs(_words([-128, -127, -1, 0, 1, 127], 8), np.random.default_rng(4)))


INT16_EDGES = [-32768, -32767, -1, 0, 1, 32767]


def dot2_domain():
    return parts_of("dot2", *_pairs(_words(INT16_EDGES, 16), np.random.default_rng(2)))


def pack16_domain():
    """fq_pack16 takes two integers and keeps their low halves: the int16 edges sign-extended, and any 32-bit words"""
    return parts_of("pack16", *_pairs(u32(np.asarray(INT16_EDGES, np.int64) & 0xFFFFFFFF), np.random.default_rng(16)))


# fq_mul24's contract is operands inside 24 signed bits. Its callers' largest (csrc/fq_kdot.h):
#   line 107 (fq_kdot45::dot)  a 6-bit scale (<= 63) times a 16-element dot of 5-bit weights and int8 activations, |dot| <= 16 * 31 * 128 = 63 488
#   line 154 (fq_kdot<Q6_K>::dot)  an int8 scale (-128 .. 127) times dot - 32 bsum, |.| < 2^18
MUL24_CALLERS = [(63, 63488), (63, -63488), (127, (1 << 18) - 1), (-128, (1 << 18) - 1), (127, -(1 << 18) + 1), (-128, -(1 << 18) + 1)]
MUL24_EDGES = [-(1 << 23), -(1 << 23) + 1, -1, 0, 1, (1 << 23) - 1]


def mul24_domain():
    rng = np.random.default_rng(24)
    ea, eb = np.meshgrid(MUL24_EDGES, MUL24_EDGES, indexing="ij")
    r = rng.integers(-(1 << 23), 1 << 23, (2, 1 << 20), dtype=np.int64)
    ca, cb = np.asarray(MUL24_CALLERS, np.int64).T
    a, b = np.concatenate([ea.ravel(), ca, cb, r[0]]), np.concatenate([eb.ravel(), cb, ca, r[1]])
    return parts_of("mul24", u32(a & 0xFFFFFFFF), u32(b & 0xFFFFFFFF))


def _fields(x, width, i):
    """field i of every word, sign-extended, int64"""
    v = (x.astype(np.int64) >> (width * i)) & ((1 << width) - 1)
    return v - ((v >> (width - 1)) << width)


def integer_ref(name, a, b):
    """numpy int64 arithmetic, wrapped to 32 bits"""
    if name in DOT4 or name in DOT2:
        width = 8 if name in DOT4 else 16
        c = next((v for k, v in ACC.items() if name.endswith(k)), 0)
        r = sum(_fields(a, width, i) * _fields(b, width, i) for i in range(32 // width)) + c
    elif name == "pack16":
        r = (a.astype(np.int64) & 0xFFFF) | ((b.astype(np.int64) & 0xFFFF) << 16)
    elif name == "pk_sub16":
        r = ((_fields(a, 16, 0) - _fields(b, 16, 0)) & 0xFFFF) | (((_fields(a, 16, 1) - _fields(b, 16, 1)) & 0xFFFF) << 16)
    else:
        assert name == "mul24"
        r = _fields(a, 32, 0) * _fields(b, 32, 0)
    return u32(r & 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ one table
def domain(name, H=None):
    """the parts of routine `name`"""
    if name == "expf":
        return expf_domain()
    if name in ("logf", "log2f"):
        return log_domain()
    if name == "powf":
        return powf_domain(H)
    if name == "f2i_x86":
        return f2i_domain()
    if name in NEGLIGIBLE:
        return negligible_domain(name == "negligible_d")
    if name in F2H_VALUE:
        return f2h_value_domain()
    if name in F2H_PRODUCT:
        return f2h_product_domain()
    if name in H2F:
        return h2f_domain()
    if name in DOT4:
        return dot4_domain()
    if name in DOT2 or name == "pk_sub16":
        return dot2_domain()
    if name == "pack16":
        return pack16_domain()
    assert name == "mul24"
    return mul24_domain()


def reference(name, a, b, H):
    if name in LIBM:
        return libm_eval(H, name, a, b)
    if name in NEGLIGIBLE:
        return negligible_ref(name, a, b)
    if name in F2H_VALUE:
        return f2h_ref(a)
    if name in F2H_PRODUCT:
        return f2h_ref(a, b)
    if name in H2F:
        return h2f_ref(a)
    return integer_ref(name, a, b)


def is_nan(name, x):
    """the NaNs of the routine's result type (two NaN results count as equal; everything else is compared as bits)"""
    if name in F2H_VALUE or name in F2H_PRODUCT:
        return (x & 0x7FFF) > 0x7C00
    if name in INTEGER or name in NEGLIGIBLE or name == "f2i_x86":
        return np.zeros(x.shape, bool)
    return (x & 0x7FFFFFFF) > 0x7F800000


def mismatches(name, got, want):
    """indices where got differs from want"""
    return np.flatnonzero((got != want) & ~(is_nan(name, got) & is_nan(name, want)))


def report(name, a, b, got, want, bad, who="device"):
    rows = ["(%s) -> %s %#x, reference %#x" % (", ".join("%#x" % int(v[i]) for v in (a, b) if v is not None), who, int(got[i]), int(want[i])) for i in bad[:5]]
    return "%s: %d of %d differ; the first: %s" % (name, bad.size, a.size, "; ".join(rows))
