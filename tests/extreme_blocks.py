"""Weight blocks and activation rows at the EXTREMES of the block encodings: seeded numpy generators only (no checker code, no
device), so that oracle/gen_golden.py, the CPU tests and the GPU tests build identical bytes.

  weights(t, family, M, K, seed)  -> [M, row_bytes] uint8
      signed_d      random planes; d (and dmin / m) dealt per block from D_VALUES: both signs, +0 and -0, fp16 subnormals down to
                    0x0001, the smallest normal, order 1; row 0: -0 in every block, row 1: one negative value in every block. Formats whose quantizer never writes a negative d or dmin get them too:
                    a file can hold them and the reference multiplies them through.
      saturated_lo  every quant at its minimum, every sub-block scale and min at its largest magnitude
      saturated_hi  every quant at its maximum, the same scales
                    (Q3_K: even rows scale -32, odd rows +31; Q6_K: even rows -128, odd rows +127. Legacy formats: ONE quant per
                    block sits at the opposite extreme -- a block of 32 equal quants times a row whose Q8 image sums to zero is
                    exactly 0 whatever the kernel does, and a case of zeros pins nothing)
      quantizer     rows the weight quantizer writes (pass quantize=): N(0, 0.02^2), one sign only, one outlier per super-block,
                    uniform, all-zero
  activations(K, seed)            -> [16, K] f32, the rows of ACT_ROWS; rows_for(A, N) repeats them for N > 16

Every generator asserts the property its case is named after, so a later edit cannot quietly turn a case into an ordinary one.
Layouts: ggml.c block_q4_0 .. block_q8_0, k_quants.h block_q2_K .. block_q6_K."""
import numpy as np

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 2, 3, 6, 7, 8
Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 10, 11, 12, 13, 14
LEGACY = [Q4_0, Q4_1, Q5_0, Q5_1, Q8_0]
KQUANTS = [Q2_K, Q3_K, Q4_K, Q5_K, Q6_K]
TYPES = LEGACY + KQUANTS
BLCK = {Q4_0: 32, Q4_1: 32, Q5_0: 32, Q5_1: 32, Q8_0: 32, Q2_K: 256, Q3_K: 256, Q4_K: 256, Q5_K: 256, Q6_K: 256}
TSIZE = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34, Q2_K: 84, Q3_K: 110, Q4_K: 144, Q5_K: 176, Q6_K: 210}
NAME = {Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1", Q8_0: "q8_0", Q2_K: "q2_K", Q3_K: "q3_K", Q4_K: "q4_K", Q5_K: "q5_K", Q6_K: "q6_K"}
# byte offsets of (d, dmin or m) inside a block
D_OFF = {Q4_0: (0, None), Q4_1: (0, 2), Q5_0: (0, None), Q5_1: (0, 2), Q8_0: (0, None),
         Q2_K: (80, 82), Q3_K: (108, None), Q4_K: (0, 2), Q5_K: (0, 2), Q6_K: (208, None)}
# (offset, bytes) of the sub-block scale bytes of a k-quant super-block
SCALE_BYTES = {Q2_K: (0, 16), Q3_K: (96, 12), Q4_K: (4, 12), Q5_K: (4, 12), Q6_K: (192, 16)}
FAMILIES = ["signed_d", "saturated_lo", "saturated_hi", "quantizer"]

D_VALUES = np.array([1e-3, -1e-3, 6e-8, -6e-8, 5.9e-5, 6.1e-5, 3e-5, -3e-5, 0.0, -0.0, 2.0, -2.0], np.float32).astype(np.float16)
D_VALUES_NO_TWO = D_VALUES[:10]
# ordinary magnitudes for the saturated cases: (d, |dmin or m| / d), weights of order 0.02 .. 0.1
_ORDINARY = {Q4_0: (4e-3, 0), Q4_1: (4e-3, 7.5), Q5_0: (2e-3, 0), Q5_1: (2e-3, 15.5), Q8_0: (3e-4, 0),
             Q2_K: (4e-3, 1.5), Q3_K: (5e-4, 0), Q4_K: (1e-4, 7.5), Q5_K: (5e-5, 15.5), Q6_K: (2e-5, 0)}


def row_bytes(t, K):
    return K // BLCK[t] * TSIZE[t]


def _rng(seed, *key):
    return np.random.default_rng([int(seed)] + [int(k) for k in key])


def _put_h(blk, off, h):
    """fp16 values h[M, nb] into bytes off, off + 1 of every block"""
    blk[:, :, off:off + 2] = np.ascontiguousarray(h, np.float16).view(np.uint8).reshape(h.shape[0], h.shape[1], 2)


def get_h(w, t, which=0):
    """the fp16 d (which = 0) or dmin / m (which = 1) of every block of w[M, row_bytes] -> uint16 bit patterns [M, nb]"""
    off = D_OFF[t][which]
    b = np.ascontiguousarray(w).reshape(w.shape[0], -1, TSIZE[t])[:, :, off:off + 2]
    return np.ascontiguousarray(b).view(np.uint16)[:, :, 0]


def _deal(values, shape, rng):
    """every entry of `values` equally often (up to one), in a seeded random order"""
    n = int(np.prod(shape))
    idx = np.resize(np.arange(len(values)), n)
    rng.shuffle(idx)
    return values[idx].reshape(shape)


def h_is_zero(bits):
    return (bits & 0x7FFF) == 0


def h_is_subnormal(bits):
    return ((bits & 0x7C00) == 0) & ((bits & 0x03FF) != 0)


def h_is_negative(bits):
    return (bits & 0x8000) != 0


def dead_rows(w, t):
    """weight rows whose every d (and dmin / m) is +-0: their outputs are 0 by construction"""
    dead = h_is_zero(get_h(w, t, 0)).all(axis=1)
    if D_OFF[t][1] is not None:
        dead &= h_is_zero(get_h(w, t, 1)).all(axis=1)
    return dead


def signed_d(t, M, K, rng, values=D_VALUES):
    nb, ts = K // BLCK[t], TSIZE[t]
    blk = rng.integers(0, 256, size=(M, nb, ts), dtype=np.uint8)
    doff, moff = D_OFF[t]
    # rows 0 and 1 are of ONE kind: -0 in every block (against the all-zero activation row every term is -0: a sum that starts from its first term
    # instead of 0 + term answers -0 where the reference answers +0), and one negative value in every block
    whole = np.array([-0.0, -1e-3], np.float16)
    for off in (doff, moff):
        if off is not None:
            _put_h(blk, off, np.concatenate([np.repeat(whole[:, None], nb, axis=1), _deal(values, (M - 2, nb), rng)]))
    w = blk.reshape(M, nb * ts)
    d = get_h(w, t, 0)
    assert (d[0] == 0x8000).all() and (d[1] == whole.view(np.uint16)[1]).all() and dead_rows(w, t)[0] and not dead_rows(w, t)[1]
    for v in values.view(np.uint16):                            # the whole list is there: both signs, both zeros, 0x0001 and the smallest normal
        assert (d[2:] == v).sum() >= ((M - 2) * nb) // len(values) >= 1, (NAME[t], hex(int(v)))
    assert h_is_negative(d).sum() >= M * nb // 3 and h_is_zero(d).sum() >= M * nb // 8 and h_is_subnormal(d).sum() >= M * nb // 3
    if moff is not None:
        m = get_h(w, t, 1)
        fd, fm = np.abs(d.view(np.float16).astype(np.float32)), np.abs(m.view(np.float16).astype(np.float32))
        assert (h_is_zero(m) & ~h_is_zero(d)).any() and (h_is_zero(d) & ~h_is_zero(m)).any() and (fm > fd).any() and (fd > fm).any(), NAME[t]
    return w


def _ordinary_scales(t, M, nb, rng):
    d0, ratio = _ORDINARY[t]
    sign = rng.choice(np.array([-1.0, 1.0]), size=(M, nb))
    d = (sign * d0 * rng.uniform(0.5, 1.5, size=(M, nb))).astype(np.float16)
    sign = rng.choice(np.array([-1.0, 1.0]), size=(M, nb))
    m = (sign * d0 * ratio * rng.uniform(0.8, 1.2, size=(M, nb))).astype(np.float16)
    return d, m


def _pack_legacy(t, q, d, m):
    """q[M, nb, 32]: unsigned codes (Q8_0: int8 values) -> block bytes"""
    M, nb, _ = q.shape
    blk = np.zeros((M, nb, TSIZE[t]), np.uint8)
    _put_h(blk, 0, d)
    o = 2
    if D_OFF[t][1] is not None:
        _put_h(blk, 2, m)
        o = 4
    if t == Q8_0:
        blk[:, :, o:] = q.astype(np.int8).view(np.uint8)
        return blk.reshape(M, -1)
    q = q.astype(np.uint32)
    if t in (Q5_0, Q5_1):
        qh = ((q >> 4) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32)      # bit i = fifth bit of element i
        blk[:, :, o:o + 4] = np.ascontiguousarray(qh).view(np.uint8).reshape(M, nb, 4)
        o += 4
    blk[:, :, o:] = ((q[:, :, :16] & 15) | ((q[:, :, 16:] & 15) << 4)).astype(np.uint8)
    return blk.reshape(M, -1)


def saturated(t, M, K, rng, hi):
    nb, ts = K // BLCK[t], TSIZE[t]
    d, m = _ordinary_scales(t, M, nb, rng)
    if t in LEGACY:
        lo_v, hi_v = {Q4_0: (0, 15), Q4_1: (0, 15), Q5_0: (0, 31), Q5_1: (0, 31), Q8_0: (-128, 127)}[t]
        ext, opp = (hi_v, lo_v) if hi else (lo_v, hi_v)
        q = np.full((M, nb, 32), ext, np.int32)
        r, b = np.meshgrid(np.arange(M), np.arange(nb), indexing="ij")
        q[r, b, (r + b) % 32] = opp
        assert ((q == ext).sum(axis=2) == 31).all()
        return _pack_legacy(t, q, d, m)
    fill = 0xFF if hi else 0x00
    blk = np.full((M, nb, ts), fill, np.uint8)
    so, sn = SCALE_BYTES[t]
    if t in (Q2_K, Q4_K, Q5_K):
        blk[:, :, so:so + sn] = 0xFF                                   # 4-bit scale and min 15 | 6-bit scale and min 63 (get_scale_min_k4)
    elif t == Q3_K:
        blk[0::2, :, so:so + sn] = 0x00                                # 6-bit code 0  -> scale -32
        blk[1::2, :, so:so + sn] = 0xFF                                # 6-bit code 63 -> scale +31
    else:
        blk[0::2, :, so:so + sn] = 0x80                                # int8 -128
        blk[1::2, :, so:so + sn] = 0x7F                                # int8 +127
    doff, moff = D_OFF[t]
    _put_h(blk, doff, d)
    if moff is not None:
        _put_h(blk, moff, m)
    planes = np.ones(ts, bool)
    planes[so:so + sn] = False
    planes[doff:doff + 2] = False
    if moff is not None:
        planes[moff:moff + 2] = False
    assert (blk[:, :, planes] == fill).all() and planes.sum() == {Q2_K: 64, Q3_K: 96, Q4_K: 128, Q5_K: 160, Q6_K: 192}[t]
    assert not h_is_zero(get_h(blk.reshape(M, -1), t, 0)).any()
    return blk.reshape(M, nb * ts)


def quantizer_rows(M, K, rng):
    """f32 rows for the weight quantizer, kind = row % 5: N(0, 0.02^2) | one sign only (alternating between such rows) | one outlier
    per super-block (six times the spread: a 4-bit format still resolves the rest) | uniform | row 3 and row M - 2: all zero"""
    assert M >= 12
    x = (rng.standard_normal((M, K)) * 0.02).astype(np.float32)
    for r in range(M):
        k = r % 5
        if k == 1:
            x[r] = np.abs(x[r]) * (1.0 if (r // 5) % 2 == 0 else -1.0)
        elif k == 2:
            for s in range(0, K, 256):
                x[r, s + int(rng.integers(0, min(256, K - s)))] = 0.125 if rng.random() < 0.5 else -0.125
        elif k == 3:
            x[r] = rng.uniform(-0.05, 0.05, size=K).astype(np.float32)
    x[3] = 0
    x[M - 2] = 0
    assert (x[1] > 0).all() and (x[6] < 0).all() and (np.abs(x[2]) == 0.125).sum() == (K + 255) // 256 and not x[3].any()
    return x


def weights(t, family, M, K, seed, quantize=None, values=D_VALUES):
    """quantize(t, x[M, K] f32) -> [M, row_bytes] uint8 is needed by the `quantizer` family only (the oracle's on the CPU, the device's on the GPU)"""
    assert K % BLCK[t] == 0 and family in FAMILIES
    rng = _rng(seed, t, FAMILIES.index(family), M, K)
    if family == "signed_d":
        return signed_d(t, M, K, rng, values)
    if family in ("saturated_lo", "saturated_hi"):
        return saturated(t, M, K, rng, family == "saturated_hi")
    w = np.ascontiguousarray(quantize(t, quantizer_rows(M, K, rng)), np.uint8).reshape(M, row_bytes(t, K))
    if t in (Q3_K, Q6_K):                                              # d = 1 / (-32 / max_scale), 1 / (-128 / max_scale): real files carry both signs
        d = get_h(w, t, 0)
        neg, pos = (h_is_negative(d) & ~h_is_zero(d)).sum(), (~h_is_negative(d) & ~h_is_zero(d)).sum()
        assert 4 * neg >= d.size and 4 * pos >= d.size, (NAME[t], int(neg), int(pos), d.size)
    return w


# ---------------------------------------------------------------------------------------------------------------- activations
ACT_ROWS = ["const_pos", "const_neg", "alt_pos_first", "alt_peaked", "sparse_per_superblock", "zero", "normal_1e4", "normal_1e-5", "normal",
            "normal_3e-5", "const_7e6", "alt_neg_first", "ramp", "const_per_16_alt", "one_per_32", "outlier_5e6"]
ACT_C, ACT_PEAK = np.float32(3.0), np.float32(4.0)
ACT_MAX = 8e6          # beyond 65504 * 127 the Q8_0 image's fp16 d is inf and the reference's result NaN: non-finite inputs are out of scope


def q8k_image(x):
    """quantize_row_q8_K_reference (k_quants.c:899-934) in numpy, for the constructed rows (whose products are exact): (q[nb, 256] int, bsums[nb, 16])"""
    x = np.asarray(x, np.float32).reshape(-1, 256)
    q = np.zeros(x.shape, np.int64)
    for b in range(x.shape[0]):
        mx = x[b, np.argmax(np.abs(x[b]))]
        if mx != 0:
            q[b] = np.minimum(127, np.rint((np.float32(-128.0) / mx) * x[b]).astype(np.int64))
    return q, q.reshape(-1, 16, 16).sum(axis=2)


def q8_0_scale_bits(x):
    """fp16 bits of the Q8_0 / Q8_1 block scales amax / 127 of a row"""
    amax = np.abs(np.asarray(x, np.float32).reshape(-1, 32)).max(axis=1)
    return (amax / np.float32(127.0)).astype(np.float16).view(np.uint16)


def activations(K, seed):
    assert K % 32 == 0
    rng = _rng(seed, 99, K)
    A = np.zeros((16, K), np.float32)
    alt = np.where(np.arange(K) % 2 == 0, 1.0, -1.0).astype(np.float32)
    starts = list(range(0, K, 256))
    A[0] = ACT_C
    A[1] = -ACT_C
    A[2] = ACT_C * alt
    A[3] = (ACT_PEAK * np.float32(127.0 / 128.0)) * -alt           # +-127/128 of the peak: Q8_K quants +-127 exactly ...
    A[3, starts] = -ACT_PEAK                                       # ... next to the one -128 a super-block always holds
    sparse = min(256, K // 4)                                      # one non-zero element per super-block; rows of less than four super-blocks: four in the
    for s in range(0, K, sparse):                                  # row, or the output is ONE product and exactly 0 wherever that weight's quant is 0
        A[4, s + int(rng.integers(0, min(sparse, K - s)))] = np.float32(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0))
    A[6] = (1e4 * rng.standard_normal(K)).astype(np.float32)
    A[7] = (1e-5 * rng.standard_normal(K)).astype(np.float32)
    A[8] = rng.standard_normal(K).astype(np.float32)
    A[9] = (3e-5 * rng.standard_normal(K)).astype(np.float32)
    A[10] = 7e6
    A[11] = -ACT_C * alt
    A[12] = np.linspace(-1.0, 1.0, K, dtype=np.float32)
    A[13] = ACT_C * np.where((np.arange(K) // 16) % 2 == 0, 1.0, -1.0)
    A[14, np.arange(0, K, 32) + rng.integers(0, 32, size=K // 32)] = (rng.choice([-1.0, 1.0], size=K // 32) * rng.uniform(0.5, 2.0, size=K // 32)).astype(np.float32)
    A[15] = (2e5 * rng.standard_normal(K)).astype(np.float32)     # next to the outlier the rest keeps a few quant levels
    A[15, starts] = 5e6
    # ---- each row is what its name says
    assert np.isfinite(A).all() and np.abs(A).max() < ACT_MAX
    assert not A[5].any() and all(np.count_nonzero(A[4, s:s + sparse]) == 1 for s in range(0, K, sparse)) and np.count_nonzero(A[4]) >= 4
    assert (np.count_nonzero(A[14].reshape(-1, 32), axis=1) == 1).all()
    for r in (2, 11):                                              # Q8_0 / Q8_1 image: d = c / 127, every |q| = 127, every block sums to zero
        assert (np.abs(A[r]) == ACT_C).all() and not A[r].reshape(-1, 32).sum(axis=1).any()
    for r in (7, 9):                                               # fp16 subnormal Q8_0 / Q8_1 scales, none flushed to zero
        h = q8_0_scale_bits(A[r])
        assert h_is_subnormal(h).all(), ACT_ROWS[r]
    assert not h_is_subnormal(q8_0_scale_bits(A[8])).any()
    if K % 256 == 0:
        q, bs = q8k_image(A[0])
        assert (q == -128).all() and (bs == -2048).all()
        q, bs = q8k_image(A[1])                                    # the largest magnitude maps to -128 WHATEVER its sign (iscale = -128 / max): the
        assert (q == -128).all() and (bs == -2048).all()           # negative constant differs in the sign of d only; +127 / 2032 groups: row 13
        for r in (2, 11):
            q, bs = q8k_image(A[r])
            assert np.isin(q, (-128, 127)).all() and (bs == -8).all()
        q, bs = q8k_image(A[3])
        assert (np.abs(q) >= 127).all() and (q == -128).sum() == len(starts) and (bs[:, 0] == -1).all() and not bs[:, 1:].any()
        q, bs = q8k_image(A[13])
        assert set(np.unique(bs)) == {-2048, 2032}
        q, bs = q8k_image(A[4])
        assert (q.min(axis=1) == -128).all() and (np.count_nonzero(q, axis=1) == 256 // sparse).all()
    return A


def rows_for(A, N):
    """N activation rows: the 16 of activations(), repeated for N = 17 and N = 33"""
    return np.ascontiguousarray(A[np.arange(N) % A.shape[0]])


Q8_1, Q8_K = 9, 15
ACT_TYPE = {Q4_0: Q8_0, Q5_0: Q8_0, Q8_0: Q8_0, Q4_1: Q8_1, Q5_1: Q8_1, Q2_K: Q8_K, Q3_K: Q8_K, Q4_K: Q8_K, Q5_K: Q8_K, Q6_K: Q8_K}


def act_values(act_t, image, K):
    """the values an activation image stands for, f64 [N, K]: block_q8_0 {fp16 d, int8 qs[32]}, block_q8_1 {f32 d, f32 s, int8 qs[32]},
    block_q8_K {f32 d, int8 qs[256], int16 bsums[16]}"""
    img = np.ascontiguousarray(image, np.uint8)
    N = img.shape[0]
    if act_t == Q8_0:
        b = img.reshape(N, K // 32, 34)
        d = np.ascontiguousarray(b[:, :, 0:2]).view(np.float16)[:, :, 0].astype(np.float64)
        q = b[:, :, 2:].view(np.int8)
    elif act_t == Q8_1:
        b = img.reshape(N, K // 32, 40)
        d = np.ascontiguousarray(b[:, :, 0:4]).view(np.float32)[:, :, 0].astype(np.float64)
        q = b[:, :, 8:].view(np.int8)
    else:
        b = img.reshape(N, K // 256, 292)
        d = np.ascontiguousarray(b[:, :, 0:4]).view(np.float32)[:, :, 0].astype(np.float64)
        q = b[:, :, 4:260].view(np.int8)
    return (d[:, :, None] * q.astype(np.float64)).reshape(N, K)


def term_error(y, wv, av):
    """max over the outputs of |y - sum_i w_i x_i| / sum_i |w_i| |x_i|, in f64 over the de-quantized weights wv[M, K] and the values av[N, K] of
    the activation image: the error in units of the terms' magnitude (a row's rms collapses where the terms cancel). Outputs whose
    every term is zero must be zero."""
    wv, av = np.asarray(wv, np.float64), np.asarray(av, np.float64)
    exact, mag = av @ wv.T, np.abs(av) @ np.abs(wv).T
    y = np.asarray(y, np.float64)
    assert np.isfinite(y).all() and not y[mag == 0].any()
    live = mag > 0
    return float((np.abs(y - exact)[live] / mag[live]).max()) if live.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------- the cases
M_ROWS = 37
K_SHAPES = {True: (256, 2304), False: (64, 4544)}       # k-quants: one super-block | a full unit column plus a partial one; legacy likewise
SEED = 20241019
DEQ_ROWS_LONG = (0, 1, 17, 36)                          # the fixture keeps these de-quantized rows of the long saturated cases (all rows of the short ones)


M_ROWS_16 = 48                                          # the k-quants' streaming forms take matrices of whole 16-row tiles only (fq_skinny_q4k_shape)


def cases_of(t, fam):
    """(name, t, family, K, M) of the recorded cases of one format and family: M = 37 at both widths; for the k-quants 48 rows at 2304; legacy signed_d also at 4096"""
    for K in K_SHAPES[t in KQUANTS]:
        yield f"{NAME[t]}_{fam}_{K}", t, fam, K, M_ROWS
    if t in KQUANTS:
        yield f"{NAME[t]}_{fam}_2304_m48", t, fam, 2304, M_ROWS_16
    elif fam == "signed_d":
        # 4544 and 64 end in a partial stage, which the kernels fill with +0 terms: a row of -0 terms sums to +0 there however the sum starts.
        # At 4096 (whole stages, whole waves of units) the sign of such a row's zero is the kernel's own
        yield f"{NAME[t]}_{fam}_4096", t, fam, 4096, M_ROWS


def cases():
    for t in TYPES:
        for fam in FAMILIES:
            yield from cases_of(t, fam)
