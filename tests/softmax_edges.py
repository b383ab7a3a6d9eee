"""Shared by test_softmax_edges_cpu.py and test_gpu_softmax_edges.py: attention inputs whose soft-max rows are known EXACTLY, over the whole fp16 range of
soft_max's EXP table (ggml.c:12426-12450: row maximum, fp16(score - max) -- an f32 subtraction, then an fp16 rounding -- as the table index, an f64 sum,
a scale by (float)(1 / sum)), with the expected outputs in plain numpy and the GPU runners. No test lives here; nothing at import time needs a GPU.

Construction. A query row is q = 8 e_c, so K.Q has ONE non-zero product and q.k / 8 == k[c] in every kernel form and summation order; the 64 components of
a key hold 64 independent score rows (row t of a launch reads component (c0 + t) mod 64). Keys obs0 .. obs0 + 63 carry V[obs0 + d] = e_d and every other
value row is zero, so output element d of a row has ONE non-zero V.P term and is exactly p[obs0 + d] = f32(e * inv). The decode op rotates q itself: raw q
is non-zero in one rotation pair, the cached keys aim 8 tau / rho at one component of the rotated q (rho), the new key's raw row is zero (score 0) and
the new value row is e_63.

Families: S every table index a soft-max can meet (0x8000 .. 0xFC00), T the fix-list inputs of the in-kernel formula, the subnormal results and the
thresholds (for launches with few slots), R differences where one rounding and two roundings part, U uniform rows, W saturated rows, M masked keys that
hold the largest score.

`python tests/softmax_edges.py [group ...]` runs the GPU checks in a process of its own (the library reads its switches once per process)."""
import functools
import os
import re
import sys

import numpy as np

D = 64
H = 8                                   # heads == kv heads: every head has score rows of its own
IDX_FIRST, IDX_LAST = 0x8000, 0xFC00    # the indices s - max <= 0 can produce: -0 .. -inf, 31745 of them
SUBNORMAL_FIRST, ZERO_FIRST = 0xC8DB, 0xCC56      # exp(x) is an fp16 subnormal for inputs 0xC8DB .. 0xCC55 (-9.71 .. -17.33), 0 from 0xCC56 on
THRESHOLDS = [0xCC00, 0xCC0E, 0xCC0F, 0xCC55, 0xCC56, 0x8000, 0x8001, 0xFBFF, 0xFC00]
FIX_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ggllm.cpp_amd", "csrc", "fq_exp_fix.h")
FAULTS = ("single", "ftz", "f32sum", "leak", "offby1")      # soft_max's deliberately wrong restatements (test_softmax_edges_cpu.py)


def fix_list_from_header(path=FIX_HEADER):
    """(input bits, table entry) pairs of csrc/fq_exp_fix.h, parsed from its numeric literals"""
    text = open(path).read()
    body = text[text.index("fq_exp_fix["):]
    words = [int(w, 16) for w in re.findall(r"0x([0-9A-Fa-f]{8})u", body)]
    n = int(re.search(r"#define\s+FQ_EXP_FIX_N\s+(\d+)", text).group(1))
    assert len(words) == n, (len(words), n)
    return [(w >> 16, w & 0xFFFF) for w in words]


def reachable(fix):
    """the fix-list inputs a soft-max can meet: s - max <= 0, i.e. the sign bit set (the list's positive inputs cannot be a soft-max index)"""
    return sorted(b for b, _ in fix if IDX_FIRST <= b <= IDX_LAST)


def table_f32(oracle):
    return oracle.exp_table().view(np.float16).astype(np.float32)


def score_for(bits):
    """f32 scores (under a row maximum of 0) whose table index is `bits`: the fp16 value itself, but -2^-30 for -0 (0 - 0 is +0 in every kernel) and -1e5 for
    -inf (every input stays finite)"""
    bits = np.asarray(bits, np.uint16)
    s = bits.view(np.float16).astype(np.float32)
    s = np.where(bits == 0x8000, np.float32(-2.0 ** -30), s)
    return np.where(bits == 0xFC00, np.float32(-1.0e5), s).astype(np.float32)


def soft_max(tab, s, vis, fault=None, fix_bits=()):
    """the reference's soft_max over the visible keys of each row, restated in numpy: s [..., K] f32, vis [..., K] bool -> (p f32, table indices uint16).
    fault: None, or one of FAULTS -- a deliberately wrong restatement, for showing that the expectations bite."""
    assert fault is None or fault in FAULTS
    s = np.asarray(s, np.float32)
    if fault == "leak":                                        # the first masked key of every row admitted
        vis = vis | np.concatenate([np.ones_like(vis[..., :1]), vis[..., :-1]], axis=-1)
    with np.errstate(over="ignore", invalid="ignore"):
        mx = np.where(vis, s, -np.inf).max(axis=-1, keepdims=True).astype(np.float32)
        if fault == "single":                                   # one rounding of the exact difference
            hb = (s.astype(np.float64) - mx.astype(np.float64)).astype(np.float16)
        else:
            hb = (s - mx).astype(np.float16)                    # f32 subtraction, then the fp16 rounding
    idx = hb.view(np.uint16)
    look = idx
    if fault == "offby1":
        look = np.where(np.isin(idx, np.asarray(list(fix_bits), np.uint16)), idx + 1, idx).astype(np.uint16)
    e = np.where(vis, tab[look], np.float32(0))
    if fault == "ftz":
        e = np.where(e < np.float32(2.0 ** -14), np.float32(0), e)
    if fault == "f32sum":
        total = np.add.accumulate(e, axis=-1, dtype=np.float32)[..., -1:].astype(np.float64)
    else:
        total = e.astype(np.float64).sum(axis=-1, keepdims=True)      # < 2^28 multiples of 2^-24 that are <= 1: exact in any order
    inv = (1.0 / total).astype(np.float32)
    return (e * inv).astype(np.float32), idx


def _fill(rng, shape):
    """random non-positive fp16-representable values (e between 1 and the subnormals): what unobserved keys hold"""
    return (-np.abs(rng.standard_normal(shape) * 4.0)).astype(np.float16).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the prefill op (ggml_hip_attention: q as given)
class PrefillCase:
    """K / V images [n_kv, H, 64] of one layer's caches for a batch of up to n_max rows behind n_past positions. A launch of N <= n_max rows whose row t
    reads component (c0 + t) % 64 sees keys [0, n_past + t]."""

    def __init__(self, name, kc, vc, n_past, n_max, obs0, q_scale=8.0):
        self.name, self.n_past, self.n_max, self.obs0, self.q_scale = name, n_past, n_max, obs0, np.float32(q_scale)
        self.kc, self.vc = np.ascontiguousarray(kc, np.float32), np.ascontiguousarray(vc, np.float32)
        assert self.kc.shape == (n_past + n_max, H, D) and self.vc.shape == self.kc.shape
        assert np.isfinite(self.kc).all() and np.isfinite(self.vc).all()

    def qkv(self, N, c0=0):
        q = np.zeros((N, 3 * H, D), np.float32)
        for t in range(N):
            q[t, :H, (c0 + t) % D] = self.q_scale
        return q

    def scores(self, N, c0=0):
        """(s [N, H, n_kv] as every kernel computes them -- one f32 product, times 0.125 --, vis [N, 1, n_kv])"""
        n_kv = self.n_past + N
        comp = (c0 + np.arange(N)) % D
        with np.errstate(over="ignore"):
            s = ((self.kc[:n_kv][:, :, comp] * self.q_scale).astype(np.float32) * np.float32(0.125)).astype(np.float32)      # [n_kv, H, N]
        vis = np.arange(n_kv)[None, :] <= (self.n_past + np.arange(N))[:, None]
        return np.ascontiguousarray(s.transpose(2, 1, 0)), vis[:, None, :]

    def observed(self, N):
        """[N, 64] bool: output element d of row t is a probability (key obs0 + d is visible); elsewhere the output is 0"""
        return (self.obs0 + np.arange(D))[None, :] <= (self.n_past + np.arange(N))[:, None]

    def expected(self, tab, N, c0=0, fault=None, fix_bits=()):
        """(out [N, H * 64], the table indices [N, H, n_kv])"""
        s, vis = self.scores(N, c0)
        p, idx = soft_max(tab, s, np.broadcast_to(vis, s.shape), fault, fix_bits)
        out = np.zeros((N, H, D), np.float32)
        n_obs = min(D, s.shape[-1] - self.obs0)
        out[:, :, :n_obs] = p[:, :, self.obs0:self.obs0 + n_obs]
        out *= self.observed(N)[:, None, :]
        return out.reshape(N, H * D), idx


def _values(n_kv, obs0):
    vc = np.zeros((n_kv, H, D), np.float32)
    for d in range(min(D, n_kv - obs0)):
        vc[obs0 + d, :, d] = 1.0
    return vc


def _prefill(name, slots, n_past, n_max, seed, key0=None, rest=None):
    """slots [H, 64 components, 64 observed keys] -> keys 1 .. 64; key 0 is `key0` (default: the zero vector, score 0: the maximum of rows <= 0);
    every other key `rest` (default: random non-positive values)"""
    rng = np.random.default_rng(seed)
    n_kv = n_past + n_max
    kc = _fill(rng, (n_kv, H, D)) if rest is None else np.broadcast_to(np.asarray(rest, np.float32), (n_kv, H, D)).copy()
    kc[0] = 0.0 if key0 is None else key0
    kc[1:1 + D] = np.asarray(slots, np.float32).reshape(H, D, D).transpose(2, 0, 1)
    return PrefillCase(name, kc, _values(n_kv, 1), n_past, n_max, 1)


def sweep_bits(n_slots, fix):
    """every index 0x8000 .. 0xFC00 once, the spare slots repeating the reachable fix-list inputs and the thresholds"""
    every = np.arange(IDX_FIRST, IDX_LAST + 1, dtype=np.uint16)
    extra = np.asarray(reachable(fix) + THRESHOLDS, np.uint16)
    assert n_slots >= every.size
    return np.concatenate([every, np.resize(extra, n_slots - every.size)])


def targeted_bits(fix):
    return np.asarray(reachable(fix) + list(range(SUBNORMAL_FIRST, ZERO_FIRST)) + THRESHOLDS, np.uint16)


def family_S(fix, n_past=65, n_max=64):
    """S: the whole sweep in one 64-row launch (8 x 64 x 64 slots). Keys 65 .. n_past - 1 (filler) and the batch's own keys are random non-positive: a row's sum
    depends on where its causal edge is."""
    bits = sweep_bits(H * D * D, fix)
    rng = np.random.default_rng(7)
    slots = score_for(rng.permutation(bits)).reshape(H, D, D)
    return _prefill(f"S@{n_past}", slots, n_past, n_max, seed=n_past)


def family_T(fix, n_past=65, n_max=64):
    """T: the targeted inputs, component-major: components 0 and 1 hold all of them (8 heads x 64 keys each), the others repeat them"""
    t = targeted_bits(fix)
    assert t.size <= 2 * H * D
    by_comp = score_for(np.resize(t, D * H * D)).reshape(D, H, D)                # [component, head, key]
    return _prefill(f"T@{n_past}", by_comp.transpose(1, 0, 2), n_past, n_max, seed=100 + n_past)


T_COMPONENTS = 2


def r_rows():
    """512 maxima m, one per (head, component): the midpoint of two neighbouring fp16 values a < a' (exact in f32: 12 significant bits). Even rows cycle
    through every fp16 binade and the subnormals (exponent fields 0 .. 30); odd rows stay in fields 13 .. 18 (0.25 <= a < 16), where neighbouring inputs
    have different table entries -- for a < 2.4e-4 every entry is 1.0, beyond 17.33 every entry is 0, and there the two ways of rounding give different
    indices but the same probability. Returns (m, tiny, a_bits): tiny = 2^-30 of m's binade, far below half an f32 ulp of m; a_bits the smaller neighbour."""
    r = np.arange(H * D)
    field = np.where(r % 2 == 0, (r // 2) % 31, 13 + (r // 2) % 6)
    a_bits = ((field << 10) | ((r * 37 + 1) % 1023)).astype(np.uint16)           # mantissas 0 .. 1022: a' stays finite
    a = a_bits.view(np.float16).astype(np.float64)
    b = (a_bits + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    m = ((a + b) / 2).astype(np.float32)
    assert (m.astype(np.float64) == (a + b) / 2).all()
    tiny = np.ldexp(1.0, np.frexp(m.astype(np.float64))[1] - 1 - 30).astype(np.float32)
    return m, tiny, a_bits


R_KINDS = 8      # what observed key d of an R row holds is kind d % 8


def family_R(n_past=65, n_max=64):
    """R: key 0 holds a positive maximum m, an fp16 tie (r_rows). Observed key d holds, by d % 8:
      0  the two-roundings score: -tiny where the tie's even neighbour is the smaller one, +tiny where it is the larger one -- f32(s - m) is -m, the tie, which goes
         to the even neighbour; the exact difference lies just off the tie on the odd neighbour's side
      1  the other sign (a near-tie in f32 terms; both ways of rounding agree)        2  s = 0: the plain tie
      3, 4  one f32 ulp of m beyond / before the tie                                  5, 6, 7  65504, 65519.9 and 65520 below the maximum (-65504 | -65504 | -inf)
    Every other key is random non-positive, i.e. below m."""
    m, tiny, a_bits = r_rows()
    even_small = (a_bits & 1) == 0
    pair = np.where(even_small, -tiny, tiny).astype(np.float32)
    ulp = np.spacing(m).astype(np.float32)
    kinds = np.stack([pair, -pair, np.zeros_like(m), -ulp, ulp, (m - np.float32(65504.0)).astype(np.float32),
                      (m - np.float32(65519.9)).astype(np.float32), (m - np.float32(65520.0)).astype(np.float32)], axis=1)          # [512, 8]
    slots = np.tile(kinds, (1, D // R_KINDS)).reshape(H, D, D)
    c = _prefill(f"R@{n_past}", slots, n_past, n_max, seed=200 + n_past, key0=m.reshape(H, D))
    c.pairs = (m, pair)
    return c


W_OTHERS = [-17.34375, -65504.0, -1.0e5, -3.0e38]
W_N16 = 2300     # keys at exactly -16.0 in row type 12: each adds 2 x 2^-24, the sum is 1 + 4600 x 2^-24
W_TYPES = 14


def family_W(n_past=2301, n_max=64):
    """W: component c's row is of type c % W_TYPES --
      0-3   key 0 at 0, every other key at W_OTHERS[type]                      4-7   key 0 at +60000, every other key at 60000 + W_OTHERS[type - 4]
      8-11  key 0 at +60000, every other key at 0, -1, -17.34375, -60000       12    key 0 at 0, keys 1 .. 2300 at -16.0, the rest at -1e5 (e = 0)
      13    as 12 with -17.0: each key adds 2^-24, HALF an f32 ulp of 1.0 -- an f32 sum that starts at key 0 never moves (type 12's 2^-23 terms it adds exactly)
    (60000 + x is formed in f32 here: the kernels get that f32)"""
    assert n_past >= W_N16 + 1
    n_kv = n_past + n_max
    kc = np.zeros((n_kv, H, D), np.float32)
    big = np.float32(60000.0)
    for c in range(D):
        k = c % W_TYPES
        if k < 4:
            key0, rest = 0.0, np.float32(W_OTHERS[k])
        elif k < 8:
            key0, rest = big, big + np.float32(W_OTHERS[k - 4])
        elif k < 12:
            key0, rest = big, np.float32([0.0, -1.0, -17.34375, -60000.0][k - 8])
        else:
            key0, rest = 0.0, np.float32(-1.0e5)
        kc[:, :, c] = rest
        kc[0, :, c] = key0
        if k >= 12:
            kc[1:1 + W_N16, :, c] = -16.0 if k == 12 else -17.0
    return PrefillCase(f"W@{n_past}", kc, _values(n_kv, 1), n_past, n_max, 1)


def family_M(n_past=65, n_max=64):
    """M: batch key u (position n_past + u) holds +30000 in every component t < u -- the rows that must not see it (launch with c0 = 0) -- and random
    non-positive values elsewhere. n_past = 0: obs0 = 0, row 0 has a single visible key."""
    rng = np.random.default_rng(300 + n_past)
    n_kv = n_past + n_max
    kc = _fill(rng, (n_kv, H, D))
    kc[0] = 0.0
    u, t = np.arange(n_max)[:, None], np.arange(D)[None, :]
    kc[n_past:] = np.where((t < u)[:, None, :], np.float32(30000.0), kc[n_past:])
    obs0 = 1 if n_past >= 1 + D else 0
    return PrefillCase(f"M@{n_past}", kc, _values(n_kv, obs0), n_past, n_max, obs0)


U_SIZES = [1, 2, 33, 257, 1025, 2369]


def family_U(n_kv, n_max=33):
    """U: q = 0, so every score is (+-)0, every e is 1.0 and p = f32(1 / visible keys); the last row of an n_max-row launch sees n_kv keys where n_kv >= n_max,
    its first rows see 1, 2, ... otherwise. Keys hold random values (times a zero q); obs0 = 0."""
    n_past = max(n_kv - n_max, 0)
    rng = np.random.default_rng(400 + n_kv)
    kc = _fill(rng, (n_past + n_max, H, D))
    return PrefillCase(f"U@{n_kv}", kc, _values(n_past + n_max, 0), n_past, n_max, 0, q_scale=0.0)


# ------------------------------------------------------------------------------------------------ the decode op (ggml_hip_attention_decode rotates q itself)
N_SEQ = 16
DEC_OBS = D - 1      # 63 observed cached keys per row; output element 63 observes the new key through the new value row


def decode_case(oracle, targets, n_past, obs0, seed, key0=None):
    """one sequence: targets [H, 63] = the scores wanted for cached keys obs0 .. obs0 + 62. Returns (decode_attn.Case, scores [H, n_past + 1] as the kernel
    computes them). Head h's raw q is 8 in component h of rotation pair (h, h + 32); rho is the larger component of its rotation."""
    import decode_attn as da
    assert n_past >= obs0 + DEC_OBS
    rng = np.random.default_rng(seed)
    qkv = np.zeros((3 * H, D), np.float32)
    qkv[np.arange(H), np.arange(H)] = 8.0
    qkv[2 * H:, D - 1] = 1.0                                    # the new value row: e_63
    q_rot = da.rope_at(oracle, qkv[:H], n_past)
    comp = np.where(np.abs(q_rot[np.arange(H), np.arange(H)]) >= np.abs(q_rot[np.arange(H), np.arange(H) + 32]), np.arange(H), np.arange(H) + 32)
    rho = q_rot[np.arange(H), comp].astype(np.float64)
    tau = _fill(rng, (n_past, H))
    tau[0] = 0.0 if key0 is None else key0
    tau[obs0:obs0 + DEC_OBS] = np.asarray(targets, np.float32).T
    kc = np.zeros((n_past, H, D), np.float32)
    kc[:, np.arange(H), comp] = (8.0 * tau.astype(np.float64) / rho[None, :]).astype(np.float32)
    vc = np.zeros((n_past, H, D), np.float32)
    for d in range(DEC_OBS):
        vc[obs0 + d, :, d] = 1.0
    s = np.zeros((H, n_past + 1), np.float32)                   # the new key's raw row is zero: score 0
    s[:, :n_past] = ((q_rot[np.arange(H), comp][None, :] * kc[:, np.arange(H), comp]).astype(np.float32) * np.float32(0.125)).T
    return da.Case(oracle, H, H, n_past, qkv, kc, vc), s


def decode_expected(tab, s, obs0, fault=None, fix_bits=()):
    """s [H, n_kv] -> (out [H * 64], indices [H, n_kv])"""
    p, idx = soft_max(tab, s, np.ones(s.shape, bool), fault, fix_bits)
    out = np.concatenate([p[:, obs0:obs0 + DEC_OBS], p[:, -1:]], axis=1)
    return out.reshape(-1), idx


DEC_SWEEP_LAUNCHES = 4


def decode_family(oracle, name, fix, positions, obs0, launch=0):
    """len(positions) sequences of family `name` -> [(Case, scores)]. S: quarter `launch` of the sweep (16 sequences); T: the targeted inputs (one launch of 16
    sequences, two launches of one); W: a cached maximum of +16.25 in key 0 (the new key's 0 - 16.25 gives the subnormal entry 1) over the targeted inputs
    raised by 16.25 where that is exact."""
    n_seq = len(positions)
    per = n_seq * H * DEC_OBS
    if name == "S":
        rng = np.random.default_rng(11)
        bits = rng.permutation(sweep_bits(DEC_SWEEP_LAUNCHES * per, fix))[launch * per:(launch + 1) * per]
        targets, key0 = score_for(bits), None
    else:
        t = targeted_bits(fix)
        targets, key0 = score_for(np.resize(t, max(t.size, (launch + 1) * per))[launch * per:(launch + 1) * per]), None
        if name == "W":
            up = (targets + np.float32(16.25)).astype(np.float32)
            exact = (up.astype(np.float64) == targets.astype(np.float64) + 16.25) & (np.abs(targets) < 60000.0)
            targets, key0 = np.where(exact, up, np.float32(-1.0e5)).astype(np.float32), np.float32(16.25)
    targets = targets.reshape(n_seq, H, DEC_OBS)
    return [decode_case(oracle, targets[i], int(positions[i]), obs0, 1000 * launch + i, key0) for i in range(n_seq)]


# ------------------------------------------------------------------------------------------------ the GPU side
def _first_diff(got, exp):
    d = np.flatnonzero(got.view(np.uint32).ravel() != exp.view(np.uint32).ravel())
    d = d[(got.ravel()[d] != exp.ravel()[d]) | np.isnan(got.ravel()[d])]                 # (+0 == -0)
    return f"{d.size} of {got.size} elements differ, first at {int(d[0])}: {got.flat[d[0]]!r} != {exp.flat[d[0]]!r}" if d.size else ""


class Gpu:
    """the library, the oracle's table, the device's fix list and a rope table, made once per process"""

    def __init__(self):
        import ggllm_cpp_amd as g
        from oracle import binding as ob
        import decode_attn as da
        self.g, self.da = g, da
        g.init(0)
        self.L = g.load()
        self.oracle = ob.Oracle()
        self.tab = table_f32(self.oracle)
        buf = np.zeros(4096, np.uint32)
        n = self.L.ggml_hip_debug_exp_boundary(buf.ctypes.data, buf.size)
        assert 0 <= n <= buf.size
        self.fix = [(int(w) >> 16, int(w) & 0xFFFF) for w in buf[:n]]
        self.rope = self.L.ggml_hip_rope_table_create(D, 512, da.ROPE_CTX)

    @functools.lru_cache(maxsize=None)
    def case(self, family, *args):
        if family in ("S", "T"):
            return {"S": family_S, "T": family_T}[family](self.fix, *args)
        return {"R": family_R, "W": family_W, "M": family_M, "U": family_U}[family](*args)

    @functools.lru_cache(maxsize=None)
    def decode_cases(self, name, positions, obs0, launch):
        return decode_family(self.oracle, name, self.fix, positions, obs0, launch)

    def prefill(self, case, N, c0=0, form=None, order=0):
        """one ggml_hip_attention launch -> complaint ('' when every output bit is the expected one)"""
        g, L = self.g, self.L
        n_kv = case.n_past + N
        qb, kb, vb, ob_ = g.DevBuf(host=case.qkv(N, c0)), g.DevBuf(host=case.kc[:n_kv]), g.DevBuf(host=case.vc[:n_kv]), g.DevBuf(N * H * D * 4)
        try:
            if form is not None:
                L.ggml_hip_debug_attention_form(form)
            L.ggml_hip_reference_order(order)
            L.ggml_hip_memset(ob_.ptr, 0xFF, N * H * D * 4)
            L.ggml_hip_attention(qb.ptr, N, H, H, D, case.n_past, kb.ptr, vb.ptr, ob_.ptr)
            got = ob_.to_host(np.float32, (N, H * D))
        finally:
            L.ggml_hip_reference_order(0)
            L.ggml_hip_debug_attention_form(0)
            for b in (qb, kb, vb, ob_):
                b.free()
        exp, _ = case.expected(self.tab, N, c0)
        bad = _first_diff(got, exp)
        return f"{case.name} N={N} c0={c0} form={form} order={order}: {bad}" if bad else ""

    def decode(self, name, positions, obs0, pos_stride, max_n_kv, order, launch=0):
        da = self.da
        cs = self.decode_cases(name, tuple(positions), obs0, launch)
        rng = np.random.default_rng(5)
        caches = [da.build_cache(c, max_n_kv, da.FILL_RANDOM, rng) for c, _ in cs]
        kcs, vcs = [k for k, _ in caches], [v for _, v in caches]
        self.L.ggml_hip_reference_order(order)
        try:
            att, k_after, v_after, _ = da.run_gpu(self.g, [c for c, _ in cs], kcs, vcs, pos_stride, max_n_kv, self.rope)
        finally:
            self.L.ggml_hip_reference_order(0)
        bad = []
        for i, (c, s) in enumerate(cs):
            d = _first_diff(att[i], decode_expected(self.tab, s, obs0)[0])
            if d:
                bad.append(f"seq {i} at {c.n_past}: {d}")
        bad += da.check_caches([c for c, _ in cs], kcs, vcs, k_after, v_after)
        return f"decode {name} launch {launch} order {order}: " + "; ".join(bad[:4]) if bad else ""


FORMS = [32, 0, 1, 16, 17]
S_N_PAST = [65, 600, 1500, 2200, 2400]       # with N = 64: flash pitch 16 / 32 / 64 / 74 tiles and the LONG form
SHORT = {"n1": (1, 65), "n3": (3, 65), "n31": (31, 65), "n16_scratch": (16, 3500)}      # N, n_past: k_attention, 2 and 4 rows per workgroup, score rows in the global scratch
# pos_stride, positions, first observed key, max_n_kv. same_300: the observed keys lie in the second 128-row step; single: one sequence (k_attn_decode / k_attn_decode_f64)
DECODE_ROUTES = {"same_65": (0, [65] * N_SEQ, 1, 128), "same_300": (0, [300] * N_SEQ, 130, 384), "ragged": (1, list(range(65, 65 + N_SEQ)), 1, 128),
                 "single": (0, [65], 1, 128)}


def _forms(G, case, N=64):
    return [G.prefill(case, N, 0, form) for form in FORMS]


def _short(G, route, family, order):
    N, n_past = SHORT[route]
    w_past = max(n_past, W_N16 + 1)
    if family == "S":                                       # N = 31: three launches whose rows read components 0-30, 31-61, 62-63 and 0-28
        return [G.prefill(G.case("S", n_past, 64), N, c0, None, order) for c0 in range(0, D, N)]
    if family == "T":
        return [G.prefill(G.case("T", n_past, 64), N, c0, None, order) for c0 in range(0, T_COMPONENTS, N)]
    if family == "R":
        return [G.prefill(G.case("R", n_past, 64), N, c0, None, order) for c0 in range(0, min(D, 8 * N), N)]
    if family == "W":
        return [G.prefill(G.case("W", w_past, 64), N, c0, None, order) for c0 in range(0, W_TYPES, N)]
    if family == "M":
        return [G.prefill(G.case("M", n_past, 64), N, 0, None, order), G.prefill(G.case("M", 0, 64), N, 0, None, order)]
    return [G.prefill(G.case("U", n_kv, N), N, 0, None, order) for n_kv in U_SIZES + [n_past + N]]      # (the last size: the route's own key count)


def gpu_checks():
    """[(group, route, family, fn(Gpu) -> list of complaints)]: every launch the GPU test file makes, in the default process and in the formula children"""
    out = []
    for fam, args in (("R", (65, 64)), ("W", (W_N16 + 1, 64)), ("M", (65, 64)), ("M", (0, 64))):
        out.append(("prefill", "forms", f"{fam}@{args[0]}", lambda G, fam=fam, args=args: _forms(G, G.case(fam, *args))))
    for n_past in S_N_PAST:
        out.append(("prefill", "forms", f"S@{n_past}", lambda G, n_past=n_past: _forms(G, G.case("S", n_past, 64))))
    out.append(("prefill", "forms", "U", lambda G: [r for n_kv in U_SIZES for r in _forms(G, G.case("U", n_kv, 33), 33)]))
    for route in SHORT:
        for order in (0, 1):
            for fam in (["S"] if route == "n31" else ["T", "R", "W", "M", "U"]):
                out.append(("short", f"{route}/order{order}", fam, lambda G, route=route, fam=fam, order=order: _short(G, route, fam, order)))
    for route, (stride, positions, obs0, max_n_kv) in DECODE_ROUTES.items():
        for order in (0, 1):
            a = (positions, obs0, stride, max_n_kv, order)
            if len(positions) == N_SEQ:
                out.append(("decode", f"{route}/order{order}", "S", lambda G, a=a: [G.decode("S", *a, launch=i) for i in range(DEC_SWEEP_LAUNCHES)]))
            out.append(("decode", f"{route}/order{order}", "T+W", lambda G, a=a: [G.decode(f, *a, launch=i) for f in "TW" for i in range(t_launches(G.fix, len(a[0])))]))
    return out


def t_launches(fix, n_seq):
    return -(-targeted_bits(fix).size // (n_seq * H * DEC_OBS))


def main(argv):
    """the checks of the named groups (default: all) in this process; one line per (route, family), exit status 1 at the first mismatch. With
    GGML_HIP_EXP_FORMULA=1 in the environment the formula must really be in use."""
    G = Gpu()
    if os.environ.get("GGML_HIP_EXP_FORMULA"):
        assert G.L.ggml_hip_exp_formula_mismatches() == 0, "the in-kernel formula is not in use"
    for group, route, family, fn in gpu_checks():
        if argv and group not in argv:
            continue
        bad = [b for b in fn(G) if b]
        print(f"{group} {route} {family}: {'ok' if not bad else bad[0]}", flush=True)
        if bad:
            return 1
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(main(sys.argv[1:]))
