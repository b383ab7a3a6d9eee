"""Shared by the decode-attention tests: the plain numpy f64 attention, host-side case builders (random cases and the "which key is
where" probe), their expected values through the oracle's orc_attention_decode, and the op-level GPU runner (ggml_hip_attention_decode).
No test lives here; the builders need no GPU, so the CPU suite can check that the expected values bite (test_decode_attn_cases_cpu.py)."""
import numpy as np

D = 64
ROPE_CTX = 2048            # the rope table's n_ctx (NTK alpha 1); any value does as long as host and device use the same
ORDER_OF = {0: 2, 1: 0}    # ggml_hip_reference_order value -> the oracle's orc_set_sum_order that restates it

# positions of the issue's B1 list
N_PAST_ALL = [0, 1, 15, 16, 17, 126, 127, 128, 129, 254, 255, 256, 257, 383, 384, 385, 511, 512, 513, 639, 640, 641, 1023, 1024, 2047, 4095, 8191]
N_PAST_WIDE = [0, 127, 128, 255, 256, 257, 384, 385, 513, 2047, 8191]
HEADS_SMALL = [(4, 1), (8, 2)]
HEADS_WIDE = [(71, 1), (128, 8), (232, 8)]       # Falcon-7B, -40B, -180B


def attention_ref(oracle, q, kc, vc, n_past, H, HKV):
    """numpy restatement of K.Q -> scale -> mask -> soft_max -> V.P with f32 products / f64 accumulation"""
    N = q.shape[0]
    out = np.zeros((N, H * D), np.float32)
    for t in range(N):
        n_kv = n_past + t + 1
        for h in range(H):
            hk = h // (H // HKV)
            prod = (kc[:n_kv, hk, :] * q[t, h][None, :]).astype(np.float32)
            s = (prod.astype(np.float64).sum(axis=1)).astype(np.float32) * np.float32(0.125)
            p = oracle.softmax_rows(s[None, :])[0]
            pv = (vc[:n_kv, hk, :] * p[:, None]).astype(np.float32)
            out[t, h * D:(h + 1) * D] = pv.astype(np.float64).sum(axis=0).astype(np.float32)
    return out


def context_bound(n_past):
    """a context-sized max_n_kv well above the position: the captured graph's sizing"""
    return 2048 if n_past < 2047 else 2 * (n_past + 1)


def rope_at(oracle, x, pos):
    """x [n_head, 64] at position pos"""
    x = np.ascontiguousarray(x, np.float32)
    return oracle.rope(x[None], D, x.shape[0], 1, pos, ROPE_CTX)[0]


def rope_rows(oracle, x):
    """x [n, n_head, 64], row j at position j"""
    x = np.ascontiguousarray(x, np.float32)
    if x.shape[0] == 0:
        return x.copy()
    return oracle.rope(x, D, x.shape[1], x.shape[0], 0, ROPE_CTX)


class Case:
    """one sequence's decode step: qkv [H + 2 HKV, 64] unrotated, kc / vc [n_past, HKV, 64] the rows already cached (keys rotated)"""

    def __init__(self, oracle, H, HKV, n_past, qkv, kc, vc):
        self.H, self.HKV, self.n_past = H, HKV, n_past
        self.qkv = np.ascontiguousarray(qkv, np.float32)
        self.kc, self.vc = np.ascontiguousarray(kc, np.float32), np.ascontiguousarray(vc, np.float32)
        self.q_rot = rope_at(oracle, self.qkv[:H], n_past)
        self.k_new = rope_at(oracle, self.qkv[H:H + HKV], n_past)          # what the kernel must append at row n_past
        self.v_new = self.qkv[H + HKV:].copy()
        self._exp = {}

    def keys(self):
        return np.concatenate([self.kc, self.k_new[None]], axis=0)

    def values(self):
        return np.concatenate([self.vc, self.v_new[None]], axis=0)

    def expected(self, oracle, order):
        """[H * 64] through orc_attention_decode under orc_set_sum_order(order)"""
        if order not in self._exp:
            oracle.lib.orc_set_sum_order(order)
            try:
                self._exp[order] = oracle.attention_decode(self.q_rot, self.keys(), self.values(), self.H, self.HKV).reshape(-1)
            finally:
                oracle.lib.orc_set_sum_order(0)
        return self._exp[order]


def random_case(oracle, H, HKV, n_past, seed):
    """standard_normal q / k / v (as test_attention draws them); the cached keys are rotated at their own positions"""
    rng = np.random.default_rng(seed)
    qkv = rng.standard_normal((H + 2 * HKV, D)).astype(np.float32)
    kc = rope_rows(oracle, rng.standard_normal((n_past, HKV, D)).astype(np.float32))
    vc = rng.standard_normal((n_past, HKV, D)).astype(np.float32)
    return Case(oracle, H, HKV, n_past, qkv, kc, vc)


def case_seed(H, HKV, n_past, salt=0):
    return 1000003 * H + 7919 * HKV + 31 * n_past + salt


PROBE_J = [0, 1, 15, 16, 126, 127, 128, 129, 254, 255, 256, 257, 383, 384, 385, 511, 512]
PROBE_N_PAST = [129, 257, 385, 513, 1025]


def probe_targets(n_past):
    return sorted({j for j in PROBE_J + [n_past - 1, n_past] if 0 <= j <= n_past})


def probe_case(oracle, H, HKV, n_past, j_star, seed):
    """Every key is zero except row j_star[hk] of kv head hk, which is r * 256 / |r|^2 for the rotated q `r` of the group's first head: that key scores 32
    (times 1 + h_in_group / 4 for the group's other heads, whose q is that multiple of the first's), every other key scores exactly 0, fp16 exp(-32) is
    exactly 0, so the probabilities are exactly 1 and 0 and head h's output is value row j_star[hk] of its kv head, bit for bit, in any association.
    j_star[hk] == n_past: the key goes into qkv unrotated (q * 256 / |q|^2; the kernel rotates both). Returns (case, expected [H * 64])."""
    rng = np.random.default_rng(seed)
    group = H // HKV
    qkv = np.zeros((H + 2 * HKV, D), np.float32)
    q0 = rng.standard_normal((HKV, D)).astype(np.float32)
    for h in range(H):
        qkv[h] = q0[h // group] * np.float32(1.0 + 0.25 * (h % group))
    qkv[H + HKV:] = rng.standard_normal((HKV, D)).astype(np.float32)
    kc = np.zeros((n_past, HKV, D), np.float32)
    vc = rng.standard_normal((n_past, HKV, D)).astype(np.float32)
    r = rope_at(oracle, qkv[:H], n_past)
    for hk in range(HKV):
        j = int(j_star[hk])
        assert 0 <= j <= n_past
        if j == n_past:
            q = q0[hk].astype(np.float64)
            qkv[H + hk] = (q * 256.0 / (q ** 2).sum()).astype(np.float32)
        else:
            rr = r[hk * group].astype(np.float64)
            kc[j, hk] = (rr * 256.0 / (rr ** 2).sum()).astype(np.float32)
    c = Case(oracle, H, HKV, n_past, qkv, kc, vc)
    V = c.values()
    exp = np.stack([V[int(j_star[h // group]), h // group] for h in range(H)]).reshape(-1)
    return c, exp


# ------------------------------------------------------------------------------------------------ the GPU side
FILL_RANDOM, FILL_ZERO, FILL_HUGE = "random", "zero", "huge"


def build_cache(case, max_n_kv, fill, rng, at_n_past=None):
    """[max_n_kv, HKV, 64] K and V images of one sequence's cache: rows [0, n_past) the case's, row n_past and the rows past it filled
    (finite values on purpose: the kernel's contract is a finite re-read times a zero weight, and the model zero-fills its caches)"""
    shape = (max_n_kv, case.HKV, D)
    out = []
    for live in (case.kc, case.vc):
        if fill == FILL_ZERO:
            a = np.zeros(shape, np.float32)
        elif fill == FILL_HUGE:
            a = np.full(shape, 3.0e38, np.float32)
            a[1::2] *= -1
        else:
            a = rng.standard_normal(shape).astype(np.float32)
        a[:case.n_past] = live
        if at_n_past is not None:
            a[case.n_past] = at_n_past
        out.append(a)
    return out


def run_gpu(g, cases, kcs, vcs, pos_stride, max_n_kv, tab, act_type=None, want_att=True):
    """ggml_hip_attention_decode over len(cases) sequences (one row each, caches [max_n_kv, HKV, 64] per sequence).
    Returns (att [n_seq, H * 64], k_after, v_after [n_seq, max_n_kv, HKV, 64], image bytes [n_seq, ...] or None)"""
    L = g.load()
    H, HKV, n_seq = cases[0].H, cases[0].HKV, len(cases)
    qkv = np.stack([c.qkv for c in cases])
    pos = np.array([c.n_past for c in cases], np.int32)
    if pos_stride == 0:
        assert (pos == pos[0]).all()
    kc, vc = np.stack(kcs), np.stack(vcs)
    assert kc.shape == (n_seq, max_n_kv, HKV, D) and vc.shape == kc.shape and int(pos.max()) < max_n_kv
    qb, kb, vb, pb = g.DevBuf(host=qkv), g.DevBuf(host=kc), g.DevBuf(host=vc), g.DevBuf(host=pos)
    ab = g.DevBuf(n_seq * H * D * 4)
    L.ggml_hip_memset(ab.ptr, 0xFF, n_seq * H * D * 4)
    acts = L.ggml_hip_acts_alloc(act_type, H * D, n_seq) if act_type is not None else None
    try:
        L.ggml_hip_attention_decode(qb.ptr, n_seq, H, HKV, pb.ptr, pos_stride, max_n_kv, tab, kb.ptr, vb.ptr, max_n_kv * HKV * D,
                                    ab.ptr if want_att else None, acts, act_type if act_type is not None else 0)
        att = ab.to_host(np.float32, (n_seq, H * D))
        k_after, v_after = kb.to_host(np.float32, kc.shape), vb.to_host(np.float32, vc.shape)
        image = None
        if acts is not None:
            nbytes = n_seq * (H * D // g.BLCK[act_type]) * g.TSIZE[act_type]
            ib = g.DevBuf(nbytes)
            L.ggml_hip_acts_export(acts, n_seq, ib.ptr)
            image = ib.to_host(np.uint8, (n_seq, nbytes // n_seq))
            ib.free()
    finally:
        if acts is not None:
            L.ggml_hip_acts_free(acts)
        for b in (qb, kb, vb, pb, ab):
            b.free()
    return att, k_after, v_after, image


def check_caches(cases, kcs, vcs, k_after, v_after):
    """row n_past of every kv head == the rotated new key / the new value, every other row untouched; returns a list of complaints"""
    bad = []
    for t, c in enumerate(cases):
        n = c.n_past
        if not np.array_equal(k_after[t, n], c.k_new):
            bad.append(f"seq {t}: key row {n} is not the rotated new key")
        if not np.array_equal(v_after[t, n], c.v_new):
            bad.append(f"seq {t}: value row {n} is not the new value")
        for name, before, after in (("key", kcs[t], k_after[t]), ("value", vcs[t], v_after[t])):
            same = (before.view(np.uint32) == after.view(np.uint32)).reshape(before.shape[0], -1).all(axis=1)
            same[n] = True
            if not same.all():
                bad.append(f"seq {t}: {name} rows {np.flatnonzero(~same)[:8].tolist()} were written")
    return bad
