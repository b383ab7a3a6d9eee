"""CPU: orc_attention_decode (the oracle's decode-step attention at op level) is pinned against the whole-model oracle and against a plain
Python loop, and the host-side expected values of the GPU decode-attention tests (tests/decode_attn.py) are shown to bite: a deliberately wrong
HOST model of the kernel -- two key rows swapped, the last key dropped, the neighbouring kv head -- gives other bits."""
import numpy as np
import pytest

from oracle import binding as ob
import synth
import decode_attn as da


def _block0_by_hand(oracle, w, mo, tok_hidden, n_past, n_ctx):
    """block 0 of a one-token eval recomputed op by op from the bindings, the attention through orc_attention_decode on the q the eval formed
    (oracle.rope of its Wqkv row) and the K / V rows the eval left in the oracle's caches. Returns (block output, rotated new key, K rows, V rows)."""
    hp = w["hparams"]
    E, H, HKV, FF = hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_ff"]
    t, lw = w["wtype"], w["layers"][0]
    x = tok_hidden
    ln = oracle.layer_norm(x, lw["ln_w"], lw["ln_b"])
    ln_att = oracle.layer_norm(x, lw["ln2_w"], lw["ln2_b"]) if hp.get("two_norms") else ln
    qkv = oracle.mul_mat(t, lw["qkv"], E, (H + 2 * HKV) * 64, ln_att, 4)[0].reshape(H + 2 * HKV, 64)
    q = oracle.rope(qkv[None, :H], 64, H, 1, n_past, n_ctx)[0]
    k_new = oracle.rope(qkv[None, H:H + HKV], 64, HKV, 1, n_past, n_ctx)[0]
    kc, vc = mo.keep[-2], mo.keep[-1]                                     # the oracle's caches: [n_layer][n_ctx][HKV][64]
    K = kc[:n_ctx * HKV * 64].reshape(n_ctx, HKV, 64)[:n_past + 1]
    V = vc[:n_ctx * HKV * 64].reshape(n_ctx, HKV, 64)[:n_past + 1]
    att = oracle.attention_decode(q, K, V, H, HKV).reshape(1, E)
    wo = oracle.mul_mat(t, lw["wo"], E, E, att, 4)
    up = oracle.gelu(oracle.mul_mat(t, lw["up"], E, FF, ln, 4))
    down = oracle.mul_mat(t, lw["down"], FF, E, up, 4)
    return ((down + wo) + x).astype(np.float32), k_new, K, V, q, att


@pytest.mark.parametrize("hp_name,wtype", [("HP_TINY_MQA", ob.Q4_0), ("HP_TINY_GQA", ob.Q5_1)])
@pytest.mark.parametrize("order", [0, 2])
def test_attention_decode_reproduces_the_whole_model_oracle(oracle, hp_name, wtype, order):
    """a decode step of a tiny model after a 150-token context: the block's output recomputed with orc_attention_decode in the middle equals
    orc_falcon_eval's hidden row bit for bit, in the reference order (0) and in the backend's (2); the key it appended is oracle.rope's.
    (The eval does not expose its attention output, so it is checked INDIRECTLY, through block 0's output row: Wo, the MLP branch and the residual are
    recomputed with the same bindings; the last lines show that a changed attention output does move that row's input.)"""
    hp = dict(getattr(synth, hp_name))
    w = synth.make_model(oracle, hp, wtype, seed=11)
    n_ctx, n_past = 256, 150
    toks = synth.tokens(n_past + 1, hp["n_vocab"], seed=5)
    oracle.lib.orc_set_sum_order(order)
    try:
        mo = oracle.model(w, n_ctx)
        for p0 in range(0, n_past, 30):                                   # chunks below the matrix-pipe attention's 32 tokens
            mo.eval(toks[p0:p0 + 30], p0, 4)
        _, hidden = mo.eval(toks[n_past:], n_past, 4, want_hidden=True)
        out, k_new, K, V, q, att = _block0_by_hand(oracle, w, mo, hidden[0], n_past, n_ctx)
        assert np.array_equal(K[n_past], k_new)
        assert np.array_equal(out, hidden[1])
        # and the comparison can fail: one key fewer, or two value rows swapped, moves the block's output
        V2 = V.copy()
        V2[[3, 4]] = V2[[4, 3]]
        for Kx, Vx in ((K[:-1], V[:-1]), (K, V2)):
            assert not np.array_equal(oracle.attention_decode(q, Kx, Vx, hp["n_head"], hp["n_head_kv"]).reshape(1, -1), att)
    finally:
        oracle.lib.orc_set_sum_order(0)


@pytest.mark.parametrize("H,HKV,n_kv", [(4, 1, 1), (8, 2, 17), (5, 1, 300), (16, 8, 129)])
def test_attention_decode_order0_is_the_plain_loop(oracle, H, HKV, n_kv):
    """order 0 == f32 products, a sequential f64 sum, the softmax_rows binding, written as a plain Python loop -- bit for bit"""
    rng = np.random.default_rng(H * 1000 + n_kv)
    q = rng.standard_normal((H, 64)).astype(np.float32)
    K = rng.standard_normal((n_kv, HKV, 64)).astype(np.float32)
    V = rng.standard_normal((n_kv, HKV, 64)).astype(np.float32)
    got = oracle.attention_decode(q, K, V, H, HKV)
    exp = np.zeros((H, 64), np.float32)
    for h in range(H):
        hk = h // (H // HKV)
        s = np.zeros(n_kv, np.float32)
        for j in range(n_kv):
            acc = 0.0
            for d in range(64):
                acc += float(np.float32(K[j, hk, d] * q[h, d]))
            s[j] = np.float32(acc) * np.float32(0.125)
        p = oracle.softmax_rows(s[None, :])[0]
        for d in range(64):
            acc = 0.0
            for j in range(n_kv):
                acc += float(np.float32(V[j, hk, d] * p[j]))
            exp[h, d] = np.float32(acc)
    assert np.array_equal(got, exp)


def _mutants(oracle, c, order):
    """wrong host models of the kernel for the case c: name -> output"""
    K, V = c.keys(), c.values()
    n = K.shape[0]
    out = {}

    def run(Kx, Vx):
        oracle.lib.orc_set_sum_order(order)
        try:
            return oracle.attention_decode(c.q_rot, Kx, Vx, c.H, c.HKV).reshape(-1)
        finally:
            oracle.lib.orc_set_sum_order(0)
    if n >= 2:
        out["last key dropped"] = run(K[:-1], V[:-1])
        out["newest key replaced by the row before it"] = run(np.concatenate([K[:-1], K[-2:-1]]), V)
        for j in sorted({0, min(n // 2, n - 2), n - 2}):
            Ks, Vs = K.copy(), V.copy()
            Ks[[j, j + 1]] = Ks[[j + 1, j]]
            out[f"key rows {j} and {j + 1} swapped"] = run(Ks, V)
            Vs[[j, j + 1]] = Vs[[j + 1, j]]
            out[f"value rows {j} and {j + 1} swapped"] = run(K, Vs)
    if n > 128:
        Kd = K.copy()
        Kd[128:] = np.concatenate([K[129:], K[-1:]])                       # a stale / shifted 128-row step
        out["keys from row 128 on shifted by one"] = run(Kd, V)
    if c.HKV > 1:
        out["kv head hk + 1"] = run(np.roll(K, -1, axis=1), np.roll(V, -1, axis=1))
    return out


@pytest.mark.parametrize("H,HKV", [(4, 1), (8, 2)])
@pytest.mark.parametrize("n_past", [1, 129, 257, 513])
@pytest.mark.parametrize("order", [0, 2])
def test_random_case_expectations_bite(oracle, H, HKV, n_past, order):
    """B1's expected value differs from every wrong host model of the kernel"""
    c = da.random_case(oracle, H, HKV, n_past, da.case_seed(H, HKV, n_past))
    exp = c.expected(oracle, order)
    assert np.isfinite(exp).all()
    muts = _mutants(oracle, c, order)
    assert len(muts) >= 4
    for name, got in muts.items():
        assert not np.array_equal(got, exp), name


@pytest.mark.parametrize("H,HKV", [(4, 1), (8, 2)])
@pytest.mark.parametrize("n_past", [129, 513])
@pytest.mark.parametrize("order", [0, 2])
def test_probe_expectations_hold_and_bite(oracle, H, HKV, n_past, order):
    """the "which key is where" probe: the oracle returns value row j* exactly in both associations, for every j* of the sweep (the newest key
    included); and a host model that reads a neighbouring row, drops the newest key or takes the neighbouring kv head does not"""
    for i, j in enumerate(da.probe_targets(n_past)):
        tg = da.probe_targets(n_past)
        j_star = [tg[(i + 3 * hk) % len(tg)] for hk in range(HKV)]
        c, exp = da.probe_case(oracle, H, HKV, n_past, j_star, seed=100 * n_past + j)
        assert np.array_equal(c.expected(oracle, order), exp), (j_star, "the probe's own premise fails on the host")
        K, V = c.keys(), c.values()
        oracle.lib.orc_set_sum_order(order)
        try:
            wrong = []
            Vs = np.roll(V, 1, axis=0)                                      # every value row read one row off
            wrong.append(("value rows off by one", oracle.attention_decode(c.q_rot, K, Vs, H, HKV).reshape(-1)))
            Ks = np.roll(K, 1, axis=0)                                      # every key row read one row off
            wrong.append(("key rows off by one", oracle.attention_decode(c.q_rot, Ks, V, H, HKV).reshape(-1)))
            if HKV > 1:
                wrong.append(("kv head hk + 1", oracle.attention_decode(c.q_rot, np.roll(K, -1, axis=1), np.roll(V, -1, axis=1), H, HKV).reshape(-1)))
            if n_past in j_star:
                wrong.append(("newest key dropped", oracle.attention_decode(c.q_rot, K[:-1], V[:-1], H, HKV).reshape(-1)))
        finally:
            oracle.lib.orc_set_sum_order(0)
        for name, got in wrong:
            assert not np.array_equal(got, exp), (j_star, name)
