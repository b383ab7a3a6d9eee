"""GPU: the decode path at model level against the whole-model oracle, past the 256 rows the decode attention requests before it knows n_past.

The merged decode launches (k_attn_out, k_attn_out_ln, k_attn_out_ref: attention groups sharing a workgroup, the in-launch hand-off) exist only inside
a model step, so they are walked here: a teacher-forced walk over EVERY position from 0 to 1100 with nothing but decode steps filling the cache, in every
launch form, each step's logits bit for bit the oracle's (test_walk_*), and the position at which a context's plain evals change launch form because two
attention groups' score rows no longer fit one workgroup's LDS (test_form_change_*). Real widths at 1024 / 2048 keys: test_gpu_configs.py."""
import os

import numpy as np
import pytest

import ggllm_cpp_amd as g
from oracle import binding as ob
import synth

pytestmark = pytest.mark.gpu
NT = max(4, min(16, (os.cpu_count() or 8)))

N_CTX, N_WALK = 1152, 1101                     # positions 0 .. 1100
MODELS = {"mqa-q4_0": (synth.HP_TINY_MQA, ob.Q4_0), "gqa-q5_1": (synth.HP_TINY_GQA, ob.Q5_1), "gqa-q4_k": (synth.HP_TINY_GQA, ob.Q4_K)}
GREEDY = [(900, 200), (120, 200)]              # (n_past, steps): continuations from the cache a walk left


@pytest.fixture(scope="module", autouse=True)
def _init():
    g.init(0)


class _Walks:
    """per model: the weights, the token stream, and the oracle's teacher-forced walk per summation order (cached: each is ~10 ms a step)"""

    def __init__(self, oracle):
        self.oracle, self.w, self.walk, self.greedy = oracle, {}, {}, {}

    def weights(self, key):
        if key not in self.w:
            hp, t = MODELS[key]
            self.w[key] = (synth.make_model(self.oracle, hp, t, seed=71), synth.tokens(N_WALK, hp["n_vocab"], seed=17))
        return self.w[key]

    def logits(self, key, order, n):
        """oracle logits of steps 0 .. n - 1 in orc_set_sum_order(order) (2: the backend's association, as _both_orders of test_gpu_falcon.py sets it up
        for its decode step; 0: the reference's), one token per eval"""
        have = self.walk.get((key, order))
        if have is None or have[0].shape[0] < n:
            w, toks = self.weights(key)
            o = self.oracle
            o.lib.orc_set_sum_order(order)
            try:
                mo = o.model(w, N_CTX)
                lg = np.stack([mo.eval(toks[i:i + 1], i, NT)[0] for i in range(n)])
            finally:
                o.lib.orc_set_sum_order(0)
            have = self.walk[(key, order)] = (lg, mo)
        return have[0][:n]

    def greedy_tokens(self, key, n_past, n):
        """the oracle's greedy continuation (order 2) from the cache its full walk left: the stream's token at n_past, then n - 1 argmax tokens"""
        if (key, n_past) not in self.greedy:
            self.logits(key, 2, N_WALK)
            _, toks = self.weights(key)
            mo = self.walk[(key, 2)][1]
            o = self.oracle
            o.lib.orc_set_sum_order(2)
            try:
                cur, out = int(toks[n_past]), []
                for i in range(n):
                    cur = int(mo.eval(np.array([cur], np.int32), n_past + i, NT)[0].argmax())
                    out.append(cur)
            finally:
                o.lib.orc_set_sum_order(0)
            self.greedy[(key, n_past)] = np.array(out, np.int32)
        return self.greedy[(key, n_past)]


@pytest.fixture(scope="module")
def walks(oracle):
    return _Walks(oracle)


def _gpu_walk(m, toks, n, form):
    """teacher-forced decode steps 0 .. n - 1, no prefill; every step's logits row kept on the host"""
    rows = []
    if form == "graph":
        for i in range(n):
            m.eval_token(toks[i], i)
            rows.append(m.logits())
    else:
        for i in range(n):
            rows.append(m.eval(toks[i:i + 1], i)[0])
    return np.stack(rows)


def _mismatching_steps(got, exp):
    return np.flatnonzero((got.view(np.uint32) != exp.view(np.uint32)).any(axis=1))


def _report(bad, what):
    if bad.size:
        return [f"{what}: {bad.size} steps differ from the oracle, first at position {int(bad[0])} (mod 128: {int(bad[0]) % 128}); positions {bad[:24].tolist()}"]
    return []


# (form, fused mode or None, eval_token?)
DEFAULT_FORMS = [("op list", 0, "eval"), ("three launches", 1, "eval"), ("merged", 2, "eval"), ("one launch per block", 3, "eval"), ("captured graph", 2, "graph")]


@pytest.mark.parametrize("key", list(MODELS))
def test_walk_every_position_default_order(walks, key):
    """C1: positions 0 .. 1100 one token at a time by m.eval under set_fused 0 / 1 / 2 / 3 and by eval_token (the captured graph: launches sized for n_ctx),
    every step's logits equal to the oracle's (order 2) bit for bit; no device-side sync error. The whole loop runs; the report lists the positions."""
    w, toks = walks.weights(key)
    exp = walks.logits(key, 2, N_WALK)
    m = g.FalconModel(w, n_ctx=N_CTX, n_batch=8)
    failures = []
    try:
        for name, fused, how in DEFAULT_FORMS:
            m.set_fused(fused)
            got = _gpu_walk(m, toks, N_WALK, how)
            failures += _report(_mismatching_steps(got, exp), f"{key}, {name}")
            if m.sync_error() != 0:
                failures.append(f"{key}, {name}: sync_error {m.sync_error()}")
    finally:
        m.free()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("key,n", [("mqa-q4_0", N_WALK), ("gqa-q5_1", 401)])
def test_walk_every_position_reference_orders(walks, key, n):
    """C1 in the reference's association: reference order 2 (k_attn_out_ref) by plain evals and through eval_token, and reference order 1, against the
    oracle's order 0. The f64 rule of test_gpu_decode_attention.py applies (the kernel associates its f64 partial sums in lane order; ~1e-9 per dot
    product that an f32 result moves), and a decoder stack carries one moved score into every later row: look at the FIRST differing step."""
    w, toks = walks.weights(key)
    exp = walks.logits(key, 0, n)
    L = g.load()
    m = g.FalconModel(w, n_ctx=N_CTX, n_batch=8)
    failures = []
    try:
        for name, order, how in (("reference order 2", 2, "eval"), ("reference order 2, captured graph", 2, "graph"), ("reference order 1", 1, "eval")):
            L.ggml_hip_reference_order(order)
            try:
                got = _gpu_walk(m, toks, n, how)
            finally:
                L.ggml_hip_reference_order(0)
            failures += _report(_mismatching_steps(got, exp), f"{key}, {name}")
            if m.sync_error() != 0:
                failures.append(f"{key}, {name}: sync_error {m.sync_error()}")
    finally:
        m.free()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("key", list(MODELS))
def test_greedy_continuations_from_a_walked_cache(walks, key):
    """C1: after a teacher-forced walk to 1100, decode_greedy for 200 steps from n_past 900 and from 120, with and without the graph, continues from the
    cache the walk left (the oracle from the cache its own walk left) and gives the oracle's greedy tokens one for one"""
    w, toks = walks.weights(key)
    exp = walks.logits(key, 2, N_WALK)
    m = g.FalconModel(w, n_ctx=N_CTX, n_batch=8)
    failures = []
    try:
        got = _gpu_walk(m, toks, N_WALK, "eval")
        failures += _report(_mismatching_steps(got, exp), f"{key}, the walk")
        for n_past, n in GREEDY:
            want = walks.greedy_tokens(key, n_past, n)
            for use_graph in (True, False):
                dev = m.decode_greedy(int(toks[n_past]), n_past, n, use_graph=use_graph)
                bad = np.flatnonzero(dev != want)
                if bad.size:
                    failures.append(f"{key}: greedy from {n_past}, graph {use_graph}: first other token at step {int(bad[0])} (position {n_past + int(bad[0])})")
        if m.sync_error() != 0:
            failures.append(f"{key}: sync_error {m.sync_error()}")
    finally:
        m.free()
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ C2: where a context changes launch form
# With plain evals the decode launches size their LDS for n_past + 1 keys, and the merged launch holds two attention groups per workgroup: it fits while
# 2 * (9024 + 4 (n_past + 1)) <= 160 KiB, i.e. up to 18 224 keys; from there a plain eval is an attention launch + an output launch, and a captured step of a
# context with n_ctx > 18 224 never merges. One-block models: block 0's K / V rows need no attention, so the oracle produces all of them in linear time
# (orc_falcon_block_sampled), where a whole-model walk to 18 432 tokens would take ten minutes.
BIG_CTX, EDGE_CTX, PRE, LAST, BATCH = 18432, 18224, 18200, 18260, 512


def _sampled_decode_rows(oracle, mo, X, pos0, K, V, order_block, order_head):
    """hidden output rows and logits of consecutive teacher-forced decode steps at pos0 .. whose block inputs are X, over the cached rows K / V [pos0, ...]"""
    lib = oracle.lib
    lib.orc_set_sum_order(order_block); lib.orc_set_backend_batch(1)
    try:
        out = mo.block_sampled(lib, 0, X, np.arange(X.shape[0]), pos0=pos0, k_prev=K[:pos0], v_prev=V[:pos0], n_threads=NT)
        lib.orc_set_sum_order(order_head)
        return out, mo.head_rows(lib, out, n_threads=NT)
    finally:
        lib.orc_set_sum_order(0); lib.orc_set_backend_batch(0)


def _prefill(m, toks, n, keep=None):
    """GPU prefill of toks[:n] in BATCH-token evals; keep: (hid0 [n, E], hid1 [n, E]) filled with block 0's input and output rows"""
    for a in range(0, n, BATCH):
        b = min(n, a + BATCH)
        if keep is None:
            m.eval(toks[a:b], a)
        else:
            _, h = m.eval(toks[a:b], a, want_hidden=True)
            keep[0][a:b], keep[1][a:b] = h[0], h[1]


class _Ctx:
    """a second context over a FalconModel's device weights, with the FalconModel's eval / eval_token / logits"""

    def __init__(self, model, n_ctx, n_batch, rope_n_ctx):
        self.hp, self.n_local = model.hp, model.n_local
        self.ctx = model.new_context(n_ctx, n_batch, rope_n_ctx)

    eval, eval_token, logits, sync_error = g.FalconModel.eval, g.FalconModel.eval_token, g.FalconModel.logits, g.FalconModel.sync_error

    def free(self):
        g.load().falcon_hip_context_free(self.ctx)


@pytest.mark.parametrize("hp0,t", [(synth.HP_TINY_MQA, ob.Q4_0), (synth.HP_TINY_GQA, ob.Q5_1)])
def test_form_change_at_18224_keys(oracle, hp0, t):
    """C2: a one-block model, n_ctx 18 432, prefilled on the GPU to 18 200 in 512-token batches (sampled prefill rows pinned against the oracle first, so that a
    prefill mismatch cannot pass for a decode bug), then teacher-forced decode steps over 18 200 .. 18 260 -- by plain eval (merged up to 18 224 keys, attention +
    output launch after), by eval_token (never merged at this n_ctx) and in reference order 2 (k_attn_out_ref -> k_attn_decode_f64 + k_gemv_out_ref; the f64 rule of
    test_gpu_decode_attention.py applies) -- hidden rows and logits of every step bit for bit the oracle's over the K / V rows the prefill left. A second
    context of n_ctx 18 224, the largest whose captured step still merges, runs the same steps up to its end through eval_token."""
    hp = dict(hp0); hp["n_layer"] = 1
    E = hp["n_embd"]
    w = synth.make_model(oracle, hp, t, seed=91)
    toks = synth.tokens(LAST + 1, hp["n_vocab"], seed=19)
    steps = range(PRE, LAST + 1)
    L = g.load()
    m = g.FalconModel(w, n_ctx=BIG_CTX, n_batch=BATCH)
    failures = []
    try:
        hid0, hid1 = np.empty((PRE, E), np.float32), np.empty((PRE, E), np.float32)
        _prefill(m, toks, PRE, (hid0, hid1))
        mo = oracle.model(w, 8, rope_n_ctx=BIG_CTX)
        sp = np.array([0, 511, 512, 9000, PRE - 281, PRE - 280, PRE - 1])
        oracle.lib.orc_set_sum_order(2); oracle.lib.orc_set_backend_batch(BATCH)
        try:
            out, K, V = mo.block_sampled(oracle.lib, 0, hid0, sp, n_threads=NT, want_kv=True)
        finally:
            oracle.lib.orc_set_sum_order(0); oracle.lib.orc_set_backend_batch(0)
        assert np.array_equal(out, hid1[sp]), "the PREFILL's sampled rows differ from the oracle's: not a decode finding"

        # plain evals, with the hidden rows
        X, H1, lg = [], [], []
        for p in steps:
            l, h = m.eval(toks[p:p + 1], p, want_hidden=True)
            X.append(h[0, 0]); H1.append(h[1, 0]); lg.append(l[0])
        X, H1, lg = np.stack(X), np.stack(H1), np.stack(lg)
        out_o, lg_o = _sampled_decode_rows(oracle, mo, X, PRE, K, V, 2, 1)
        failures += _report(_mismatching_steps(H1, out_o) + PRE, "plain eval, block output rows")
        failures += _report(_mismatching_steps(lg, lg_o) + PRE, "plain eval, logits")
        # the captured graph (sized for n_ctx: attention launch + output launch at every position)
        got = np.stack([(m.eval_token(toks[p], p), m.logits())[1] for p in steps])
        failures += _report(_mismatching_steps(got, lg_o) + PRE, "eval_token, n_ctx %d" % BIG_CTX)
        # reference order 2 over the same prefilled rows
        out_r, lg_r = _sampled_decode_rows(oracle, mo, X, PRE, K, V, 0, 0)
        L.ggml_hip_reference_order(2)
        try:
            H1r, lgr = [], []
            for p in steps:
                l, h = m.eval(toks[p:p + 1], p, want_hidden=True)
                H1r.append(h[1, 0]); lgr.append(l[0])
        finally:
            L.ggml_hip_reference_order(0)
        failures += _report(_mismatching_steps(np.stack(H1r), out_r) + PRE, "reference order 2, block output rows")
        failures += _report(_mismatching_steps(np.stack(lgr), lg_r) + PRE, "reference order 2, logits")
        if m.sync_error() != 0:
            failures.append("sync_error %d" % m.sync_error())
        # the largest context whose captured step still merges: the same rope, the same steps up to its end
        c2 = _Ctx(m, EDGE_CTX, BATCH, BIG_CTX)
        try:
            _prefill(c2, toks, PRE)
            n2 = EDGE_CTX - PRE
            got = np.stack([(c2.eval_token(toks[p], p), c2.logits())[1] for p in range(PRE, EDGE_CTX)])
            failures += _report(_mismatching_steps(got, lg_o[:n2]) + PRE, "eval_token, n_ctx %d" % EDGE_CTX)
            if c2.sync_error() != 0:
                failures.append("n_ctx %d: sync_error %d" % (EDGE_CTX, c2.sync_error()))
        finally:
            c2.free()
    finally:
        m.free()
    assert not failures, "\n".join(failures)
