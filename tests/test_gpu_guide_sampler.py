"""GPU: a sampler row with a guide row (ggml_hip_sampler_set_guidance). ggml_hip_sampler_sample with pairs over 24 consecutive draws against
the host mix (tests/host/guide_harness.cpp) followed by (1) the reference's own sampling functions (tests/sample_ref.py) on rows whose
mixed top-k has no ties, (2) the host restatements with their defined tie rule (tests/host/sample_harness.cpp, sample_chain_harness.cpp);
what a guide row keeps, what a budget freezes, what a grammar allows, and what set_guidance refuses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ggllm_cpp_amd as g
import grammar_ref
import guide_ref as gr
import sample_chain_ref as scr
import sample_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DRAWS = 24


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return gr.build_harness(tmp_path_factory.mktemp("guide"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not os.path.exists(sample_ref.REF_SO):
        pytest.skip("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    r = sample_ref.RefSampler(sample_ref.tiny_ggcc(str(tmp_path_factory.mktemp("ggcc") / "tiny.ggcc")))
    yield r
    r.free()


@pytest.fixture(scope="module")
def HS(tmp_path_factory):
    """tests/host/sample_harness.cpp: fq_sample.h's chain with its tie rule (value descending, id ascending)"""
    so = str(tmp_path_factory.mktemp("sample") / "libsample_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I",
                           os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "host", "sample_harness.cpp")])
    HS = C.CDLL(so)
    HS.sample_mt_seed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    HS.sample_chain.restype = C.c_int
    HS.sample_chain.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return HS


@pytest.fixture(scope="module")
def HC(tmp_path_factory):
    return scr.build_harness(tmp_path_factory.mktemp("sample_chain"))


def rng_of(L, s, row):
    w, p = np.zeros(624, np.uint32), C.c_int32(0)
    assert L.ggml_hip_sampler_get_rng(s, row, w.ctypes.data, C.byref(p)) == 0
    return w.tolist(), p.value


def guidance_of(L, s, R):
    gs, sc = np.zeros(R, np.int32), np.zeros(R, np.float32)
    assert L.ggml_hip_sampler_get_guidance(s, gs.ctypes.data, sc.ctypes.data) == 0
    return gs.tolist(), sc.tolist()


class Pairs:
    """a sampler of 2 * len(cases) rows, pair i in rows 2i and 2i + 1: the guide row above its leader for even i, below it for odd i.
    The guide rows get parameters, a window and a seed of their own, which must never matter."""

    def __init__(self, L, V, params, windows, scales, n_ctx=64):
        self.L, self.V, self.n = L, V, len(params)
        self.R = 2 * self.n
        self.lead = [2 * i + (i & 1) for i in range(self.n)]
        self.guide = [2 * i + 1 - (i & 1) for i in range(self.n)]
        self.s = L.ggml_hip_sampler_create(self.R, V, n_ctx)
        assert self.s
        self.lg, self.tk = g.DevBuf(self.R * V * 4), g.DevBuf(host=np.full(self.R, -5, np.int32))
        other = g.sampling_ext(temp=1.3, top_k=7, top_p=0.5, repeat_penalty=1.2, repeat_last_n=8, seed=999)
        for i, (p, w) in enumerate(zip(params, windows)):
            h = np.ascontiguousarray(w, np.int32)
            assert L.ggml_hip_sampler_set_row_ext(self.s, self.lead[i], C.byref(p), h.ctypes.data if h.size else None, h.size) == 0
            hg = np.arange(8, dtype=np.int32) % V
            assert L.ggml_hip_sampler_set_row_ext(self.s, self.guide[i], C.byref(other), hg.ctypes.data, hg.size) == 0
            assert L.ggml_hip_sampler_set_guidance(self.s, self.lead[i], self.guide[i], scales[i]) == 0
        self.guide_rng = [rng_of(L, self.s, r) for r in self.guide]

    def draw(self, lead_rows, guide_rows):
        """one ggml_hip_sampler_sample; returns the R tokens"""
        x = np.empty((self.R, self.V), np.float32)
        for i in range(self.n):
            x[self.lead[i]], x[self.guide[i]] = lead_rows[i], guide_rows[i]
        self.L.ggml_hip_memcpy_h2d(self.lg.ptr, x.ctypes.data, x.nbytes)
        self.L.ggml_hip_sampler_sample(self.s, self.lg.ptr, self.V, self.tk.ptr)
        self.L.ggml_hip_synchronize()
        return self.tk.to_host(np.int32, (self.R,))

    def check_guides_untouched(self):
        for i, r in enumerate(self.guide):
            assert rng_of(self.L, self.s, r) == self.guide_rng[i], "a guide row's generator moved"

    def free(self):
        self.lg.free()
        self.tk.free()
        self.L.ggml_hip_sampler_free(self.s)


def pair_rows(seed, V, spread=3.0):
    """3 leader rows and 3 guide rows, drawn in turn"""
    x = (np.random.default_rng(seed).standard_normal((6, V)) * spread).astype(np.float32)
    return x[:3], x[3:]


def mixed_of(H, lead_rows, guide_rows, scale):
    V = lead_rows.shape[1]
    return gr.host_mix(H, np.concatenate([lead_rows, guide_rows]), V, [0, 1, 2], [3, 4, 5], [scale] * 3)[0]


def run_pairs(L, H, V, params, windows, scales, seeds, spread=3.0):
    """24 draws of every pair; returns (leaders' tokens [24][n], the host-mixed rows per case [3][V]); asserts what holds in every case"""
    rows = [pair_rows(s, V, spread) for s in seeds]
    dev = Pairs(L, V, params, windows, scales)
    try:
        got = np.stack([dev.draw([rows[i][0][d % 3] for i in range(dev.n)], [rows[i][1][d % 3] for i in range(dev.n)]) for d in range(N_DRAWS)])
        dev.check_guides_untouched()
        assert np.array_equal(got[:, dev.guide], got[:, dev.lead]), "a guide row's token is not its leader's"
        assert guidance_of(L, dev.s, dev.R)[0] == [dev.guide[r // 2] if r == dev.lead[r // 2] else -1 for r in range(dev.R)]
        return got[:, dev.lead], [mixed_of(H, rows[i][0], rows[i][1], scales[i]) for i in range(dev.n)]
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------- yardstick 1: the reference's functions
# (top_k, scale, penalties, seed of the rows at V = 65024, at V = 333): seeds at which the mixed rows have no tie among their top_k + 1 largest
# values -- a full-width mixed row always holds ties somewhere, and the reference's std::sort order on ties is out of scope
REF_CASES = [(1, 1.5, False, 1, 4), (40, 7.5, True, 101, 104), (1024, -0.5, False, 201, 204), (1024, 1.5, False, 302, 304)]


@pytest.mark.parametrize("V", [65024, 333])
def test_pairs_match_reference_functions(L, H, ref, V):
    rng = np.random.default_rng(V)
    params, windows, scales, seeds = [], [], [], []
    for i, (top_k, scale, pen, s_wide, s_small) in enumerate(REF_CASES):
        w = [int(t) for t in rng.integers(0, V, 64)] if pen else []
        params.append(g.sampling_ext(temp=0.8, top_k=top_k, top_p=0.95, repeat_penalty=1.1 if pen else 1.0, repeat_last_n=len(w),
                                     frequency_penalty=0.25 if pen else 0.0, presence_penalty=0.5 if pen else 0.0, seed=500 + 13 * i))
        windows.append(w)
        scales.append(scale)
        seeds.append(s_wide if V == 65024 else s_small)
    got, mixed = run_pairs(L, H, V, params, windows, scales, seeds)
    for i, p in enumerate(params):
        k = min(REF_CASES[i][0] + 1, V)
        for y in mixed[i]:
            top = np.sort(y)[::-1][:k]
            assert np.unique(top).size == k, ("the host-mixed row has a tie among its top_k + 1 largest values", REF_CASES[i])
        want = sample_ref.run_ref(ref, list(mixed[i]), p.base, windows[i], N_DRAWS)
        assert list(got[:, i]) == want, REF_CASES[i]


# ---------------------------------------------------------------------------------------------- yardstick 2: the host restatements
def test_pairs_match_host_chain_whole_vocabulary_and_greedy(L, H, HS):
    """top_k = 0 (the HBM sort of the whole mixed row) and greedy, at V = 65024 and with penalties: fq_sample.h's chain on the host"""
    V = 65024
    rng = np.random.default_rng(7)
    w = [int(t) for t in rng.integers(0, V, 64)]
    cases = [(0, 0.95, 0.8, 1.5), (0, 1.0, 0.0, 7.5), (40, 0.95, 0.0, -0.5)]
    params = [g.sampling_ext(temp=t, top_k=k, top_p=tp, repeat_penalty=1.1, repeat_last_n=64, frequency_penalty=0.25, presence_penalty=0.5, seed=70 + i)
              for i, (k, tp, t, _) in enumerate(cases)]
    got, mixed = run_pairs(L, H, V, params, [w] * 3, [c[3] for c in cases], [11, 12, 13])
    for i, p in enumerate(params):
        b = p.base
        mt, mti = (C.c_uint32 * 624)(), C.c_int()
        HS.sample_mt_seed(mt, C.byref(mti), b.seed)
        win, want = list(w), []
        for d in range(N_DRAWS):
            x = np.ascontiguousarray(mixed[i][d % 3])
            wa = np.ascontiguousarray(win, np.int32)
            t = HS.sample_chain(x.ctypes.data, V, b.temp, b.top_k, b.top_p, b.repeat_penalty, b.alpha_frequency, b.alpha_presence,
                                wa.ctypes.data, wa.size, 0, None, None, mt, C.byref(mti))
            want.append(t)
            win = win[1:] + [t]
        assert list(got[:, i]) == want, cases[i]


@pytest.mark.parametrize("V", [333, 4000])
def test_pairs_match_host_chain_other_branches(L, H, HC, V):
    """tail-free with typical, mirostat 1, mirostat 2 and the default chain in one launch: fq_sample_chain.h's chain on the host, mu bit for bit"""
    rng = np.random.default_rng(V + 3)
    w = [int(t) for t in rng.integers(0, V, 64)]
    params = [g.sampling_ext(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64, seed=21),
              g.sampling_ext(tfs_z=0.95, typical_p=0.9, temp=0.9, top_k=200, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64, frequency_penalty=0.2, seed=22, logit_bias={5: 2.5}),
              g.sampling_ext(mirostat=1, mirostat_tau=5.0, mirostat_eta=0.1, temp=0.8, repeat_penalty=1.0, repeat_last_n=0, seed=23),
              g.sampling_ext(mirostat=2, mirostat_tau=3.0, mirostat_eta=0.5, temp=1.5, repeat_penalty=1.1, repeat_last_n=64, presence_penalty=0.5, seed=24)]
    windows, scales = [w, w[::-1], [], w], [1.5, 1.0, 0.0, -0.5]
    rows = [pair_rows(40 + i, V) for i in range(4)]
    dev = Pairs(L, V, params, windows, scales)
    try:
        got = np.stack([dev.draw([rows[i][0][d % 3] for i in range(4)], [rows[i][1][d % 3] for i in range(4)]) for d in range(N_DRAWS)])
        mu = np.zeros(dev.R, np.float32)
        assert L.ggml_hip_sampler_get_mu(dev.s, mu.ctypes.data) == 0
        dev.check_guides_untouched()
        assert np.array_equal(got[:, dev.guide], got[:, dev.lead])
        for i, p in enumerate(params):
            h = scr.HostChain(HC, p, V)
            want, mus = h.run(list(mixed_of(H, rows[i][0], rows[i][1], scales[i])), windows[i], N_DRAWS)
            assert list(got[:, dev.lead[i]]) == want, i
            assert np.float32(mu[dev.lead[i]]).view(np.uint32).item() == mus[-1], i
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------- what else holds
def test_guided_sampler_equals_plain_sampler_on_mixed_rows(L, H):
    """sampler A holds two pairs and an unguided row, sampler B no pair and gets the host-mixed rows in the leaders' places: the same tokens,
    generators and stop states draw for draw. The leaders have a budget of 5 and 9 draws: both rows of a pair freeze with their leader --
    same token, nothing moves -- and the unguided row draws on. Turning guidance off again leaves A drawing what B draws from the raw rows."""
    V, R = 333, 5
    lead, guide = [1, 2], [0, 4]
    A, B = L.ggml_hip_sampler_create(R, V, 32), L.ggml_hip_sampler_create(R, V, 32)
    lgA, lgB = g.DevBuf(R * V * 4), g.DevBuf(R * V * 4)
    tkA, tkB = g.DevBuf(host=np.full(R, -5, np.int32)), g.DevBuf(host=np.full(R, -5, np.int32))
    rng = np.random.default_rng(5)
    try:
        for r in range(R):
            p = g.sampling_ext(temp=0.9, top_k=40 if r != 3 else 0, top_p=0.95, repeat_penalty=1.2, repeat_last_n=16, seed=80 + r)
            h = np.ascontiguousarray(rng.integers(0, V, 16), np.int32)
            for s in (A, B):
                assert L.ggml_hip_sampler_set_row_ext(s, r, C.byref(p), h.ctypes.data, h.size) == 0
        for s in (A, B):
            assert L.ggml_hip_sampler_set_stops(s, 1, C.byref(g.stops(max_tokens=5))) == 0
            assert L.ggml_hip_sampler_set_stops(s, 2, C.byref(g.stops(max_tokens=9))) == 0
        assert L.ggml_hip_sampler_set_guidance(A, 1, 0, 1.5) == 0 and L.ggml_hip_sampler_set_guidance(A, 2, 4, -0.5) == 0
        guide_rng = [rng_of(L, A, r) for r in guide]
        last = None
        for d in range(12):
            x = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)
            y = x.copy()
            y[lead] = gr.host_mix(H, x, V, lead, guide, [1.5, -0.5])[0]
            L.ggml_hip_memcpy_h2d(lgA.ptr, x.ctypes.data, x.nbytes)
            L.ggml_hip_memcpy_h2d(lgB.ptr, y.ctypes.data, y.nbytes)
            L.ggml_hip_sampler_sample(A, lgA.ptr, V, tkA.ptr)
            L.ggml_hip_sampler_sample(B, lgB.ptr, V, tkB.ptr)
            L.ggml_hip_synchronize()
            a, b = tkA.to_host(np.int32, (R,)), tkB.to_host(np.int32, (R,))
            assert np.array_equal(a[[1, 2, 3]], b[[1, 2, 3]]) and np.array_equal(a[guide], a[lead]), d
            if last is not None:
                if d >= 5:
                    assert a[1] == last[1] and a[0] == last[0]          # the budget of 5: the pair is frozen, the token stays
                if d >= 9:
                    assert a[2] == last[2] and a[4] == last[4]
            last = a
        for r in (1, 2, 3):
            assert rng_of(L, A, r) == rng_of(L, B, r), r
        assert [rng_of(L, A, r) for r in guide] == guide_rng
        nA, rA, nB, rB = (np.zeros(R, np.int32) for _ in range(4))
        assert L.ggml_hip_sampler_get_stops(A, nA.ctypes.data, rA.ctypes.data) == 0 and L.ggml_hip_sampler_get_stops(B, nB.ctypes.data, rB.ctypes.data) == 0
        assert nA.tolist() == nB.tolist() == [0, 5, 9, 0, 0] and rA.tolist() == rB.tolist()
        # off again: A is a plain sampler (rows 0 and 4 draw for themselves; their generators start to move only now)
        assert L.ggml_hip_sampler_set_guidance(A, 1, -1, 0.0) == 0 and L.ggml_hip_sampler_set_guidance(A, 2, -1, 0.0) == 0
        assert guidance_of(L, A, R) == ([-1] * R, [1.0] * R)
        for s in (A, B):
            for r in (1, 2):
                assert L.ggml_hip_sampler_set_stops(s, r, None) == 0
        for r in guide:
            assert L.ggml_hip_sampler_copy_row(B, r, A, r) == 0
        x = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)
        L.ggml_hip_memcpy_h2d(lgA.ptr, x.ctypes.data, x.nbytes)
        L.ggml_hip_sampler_sample(A, lgA.ptr, V, tkA.ptr)
        L.ggml_hip_sampler_sample(B, lgA.ptr, V, tkB.ptr)
        L.ggml_hip_synchronize()
        assert np.array_equal(tkA.to_host(np.int32, (R,)), tkB.to_host(np.int32, (R,)))
        assert [rng_of(L, A, r) for r in guide] != guide_rng
    finally:
        L.ggml_hip_sampler_free(A)
        L.ggml_hip_sampler_free(B)
        for b in (lgA, lgB, tkA, tkB):
            b.free()


def test_leader_with_grammar_draws_allowed_tokens_from_the_mixed_row(L, H):
    """the leader holds a grammar whose first state allows few tokens; the guide row's favourite and the leader's raw favourite are forbidden ones. Every
    draw is allowed, the state follows it, and the greedy draw is the allowed argmax of the MIXED row"""
    V, EOS = 300, 0
    vocab = grammar_ref.vocab300(np.random.default_rng(11))
    d = g.regex_dfa(b"(ab|cd)+")
    gram = g.Grammar.make(vocab, d, EOS)
    s = L.ggml_hip_sampler_create(2, V, 32)
    lg, tk = g.DevBuf(2 * V * 4), g.DevBuf(2 * 4)
    rng = np.random.default_rng(3)
    try:
        p = g.sampling_ext(temp=0.0, repeat_penalty=1.0, repeat_last_n=0, seed=1)
        assert L.ggml_hip_sampler_set_row_ext(s, 1, C.byref(p), None, 0) == 0
        assert L.ggml_hip_sampler_set_grammar(s, 1, gram.h, -1) == 0
        assert L.ggml_hip_sampler_set_guidance(s, 1, 0, 1.5) == 0
        state = d.start
        for draw in range(12):
            x = (rng.standard_normal((2, V)) * 3.0).astype(np.float32)
            ok = grammar_ref.allowed_row(d.trans, d.accept, state, EOS, vocab)
            bad = np.flatnonzero(~ok)
            x[1, bad[0]] += 30.0                                    # the leader's raw favourite: forbidden
            y = gr.host_mix(H, x, V, [1], [0], [1.5])[0][0]
            L.ggml_hip_memcpy_h2d(lg.ptr, x.ctypes.data, x.nbytes)
            L.ggml_hip_sampler_sample(s, lg.ptr, V, tk.ptr)
            L.ggml_hip_synchronize()
            t = tk.to_host(np.int32, (2,))
            assert t[0] == t[1] and ok[t[1]], draw
            assert t[1] == int(np.argmax(grammar_ref.masked(y, ok))), draw
            state = grammar_ref.advance(d.trans, state, int(t[1]), EOS, vocab)
            st = np.zeros(2, np.int32)
            assert L.ggml_hip_sampler_get_grammar_state(s, st.ctypes.data) == 0 and st.tolist() == [-1, state]
    finally:
        L.ggml_hip_sampler_set_grammar(s, 1, None, 0)
        L.ggml_hip_sampler_free(s)
        gram.free()
        lg.free()
        tk.free()


def test_refusals_change_nothing(L, H):
    """everything set_guidance refuses, on a sampler with one pair (2 led by ... guided by 0): the bindings read back as they were and the next draw is
    the pair's; a context stop and guidance refuse one another"""
    V, R = 333, 5
    s = L.ggml_hip_sampler_create(R, V, 32)
    lg, tk = g.DevBuf(R * V * 4), g.DevBuf(R * 4)
    rng = np.random.default_rng(9)
    nan, inf = float("nan"), float("inf")
    try:
        p = g.sampling_ext(temp=0.0, repeat_penalty=1.0, repeat_last_n=0, seed=1)
        for r in range(R):
            assert L.ggml_hip_sampler_set_row_ext(s, r, C.byref(p), None, 0) == 0
        assert guidance_of(L, s, R) == ([-1] * R, [1.0] * R)
        assert L.ggml_hip_sampler_set_guidance(s, 3, -1, 1.0) == 0          # off where nothing is on
        assert L.ggml_hip_sampler_set_guidance(s, 2, 0, 1.5) == 0
        want = ([-1, -1, 0, -1, -1], [1.0, 1.0, 1.5, 1.0, 1.0])
        assert guidance_of(L, s, R) == want
        bad = [(1, 1, 1.5),            # row == guide_row
               (5, 1, 1.5), (-1, 1, 1.5), (1, 5, 1.5), (1, -2, 1.5),       # out of range
               (1, 2, 1.5),            # the guide row leads a row
               (1, 0, 1.5),            # the guide row guides another row already
               (0, 1, 1.5),            # the row is itself a guide row
               (3, 4, nan), (3, 4, inf), (3, 4, -inf)]
        for row, gd, sc in bad:
            assert L.ggml_hip_sampler_set_guidance(s, row, gd, sc) == 1, (row, gd, sc)
            assert guidance_of(L, s, R) == want
        assert L.ggml_hip_sampler_set_context_stop(s, 32) == 1                 # refused while a pair exists ...
        x = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)
        L.ggml_hip_memcpy_h2d(lg.ptr, x.ctypes.data, x.nbytes)
        L.ggml_hip_sampler_sample(s, lg.ptr, V, tk.ptr)
        L.ggml_hip_synchronize()
        t = tk.to_host(np.int32, (R,))
        y = gr.host_mix(H, x, V, [2], [0], [1.5])[0][0]
        assert t[2] == t[0] == int(np.argmax(y)) and t[1] == int(np.argmax(x[1])) and t[3] == int(np.argmax(x[3]))
        # a pair may change its scale and its guide row; the old guide row is free again
        assert L.ggml_hip_sampler_set_guidance(s, 2, 0, 7.5) == 0 and L.ggml_hip_sampler_set_guidance(s, 2, 4, 7.5) == 0
        assert guidance_of(L, s, R) == ([-1, -1, 4, -1, -1], [1.0, 1.0, 7.5, 1.0, 1.0])
        assert L.ggml_hip_sampler_set_guidance(s, 1, 0, 1.0) == 0
        assert L.ggml_hip_sampler_set_guidance(s, 1, -1, 0.0) == 0 and L.ggml_hip_sampler_set_guidance(s, 2, -1, 0.0) == 0
        # ... and guidance while the context stop is on
        assert L.ggml_hip_sampler_set_context_stop(s, 32) == 0
        assert L.ggml_hip_sampler_set_guidance(s, 2, 0, 1.5) == 1 and guidance_of(L, s, R) == ([-1] * R, [1.0] * R)
        assert L.ggml_hip_sampler_set_context_stop(s, 0) == 0
        assert L.ggml_hip_sampler_set_guidance(s, 2, 0, 1.5) == 0
    finally:
        L.ggml_hip_sampler_free(s)
        lg.free()
        tk.free()
