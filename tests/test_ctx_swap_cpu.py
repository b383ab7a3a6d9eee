"""CPU: falcon_main's context swap as the library plans it. csrc/fq_ctx_swap.h (the planner) and the context branch of csrc/fq_stop.h
are host-compiled with g++ (tests/host/ctx_swap_harness.cpp) and checked against restatements in Python (tests/ctx_swap_ref.py):
the planner exhaustively over small contexts, and against every reset block the reference printed (tests/golden/ctx_swap.npz, from
the golden's own token stream); the stop rule's new branch for its place in the order and for what it leaves alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ctx_swap_ref as cr
import ggllm_cpp_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNING, BUDGET, CONTEXT, TEXT0 = g.STOP_RUNNING, g.STOP_BUDGET, g.STOP_CONTEXT, g.STOP_TEXT0


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ctx_swap") / "libctx_swap_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"),
                           "-o", out, os.path.join(ROOT, "tests", "host", "ctx_swap_harness.cpp")])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.swap_plan.restype, L.swap_plan.argtypes = C.c_int, [C.c_int] * 6 + [vp, vp]
    L.swap_plan_all.restype, L.swap_plan_all.argtypes = None, [C.c_int] * 6 + [vp]
    L.swap_history.restype, L.swap_history.argtypes = C.c_int, [vp, C.c_int, C.c_int, vp]
    L.ctx_draw.restype = C.c_int
    L.ctx_draw.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int]
    L.ctx_resume.restype, L.ctx_resume.argtypes = C.c_int, [vp]
    L.ctx_reset.restype, L.ctx_reset.argtypes = None, [vp, vp]
    assert L.stop_state_words() == 10 and L.stop_context_reason() == CONTEXT == -3
    return L


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "ctx_swap.npz")) as z:
        return {k: z[k] for k in z.files}


def blocks_of(golden, name):
    ids, out = golden[name + ".block_ids"].tolist(), []
    for n in golden[name + ".block_len"].tolist():
        out.append(ids[:n])
        ids = ids[n:]
    assert not ids
    return out


def test_planner_matches_the_restatement_exhaustively(H):
    """every prompt size, keep (negative and beyond the prompt included), system size and history length of three small contexts:
    an even one, the fixture's, and an odd one (n_ctx / 2 rounds down)"""
    n = 0
    for n_ctx in (16, 32, 33):
        out = np.zeros(2 * (n_ctx + 5), np.int32)
        for prompt_size in range(0, n_ctx + 1):
            for n_system in range(0, prompt_size + 1):
                for n_keep in range(-1, prompt_size + 3):
                    for n_pending in (0, 1):
                        H.swap_plan_all(n_ctx, n_system, n_keep, prompt_size, n_pending, n_ctx + 4, out.ctypes.data)
                        for h in range(n_ctx + 5):
                            want = cr.plan(n_ctx, n_system, n_keep, prompt_size, h, n_pending) if h >= n_pending else (-1, -1)
                            assert (int(out[2 * h]), int(out[2 * h + 1])) == want, (n_ctx, n_system, n_keep, prompt_size, h, n_pending)
                            n += 1
    assert n > 1000000


def test_planner_refuses_what_no_generation_has(H):
    a, b = C.c_int(7), C.c_int(7)
    for args in ((0, 0, 0, 4, 5, 1), (32, 5, 0, 4, 5, 1), (32, 0, 0, -1, 5, 1), (32, 0, 0, 4, 0, 1), (32, 0, 0, 4, 5, -1), (32, -1, 0, 4, 5, 1)):
        assert H.swap_plan(*args, C.byref(a), C.byref(b)) == 1 and (a.value, b.value) == (7, 7), args
    assert H.swap_plan(32, 0, 0, 11, 23, 1, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 16)


def test_prompt_history_is_the_last_token_of_every_batch(H):
    rng = np.random.default_rng(3)
    for n in range(0, 40):
        p = rng.integers(0, 1000, n).astype(np.int32)
        for nb in (1, 2, 4, 7, 8, 39, 40, 512):
            out = np.zeros(max(n, 1), np.int32)
            k = H.swap_history(p.ctypes.data, n, nb, out.ctypes.data)
            assert out[:k].tolist() == cr.prompt_history(p.tolist(), nb)
            assert H.swap_history(p.ctypes.data, n, nb, None) == k == (n + nb - 1) // nb
    assert H.swap_history(None, 5, 0, None) == 0


def test_planner_reproduces_every_block_of_the_golden(H, golden):
    """from the golden's own token stream: the prompt's history, then draw by draw; at every full cache the planner's tail of the history plus
    the waiting token is the block falcon_main printed. The clamp case pulls prompt-batch-last tokens in; keep -1 on the long prompt regenerates nothing"""
    sizes = {}
    for name, (prompt, n_predict, n_batch, seed, keep, system, flags) in cr.CASES.items():
        ids, drawn, n_sys = golden[name + ".prompt_ids"].tolist(), golden[name + ".drawn"].tolist(), int(golden[name + ".n_system"])
        assert len(drawn) == n_predict
        p = np.array(ids, np.int32)
        hist = np.zeros(len(ids), np.int32)
        hist = hist[:H.swap_history(p.ctypes.data, len(ids), n_batch, hist.ctypes.data)].tolist()
        n_past, got = len(ids), []
        a, b = C.c_int(0), C.c_int(0)
        for i, t in enumerate(drawn[:-1]):
            hist.append(t)
            if n_past + 1 > cr.N_CTX:
                assert H.swap_plan(cr.N_CTX, n_sys, keep, len(ids), len(hist), 1, C.byref(a), C.byref(b)) == 0
                got.append(hist[len(hist) - 1 - b.value:])
                n_past = a.value + b.value
            n_past += 1
        assert got == blocks_of(golden, name), name
        assert got == [blk for _, blk in cr.replay(ids, drawn, cr.N_CTX, n_batch, keep, n_sys)]
        sizes[name] = [len(x) for x in got]
    assert sizes["p_keep0"] == [17] * 4 and sizes["p_keep6"] == [11] * 4 and sizes["p_temp_keepall"] == [6] * 4
    assert sizes["p25_keep0"] == [12, 17] and sizes["p25_keepall"] == [1] * 5 and sizes["sys_mirostat2"] == [5] * 3
    assert all(len(v) >= 2 for v in sizes.values())
    # the clamp: 4 prompt-batch-last tokens (25 tokens in batches of 8) stand at the head of the first block
    ids = golden["p25_keep0.prompt_ids"].tolist()
    assert blocks_of(golden, "p25_keep0")[0][:4] == [ids[7], ids[15], ids[23], ids[24]]


def test_package_planner_is_the_header(H):
    """ggllm_cpp_amd.swap_plan / swap_history go through the library's exports (host only: no device is touched)"""
    a, b = C.c_int(0), C.c_int(0)
    for args in ((32, 0, 0, 11, 23), (32, 8, 4, 19, 9), (32, 0, -1, 25, 12), (33, 0, 3, 9, 2), (16, 0, 0, 5, 40)):
        n_ctx, n_system, n_keep, prompt_size, n_history = args
        assert H.swap_plan(n_ctx, n_system, n_keep, prompt_size, n_history, 1, C.byref(a), C.byref(b)) == 0
        assert g.swap_plan(n_ctx, prompt_size, n_history, n_keep=n_keep, n_system=n_system) == (a.value, b.value)
    assert g.swap_history(list(range(25)), 8) == [7, 15, 23, 24]
    with pytest.raises(ValueError):
        g.swap_plan(32, 4, 5, n_system=5)


# ---- the stop rule's new branch
class Row:
    """one row's stops and loop state on the host, the rules in the device's order"""

    def __init__(self, H, seqs=(), max_tokens=0, texts=(), pos=0, limit=0):
        self.H, self.limit, self.max_tokens = H, limit, max_tokens
        self.n, self.len, self.tok = len(seqs), np.zeros(16, np.int32), np.zeros((16, 8), np.int32)
        for k, q in enumerate(seqs):
            self.len[k] = len(q)
            self.tok[k, :len(q)] = q
        self.nt, self.tlen, self.tbytes = len(texts), np.zeros(16, np.int32), np.zeros((16, 32), np.uint8)
        for k, b in enumerate(texts):
            self.tlen[k] = len(b)
            self.tbytes[k, :len(b)] = list(b)
        self.state, self.text = np.zeros(10, np.int32), np.zeros(10, np.int32)
        H.ctx_reset(self.state.ctypes.data, self.text.ctypes.data)
        self.loop = np.array([pos, -7], np.int32)

    def draw(self, t, b=b""):
        raw = np.frombuffer(bytes(b) or b"\0", np.uint8).copy()
        return self.H.ctx_draw(self.n, self.len.ctypes.data, self.tok.ctypes.data, self.max_tokens, self.nt, self.tlen.ctypes.data, self.tbytes.ctypes.data,
                               self.state.ctypes.data, self.text.ctypes.data, self.loop.ctypes.data, self.limit, int(t), raw.ctypes.data, len(b))


def rule(limit, pos, reason):
    """the new branch, restated: (reason afterwards, whether position and token move) for a draw made at pos whose other rules said `reason`"""
    full = limit > 0 and pos + 1 >= limit
    return (CONTEXT if full and reason == RUNNING else reason), not full


def test_context_ends_the_row_at_the_filling_draw_and_nothing_moves(H):
    r = Row(H, pos=28, limit=32)
    for i, t in enumerate((5, 6, 7)):
        assert r.draw(t) == RUNNING and r.loop.tolist() == [29 + i, t]
    before = r.loop.tolist()
    assert r.draw(9) == CONTEXT                              # made at position 31: the cache is full
    assert r.loop.tolist() == before == [31, 7]              # the same token at the same position again
    assert r.state[0] == 4 and r.state[2:6].tolist() == [5, 6, 7, 9]      # the draw counted and entered the tail
    assert H.ctx_resume(r.state.ctypes.data) == 0 and r.state[1] == RUNNING
    assert r.state[0] == 4 and r.state[2:6].tolist() == [5, 6, 7, 9]
    assert H.ctx_resume(r.state.ctypes.data) == 1            # a running row is not resumed


def test_off_is_the_rule_as_it_was(H):
    r = Row(H, pos=30, limit=0)
    for i, t in enumerate((1, 2, 3, 4)):
        assert r.draw(t) == RUNNING and r.loop.tolist() == [31 + i, t]


def test_precedence_and_no_position_change_against_the_restatement(H):
    """a sequence, the budget and a string that complete on the filling draw each keep their reason; the position stays all the same; only a
    row ended by the context resumes"""
    cases = [(dict(seqs=[[4, 9]]), 0), (dict(max_tokens=2), BUDGET), (dict(texts=[b"xy"]), TEXT0), (dict(seqs=[[4, 9]], max_tokens=2, texts=[b"xy"]), 0),
             (dict(max_tokens=2, texts=[b"xy"]), TEXT0), (dict(seqs=[[1, 1]], max_tokens=5, texts=[b"zz"]), CONTEXT)]
    for kw, want in cases:
        for limit, pos in ((32, 30), (32, 12), (0, 30)):
            r = Row(H, pos=pos, limit=limit, **kw)
            assert r.draw(4, b"ax") == RUNNING and r.loop.tolist() == [pos + 1, 4]
            other = want if want != CONTEXT else RUNNING
            exp, moves = rule(limit, pos + 1, other)
            assert r.draw(9, b"yb") == exp, (kw, limit, pos)
            assert r.loop.tolist() == ([pos + 2, 9] if moves else [pos + 1, 4]), (kw, limit, pos)
            assert H.ctx_resume(r.state.ctypes.data) == (0 if exp == CONTEXT else 1)
            if exp >= TEXT0:
                assert r.text[1] == 3                       # cut_bytes: "xy" completed one byte before the token's end


def test_state_survives_the_swap(H):
    """a stop sequence and a stop string whose halves lie on either side of the context end, and a budget across two ends"""
    r = Row(H, seqs=[[8, 3]], pos=30, limit=32)
    assert r.draw(1) == RUNNING and r.draw(8) == CONTEXT
    assert H.ctx_resume(r.state.ctypes.data) == 0
    r.loop[0] = 16                                           # (the swap: the row goes on behind the regenerated tokens)
    assert r.draw(3) == 0
    r = Row(H, texts=[b"ser:"], pos=31, limit=32)
    assert r.draw(1, b" Use") == CONTEXT and H.ctx_resume(r.state.ctypes.data) == 0
    r.loop[0] = 16
    assert r.draw(2, b"r: hi") == TEXT0 and r.text[1] == 7
    r = Row(H, max_tokens=5, pos=30, limit=32)
    seen = []
    for t in range(5):
        seen.append(r.draw(t))
        if seen[-1] == CONTEXT:
            assert H.ctx_resume(r.state.ctypes.data) == 0
            r.loop[0] = 30
    assert seen == [RUNNING, CONTEXT, RUNNING, CONTEXT, BUDGET] and r.state[0] == 5
