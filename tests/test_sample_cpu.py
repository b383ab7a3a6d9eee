"""CPU: the sampler restatement the device compiles (ggllm.cpp_amd/csrc/fq_sample.h) is host-compiled with g++
(tests/host/sample_harness.cpp) and checked bit for bit: its expf against the host libm's on every input the chain can
meet, its mt19937 against std::mt19937, and the whole chain against the reference's own sampling functions
(oracle/_ref/libfalcon_ref.so, skipped when that build is absent)."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import ggllm_cpp_amd as g
import sample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host", "sample_harness.cpp")
    out = str(tmp_path_factory.mktemp("sample") / "libsample_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I",
                           os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", out, src])
    L = C.CDLL(out)
    L.sample_expf_mismatches.restype = C.c_longlong
    L.sample_expf_mismatches.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    L.sample_mt_mismatches.restype, L.sample_mt_mismatches.argtypes = C.c_int, [C.c_uint32, C.c_int]
    L.sample_mt_seed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.sample_canonical.restype, L.sample_canonical.argtypes = C.c_double, [C.c_void_p, C.c_void_p]
    L.sample_chain.restype = C.c_int
    L.sample_chain.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                               C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_expf_equals_libm_on_every_input_of_the_chain(harness):
    """the softmaxes subtract the maximum first: every f32 in [-104, -0] (below -103.97 expf is 0), about 1.1 G inputs"""
    first = C.c_uint32()
    bad = harness.sample_expf_mismatches(_bits(-0.0), _bits(-104.0), 16, C.byref(first))
    assert bad == 0, f"{bad} inputs differ from libm expf, the first at {struct.unpack('<f', struct.pack('<I', first.value))[0]!r}"


@pytest.mark.parametrize("seed", [0, 1, 7, 5489, 2 ** 31 - 1, (-1) % 2 ** 32, (-123456) % 2 ** 32])
def test_mt19937_matches_std(harness, seed):
    """several twists deep (3000 draws > 624); negative int32 seeds reduced mod 2^32 as std::mt19937::seed does"""
    assert harness.sample_mt_mismatches(seed, 3000) == 0


def test_canonical_is_two_draws(harness):
    """generate_canonical<double, 53>: (g1 + g2 * 2^32) / 2^64 from two consecutive outputs"""
    mt, mti = (C.c_uint32 * 624)(), C.c_int()
    harness.sample_mt_seed(mt, C.byref(mti), 42)
    rng = np.random.RandomState()          # (numpy's MT19937 shares std::mt19937's init_genrand seeding)
    rng.seed(42)
    for _ in range(700):
        g1, g2 = (int(x) for x in rng.randint(0, 2 ** 32, size=2, dtype=np.uint64))
        exp = (float(g1) + float(g2) * 4294967296.0) / 18446744073709551616.0
        assert harness.sample_canonical(mt, C.byref(mti)) == exp


class HostChain:
    """fq_sample.h's chain on the host, with falcon_main's loop state: one generator, a window that takes every draw"""

    def __init__(self, L, p):
        self.L, self.p = L, p
        self.mt, self.mti = (C.c_uint32 * 624)(), C.c_int()
        L.sample_mt_seed(self.mt, C.byref(self.mti), p.seed)

    def run(self, rows, window, n_draws):
        p, win, out = self.p, list(window), []
        ids = np.array(list(p.bias_id), np.int32)
        bias = np.array(list(p.bias), np.float32)
        for d in range(n_draws):
            x = np.ascontiguousarray(rows[d % len(rows)], np.float32)
            w = np.ascontiguousarray(win, np.int32)
            t = self.L.sample_chain(x.ctypes.data, x.size, p.temp, p.top_k, p.top_p, p.repeat_penalty, p.alpha_frequency, p.alpha_presence,
                                    w.ctypes.data if w.size else None, w.size, p.n_bias, ids.ctypes.data, bias.ctypes.data,
                                    self.mt, C.byref(self.mti))
            out.append(t)
            if win:
                win = win[1:] + [t]
        return out


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not os.path.exists(sample_ref.REF_SO):
        pytest.skip("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    r = sample_ref.RefSampler(sample_ref.tiny_ggcc(str(tmp_path_factory.mktemp("ggcc") / "tiny.ggcc")))
    yield r
    r.free()


GRID = list(itertools.product([1, 40, 5000, 0], [1.0, 0.95, 0.1], [0.0, 0.3, 0.8, 1.5], [False, True]))


@pytest.mark.parametrize("n_vocab", [65024, 300, 7])
def test_chain_matches_reference(harness, ref, n_vocab):
    """same tokens and the same generator stream as the reference's functions over consecutive draws, for every point of a
    (top_k, top_p, temp, penalties) grid; -inf bias on one id (--ignore-eos) in the penalised half"""
    rng = np.random.default_rng(n_vocab)
    big = n_vocab > 10000
    n_rows, n_draws = (2, 5) if big else (6, 24)
    rows = [sample_ref.tie_free_row(rng, n_vocab, spread=s) for s in ([2.0, 6.0] if big else [1.0, 3.0, 10.0, 0.5, 2.0, 30.0])]
    for top_k, top_p, temp, pen in GRID:
        window = [int(t) for t in rng.integers(0, n_vocab, 64)] + [0] * 8 if pen else []
        window = window[-64:]
        p = g.sampling(temp=temp, top_k=top_k, top_p=top_p, repeat_penalty=1.1 if pen else 1.0, repeat_last_n=len(window),
                       frequency_penalty=0.3 if pen else 0.0, presence_penalty=0.2 if pen else 0.0,
                       seed=int(rng.integers(0, 2 ** 31)), logit_bias={n_vocab - 1: float("-inf")} if pen else None)
        want = sample_ref.run_ref(ref, rows[:n_rows], p, window, n_draws)
        got = HostChain(harness, p).run(rows[:n_rows], window, n_draws)
        assert got == want, (top_k, top_p, temp, pen)


def test_chain_generator_stream_continues(harness, ref):
    """the draws after a run of single-candidate (no-draw) steps still match: top_k 1 consumes nothing, then top_k 40 draws"""
    rng = np.random.default_rng(3)
    rows = [sample_ref.tie_free_row(rng, 1000) for _ in range(3)]
    p1 = g.sampling(temp=0.8, top_k=1, top_p=1.0, repeat_penalty=1.0, seed=11)
    p2 = g.sampling(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.0, seed=11)
    ref.seed(11)
    want = [ref.draw(rows[i % 3], p1, []) for i in range(5)] + [ref.draw(rows[i % 3], p2, []) for i in range(30)]
    h = HostChain(harness, p1)
    got = h.run(rows, [], 5)
    h.p = p2
    got += h.run(rows, [], 30)
    assert got == want


def test_window_helper_pads_with_zeros():
    assert g.sampling_window([5, 6, 7], n_ctx=8, repeat_last_n=5) == [0, 0, 5, 6, 7]
    assert g.sampling_window([5, 6, 7], n_ctx=4, repeat_last_n=-1) == [0, 5, 6, 7]
    assert g.sampling_window(range(100), n_ctx=16, repeat_last_n=64) == list(range(84, 100))
    assert g.sampling_window([1], n_ctx=16, repeat_last_n=0) == []
