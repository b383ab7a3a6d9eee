"""The reference's sampling functions in ALL of falcon_main's branches (examples/falcon/falcon_main.cpp:960-981): the default
chain with tail-free and typical (tests/sample_ref.py already calls them in chain order) and mirostat 1 / 2 with the `mu`
falcon_main keeps in a static. Plus the host restatement (tests/host/sample_chain_harness.cpp) the tests compare with."""
import ctypes as C
import os
import subprocess

import numpy as np

import sample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIROSTAT_M = 100        # falcon_main.cpp:966


def ggcc_with_vocab(path, n_vocab):
    """a GGCC file whose n_vocab is the row length: llama_sample_token_mirostat reads N from falcon_n_vocab(ctx)"""
    import ggcc_writer
    import synth
    from oracle import binding as ob
    ob.build_oracle()
    hp = dict(n_vocab=n_vocab, n_embd=64, n_head=1, n_head_kv=1, n_layer=1, n_ff=256, two_norms=False)
    ggcc_writer.write_ggcc(path, synth.make_model_fast(hp, ob.Q4_0, seed=5))
    return path


class RefChain(sample_ref.RefSampler):
    """sample_ref.RefSampler with falcon_main's three sampling branches; p: a ggllm_cpp_amd.SamplingExt"""

    def __init__(self, ggcc_path, n_ctx=64):
        super().__init__(ggcc_path, n_ctx)
        L, vp, P = self.L, C.c_void_p, C.POINTER(sample_ref.TokenDataArray)
        L.llama_sample_token_mirostat.restype = C.c_int
        L.llama_sample_token_mirostat.argtypes = [vp, P, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float)]
        L.llama_sample_token_mirostat_v2.restype = C.c_int
        L.llama_sample_token_mirostat_v2.argtypes = [vp, P, C.c_float, C.c_float, C.POINTER(C.c_float)]
        L.reff_n_vocab.restype, L.reff_n_vocab.argtypes = C.c_int, [vp]
        self.n_vocab = L.reff_n_vocab(self.ctx)
        self.mu = C.c_float(0.0)

    def start(self, p):
        """a generation's start: the generator seeded, mu = 2 tau"""
        self.seed(p.base.seed)
        self.mu = C.c_float(np.float32(2.0) * np.float32(p.mirostat_tau))

    def draw_ext(self, logits, p, window):
        if p.base.mirostat == 0 or p.base.temp <= 0:
            return self.draw(logits, p.base, window)
        L, ctx, b = self.L, self.ctx, p.base
        lg = np.array(logits, np.float32)
        for i in range(b.n_bias):
            lg[b.bias_id[i]] += np.float32(b.bias[i])
        cand = np.zeros(lg.size, sample_ref.TOKEN_DATA)
        cand["id"] = np.arange(lg.size)
        cand["logit"] = lg
        arr = sample_ref.TokenDataArray(cand.ctypes.data, lg.size, False)
        ref = C.byref(arr)
        win = np.ascontiguousarray(window, np.int32)
        wp = win.ctypes.data if win.size else None
        L.llama_sample_repetition_penalty(ctx, ref, wp, win.size, b.repeat_penalty)
        L.llama_sample_frequency_and_presence_penalties(ctx, ref, wp, win.size, b.alpha_frequency, b.alpha_presence)
        L.llama_sample_temperature(ctx, ref, b.temp)
        if b.mirostat == 1:
            return int(L.llama_sample_token_mirostat(ctx, ref, p.mirostat_tau, p.mirostat_eta, MIROSTAT_M, C.byref(self.mu)))
        return int(L.llama_sample_token_mirostat_v2(ctx, ref, p.mirostat_tau, p.mirostat_eta, C.byref(self.mu)))


def run_ref(ref, rows, p, window, n_draws):
    """n_draws consecutive draws from one seeded generator and one mu; returns (tokens, mu bits after every draw)"""
    ref.start(p)
    win, out, mus = list(window), [], []
    for d in range(n_draws):
        t = ref.draw_ext(rows[d % len(rows)], p, win)
        out.append(t)
        mus.append(np.float32(ref.mu.value).view(np.uint32).item())
        if win:
            win = win[1:] + [t]
    return out, mus


def build_harness(out_dir):
    """g++ on tests/host/sample_chain_harness.cpp (which includes the header the device compiles), typed for ctypes"""
    src = os.path.join(ROOT, "tests", "host", "sample_chain_harness.cpp")
    out = os.path.join(str(out_dir), "libsample_chain_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I",
                           os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", out, src])
    H = C.CDLL(out)
    u32, u64, f, i, vp = C.c_uint32, C.c_uint64, C.c_float, C.c_int, C.c_void_p
    H.chain_fn_mismatches.restype, H.chain_fn_mismatches.argtypes = C.c_longlong, [i, u32, u32, i, vp]
    H.chain_powf_mismatches.restype, H.chain_powf_mismatches.argtypes = C.c_longlong, [f, u32, u32, i, vp]
    H.chain_powf_random_mismatches.restype, H.chain_powf_random_mismatches.argtypes = C.c_longlong, [u64, u64, i, vp]
    H.chain_powf_pair.argtypes = [u64, u64, vp, vp]
    H.chain_powf_same.restype, H.chain_powf_same.argtypes = i, [f, f]
    H.chain_powf_bits.restype, H.chain_powf_bits.argtypes = u32, [f, f]
    H.chain_f2i.restype, H.chain_f2i.argtypes = i, [f]
    H.chain_mt_seed.argtypes = [vp, vp, u32]
    H.chain_draw.restype = i
    H.chain_draw.argtypes = [vp, i, f, i, f, f, f, i, f, f, i, f, f, f, vp, i, i, vp, vp, vp, vp, vp, vp]
    return H


class HostChain:
    """fq_sample_chain.h's chain on the host with falcon_main's loop state: one generator, one mu, a window that takes every draw"""

    def __init__(self, H, p, model_n_vocab=None):
        self.H, self.p, self.N = H, p, model_n_vocab
        self.mt, self.mti = (C.c_uint32 * 624)(), C.c_int()
        H.chain_mt_seed(self.mt, C.byref(self.mti), p.base.seed)
        self.mu = C.c_float(np.float32(2.0) * np.float32(p.mirostat_tau))
        self.ambiguous = C.c_int(0)

    def draw(self, x, win):
        p, b = self.p, self.p.base
        ids = np.array(list(b.bias_id), np.int32)
        bias = np.array(list(b.bias), np.float32)
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(win, np.int32)
        return self.H.chain_draw(x.ctypes.data, x.size, b.temp, b.top_k, b.top_p, b.tfs_z, b.typical_p, b.mirostat, p.mirostat_tau, p.mirostat_eta,
                                 self.N or x.size, b.repeat_penalty, b.alpha_frequency, b.alpha_presence, w.ctypes.data if w.size else None, w.size,
                                 b.n_bias, ids.ctypes.data, bias.ctypes.data, self.mt, C.byref(self.mti), C.byref(self.mu), C.byref(self.ambiguous))

    def run(self, rows, window, n_draws):
        win, out, mus = list(window), [], []
        for d in range(n_draws):
            t = self.draw(rows[d % len(rows)], win)
            out.append(t)
            mus.append(np.float32(self.mu.value).view(np.uint32).item())
            if win:
                win = win[1:] + [t]
        return out, mus
