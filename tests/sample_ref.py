"""The reference's own sampling functions (libfalcon.cpp:3038-3466, exported by oracle/_ref/libfalcon_ref.so), called in
falcon_main's order (examples/falcon/falcon_main.cpp:896-980) through ctypes: the yardstick of the device sampler."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libfalcon_ref.so")

TOKEN_DATA = np.dtype([("id", np.int32), ("logit", np.float32), ("p", np.float32)])


class TokenDataArray(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_size_t), ("sorted", C.c_bool)]


def tiny_ggcc(path):
    """a tiny GGCC file: the reference needs a context to hold its generator, the model itself is never evaluated"""
    import ggcc_writer
    import synth
    from oracle import binding as ob
    ob.build_oracle()
    w = synth.make_model(ob.Oracle(), synth.HP_TINY_MQA, ob.Q4_0, seed=5)
    ggcc_writer.write_ggcc(path, w)
    return path


class RefSampler:
    """one reference context = one generator (ctx->rng, persistent across draws)"""

    def __init__(self, ggcc_path, n_ctx=64):
        L = C.CDLL(REF_SO)
        L.reff_load.restype, L.reff_load.argtypes = C.c_void_p, [C.c_char_p, C.c_int, C.c_int]
        L.reff_free.argtypes = [C.c_void_p]
        vp, P = C.c_void_p, C.POINTER(TokenDataArray)
        L.llama_set_rng_seed.argtypes = [vp, C.c_int]
        L.llama_sample_repetition_penalty.argtypes = [vp, P, vp, C.c_size_t, C.c_float]
        L.llama_sample_frequency_and_presence_penalties.argtypes = [vp, P, vp, C.c_size_t, C.c_float, C.c_float]
        L.llama_sample_token_greedy.restype, L.llama_sample_token_greedy.argtypes = C.c_int, [vp, P]
        L.llama_sample_top_k.argtypes = [vp, P, C.c_int, C.c_size_t]
        L.llama_sample_tail_free.argtypes = [vp, P, C.c_float, C.c_size_t]
        L.llama_sample_typical.argtypes = [vp, P, C.c_float, C.c_size_t]
        L.llama_sample_top_p.argtypes = [vp, P, C.c_float, C.c_size_t]
        L.llama_sample_temperature.argtypes = [vp, P, C.c_float]
        L.llama_sample_token.restype, L.llama_sample_token.argtypes = C.c_int, [vp, P]
        self.L = L
        self.ctx = L.reff_load(os.fsencode(ggcc_path), n_ctx, 8)
        assert self.ctx, "reff_load failed"

    def seed(self, seed):
        assert 0 <= seed < 2 ** 31          # (llama_set_rng_seed replaces a negative seed by the time)
        self.L.llama_set_rng_seed(self.ctx, int(seed))

    def draw(self, logits, p, window):
        """falcon_main.cpp:898-980 on a copy of logits; p a ggllm_cpp_amd.Sampling, window the penalty window (list of ids)"""
        L, ctx = self.L, self.ctx
        lg = np.array(logits, np.float32)
        for i in range(p.n_bias):
            lg[p.bias_id[i]] += np.float32(p.bias[i])
        cand = np.zeros(lg.size, TOKEN_DATA)
        cand["id"] = np.arange(lg.size)
        cand["logit"] = lg
        arr = TokenDataArray(cand.ctypes.data, lg.size, False)
        ref = C.byref(arr)
        win = np.ascontiguousarray(window, np.int32)
        wp = win.ctypes.data if win.size else None
        L.llama_sample_repetition_penalty(ctx, ref, wp, win.size, p.repeat_penalty)
        L.llama_sample_frequency_and_presence_penalties(ctx, ref, wp, win.size, p.alpha_frequency, p.alpha_presence)
        if p.temp <= 0:
            return int(L.llama_sample_token_greedy(ctx, ref))
        L.llama_sample_top_k(ctx, ref, lg.size if p.top_k <= 0 else p.top_k, 1)
        L.llama_sample_tail_free(ctx, ref, p.tfs_z, 1)
        L.llama_sample_typical(ctx, ref, p.typical_p, 1)
        L.llama_sample_top_p(ctx, ref, p.top_p, 1)
        L.llama_sample_temperature(ctx, ref, p.temp)
        return int(L.llama_sample_token(ctx, ref))

    def free(self):
        self.L.reff_free(self.ctx)


def tie_free_row(rng, n_vocab, spread=3.0):
    """a logits row without equal values (the reference's unstable sorts leave the order of ties open)"""
    x = (rng.standard_normal(n_vocab) * spread).astype(np.float32)
    while True:
        _, first = np.unique(x, return_index=True)
        dup = np.setdiff1d(np.arange(n_vocab), first)
        if dup.size == 0:
            return x
        x[dup] = (rng.standard_normal(dup.size) * spread).astype(np.float32)


def run_ref(ref, rows, p, window, n_draws):
    """n_draws consecutive draws per row from one seeded generator; each drawn token enters the window (falcon_main.cpp:985-986)"""
    ref.seed(p.seed)
    win, out = list(window), []
    for d in range(n_draws):
        t = ref.draw(rows[d % len(rows)], p, win)
        out.append(t)
        if win:
            win = win[1:] + [t]
    return out
