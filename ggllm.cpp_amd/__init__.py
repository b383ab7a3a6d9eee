"""ggllm.cpp_amd -- thin ctypes view of libggml_hip.so (the MI355X-native backend for ggllm.cpp's hot path).

The product is the C-ABI shared library built from csrc/ (HIP kernels for gfx950 + the C entry points declared in
include/*.h). This module only loads it and wraps pointers for tests / bench.py; there is no Python compute path and
no CPU fallback: importing works anywhere, but every call needs the library AND a HIP device, otherwise it raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("GGLLM_HIP_LIB") or os.path.join(PKG_DIR, "libggml_hip.so")      # (GGLLM_HIP_LIB: A/B builds of the same library)

# enum ggml_type values (ggml.h:247-268)
F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q8_1 = 0, 1, 2, 3, 6, 7, 8, 9
Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, Q8_K = 10, 11, 12, 13, 14, 15
BLCK = {Q4_0: 32, Q4_1: 32, Q5_0: 32, Q5_1: 32, Q8_0: 32, Q8_1: 32, Q2_K: 256, Q3_K: 256, Q4_K: 256, Q5_K: 256, Q6_K: 256, Q8_K: 256}
TSIZE = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34, Q8_1: 40, Q2_K: 84, Q3_K: 110, Q4_K: 144, Q5_K: 176, Q6_K: 210, Q8_K: 292}
LEGACY = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
KQUANTS = (Q2_K, Q3_K, Q4_K, Q5_K, Q6_K)
TYPE_NAME = {Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1", Q8_0: "q8_0", Q8_1: "q8_1",
             Q2_K: "q2_K", Q3_K: "q3_K", Q4_K: "q4_K", Q5_K: "q5_K", Q6_K: "q6_K", Q8_K: "q8_K"}
VEC_DOT = {Q4_0: Q8_0, Q5_0: Q8_0, Q8_0: Q8_0, Q4_1: Q8_1, Q5_1: Q8_1, Q2_K: Q8_K, Q3_K: Q8_K, Q4_K: Q8_K, Q5_K: Q8_K, Q6_K: Q8_K}

EXPORTS_OPS = """ggml_hip_init ggml_hip_split_configure ggml_hip_tensor_split_rows ggml_hip_weight_upload_rows ggml_hip_split_comm_create ggml_hip_split_comm_free ggml_hip_split_comm_agree ggml_hip_mul_mat_q_split ggml_hip_mul_mat_q_split_local ggml_hip_split_comm_create_loopback ggml_hip_split_comm_rccl_ranks ggml_hip_mul_mat_q_split_loopback ggml_hip_shim_pool_stats ggml_hip_get_reference_order ggml_hip_debug_force_gemv ggml_hip_debug_ring_general ggml_hip_debug_attention_form ggml_hip_debug_attention_plan ggml_hip_debug_mul_mat_plan ggml_hip_debug_exp_boundary ggml_hip_debug_scalar_eval ggml_hip_gemm_sequential ggml_hip_reference_order ggml_hip_debug_stamps ggml_hip_selftest ggml_hip_exp_formula_mismatches ggml_hip_device_count ggml_hip_stream ggml_hip_malloc ggml_hip_free ggml_hip_memcpy_h2d
ggml_hip_memcpy_d2h ggml_hip_memcpy_d2d ggml_hip_memset ggml_hip_synchronize ggml_hip_event_create ggml_hip_event_record
ggml_hip_event_elapsed_ms ggml_hip_event_destroy ggml_hip_profile_begin ggml_hip_profile_end ggml_hip_profile_bracket_overhead_us ggml_hip_gelu_table_dev ggml_hip_exp_table_dev ggml_hip_weight_upload
ggml_hip_weight_free ggml_hip_weight_nbytes ggml_hip_dequantize_rows ggml_hip_quantize_rows ggml_hip_weight_quantize ggml_hip_fp16_to_fp32_row ggml_hip_acts_alloc ggml_hip_acts_free
ggml_hip_quantize_acts ggml_hip_acts_export ggml_hip_mul_mat_q ggml_hip_mul_mat_f16 ggml_hip_mul_mat_q_acts ggml_hip_layer_norm ggml_hip_gelu
ggml_hip_add3 ggml_hip_rope_table_create ggml_hip_rope_kv_store ggml_hip_attention ggml_hip_attention_decode
ggml_hip_sampler_create ggml_hip_sampler_free ggml_hip_sampler_set_row ggml_hip_sampler_sample ggml_hip_sampler_copy_row
ggml_hip_sampler_set_stops ggml_hip_sampler_get_stops ggml_hip_sampler_set_row_ext ggml_hip_sampler_get_mu
ggml_hip_sampler_set_vocab_bytes ggml_hip_sampler_set_stop_text ggml_hip_sampler_get_stop_text
ggml_hip_sampler_set_context_stop ggml_hip_sampler_resume
ggml_hip_score_rows ggml_hip_logprob_rows ggml_hip_embed_pool_accum ggml_hip_embed_pool_finish
ggml_hip_sampler_get_rng ggml_hip_sampler_set_rng ggml_hip_kv_pack ggml_hip_kv_unpack
ggml_hip_sampler_verify_rows ggml_hip_draft_lookup
ggml_hip_guide_rows ggml_hip_sampler_set_guidance ggml_hip_sampler_get_guidance
ggml_hip_grammar_create ggml_hip_grammar_last_error ggml_hip_grammar_free ggml_hip_grammar_get_index ggml_hip_sampler_set_grammar ggml_hip_sampler_get_grammar_state""".split()
EXPORTS_FALCON = """falcon_hip_model_create falcon_hip_model_free falcon_hip_model_set_tensor falcon_hip_model_weight_bytes
falcon_hip_context_create falcon_hip_context_free falcon_hip_eval falcon_hip_eval_stage falcon_hip_stage_step falcon_hip_decode_greedy falcon_hip_eval_token falcon_hip_context_last_error falcon_hip_context_set_rope_n_ctx
falcon_hip_get_logits falcon_hip_context_keep_hidden falcon_hip_get_hidden falcon_hip_context_use_graph falcon_hip_context_graph_captures
falcon_hip_eval_debug_timings falcon_hip_context_set_fused falcon_hip_context_sync_error falcon_hip_model_load_ggcc falcon_hip_ggcc_scan falcon_hip_plan_stages falcon_hip_model_quantize falcon_hip_perplexity
falcon_hip_vocab_load_ggcc falcon_hip_vocab_error falcon_hip_vocab_free falcon_hip_vocab_size falcon_hip_vocab_merges falcon_hip_tokenize
falcon_hip_token_to_bytes falcon_hip_token_bos falcon_hip_token_eos
falcon_hip_model_get_hparams falcon_hip_context_create_seqs falcon_hip_context_n_seq falcon_hip_eval_seqs falcon_hip_decode_greedy_seqs falcon_hip_context_copy_seq
falcon_hip_context_set_sampling falcon_hip_sample falcon_hip_decode_sample falcon_hip_decode_sample_seqs falcon_hip_context_copy_sampling falcon_hip_eval_score falcon_hip_context_set_logprobs falcon_hip_get_logprobs
falcon_hip_context_set_stops falcon_hip_context_get_stops falcon_hip_context_set_stop_poll falcon_hip_context_loop_steps
falcon_hip_context_set_sampling_ext falcon_hip_context_get_mirostat_mu
falcon_hip_model_set_vocab falcon_hip_context_set_stop_text falcon_hip_context_get_stop_text
falcon_hip_swap_plan falcon_hip_swap_history falcon_hip_context_set_context_stop falcon_hip_context_resume falcon_hip_context_swap
falcon_hip_context_set_guidance falcon_hip_context_get_guidance
falcon_hip_session_hparams_ggcc falcon_hip_state_size falcon_hip_copy_state falcon_hip_set_state falcon_hip_session_save falcon_hip_session_load
falcon_hip_model_apply_lora falcon_hip_lora_scan falcon_hip_model_get_tensor
falcon_hip_context_set_spec falcon_hip_context_set_spec_guess falcon_hip_decode_spec falcon_hip_context_get_spec_stats
falcon_hip_grammar_create falcon_hip_grammar_free falcon_hip_context_set_grammar falcon_hip_context_get_grammar_state
falcon_hip_context_set_embedding falcon_hip_get_embeddings falcon_hip_embed falcon_hip_embedding_pool_reset falcon_hip_get_embedding_pooled falcon_hip_embedding_pool_count
falcon_hip_pipeline_unique_id falcon_hip_pipeline_create falcon_hip_pipeline_create_local falcon_hip_pipeline_free falcon_hip_pipeline_rccl_ranks falcon_hip_pipeline_transport falcon_hip_rccl_selftest falcon_hip_pipeline_set_tokens
falcon_hip_pipeline_run falcon_hip_pipeline_run_local falcon_hip_pipeline_local_attach_rccl falcon_hip_pipeline_get_history falcon_hip_pipeline_schedule""".split()


def build(verbose=False):
    """hipcc every HIP source for gfx950 into ggllm.cpp_amd/libggml_hip.so (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(PKG_DIR, "csrc"), "-j", str(min(16, os.cpu_count() or 4))]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd + ["all"])
    return LIB_PATH


class Sampling(C.Structure):
    """ggml_hip_sampling (include/ggml-hip-ops.h): falcon_main's sampler parameters"""
    _fields_ = [("temp", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("repeat_penalty", C.c_float), ("repeat_last_n", C.c_int32),
                ("alpha_frequency", C.c_float), ("alpha_presence", C.c_float), ("tfs_z", C.c_float), ("typical_p", C.c_float),
                ("mirostat", C.c_int32), ("seed", C.c_uint32), ("n_bias", C.c_int32), ("bias_id", C.c_int32 * 16), ("bias", C.c_float * 16)]


def sampling(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64, frequency_penalty=0.0, presence_penalty=0.0,
             seed=0, logit_bias=None, tfs_z=1.0, typical_p=1.0, mirostat=0):
    """a Sampling; the defaults are falcon_main's (examples/falcon_common.h:41-52). logit_bias: {token id: bias} (float("-inf") for
    --ignore-eos)"""
    p = Sampling(temp, top_k, top_p, repeat_penalty, repeat_last_n, frequency_penalty, presence_penalty, tfs_z, typical_p, mirostat,
                 int(seed) % (1 << 32), 0)
    for i, (tid, b) in enumerate(sorted((logit_bias or {}).items())):
        if i >= 16:
            p.n_bias = len(logit_bias)          # (refused by set_sampling)
            break
        p.bias_id[i], p.bias[i] = int(tid), float(b)
        p.n_bias = i + 1
    return p


class SamplingExt(C.Structure):
    """ggml_hip_sampling_ext (include/ggml-hip-ops.h): a Sampling whose tfs_z, typical_p and mirostat are honoured, and mirostat's
    target surprise tau and learning rate eta"""
    _fields_ = [("base", Sampling), ("mirostat_tau", C.c_float), ("mirostat_eta", C.c_float)]


def sampling_ext(tfs_z=1.0, typical_p=1.0, mirostat=0, mirostat_tau=5.0, mirostat_eta=0.1, **base):
    """a SamplingExt for set_sampling_ext: sampling(**base) plus tail-free, typical and mirostat 1 / 2 (falcon_main's --tfs,
    --typical, --mirostat, --mirostat-ent, --mirostat-lr; the defaults are its own)"""
    return SamplingExt(sampling(tfs_z=tfs_z, typical_p=typical_p, mirostat=mirostat, **base), mirostat_tau, mirostat_eta)


EMBED_LAST, EMBED_POOL = 1, 2                           # falcon_hip_context_set_embedding's mode bits
SPEC_MAX_DRAFT, SPEC_LOOKUP, SPEC_GIVEN = 15, 1, 2        # draft-and-verify decode (set_spec): drafts per pass, the two sources
STOP_MAX_SEQS, STOP_MAX_LEN, STOP_RUNNING, STOP_BUDGET = 16, 8, -1, -2
STOP_CONTEXT = -3         # the draw filled the sequence's cache (set_context_stop): swap and go on


class Stops(C.Structure):
    """ggml_hip_stops (include/ggml-hip-ops.h): a row's stop sequences (token ids) and its budget of drawn tokens"""
    _fields_ = [("n_seqs", C.c_int32), ("len", C.c_int32 * STOP_MAX_SEQS), ("tok", (C.c_int32 * STOP_MAX_LEN) * STOP_MAX_SEQS), ("max_tokens", C.c_int32)]


def stops(seqs=(), max_tokens=0):
    """a Stops: seqs up to 16 sequences of 1..8 token ids each, max_tokens the budget of drawn tokens (0: none). ValueError for more
    sequences or longer ones than the structure holds (ids and the budget are checked where the stops are set)"""
    seqs = [[int(t) for t in q] for q in seqs]
    if len(seqs) > STOP_MAX_SEQS:
        raise ValueError("%d stop sequences (at most %d)" % (len(seqs), STOP_MAX_SEQS))
    st = Stops()
    st.n_seqs, st.max_tokens = len(seqs), int(max_tokens)
    for k, q in enumerate(seqs):
        if not 1 <= len(q) <= STOP_MAX_LEN:
            raise ValueError("stop sequence %d has %d tokens (1..%d)" % (k, len(q), STOP_MAX_LEN))
        st.len[k] = len(q)
        for j, t in enumerate(q):
            st.tok[k][j] = t
    return st


STOP_TEXT_MAX, STOP_TEXT_MAX_LEN, STOP_TEXT0 = 16, 32, 16


class StopText(C.Structure):
    """ggml_hip_stop_text (include/ggml-hip-ops.h): a row's stop strings, matched on the bytes of the drawn tokens"""
    _fields_ = [("n", C.c_int32), ("len", C.c_int32 * STOP_TEXT_MAX), ("bytes", (C.c_uint8 * STOP_TEXT_MAX_LEN) * STOP_TEXT_MAX)]


def stop_text(strings=()):
    """a StopText: up to 16 strings of 1..32 bytes each (bytes, or str encoded as UTF-8); a row that ends on string k reports the reason
    STOP_TEXT0 + k. ValueError for more strings or longer ones than the structure holds"""
    raw = [x if isinstance(x, (bytes, bytearray)) else str(x).encode("utf-8") for x in strings]
    if len(raw) > STOP_TEXT_MAX:
        raise ValueError("%d stop strings (at most %d)" % (len(raw), STOP_TEXT_MAX))
    st = StopText()
    st.n = len(raw)
    for k, b in enumerate(raw):
        if not 1 <= len(b) <= STOP_TEXT_MAX_LEN:
            raise ValueError("stop string %d has %d bytes (1..%d)" % (k, len(b), STOP_TEXT_MAX_LEN))
        st.len[k] = len(b)
        for j, x in enumerate(bytes(b)):
            st.bytes[k][j] = x
    return st


from .grammar import Dfa, dfa, regex_dfa, choice_dfa       # byte automata for constrained decoding (host side, pure Python)  # noqa: E402

GRAMMAR_MAX_STATES, GRAMMAR_BAD_ARGS, GRAMMAR_BAD_TRANS, GRAMMAR_DEAD_END = 16384, 1, 2, 3


class DfaStruct(C.Structure):
    """ggml_hip_dfa (include/ggml-hip-ops.h): a byte automaton's table as the library takes it"""
    _fields_ = [("n_states", C.c_int32), ("start", C.c_int32), ("trans", C.c_void_p), ("accept", C.c_void_p)]


def dfa_struct(d):
    """the DfaStruct of a Dfa; it points into d's arrays, which must outlive its use"""
    return DfaStruct(d.n_states, d.start, d.trans.ctypes.data, d.accept.ctypes.data)


class GrammarError(ValueError):
    """a grammar the library refused: .code is GRAMMAR_BAD_ARGS / GRAMMAR_BAD_TRANS / GRAMMAR_DEAD_END, .state the state to blame (-1: none)"""

    def __init__(self, what, code, state):
        super().__init__("%s (code %d, state %d)" % (what, code, state))
        self.code, self.state = code, state


class Grammar:
    """ggml_hip_grammar: an automaton indexed on the device against one vocabulary (FalconModel.grammar, or make() over raw bytes)"""

    def __init__(self, handle, d):
        self.h, self.dfa = handle, d

    @classmethod
    def make(cls, vocab_bytes, d, eos_id=None):
        """ggml_hip_grammar_create over a list of the tokens' byte strings; GrammarError when refused"""
        offs = np.zeros(len(vocab_bytes) + 1, np.int32)
        offs[1:] = np.cumsum([len(b) for b in vocab_bytes])
        pool = np.frombuffer(b"".join(vocab_bytes) or b"\0", np.uint8).copy()
        bad = C.c_int(-1)
        L = load()
        h = L.ggml_hip_grammar_create(len(vocab_bytes), pool.ctypes.data, offs.ctypes.data, C.byref(dfa_struct(d)), -1 if eos_id is None else int(eos_id), C.byref(bad))
        if not h:
            raise GrammarError("ggml_hip_grammar_create refused this grammar", L.ggml_hip_grammar_last_error(), bad.value)
        gr = cls(h, d)
        gr._n_words = (len(vocab_bytes) + 63) // 64
        return gr

    def index(self, state0=0, n=None):
        """rows [state0, state0 + n) of the index, uint64 [n][ceil(n_vocab / 64)] (ggml_hip_grammar_get_index)"""
        n = self.dfa.n_states - state0 if n is None else n
        words = np.zeros((n, self._n_words), np.uint64)
        if load().ggml_hip_grammar_get_index(self.h, int(state0), int(n), words.ctypes.data) != 0:
            raise ValueError("ggml_hip_grammar_get_index refused")
        return words

    def free(self):
        """ggml_hip_grammar_free; ValueError while a sampler row or sequence still holds the grammar"""
        if self.h:
            if load().ggml_hip_grammar_free(self.h) != 0:
                raise ValueError("ggml_hip_grammar_free: the grammar is still bound")
            self.h = None


def _make_model_grammar(model_handle, n_vocab, d, eos_id):
    bad = C.c_int(-1)
    L = load()
    h = L.falcon_hip_grammar_create(model_handle, C.byref(dfa_struct(d)), -1 if eos_id is None else int(eos_id), C.byref(bad))
    if not h:
        raise GrammarError("falcon_hip_grammar_create refused this grammar", L.ggml_hip_grammar_last_error(), bad.value)
    gr = Grammar(h, d)
    gr._n_words = (n_vocab + 63) // 64
    return gr


def _set_grammar(ctx, seq, gr, state):
    if load().falcon_hip_context_set_grammar(ctx, int(seq), gr.h if gr is not None else None, -1 if state is None else int(state)) != 0:
        raise ValueError("falcon_hip_context_set_grammar refused")


def _grammar_state(ctx, B):
    st = np.zeros(B, np.int32)
    if load().falcon_hip_context_get_grammar_state(ctx, st.ctypes.data) != 0:
        raise RuntimeError("falcon_hip_context_get_grammar_state failed")
    return st


class SwapCfg(C.Structure):
    """falcon_hip_swap_cfg (include/falcon-hip.h): one generation's constants for the context-swap planner"""
    _fields_ = [("n_ctx", C.c_int32), ("n_system", C.c_int32), ("n_keep", C.c_int32), ("prompt_size", C.c_int32)]


def swap_plan(n_ctx, prompt_size, n_history, n_keep=0, n_system=0, n_pending=1):
    """falcon_hip_swap_plan (host only): (n_past_new, n_regen) of falcon_main's context swap for a history of n_history tokens whose
    last n_pending wait to be evaluated; the regenerated tokens are history[n_history - n_pending - n_regen : n_history - n_pending].
    n_keep as falcon_main's --keep (negative: the whole prompt); prompt_size counts the n_system system tokens. ValueError when refused"""
    cfg = SwapCfg(int(n_ctx), int(n_system), int(n_keep), int(prompt_size))
    a, b = C.c_int(0), C.c_int(0)
    if load().falcon_hip_swap_plan(C.byref(cfg), int(n_history), int(n_pending), C.byref(a), C.byref(b)) != 0:
        raise ValueError("falcon_hip_swap_plan refused this configuration")
    return a.value, b.value


def swap_history(prompt, n_batch):
    """falcon_hip_swap_history: what a prompt consumed in batches of n_batch leaves in falcon_main's history -- the last token of
    every batch (a list; the caller appends every drawn token)"""
    tok = np.ascontiguousarray(prompt, np.int32)
    out = np.zeros(max(tok.size, 1), np.int32)
    n = load().falcon_hip_swap_history(tok.ctypes.data, tok.size, int(n_batch), out.ctypes.data)
    return out[:n].tolist()


def _context_swap(ctx, seq, n_past_new, regen, n_batch):
    r = np.ascontiguousarray(regen, np.int32)
    rc = load().falcon_hip_context_swap(ctx, int(seq), int(n_past_new), r.ctypes.data if r.size else None, r.size, int(n_batch))
    if rc != 0:
        raise ValueError("falcon_hip_context_swap refused (%d)" % rc)


def _set_context_stop(ctx, on):
    if load().falcon_hip_context_set_context_stop(ctx, 1 if on else 0) != 0:
        raise ValueError("falcon_hip_context_set_context_stop refused")


def _resume(ctx, seq):
    if load().falcon_hip_context_resume(ctx, int(seq)) != 0:
        raise ValueError("falcon_hip_context_resume: sequence %d did not end with STOP_CONTEXT" % int(seq))


def generate_swap(model, prompt, n_predict, params, n_keep=0, n_system=0, n_batch=512, stops=None, stop_text=None, use_graph=True):
    """The context-swap driver -- falcon_main's generation (falcon_main.cpp:694-751 around its sampling loop) through this library:
    prompt in batches of n_batch, then loop -> plan -> swap -> loop until n_predict tokens are drawn or a stop ends the sequence.
    model: a FalconModel (its context's n_batch >= min(n_batch, len(prompt))); prompt: token ids, the n_system system tokens first,
    at most n_ctx - 4 of them (falcon_main.cpp:475); n_predict: draws in all (<= 0: until a stop); params: a Sampling or SamplingExt
    (greedy past n_ctx is temp <= 0); n_keep: falcon_main's --keep; stops: a Stops (default: a budget of n_predict draws);
    stop_text: a StopText (the model's vocabulary must be set). The rope context is falcon_main's (:835-836): min(n_ctx, prompt +
    n_predict) for n_predict > 0, else n_ctx. Leaves the context stop on. Returns (the drawn tokens, [(n_past_new, regen ids)] per swap)."""
    n_ctx = model.n_ctx
    ids = [int(t) for t in np.asarray(prompt).ravel()]
    if not 1 <= len(ids) <= n_ctx - 4:
        raise ValueError("a prompt of %d tokens (1..n_ctx - 4 = %d)" % (len(ids), n_ctx - 4))
    model.set_rope_n_ctx(min(n_ctx, len(ids) + n_predict) if n_predict > 0 else n_ctx)
    for i in range(0, len(ids), n_batch):
        model.eval(ids[i:i + n_batch], i, logits_all=False)
    if isinstance(params, SamplingExt):
        model.set_sampling_ext(params, ids)
    else:
        model.set_sampling(params, ids)
    model.set_stops(stops if stops is not None else Stops(max_tokens=max(int(n_predict), 0)))
    if stop_text is not None:
        model.set_stop_text(stop_text)
    model.set_context_stop(True)
    hist = swap_history(ids, n_batch)
    out, swaps = [], []
    tok, pos = model.sample(), len(ids)
    while tok >= 0:
        out.append(tok)
        hist.append(tok)
        reason = model.stop_state()[1]
        if (n_predict > 0 and len(out) >= n_predict) or reason not in (STOP_RUNNING, STOP_CONTEXT):
            break
        if reason == STOP_CONTEXT:                               # the cache is full and tok waits: keep, regenerate, go on behind them
            nk, nr = swap_plan(n_ctx, len(ids), len(hist), n_keep, n_system)
            regen = hist[len(hist) - 1 - nr:len(hist) - 1]
            model.context_swap(nk, regen, n_batch)
            swaps.append((nk, regen))
            pos = nk + nr
        want = n_ctx - pos if n_predict <= 0 else min(n_predict - len(out), n_ctx - pos)
        got = [int(t) for t in model.decode_sample(tok, pos, want, use_graph=use_graph) if t >= 0]
        if not got:
            break
        out += got[:-1]
        hist += got[:-1]
        pos += len(got)
        tok = got[-1]
    return out, swaps


def generate_guided(model, prompt, negative, n_predict, params, scale, stops=None, stop_text=None, grammar=None, use_graph=True, end=None):
    """Classifier-free guidance (falcon_hip_context_set_guidance) end to end: prompt[:-1] and negative[:-1] are prefilled in plain contexts and copied
    into slots 0 and 1 of a two-sequence context, slot 0 gets params with the prompt as its history and slot 1 as its guide at `scale`, and one sampled
    loop of n_predict steps starts from the two last prompt tokens at their own positions -- the first generated token is guided too.
    model: a FalconModel (n_batch >= the longer of the two prefills); prompt, negative: token ids (at least one each; len + n_predict <= n_ctx);
    params: a Sampling or SamplingExt; stops / stop_text / grammar: slot 0's (a Stops, a StopText, a Grammar of the model).
    Returns the drawn tokens, up to the end a stop rule made; end: a dict that receives slot 0's n_drawn, reason and cut_bytes (stop_state, stop_text_state)."""
    ids, neg = [int(t) for t in np.asarray(prompt).ravel()], [int(t) for t in np.asarray(negative).ravel()]
    n_ctx = model.n_ctx
    if not ids or not neg or n_predict < 1 or max(len(ids), len(neg)) - 1 + n_predict > n_ctx:
        raise ValueError("prompts of %d and %d tokens and %d steps (at least one token each, the longer + steps - 1 <= n_ctx = %d)" % (len(ids), len(neg), n_predict, n_ctx))
    sc = SeqContext(model, n_ctx, 2)
    try:
        for slot, toks in enumerate((ids, neg)):
            if len(toks) > 1:
                model.eval(toks[:-1], 0, logits_all=False)
                if copy_seq(sc, slot, model, 0, len(toks) - 1) != 0:
                    raise RuntimeError("falcon_hip_context_copy_seq refused slot %d" % slot)
        if isinstance(params, SamplingExt):
            sc.set_sampling_ext(0, params, ids)
        else:
            sc.set_sampling(0, params, ids)
        if stops is not None:
            sc.set_stops(0, stops)
        if stop_text is not None:
            sc.set_stop_text(0, stop_text)
        if grammar is not None:
            sc.set_grammar(0, grammar)
        sc.set_guidance(0, 1, scale)
        out = sc.decode_sample([ids[-1], neg[-1]], [len(ids) - 1, len(neg) - 1], n_predict, use_graph=use_graph)
        if end is not None:
            n_drawn, reason = sc.stop_state()
            end.update(n_drawn=int(n_drawn[0]) if stops is not None or stop_text is not None else int(n_predict), reason=int(reason[0]),
                       cut_bytes=int(sc.stop_text_state()[0]) if stop_text is not None else 0)
        return [int(t) for t in out[:, 0] if t >= 0]
    finally:
        sc.free()


def sampling_window(history, n_ctx, repeat_last_n=64):
    """falcon_main's penalty window for a token history: the last min(repeat_last_n, n_ctx) (-1: n_ctx) entries of n_ctx zeros
    followed by the history (falcon_main.cpp:620-622, 949); what set_sampling builds from the history on the device side"""
    n = n_ctx if repeat_last_n < 0 else min(repeat_last_n, n_ctx)
    full = [0] * n_ctx + [int(t) for t in history]
    return full[len(full) - n:] if n else []


class HParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_vocab", "n_embd", "n_head", "n_head_kv", "n_layer", "n_ff", "two_norms", "layer_begin", "layer_end")]


class SessionHParams(C.Structure):
    """falcon_hip_session_hparams (include/falcon-hip.h): the hparams record of a session file, the reference's nine int32 in its order"""
    _fields_ = [(n, C.c_int32) for n in
                ("n_vocab", "n_ctx", "n_embd", "n_head", "n_head_kv", "n_layer", "n_falcon_type", "n_bpe_merges", "ftype")]


# llama_ftype of a file whose matrices have one ggml type (libfalcon.h; what falcon_quantize writes into the header)
FTYPE_OF_TYPE = {F32: 0, 1: 1, Q4_0: 2, Q4_1: 3, Q8_0: 7, Q5_0: 8, Q5_1: 9, Q2_K: 10, Q3_K: 12, Q4_K: 15, Q5_K: 17, Q6_K: 18}
SESSION_ERRORS = {1: "not a session file (magic, version)", 2: "the hparams record differs", 3: "more tokens than the buffer holds", 4: "truncated",
                  5: "kv_ntok outside 0..n_ctx", 6: "kv_size differs", 7: "an embedding section", 8: "unreadable generator text", 9: "logits size above capacity",
                  16: "bad argument", 17: "a pipeline stage holds no whole session", 18: "sequence out of range", 19: "the stream is capturing",
                  20: "staging allocation failed", 21: "file i/o"}


class SessionError(RuntimeError):
    """a session call was refused; .code is the C ABI's (FALCON_HIP_SESSION_E_*, include/falcon-hip.h). Nothing was changed."""

    def __init__(self, what, code):
        RuntimeError.__init__(self, "%s refused: %s (%d)" % (what, SESSION_ERRORS.get(code, "?"), code))
        self.code = code


LORA_ERRORS = {1: "the adapter cannot be read", 2: "bad file magic", 3: "unsupported file version", 4: "r is not positive", 5: "truncated",
               6: "a name without .loraA / .loraB", 7: "not a 2-D matrix of this model", 8: "n_dims is not 2", 9: "a data type other than F32 / F16",
               10: "the adapter's K or M is not the matrix's", 11: "loraA and loraB differ in their inner length", 12: "a half without its other half",
               13: "a type pair other than (F32, F32) / (F16 loraA, F32 loraB)", 32: "bad argument", 33: "a row-split model", 34: "the base model file cannot be read",
               35: "the base file lacks the tensor, or holds it in another shape or a quantized type", 36: "a base file with an F16 destination matrix",
               37: "the stream is capturing", 38: "staging allocation failed"}


class LoraError(RuntimeError):
    """an adapter was refused; .code is the C ABI's (FALCON_HIP_LORA_E_*, include/falcon-hip.h). No weight was changed."""

    def __init__(self, what, code):
        RuntimeError.__init__(self, "%s refused: %s (%d)" % (what, LORA_ERRORS.get(code, "?"), code))
        self.code = code


def lora_scan(path, hp):
    """host-only check of a 'ggla' adapter against a model's hparams dict (falcon_hip_lora_scan): (r, alpha, pairs it would apply); raises
    LoraError with the reader's code"""
    c_hp = HParams(hp["n_vocab"], hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_layer"], hp["n_ff"], 1 if hp.get("two_norms") else 0, 0, hp["n_layer"])
    r, alpha, n = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = load().falcon_hip_lora_scan(os.fsencode(path), C.byref(c_hp), C.byref(r), C.byref(alpha), C.byref(n))
    if rc != 0:
        raise LoraError("falcon_hip_lora_scan", rc)
    return r.value, alpha.value, n.value


def session_hparams(hp=None, n_ctx=None, wtype=None, path=None, n_falcon_type=None, n_bpe_merges=0, ftype=None):
    """the hparams record of a session file (SessionHParams). path: a GGCC model file (falcon_hip_session_hparams_ggcc, host only);
    else hp (a model's hparams dict) with wtype (the matrices' ggml type) or ftype, n_falcon_type (default 40 with two norms, else 7)
    and n_bpe_merges as the model file's header would hold them. n_ctx: the context's."""
    if n_ctx is None:
        raise ValueError("session_hparams: n_ctx (the context's length) is part of the record")
    out = SessionHParams()
    if path is not None:
        if load().falcon_hip_session_hparams_ggcc(os.fsencode(path), int(n_ctx), C.byref(out)) != 0:
            raise RuntimeError("not a readable GGCC v10 file: %s" % path)
        return out
    if ftype is None:
        ftype = FTYPE_OF_TYPE[wtype]
    if n_falcon_type is None:
        n_falcon_type = 40 if hp.get("two_norms") else 7
    return SessionHParams(hp["n_vocab"], int(n_ctx), hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_layer"], int(n_falcon_type), int(n_bpe_merges), int(ftype))


def _state_size(ctx, n_tokens, logits_all):
    return int(load().falcon_hip_state_size(ctx, int(n_tokens), 1 if logits_all else 0))


def _copy_state(ctx, seq, n_tokens, logits_all):
    n = _state_size(ctx, n_tokens, logits_all)
    if n == 0:
        raise SessionError("falcon_hip_copy_state", 16)
    out = np.empty(n, np.uint8)
    rc = load().falcon_hip_copy_state(ctx, int(seq), int(n_tokens), 1 if logits_all else 0, out.ctypes.data)
    if rc != 0:
        raise SessionError("falcon_hip_copy_state", rc)
    return out


def _set_state(ctx, seq, blob):
    b = np.ascontiguousarray(np.frombuffer(bytes(blob), np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8)
    n = C.c_int(0)
    rc = load().falcon_hip_set_state(ctx, int(seq), b.ctypes.data, b.size, C.byref(n))
    if rc != 0:
        raise SessionError("falcon_hip_set_state", rc)
    return n.value


def _save_session(ctx, seq, path, hparams, tokens, logits_all):
    tok = np.ascontiguousarray(tokens, np.int32)
    rc = load().falcon_hip_session_save(ctx, int(seq), os.fsencode(path), C.byref(hparams), tok.ctypes.data if tok.size else None, tok.size, 1 if logits_all else 0)
    if rc != 0:
        raise SessionError("falcon_hip_session_save", rc)


def _load_session(ctx, seq, path, hparams, capacity):
    tok, n = np.zeros(max(int(capacity), 1), np.int32), C.c_int(0)
    rc = load().falcon_hip_session_load(ctx, int(seq), os.fsencode(path), C.byref(hparams), tok.ctypes.data, int(capacity), C.byref(n))
    if rc != 0:
        raise SessionError("falcon_hip_session_load", rc)
    return tok[:n.value].copy()


def kv_pack(k_cache, v_cache, staging, n_layer, n_head_kv, n_tok, layer_pitch_rows, first_row=0):
    """ggml_hip_kv_pack over DevBufs (stream-ordered): rows [first_row, first_row + n_tok) of every layer of the f32 caches -> staging in the
    session file's layout (K as it lies, then V transposed); returns 0, or 1 when refused (nothing launched)"""
    return load().ggml_hip_kv_pack(k_cache.ptr, v_cache.ptr, staging.ptr, int(n_layer), int(n_head_kv), int(n_tok), int(layer_pitch_rows), int(first_row))


def kv_unpack(k_cache, v_cache, staging, n_layer, n_head_kv, n_tok, layer_pitch_rows, first_row=0):
    """ggml_hip_kv_unpack: the inverse of kv_pack, into those cache rows and no others"""
    return load().ggml_hip_kv_unpack(k_cache.ptr, v_cache.ptr, staging.ptr, int(n_layer), int(n_head_kv), int(n_tok), int(layer_pitch_rows), int(first_row))


_lib = None


def load():
    """dlopen the library and declare the signatures. Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc) first; there is no fallback path")
    L = C.CDLL(LIB_PATH)
    vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
    sig = {
        "ggml_hip_init": (C.c_int, [C.c_int]), "ggml_hip_selftest": (C.c_int, []), "ggml_hip_exp_formula_mismatches": (C.c_int, []), "ggml_hip_debug_force_gemv": (None, [C.c_int]), "ggml_hip_debug_ring_general": (None, [C.c_int]), "ggml_hip_debug_attention_form": (None, [C.c_int]), "ggml_hip_debug_attention_plan": (None, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]), "ggml_hip_debug_mul_mat_plan": (None, [vp, i64, vp]), "ggml_hip_debug_exp_boundary": (C.c_int, [vp, C.c_int]), "ggml_hip_debug_scalar_eval": (C.c_int, [C.c_int, vp, vp, i64, vp]), "ggml_hip_debug_stamps": (None, [C.c_int, vp]), "ggml_hip_device_count": (C.c_int, []), "ggml_hip_stream": (vp, []),
        "ggml_hip_malloc": (vp, [sz]), "ggml_hip_free": (None, [vp]),
        "ggml_hip_memcpy_h2d": (None, [vp, vp, sz]), "ggml_hip_memcpy_d2h": (None, [vp, vp, sz]), "ggml_hip_memcpy_d2d": (None, [vp, vp, sz]),
        "ggml_hip_memset": (None, [vp, C.c_int, sz]), "ggml_hip_synchronize": (None, []),
        "ggml_hip_event_create": (vp, []), "ggml_hip_event_record": (None, [vp]), "ggml_hip_event_elapsed_ms": (C.c_float, [vp, vp]),
        "ggml_hip_profile_begin": (None, []), "ggml_hip_profile_bracket_overhead_us": (C.c_double, []), "ggml_hip_profile_end": (None, [vp, vp, vp]),
        "ggml_hip_event_destroy": (None, [vp]), "ggml_hip_gelu_table_dev": (vp, []), "ggml_hip_exp_table_dev": (vp, []),
        "ggml_hip_weight_upload": (vp, [C.c_int, vp, i64, i64]), "ggml_hip_weight_free": (None, [vp]), "ggml_hip_weight_nbytes": (sz, [vp]),
        "ggml_hip_dequantize_rows": (None, [vp, vp, i64, vp]), "ggml_hip_gemm_sequential": (None, [C.c_int]), "ggml_hip_reference_order": (None, [C.c_int]), "ggml_hip_get_reference_order": (C.c_int, []), "ggml_hip_shim_pool_stats": (None, [vp, vp, vp]),
        "ggml_hip_tensor_split_rows": (None, [vp, C.c_int, i64, vp, vp]), "ggml_hip_weight_upload_rows": (vp, [C.c_int, vp, i64, i64, i64, i64]),
        "ggml_hip_split_comm_create": (vp, [C.c_int, C.c_int, vp]), "ggml_hip_split_configure": (C.c_int, [C.c_int, C.c_int, vp]), "ggml_hip_split_comm_free": (None, [vp]), "ggml_hip_split_comm_agree": (C.c_int, [vp, vp, C.c_size_t]),
        "ggml_hip_mul_mat_q_split": (C.c_int, [vp, vp, vp, i64, i64, vp, i64, vp, vp]),
        "ggml_hip_mul_mat_q_split_local": (C.c_int, [vp, C.c_int, vp, i64, i64, vp, i64, vp, vp]),
        "ggml_hip_split_comm_create_loopback": (vp, [C.c_int]), "ggml_hip_split_comm_rccl_ranks": (C.c_int, [vp]),
        "ggml_hip_mul_mat_q_split_loopback": (C.c_int, [vp, vp, vp, i64, i64, vp, i64, vp, vp]),
        "ggml_hip_quantize_rows": (C.c_int, [C.c_int, vp, i64, i64, vp, vp]), "ggml_hip_weight_quantize": (vp, [C.c_int, vp, i64, i64]),
        "ggml_hip_fp16_to_fp32_row": (None, [vp, vp, i64]),
        "ggml_hip_acts_alloc": (vp, [C.c_int, i64, i64]), "ggml_hip_acts_free": (None, [vp]),
        "ggml_hip_quantize_acts": (None, [vp, vp, i64, i64]), "ggml_hip_acts_export": (None, [vp, i64, vp]),
        "ggml_hip_mul_mat_q": (None, [vp, vp, i64, i64, vp, i64]),
        "ggml_hip_mul_mat_f16": (None, [vp, vp, i64, i64, vp, i64]),
        "ggml_hip_mul_mat_q_acts": (None, [vp, vp, i64, vp, i64, C.c_int, vp, vp]),
        "ggml_hip_layer_norm": (None, [vp, i64, i64, vp, vp, vp]), "ggml_hip_gelu": (None, [vp, vp, i64]),
        "ggml_hip_add3": (None, [vp, vp, vp, vp, i64]), "ggml_hip_rope_table_create": (vp, [C.c_int, C.c_int, C.c_int]),
        "ggml_hip_rope_kv_store": (None, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "ggml_hip_attention": (None, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "ggml_hip_attention_decode": (None, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, i64, vp, vp, C.c_int]),
        "falcon_hip_model_create": (vp, [C.POINTER(HParams)]), "falcon_hip_model_free": (None, [vp]),
        "falcon_hip_model_set_tensor": (C.c_int, [vp, C.c_char_p, C.c_int, vp, i64, i64]),
        "falcon_hip_model_weight_bytes": (sz, [vp]),
        "falcon_hip_model_get_hparams": (None, [vp, vp]),
        "falcon_hip_context_create_seqs": (vp, [vp, C.c_int, C.c_int, C.c_int]), "falcon_hip_context_n_seq": (C.c_int, [vp]),
        "falcon_hip_eval_seqs": (C.c_int, [vp, vp, vp]), "falcon_hip_decode_greedy_seqs": (C.c_int, [vp, vp, vp, C.c_int, vp]),
        "falcon_hip_context_copy_seq": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int]),
        "ggml_hip_sampler_create": (vp, [C.c_int, C.c_int, C.c_int]), "ggml_hip_sampler_free": (None, [vp]),
        "ggml_hip_sampler_set_row": (C.c_int, [vp, C.c_int, C.POINTER(Sampling), vp, C.c_int]), "ggml_hip_sampler_sample": (None, [vp, vp, i64, vp]),
        "ggml_hip_sampler_copy_row": (C.c_int, [vp, C.c_int, vp, C.c_int]), "falcon_hip_context_copy_sampling": (C.c_int, [vp, C.c_int, vp, C.c_int]),
        "falcon_hip_context_set_sampling": (C.c_int, [vp, C.c_int, C.POINTER(Sampling), vp, C.c_int]), "falcon_hip_sample": (C.c_int, [vp, vp]),
        "falcon_hip_decode_sample": (C.c_int, [vp, i32, C.c_int, C.c_int, vp]), "falcon_hip_decode_sample_seqs": (C.c_int, [vp, vp, vp, C.c_int, vp]),
        "falcon_hip_pipeline_unique_id": (C.c_int, [vp]), "falcon_hip_pipeline_create": (vp, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int]),
        "falcon_hip_pipeline_create_local": (vp, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]), "falcon_hip_pipeline_free": (None, [vp]), "falcon_hip_pipeline_rccl_ranks": (C.c_int, [vp]), "falcon_hip_pipeline_transport": (C.c_int, [vp]), "falcon_hip_rccl_selftest": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_int]),
        "falcon_hip_pipeline_set_tokens": (C.c_int, [vp, vp]), "falcon_hip_pipeline_run": (C.c_int, [vp, C.c_int, C.c_int]),
        "falcon_hip_pipeline_run_local": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]), "falcon_hip_pipeline_local_attach_rccl": (C.c_int, [vp, C.c_int]),
        "falcon_hip_pipeline_get_history": (C.c_int, [vp, vp, C.c_int, C.c_int]),
        "falcon_hip_pipeline_schedule": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "falcon_hip_context_create": (vp, [vp, C.c_int, C.c_int, C.c_int]), "falcon_hip_context_free": (None, [vp]),
        "falcon_hip_eval": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int]),
        "falcon_hip_eval_stage": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "falcon_hip_decode_greedy": (C.c_int, [vp, i32, C.c_int, C.c_int, vp]),
        "falcon_hip_eval_token": (C.c_int, [vp, i32, C.c_int]), "falcon_hip_context_last_error": (C.c_int, [vp]), "falcon_hip_context_set_rope_n_ctx": (None, [vp, C.c_int]),
        "falcon_hip_stage_step": (C.c_int, [vp, vp, vp, C.c_int, vp, vp]),
        "falcon_hip_get_logits": (C.POINTER(C.c_float), [vp]),
        "falcon_hip_context_keep_hidden": (None, [vp, C.c_int]), "falcon_hip_get_hidden": (None, [vp, vp]),
        "falcon_hip_vocab_load_ggcc": (vp, [C.c_char_p]), "falcon_hip_vocab_error": (C.c_char_p, [vp]), "falcon_hip_vocab_free": (None, [vp]),
        "falcon_hip_vocab_size": (C.c_int, [vp]), "falcon_hip_vocab_merges": (C.c_int, [vp]),
        "falcon_hip_tokenize": (C.c_int, [vp, C.c_char_p, vp, C.c_int, C.c_int]),
        "falcon_hip_token_to_bytes": (C.c_int, [vp, C.c_int32, C.POINTER(C.c_char_p)]),
        "falcon_hip_token_bos": (C.c_int32, []), "falcon_hip_token_eos": (C.c_int32, []),
        "falcon_hip_context_use_graph": (None, [vp, C.c_int]), "falcon_hip_context_set_fused": (None, [vp, C.c_int]), "falcon_hip_eval_debug_timings": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int]), "falcon_hip_context_sync_error": (C.c_int, [vp]),
        "falcon_hip_context_graph_captures": (C.c_int, [vp]),
        "falcon_hip_model_load_ggcc": (vp, [C.c_char_p, C.c_int, C.c_int, vp]), "falcon_hip_ggcc_scan": (C.c_int, [C.c_char_p, vp, vp, C.c_char_p, C.c_size_t]),
        "falcon_hip_model_quantize": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, vp]),
        "falcon_hip_plan_stages": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, vp]),
        "falcon_hip_perplexity": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, vp]),
        "ggml_hip_score_rows": (None, [vp, i64, C.c_int, C.c_int, vp, vp, vp, vp]),
        "falcon_hip_eval_score": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
        "ggml_hip_logprob_rows": (C.c_int, [vp, i64, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]),
        "falcon_hip_context_set_logprobs": (C.c_int, [vp, C.c_int]), "falcon_hip_get_logprobs": (C.c_int, [vp, vp, vp, vp]),
        "ggml_hip_sampler_set_row_ext": (C.c_int, [vp, C.c_int, C.POINTER(SamplingExt), vp, C.c_int]), "ggml_hip_sampler_get_mu": (C.c_int, [vp, vp]),
        "falcon_hip_context_set_sampling_ext": (C.c_int, [vp, C.c_int, C.POINTER(SamplingExt), vp, C.c_int]), "falcon_hip_context_get_mirostat_mu": (C.c_int, [vp, vp]),
        "ggml_hip_sampler_set_stops": (C.c_int, [vp, C.c_int, C.POINTER(Stops)]), "ggml_hip_sampler_get_stops": (C.c_int, [vp, vp, vp]),
        "falcon_hip_context_set_stops": (C.c_int, [vp, C.c_int, C.POINTER(Stops)]), "falcon_hip_context_get_stops": (C.c_int, [vp, vp, vp]),
        "falcon_hip_context_set_stop_poll": (None, [vp, C.c_int]), "falcon_hip_context_loop_steps": (C.c_int, [vp]),
        "ggml_hip_sampler_set_vocab_bytes": (C.c_int, [vp, vp, vp]), "ggml_hip_sampler_set_stop_text": (C.c_int, [vp, C.c_int, C.POINTER(StopText)]),
        "ggml_hip_sampler_get_stop_text": (C.c_int, [vp, vp]), "falcon_hip_model_set_vocab": (C.c_int, [vp, vp]),
        "falcon_hip_context_set_stop_text": (C.c_int, [vp, C.c_int, C.POINTER(StopText)]), "falcon_hip_context_get_stop_text": (C.c_int, [vp, vp]),
        "ggml_hip_sampler_get_rng": (C.c_int, [vp, C.c_int, vp, vp]), "ggml_hip_sampler_set_rng": (C.c_int, [vp, C.c_int, vp, i32]),
        "ggml_hip_kv_pack": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, i64, i64]), "ggml_hip_kv_unpack": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, i64, i64]),
        "falcon_hip_session_hparams_ggcc": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(SessionHParams)]), "falcon_hip_state_size": (sz, [vp, C.c_int, C.c_int]),
        "falcon_hip_copy_state": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]), "falcon_hip_set_state": (C.c_int, [vp, C.c_int, vp, sz, vp]),
        "falcon_hip_session_save": (C.c_int, [vp, C.c_int, C.c_char_p, C.POINTER(SessionHParams), vp, C.c_int, C.c_int]),
        "falcon_hip_session_load": (C.c_int, [vp, C.c_int, C.c_char_p, C.POINTER(SessionHParams), vp, C.c_int, vp]),
        "falcon_hip_model_apply_lora": (C.c_int, [vp, C.c_char_p, C.c_char_p]), "falcon_hip_lora_scan": (C.c_int, [C.c_char_p, C.POINTER(HParams), vp, vp, vp]),
        "falcon_hip_model_get_tensor": (i64, [vp, C.c_char_p, vp, sz]),
        "ggml_hip_sampler_set_context_stop": (C.c_int, [vp, C.c_int]), "ggml_hip_sampler_resume": (C.c_int, [vp, C.c_int]),
        "ggml_hip_sampler_verify_rows": (C.c_int, [vp, vp, i64, C.c_int, vp, vp, vp]), "ggml_hip_draft_lookup": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "falcon_hip_context_set_spec": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int]), "falcon_hip_context_set_spec_guess": (C.c_int, [vp, vp, C.c_int]),
        "falcon_hip_decode_spec": (C.c_int, [vp, i32, C.c_int, C.c_int, vp, vp]), "falcon_hip_context_get_spec_stats": (C.c_int, [vp, vp, vp, vp]),
        "falcon_hip_swap_plan": (C.c_int, [C.POINTER(SwapCfg), C.c_int, C.c_int, vp, vp]), "falcon_hip_swap_history": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "falcon_hip_context_set_context_stop": (C.c_int, [vp, C.c_int]), "falcon_hip_context_resume": (C.c_int, [vp, C.c_int]),
        "falcon_hip_context_swap": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]),
        "ggml_hip_grammar_create": (vp, [C.c_int, vp, vp, C.POINTER(DfaStruct), C.c_int, vp]), "ggml_hip_grammar_last_error": (C.c_int, []),
        "ggml_hip_grammar_free": (C.c_int, [vp]), "ggml_hip_grammar_get_index": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "ggml_hip_sampler_set_grammar": (C.c_int, [vp, C.c_int, vp, C.c_int]), "ggml_hip_sampler_get_grammar_state": (C.c_int, [vp, vp]),
        "falcon_hip_grammar_create": (vp, [vp, C.POINTER(DfaStruct), C.c_int, vp]), "falcon_hip_grammar_free": (C.c_int, [vp]),
        "falcon_hip_context_set_grammar": (C.c_int, [vp, C.c_int, vp, C.c_int]), "falcon_hip_context_get_grammar_state": (C.c_int, [vp, vp]),
        "ggml_hip_guide_rows": (None, [vp, i64, C.c_int, C.c_int, vp, vp, vp, vp, i64, vp, vp]),
        "falcon_hip_context_set_guidance": (C.c_int, [vp, C.c_int, C.c_int, C.c_float]), "falcon_hip_context_get_guidance": (C.c_int, [vp, vp, vp]),
        "ggml_hip_sampler_set_guidance": (C.c_int, [vp, C.c_int, C.c_int, C.c_float]), "ggml_hip_sampler_get_guidance": (C.c_int, [vp, vp, vp]),
        "ggml_hip_embed_pool_accum": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]), "ggml_hip_embed_pool_finish": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
        "falcon_hip_context_set_embedding": (C.c_int, [vp, C.c_int]), "falcon_hip_get_embeddings": (C.POINTER(C.c_float), [vp]),
        "falcon_hip_embed": (C.c_int, [vp, vp, C.c_int, C.c_int]), "falcon_hip_embedding_pool_reset": (C.c_int, [vp]),
        "falcon_hip_get_embedding_pooled": (C.c_int, [vp, C.c_int, vp]), "falcon_hip_embedding_pool_count": (i64, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)          # AttributeError here = an include/*.h symbol is not exported
        f.restype, f.argtypes = res, args
    _lib = L
    return L


def init(device=0):
    """Initialise the HIP backend on `device`. Aborts (exit 1) when no GPU is visible -- by design."""
    return load().ggml_hip_init(device)


# ------------------------------------------------------------------------------------------- small host helpers
class DevBuf:
    """device allocation + numpy transfer (tests / bench plumbing)"""

    def __init__(self, nbytes=None, host=None):
        L = load()
        if host is not None:
            host = np.ascontiguousarray(host)
            nbytes = host.nbytes
        self.nbytes = int(nbytes)
        self.ptr = L.ggml_hip_malloc(max(self.nbytes, 16))
        if host is not None and self.nbytes:
            L.ggml_hip_memcpy_h2d(self.ptr, host.ctypes.data, self.nbytes)

    def to_host(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        load().ggml_hip_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes)
        return out

    def free(self):
        if self.ptr:
            load().ggml_hip_free(self.ptr)
            self.ptr = None


# enum GGML_HIP_SCALAR_* (include/ggml-hip-ops.h), in its order
SCALAR_FN = {n: i for i, n in enumerate("""expf logf log2f powf f2i_x86 negligible_f negligible_d f2h_bits f2h f32_to_f16_bits f2h_bits_product f2h_product
f32_to_f16_bits_product h2f_bits h2f f16_bits_to_f32 dot4 dot4_c_high dot4_c_low dot4_c_mid dot4z dot2 dot2_c_high dot2_c_low dot2_c_mid dot2z pack16 pk_sub16
mul24""".split())}


def scalar_eval(fn, a, b=None):
    """ggml_hip_debug_scalar_eval: routine fn (a name of SCALAR_FN or its number) of every (a[i], b[i]) as compiled for the device; a, b and the result are
    raw bits in uint32 arrays (b None: a one-argument routine)"""
    L = load()
    a = np.ascontiguousarray(a, np.uint32).ravel()
    ab = DevBuf(host=a)
    bb = None
    if b is not None:
        b = np.ascontiguousarray(b, np.uint32).ravel()
        assert b.shape == a.shape
        bb = DevBuf(host=b)
    ob = DevBuf(a.nbytes)
    try:
        rc = L.ggml_hip_debug_scalar_eval(SCALAR_FN.get(fn, fn), ab.ptr, bb.ptr if bb else None, a.size, ob.ptr)
        if rc != 0:
            raise ValueError(f"ggml_hip_debug_scalar_eval refused fn {fn!r}")
        return ob.to_host(np.uint32, a.shape)
    finally:
        for d in (ab, bb, ob):
            if d:
                d.free()


def quantize_rows(wtype, x, hist=False):
    """x: [nrows, K] f32 -> ggml blocks (uint8 [nrows, K/blck*tsize]) through ggml_hip_quantize_rows; hist=True also
    returns the 16-bin histogram the reference's quantizer prints"""
    L = load()
    x = np.ascontiguousarray(x, np.float32)
    nrows, K = x.shape
    xb = DevBuf(host=x)
    ob = DevBuf(nrows * (K // BLCK[wtype]) * TSIZE[wtype])
    hb = DevBuf(host=np.zeros(16, np.int64)) if hist else None
    rc = L.ggml_hip_quantize_rows(wtype, xb.ptr, K, nrows, ob.ptr, hb.ptr if hb else None)
    if rc != 0:
        raise ValueError("ggml_hip_quantize_rows failed")
    out = ob.to_host(np.uint8, (nrows, (K // BLCK[wtype]) * TSIZE[wtype]))
    h = hb.to_host(np.int64, (16,)) if hb else None
    for b in (xb, ob, hb):
        if b:
            b.free()
    return (out, h) if hist else out


class Weight:
    @classmethod
    def quantize(cls, wtype, x):
        """x: [M, K] f32, quantized and re-tiled on the device (ggml_hip_weight_quantize)"""
        x = np.ascontiguousarray(x, np.float32)
        self = cls.__new__(cls)
        self.type, self.M, self.K = wtype, x.shape[0], x.shape[1]
        xb = DevBuf(host=x)
        self.h = load().ggml_hip_weight_quantize(wtype, xb.ptr, self.K, self.M)
        xb.free()
        if not self.h:
            raise ValueError("ggml_hip_weight_quantize failed")
        return self

    @classmethod
    def upload(cls, wtype, data, K=None, M=None):
        """ggml_hip_weight_upload: ggml block bytes of a quantized type, or -- wtype F16 -- an [M, K] float16 array"""
        if wtype == F16:
            data = np.ascontiguousarray(data, np.float16)
            M, K = data.shape
            return cls(F16, data.view(np.uint8), K, M)
        return cls(wtype, data, K, M)

    def __init__(self, wtype, blocks, K, M):
        blocks = np.ascontiguousarray(blocks).view(np.uint8) if wtype == F16 else np.ascontiguousarray(blocks, np.uint8)
        assert blocks.size == (2 * M * K if wtype == F16 else M * (K // BLCK[wtype]) * TSIZE[wtype])
        self.type, self.K, self.M = wtype, K, M
        self.h = load().ggml_hip_weight_upload(wtype, blocks.ctypes.data, K, M)

    def dequantize(self, rows=None):
        L = load()
        n = self.M if rows is None else len(rows)
        out = DevBuf(n * self.K * 4)
        rb = DevBuf(host=np.asarray(rows, np.int32)) if rows is not None else None
        L.ggml_hip_dequantize_rows(self.h, rb.ptr if rb else None, n, out.ptr)
        y = out.to_host(np.float32, (n, self.K))
        out.free()
        if rb:
            rb.free()
        return y

    def mul_mat(self, x):
        """x: [N, K] f32 -> [N, M] f32 through ggml_hip_mul_mat_q"""
        L = load()
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.K)
        N = x.shape[0]
        xb, yb = DevBuf(host=x), DevBuf(N * self.M * 4)
        L.ggml_hip_mul_mat_q(self.h, xb.ptr, self.K, N, yb.ptr, self.M)
        y = yb.to_host(np.float32, (N, self.M))
        xb.free()
        yb.free()
        return y

    def mul_mat_f16(self, x, ldx=None):
        """x: [N, K] f32 (rows ldx >= K floats apart on the device) -> [N, M] f32 through ggml_hip_mul_mat_f16: the reference's f64 row sums"""
        L = load()
        assert self.type == F16
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.K)
        N = x.shape[0]
        ldx = self.K if ldx is None else int(ldx)
        assert ldx >= self.K
        if ldx > self.K:
            padded = np.full((N, ldx), np.float32(np.nan), np.float32)      # (what lies between the rows must not matter)
            padded[:, :self.K] = x
            x = padded
        xb, yb = DevBuf(host=x), DevBuf(N * self.M * 4)
        L.ggml_hip_mul_mat_f16(self.h, xb.ptr, ldx, N, yb.ptr, self.M)
        y = yb.to_host(np.float32, (N, self.M))
        xb.free()
        yb.free()
        return y

    def nbytes(self):
        return load().ggml_hip_weight_nbytes(self.h)

    def free(self):
        if self.h:
            load().ggml_hip_weight_free(self.h)
            self.h = None


def ggcc_scan(path):
    """host-only parse of a GGCC v10 file: (hparams dict, ftype, [(name, ggml type, ne0, ne1, offset, bytes)])"""
    L = load()
    hp, ft = HParams(), C.c_int(0)
    buf = C.create_string_buffer(1 << 20)
    n = L.falcon_hip_ggcc_scan(os.fsencode(path), C.byref(hp), C.byref(ft), buf, len(buf))
    if n < 0:
        raise RuntimeError("not a readable GGCC v10 file: %s" % path)
    rows = []
    for line in buf.value.decode().splitlines():
        name, t, ne0, ne1, off, sz = line.rsplit(" ", 5)
        rows.append((name, int(t), int(ne0), int(ne1), int(off), int(sz)))
    assert len(rows) == n
    d = dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head, n_head_kv=hp.n_head_kv, n_layer=hp.n_layer, n_ff=hp.n_ff, two_norms=bool(hp.two_norms))
    return d, ft.value, rows


def plan_stages(path, n_stages, n_ctx=2048, n_batch=1, n_streams=1, vram_per_gpu=0):
    """host-only: ([(layer_begin, layer_end)], [device bytes per stage], fits) for a layer pipeline over a GGCC file"""
    lb, le = (C.c_int * n_stages)(), (C.c_int * n_stages)()
    sb = (C.c_size_t * n_stages)()
    rc = load().falcon_hip_plan_stages(os.fsencode(path), n_stages, n_ctx, n_batch, n_streams, vram_per_gpu, lb, le, sb)
    if rc < 0:
        raise RuntimeError("falcon_hip_plan_stages(%s, %d) failed" % (path, n_stages))
    return [(lb[i], le[i]) for i in range(n_stages)], [int(sb[i]) for i in range(n_stages)], rc == 0


def quantize_model(path_in, path_out, ftype, quantize_output_tensor=True, allow_requantize=False):
    """falcon_model_quantize on the device (falcon_hip_model_quantize); returns the 16-bin histogram"""
    hist = np.zeros(16, np.int64)
    rc = load().falcon_hip_model_quantize(os.fsencode(path_in), os.fsencode(path_out), int(ftype), int(bool(quantize_output_tensor)),
                                          int(bool(allow_requantize)), hist.ctypes.data)
    if rc != 0:
        raise RuntimeError("falcon_hip_model_quantize(%s, ftype %d) failed" % (path_in, ftype))
    return hist


def quantize_acts(act_type, x):
    """x: [N, K] f32 -> ggml block bytes [N, K/blck*tsize] produced on the device"""
    L = load()
    x = np.ascontiguousarray(x, np.float32)
    N, K = x.shape
    a = L.ggml_hip_acts_alloc(act_type, K, N)
    xb = DevBuf(host=x)
    L.ggml_hip_quantize_acts(a, xb.ptr, K, N)
    nbytes = N * (K // BLCK[act_type]) * TSIZE[act_type]
    ob = DevBuf(nbytes)
    L.ggml_hip_acts_export(a, N, ob.ptr)
    out = ob.to_host(np.uint8, (N, nbytes // N))
    for b in (xb, ob):
        b.free()
    L.ggml_hip_acts_free(a)
    return out


TENSOR_NAMES_7B = dict(ln_w="input_layernorm.weight", ln_b="input_layernorm.bias")
TENSOR_NAMES_40B = dict(ln_w="ln_mlp.weight", ln_b="ln_mlp.bias", ln2_w="ln_attn.weight", ln2_b="ln_attn.bias")


class FalconModel:
    """weights dict (tests/synth.py::make_model layout) -> device-resident model + context"""

    def __init__(self, weights, n_ctx, n_batch, rope_n_ctx=0, layer_begin=0, layer_end=0):
        L = load()
        hp = weights["hparams"]
        self.hp = hp
        wt = weights["wtype"]
        E, H, HKV, FF, V = hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_ff"], hp["n_vocab"]
        self.c_hp = HParams(V, E, H, HKV, hp["n_layer"], FF, 1 if hp.get("two_norms") else 0, layer_begin, layer_end or hp["n_layer"])
        self.m = L.falcon_hip_model_create(C.byref(self.c_hp))

        def put(name, t, arr, ne0, ne1):
            arr = np.ascontiguousarray(arr)
            L.falcon_hip_model_set_tensor(self.m, name.encode(), t, arr.ctypes.data, ne0, ne1)

        put("transformer.word_embeddings.weight", wt, weights["tok_emb"], E, V)
        put("lm_head.weight", wt, weights["lm_head"], E, V)
        put("transformer.ln_f.weight", F32, weights["out_norm_w"], E, 1)
        put("transformer.ln_f.bias", F32, weights["out_norm_b"], E, 1)
        names = TENSOR_NAMES_40B if hp.get("two_norms") else TENSOR_NAMES_7B
        for i, lw in enumerate(weights["layers"]):
            if lw is None:
                continue
            p = f"transformer.h.{i}."
            put(p + "self_attention.query_key_value.weight", wt, lw["qkv"], E, (H + 2 * HKV) * 64)
            put(p + "self_attention.dense.weight", wt, lw["wo"], E, E)
            put(p + "mlp.dense_h_to_4h.weight", wt, lw["up"], E, FF)
            put(p + "mlp.dense_4h_to_h.weight", wt, lw["down"], FF, E)
            for k, leaf in names.items():
                put(p + leaf, F32, lw[k], E, 1)
        self.ctx = L.falcon_hip_context_create(self.m, n_ctx, n_batch, rope_n_ctx)
        self.n_local = (layer_end or hp["n_layer"]) - layer_begin
        self.n_ctx, self.path, self.wtype = n_ctx, None, wt
        self.n_batch = n_batch

    @classmethod
    def from_ggcc(cls, path, n_ctx, n_batch, rope_n_ctx=0, layer_begin=0, layer_end=0):
        """load a GGCC v10 model file (the reference's format) through falcon_hip_model_load_ggcc"""
        L = load()
        self = cls.__new__(cls)
        self.c_hp = HParams()
        self.m = L.falcon_hip_model_load_ggcc(os.fsencode(path), layer_begin, layer_end, C.byref(self.c_hp))
        if not self.m:
            raise RuntimeError("cannot load %s" % path)
        self.hp = dict(n_vocab=self.c_hp.n_vocab, n_embd=self.c_hp.n_embd, n_head=self.c_hp.n_head, n_head_kv=self.c_hp.n_head_kv,
                       n_layer=self.c_hp.n_layer, n_ff=self.c_hp.n_ff, two_norms=bool(self.c_hp.two_norms))
        self.ctx = L.falcon_hip_context_create(self.m, n_ctx, n_batch, rope_n_ctx)
        self.n_local = self.c_hp.layer_end - self.c_hp.layer_begin
        self.n_ctx, self.path, self.wtype = n_ctx, path, None
        self.n_batch = n_batch
        return self

    def new_context(self, n_ctx, n_batch=1, rope_n_ctx=0):
        """another context (own KV cache / scratch) over the same device weights: one per concurrent decode stream"""
        return load().falcon_hip_context_create(self.m, n_ctx, n_batch, rope_n_ctx)

    def eval(self, tokens, n_past, logits_all=True, want_hidden=False):
        L = load()
        tok = np.ascontiguousarray(tokens, np.int32)
        N = tok.size
        if want_hidden:
            L.falcon_hip_context_keep_hidden(self.ctx, 1)
        rc = L.falcon_hip_eval(self.ctx, tok.ctypes.data, N, n_past, 1 if logits_all else 0)
        if rc != 0:
            raise RuntimeError("falcon_hip_eval failed (%d)" % rc)
        rows = N if logits_all else 1
        lg = np.ctypeslib.as_array(L.falcon_hip_get_logits(self.ctx), (rows, self.hp["n_vocab"])).copy()
        if want_hidden:
            hid = np.empty((self.n_local + 1, N, self.hp["n_embd"]), np.float32)
            L.falcon_hip_get_hidden(self.ctx, hid.ctypes.data)
            L.falcon_hip_context_keep_hidden(self.ctx, 0)
            return lg, hid
        return lg

    def score(self, tokens, n_past, targets):
        """falcon_hip_eval_score: evaluates tokens at n_past like eval(), the logits stay on the device; returns float32 [N], entry r
        the reference's soft-max probability of targets[r] in row r (falcon_perplexity.cpp:12-27), NaN where targets[r] < 0.
        ValueError (nothing evaluated) for a target >= n_vocab."""
        tok = np.ascontiguousarray(tokens, np.int32)
        tgt = np.ascontiguousarray(targets, np.int32)
        if tgt.shape != tok.shape:
            raise ValueError("score: one target per token (-1: do not score the row)")
        out = np.full(tok.size, np.nan, np.float32)
        rc = load().falcon_hip_eval_score(self.ctx, tok.ctypes.data, tok.size, int(n_past), tgt.ctypes.data, out.ctypes.data)
        if rc == 2 and tgt.size and int(tgt.max()) >= self.hp["n_vocab"]:
            raise ValueError("score: target id %d is outside the vocabulary (%d)" % (int(tgt.max()), self.hp["n_vocab"]))
        if rc != 0:
            raise RuntimeError("falcon_hip_eval_score failed (%d)" % rc)
        return out

    # ---- embeddings (falcon_hip_context_set_embedding, include/falcon-hip.h)
    def set_embedding(self, last=True, pool=False):
        """keep the ln_f row of every eval's last token (last: the reference's params.embedding) and / or sum the rows of all tokens
        for pooled() (pool); both False switches it off. ValueError when refused (lock-step context, pipeline stage, row-split model)"""
        if load().falcon_hip_context_set_embedding(self.ctx, (EMBED_LAST if last else 0) | (EMBED_POOL if pool else 0)) != 0:
            raise ValueError("falcon_hip_context_set_embedding refused")

    def embeddings(self):
        """falcon_hip_get_embeddings: float32 [n_embd], the ln_f row of the last evaluated token; None while off or before an eval"""
        p = load().falcon_hip_get_embeddings(self.ctx)
        return np.ctypeslib.as_array(p, (self.hp["n_embd"],)).copy() if p else None

    def embed_tokens(self, tokens, n_past):
        """falcon_hip_embed: eval() that ends after ln_f (no lm_head, no logits)"""
        tok = np.ascontiguousarray(tokens, np.int32)
        rc = load().falcon_hip_embed(self.ctx, tok.ctypes.data, tok.size, int(n_past))
        if rc != 0:
            raise RuntimeError("falcon_hip_embed failed (%d)" % rc)

    def pool_reset(self):
        load().falcon_hip_embedding_pool_reset(self.ctx)

    def pool_count(self):
        return int(load().falcon_hip_embedding_pool_count(self.ctx))

    def pooled(self, normalize=True):
        """falcon_hip_get_embedding_pooled: float32 [n_embd], the mean of the rows pooled since pool_reset(), or that mean at unit length;
        ValueError when nothing was pooled, the mean is the zero vector or pooling is off"""
        out = np.empty(self.hp["n_embd"], np.float32)
        rc = load().falcon_hip_get_embedding_pooled(self.ctx, 1 if normalize else 0, out.ctypes.data)
        if rc != 0:
            raise ValueError("falcon_hip_get_embedding_pooled refused (%d)" % rc)
        return out

    def embed(self, tokens, pool="mean", normalize=True):
        """a text's vector: the tokens from an empty context in chunks of n_batch through falcon_hip_embed; pool "mean": the mean over
        every token's ln_f row (at unit length with normalize), "last": the last token's row (the reference's embedding; normalize is
        applied on the host in f64). Leaves the embedding mode it needed set."""
        if pool not in ("mean", "last"):
            raise ValueError('embed: pool is "mean" or "last"')
        tok = np.ascontiguousarray(tokens, np.int32).ravel()
        if not 1 <= tok.size <= self.n_ctx:
            raise ValueError("embed: %d tokens, the context holds 1..%d" % (tok.size, self.n_ctx))
        self.set_embedding(last=True, pool=pool == "mean")
        self.pool_reset()
        for i in range(0, tok.size, self.n_batch):
            self.embed_tokens(tok[i:i + self.n_batch], i)
        if pool == "mean":
            return self.pooled(normalize)
        v = self.embeddings()
        if normalize:
            n = np.sqrt((v.astype(np.float64) ** 2).sum())
            if n == 0:
                raise ValueError("embed: the row is the zero vector")
            v = (v.astype(np.float64) / n).astype(np.float32)
        return v

    def eval_token(self, token, n_past):
        """one token through the captured graph, no host round trip; logits() fetches the row"""
        rc = load().falcon_hip_eval_token(self.ctx, int(token), int(n_past))
        if rc != 0:
            raise RuntimeError("falcon_hip_eval_token failed (%d)" % rc)

    def logits(self):
        n = self.hp["n_vocab"]
        return np.ctypeslib.as_array(load().falcon_hip_get_logits(self.ctx), shape=(n,)).copy()

    def set_rope_n_ctx(self, n):
        load().falcon_hip_context_set_rope_n_ctx(self.ctx, int(n))

    def decode_greedy(self, first_token, n_past, n_steps, use_graph=False):
        L = load()
        L.falcon_hip_context_use_graph(self.ctx, 1 if use_graph else 0)
        out = np.zeros(n_steps, np.int32)
        rc = L.falcon_hip_decode_greedy(self.ctx, int(first_token), n_past, n_steps, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("falcon_hip_decode_greedy failed (%d)" % rc)
        self._lp_steps = 0
        return out

    def set_sampling(self, params, history=()):
        """falcon_hip_context_set_sampling: params a Sampling (see sampling()), history the tokens so far (the window's source);
        raises ValueError when refused"""
        return _set_sampling(self.ctx, 0, params, history)

    def set_sampling_ext(self, params, history=()):
        """falcon_hip_context_set_sampling_ext: params a SamplingExt (see sampling_ext()) -- tail-free, typical and mirostat 1 / 2
        honoured; raises ValueError when refused"""
        return _set_sampling_ext(self.ctx, 0, params, history)

    def mirostat_mu(self):
        """falcon_hip_context_get_mirostat_mu: the sequence's mirostat state (2 * tau when set, moved by every draw)"""
        return float(_mirostat_mu(self.ctx, 1)[0])

    def sample(self):
        """falcon_hip_sample: one draw from the last eval's last logits row (it enters the window); -1 when the row's stops had ended it"""
        out = np.zeros(1, np.int32)
        if load().falcon_hip_sample(self.ctx, out.ctypes.data) != 0:
            raise RuntimeError("falcon_hip_sample failed")
        self._lp_steps = 1
        return int(out[0])

    def decode_sample(self, first_token, n_past, n_steps, use_graph=False):
        """falcon_hip_decode_sample: decode_greedy with the sampler chain set by set_sampling"""
        L = load()
        L.falcon_hip_context_use_graph(self.ctx, 1 if use_graph else 0)
        out = np.zeros(n_steps, np.int32)
        rc = L.falcon_hip_decode_sample(self.ctx, int(first_token), n_past, n_steps, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("falcon_hip_decode_sample failed (%d)" % rc)
        self._lp_steps = n_steps
        return out

    def set_spec(self, n_draft, source=SPEC_LOOKUP, ngram=(1, 3), history=()):
        """falcon_hip_context_set_spec: draft-and-verify decode with n_draft (1..15; 0: off) drafts per pass. SPEC_LOOKUP: prompt lookup
        with n-grams ngram[0]..ngram[1] over history = every token of the sequence so far, the last one the token decode_spec is called
        with; SPEC_GIVEN: the guess of set_spec_guess. Resets the counters of spec_stats; raises ValueError when refused"""
        h = np.ascontiguousarray(history, np.int32)
        if load().falcon_hip_context_set_spec(self.ctx, int(n_draft), int(source), int(ngram[0]), int(ngram[1]), h.ctypes.data if h.size else None, int(h.size)) != 0:
            raise ValueError("falcon_hip_context_set_spec refused")

    def set_spec_guess(self, tokens):
        """falcon_hip_context_set_spec_guess: tokens[i] guesses draw number i from now on (-1: no guess); raises ValueError when refused"""
        t = np.ascontiguousarray(tokens, np.int32)
        if load().falcon_hip_context_set_spec_guess(self.ctx, t.ctypes.data if t.size else None, int(t.size)) != 0:
            raise ValueError("falcon_hip_context_set_spec_guess refused")

    def decode_spec(self, first_token, n_past, n_tokens, use_graph=False):
        """falcon_hip_decode_spec: decode_sample's tokens, several per pass over the weights where the drafts are right. Returns the
        draws (int32 [n_drawn]: fewer than n_tokens when the sequence's stops ended it)"""
        L = load()
        L.falcon_hip_context_use_graph(self.ctx, 1 if use_graph else 0)
        out = np.full(n_tokens, -1, np.int32)
        n = C.c_int(0)
        rc = L.falcon_hip_decode_spec(self.ctx, int(first_token), int(n_past), int(n_tokens), out.ctypes.data, C.addressof(n))
        if rc != 0:
            raise RuntimeError("falcon_hip_decode_spec failed (%d)" % rc)
        self._lp_steps = 0
        assert (out[n.value:] == -1).all() and (out[:n.value] >= 0).all()
        return out[:n.value]

    def spec_stats(self):
        """falcon_hip_context_get_spec_stats: (passes that drew, draws, hist [16]: hist[d - 1] = passes that made d draws) since set_spec"""
        p, d, h = C.c_int64(0), C.c_int64(0), np.zeros(16, np.int64)
        if load().falcon_hip_context_get_spec_stats(self.ctx, C.addressof(p), C.addressof(d), h.ctypes.data) != 0:
            raise ValueError("falcon_hip_context_get_spec_stats refused")
        return int(p.value), int(d.value), h

    def set_logprobs(self, n_top):
        """falcon_hip_context_set_logprobs: -1 off (default), 0 the chosen token's probability only, 1..32 also the n_top most likely
        ids; while on, sample() and decode_sample() record them on the device (see logprobs()); raises ValueError when refused"""
        _set_logprobs(self, n_top)

    def logprobs(self):
        """the records of the last sample() / decode_sample(): (prob float32 [steps], top_ids int32 [steps][n_top], top_probs float32
        [steps][n_top]) -- soft-max probabilities of the raw logits rows (what score() gives for those tokens), not logarithms"""
        p, i, q = _get_logprobs(self, 1)
        return p[:, 0], i[:, 0], q[:, 0]

    def set_stops(self, st):
        """falcon_hip_context_set_stops: a Stops (see stops()) or None (off); the drawn count, tail and reason start afresh; raises
        ValueError when refused"""
        _set_stops(self.ctx, 0, st)

    def stop_state(self):
        """falcon_hip_context_get_stops: (tokens drawn since the stops were set, reason: the matched sequence's index, STOP_BUDGET, or
        STOP_RUNNING while running or off)"""
        n, r = _stop_state(self.ctx, 1)
        return int(n[0]), int(r[0])

    def set_vocab(self, vocab):
        """falcon_hip_model_set_vocab: the bytes of every token of a Vocab go to the device, once for all contexts of the model (stop
        strings match on them); raises ValueError when refused (a vocabulary of another size, bytes beyond 16 MB)"""
        if load().falcon_hip_model_set_vocab(self.m, vocab.h) != 0:
            raise ValueError("falcon_hip_model_set_vocab refused this vocabulary")

    def set_stop_text(self, st):
        """falcon_hip_context_set_stop_text: a StopText (see stop_text()) or None (off); drawn count, reason, id tail, byte ring and
        cut_bytes start afresh; raises ValueError when refused"""
        _set_stop_text(self.ctx, 0, st)

    def stop_text_state(self):
        """falcon_hip_context_get_stop_text: cut_bytes -- bytes from the first byte of the matched stop string to the end of the drawn
        text (0 while the sequence has not ended by text)"""
        return int(_stop_text_state(self.ctx, 1)[0])

    def grammar(self, d, eos_id=None):
        """falcon_hip_grammar_create: a Grammar of the Dfa d (regex_dfa, choice_dfa, dfa) over the vocabulary of set_vocab; eos_id: the token
        allowed exactly in accepting states (None: none). GrammarError when refused. Free it with Grammar.free() once no sequence holds it"""
        return _make_model_grammar(self.m, self.hp["n_vocab"], d, eos_id)

    def set_grammar(self, gr, state=None):
        """falcon_hip_context_set_grammar: the sequence draws only what gr allows from `state` on (None: its start state); gr None: off.
        ValueError when refused (a state out of range, draft-and-verify decode on)"""
        _set_grammar(self.ctx, 0, gr, state)

    @property
    def grammar_state(self):
        """falcon_hip_context_get_grammar_state: the automaton's state after the tokens drawn so far, -1 without a grammar"""
        return int(_grammar_state(self.ctx, 1)[0])

    def set_context_stop(self, on):
        """falcon_hip_context_set_context_stop: the sequence ends with STOP_CONTEXT at the draw that fills its cache, and decode_sample
        takes any n_steps (-1 past the end)"""
        _set_context_stop(self.ctx, on)

    def resume(self):
        """falcon_hip_context_resume: a sequence that ended with STOP_CONTEXT runs again, nothing else changed; ValueError otherwise"""
        _resume(self.ctx, 0)

    def context_swap(self, n_past_new, regen, n_batch=512):
        """falcon_hip_context_swap: evaluates regen at positions n_past_new .. in chunks of n_batch and resumes the sequence (see
        swap_plan, generate_swap); ValueError when refused"""
        _context_swap(self.ctx, 0, n_past_new, regen, n_batch)

    def set_stop_poll(self, every_steps):
        """steps between two looks at the stop states inside a sampled loop (falcon_hip_context_set_stop_poll)"""
        load().falcon_hip_context_set_stop_poll(self.ctx, int(every_steps))

    def loop_steps(self):
        """steps the last decode loop launched (falcon_hip_context_loop_steps)"""
        return load().falcon_hip_context_loop_steps(self.ctx)

    def perplexity(self, tokens, n_ctx, n_batch):
        """(summed NLL, scored tokens) of the reference's perplexity loop over a token stream"""
        tok = np.ascontiguousarray(tokens, np.int32)
        nll = C.c_double(0.0)
        n = load().falcon_hip_perplexity(self.ctx, tok.ctypes.data, tok.size, n_ctx, n_batch, C.byref(nll))
        return nll.value, n

    def session_hparams(self, n_ctx=None):
        """the record this model's session files carry for a context of n_ctx positions (default: its own context's): from the GGCC
        file it was loaded from, else as ggcc_writer would write its header (no BPE merges)"""
        n_ctx = self.n_ctx if n_ctx is None else n_ctx
        return session_hparams(path=self.path, n_ctx=n_ctx) if self.path else session_hparams(self.hp, n_ctx, wtype=self.wtype)

    def save_session(self, path, tokens, hparams=None, logits_all=False):
        """falcon_hip_session_save: the context's state after `tokens` (generator, last logits, K / V rows [0, len(tokens))) as a session
        file of the reference (llama_save_session_file's bytes). Raises SessionError when refused."""
        _save_session(self.ctx, 0, path, hparams or self.session_hparams(), tokens, logits_all)

    def load_session(self, path, hparams=None):
        """falcon_hip_session_load: restores the file's state into the context and returns its tokens (int32). The penalty window, stops
        and mirostat's mu are not in the file: set_sampling(history=tokens) re-creates them and keeps the loaded generator. Raises
        SessionError (nothing changed) when refused."""
        return _load_session(self.ctx, 0, path, hparams or self.session_hparams(), self.n_ctx)

    def copy_state(self, n_tokens, logits_all=False):
        """falcon_hip_copy_state: the state blob (uint8 array) of falcon_copy_state_data"""
        return _copy_state(self.ctx, 0, n_tokens, logits_all)

    def set_state(self, blob):
        """falcon_hip_set_state: restores a blob; returns the rows it held"""
        return _set_state(self.ctx, 0, blob)

    def apply_lora(self, path, base=None):
        """falcon_hip_model_apply_lora: merges the 'ggla' adapter at path into the device-resident matrices with the reference's bits
        (llama_apply_lora_from_file); base: a GGCC model file whose F16 / F32 tensors stand in for the quantized rows (--lora-base).
        Every context of the model sees the patched weights from its next call on. Raises LoraError (nothing changed) when refused."""
        rc = load().falcon_hip_model_apply_lora(self.m, os.fsencode(path), os.fsencode(base) if base is not None else None)
        if rc != 0:
            raise LoraError("falcon_hip_model_apply_lora", rc)

    def get_tensor(self, name):
        """falcon_hip_model_get_tensor: the bytes (uint8 array) of a matrix this model holds, in ggml's block layout (F16: the fp16 rows)"""
        L = load()
        n = L.falcon_hip_model_get_tensor(self.m, name.encode(), None, 0)
        if n < 0:
            raise KeyError(name)
        out = np.empty(n, np.uint8)
        if L.falcon_hip_model_get_tensor(self.m, name.encode(), out.ctypes.data, out.size) != n:
            raise RuntimeError("falcon_hip_model_get_tensor(%s) failed" % name)
        return out

    def set_fused(self, mode):
        """0 = op list, 1 = three launches per block, 2 (True) = two (default), 3 = one launch per block, 5 = two launches, ring form forced (4, the removed persistent engine, selects 2)"""
        load().falcon_hip_context_set_fused(self.ctx, 2 if mode is True else int(mode))

    def sync_error(self):
        return load().falcon_hip_context_sync_error(self.ctx)

    def weight_bytes(self):
        return load().falcon_hip_model_weight_bytes(self.m)

    def free(self):
        L = load()
        L.falcon_hip_context_free(self.ctx)
        L.falcon_hip_model_free(self.m)


class SeqContext:
    """n_seq independent sequences of one model advancing in lock step (falcon_hip_context_create_seqs): eval takes one
    token per sequence and returns one logits row per sequence"""

    def __init__(self, model, n_ctx, n_seq, rope_n_ctx=0):
        self.model, self.n_seq, self.n_ctx = model, n_seq, n_ctx
        self.ctx = load().falcon_hip_context_create_seqs(model.m, n_ctx, n_seq, rope_n_ctx)
        if not self.ctx:
            raise RuntimeError("falcon_hip_context_create_seqs failed")

    def eval(self, tokens, n_past):
        """n_past an int: every sequence at that position (falcon_hip_eval_stage); a sequence of n_seq ints: sequence t at
        n_past[t] (falcon_hip_eval_seqs, a ragged step)"""
        L = load()
        tok = np.ascontiguousarray(tokens, np.int32)
        assert tok.size == self.n_seq
        if isinstance(n_past, (int, np.integer)):
            rc = L.falcon_hip_eval_stage(self.ctx, tok.ctypes.data, None, tok.size, int(n_past), 1, None)
            what = "falcon_hip_eval_stage"
        else:
            pos = np.ascontiguousarray(n_past, np.int32)
            assert pos.size == self.n_seq
            rc = L.falcon_hip_eval_seqs(self.ctx, tok.ctypes.data, pos.ctypes.data)
            what = "falcon_hip_eval_seqs"
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (what, rc))
        return np.ctypeslib.as_array(L.falcon_hip_get_logits(self.ctx), (self.n_seq, self.model.hp["n_vocab"])).copy()

    def decode_greedy(self, first_tokens, n_past, n_steps, use_graph=False):
        """falcon_hip_decode_greedy_seqs: sequence t evaluates first_tokens[t] at n_past[t], then n_steps - 1 argmax tokens;
        returns the sampled ids [n_steps][n_seq]"""
        L = load()
        tok = np.ascontiguousarray(first_tokens, np.int32)
        pos = np.ascontiguousarray(n_past, np.int32)
        assert tok.size == self.n_seq and pos.size == self.n_seq
        L.falcon_hip_context_use_graph(self.ctx, 1 if use_graph else 0)
        out = np.zeros((n_steps, self.n_seq), np.int32)
        rc = L.falcon_hip_decode_greedy_seqs(self.ctx, tok.ctypes.data, pos.ctypes.data, int(n_steps), out.ctypes.data)
        if rc != 0:
            raise RuntimeError("falcon_hip_decode_greedy_seqs failed (%d)" % rc)
        self._lp_steps = 0
        return out

    def set_sampling(self, seq, params, history=()):
        """falcon_hip_context_set_sampling for sequence seq (re-seeds it: how a prompt entering a slot gets its own stream)"""
        return _set_sampling(self.ctx, seq, params, history)

    def set_sampling_ext(self, seq, params, history=()):
        """falcon_hip_context_set_sampling_ext for sequence seq: a SamplingExt (tail-free, typical, mirostat 1 / 2 honoured)"""
        return _set_sampling_ext(self.ctx, seq, params, history)

    def mirostat_mu(self):
        """float32 [n_seq]: every sequence's mirostat state (falcon_hip_context_get_mirostat_mu)"""
        return _mirostat_mu(self.ctx, self.n_seq)

    def sample(self):
        """falcon_hip_sample: one draw per sequence from the last eval's rows; returns [n_seq] (-1 for a sequence its stops had ended)"""
        out = np.zeros(self.n_seq, np.int32)
        if load().falcon_hip_sample(self.ctx, out.ctypes.data) != 0:
            raise RuntimeError("falcon_hip_sample failed")
        self._lp_steps = 1
        return out

    def decode_sample(self, first_tokens, n_past, n_steps, use_graph=False):
        """falcon_hip_decode_sample_seqs: decode_greedy with every sequence's sampler chain; returns [n_steps][n_seq]"""
        L = load()
        tok = np.ascontiguousarray(first_tokens, np.int32)
        pos = np.ascontiguousarray(n_past, np.int32)
        assert tok.size == self.n_seq and pos.size == self.n_seq
        L.falcon_hip_context_use_graph(self.ctx, 1 if use_graph else 0)
        out = np.zeros((n_steps, self.n_seq), np.int32)
        rc = L.falcon_hip_decode_sample_seqs(self.ctx, tok.ctypes.data, pos.ctypes.data, int(n_steps), out.ctypes.data)
        if rc != 0:
            raise RuntimeError("falcon_hip_decode_sample_seqs failed (%d)" % rc)
        self._lp_steps = int(n_steps)
        return out

    def set_logprobs(self, n_top):
        """falcon_hip_context_set_logprobs for every sequence of this context (see FalconModel.set_logprobs)"""
        _set_logprobs(self, n_top)

    def logprobs(self):
        """the records of the last sample() / decode_sample(): (prob [steps][n_seq], top_ids [steps][n_seq][n_top], top_probs likewise)"""
        return _get_logprobs(self, self.n_seq)

    def set_stops(self, seq, st):
        """falcon_hip_context_set_stops for sequence seq: a Stops or None (see FalconModel.set_stops)"""
        _set_stops(self.ctx, seq, st)

    def stop_state(self):
        """(n_drawn int32 [n_seq], reason int32 [n_seq]) of falcon_hip_context_get_stops"""
        return _stop_state(self.ctx, self.n_seq)

    def set_stop_text(self, seq, st):
        """falcon_hip_context_set_stop_text for sequence seq: a StopText or None (see FalconModel.set_stop_text)"""
        _set_stop_text(self.ctx, seq, st)

    def set_grammar(self, seq, gr, state=None):
        """falcon_hip_context_set_grammar for sequence seq: a Grammar of the model (FalconModel.grammar) or None, from `state` (None: its start)"""
        _set_grammar(self.ctx, seq, gr, state)

    @property
    def grammar_state(self):
        """int32 [n_seq] of falcon_hip_context_get_grammar_state: -1 for sequences without a grammar"""
        return _grammar_state(self.ctx, self.n_seq)

    def stop_text_state(self):
        """cut_bytes int32 [n_seq] of falcon_hip_context_get_stop_text"""
        return _stop_text_state(self.ctx, self.n_seq)

    def set_guidance(self, seq, guide_seq, scale=1.5):
        """falcon_hip_context_set_guidance: sequence seq draws from the classifier-free-guidance mix of its row and guide_seq's (the slot that holds the
        negative prompt), and guide_seq is fed seq's tokens; guide_seq None or -1 takes seq's pair apart. ValueError when refused (nothing changed)"""
        if load().falcon_hip_context_set_guidance(self.ctx, int(seq), -1 if guide_seq is None else int(guide_seq), float(scale)) != 0:
            raise ValueError("falcon_hip_context_set_guidance refused sequence %d guided by %s at scale %r" % (int(seq), guide_seq, scale))

    def guidance(self):
        """(guide_seq int32 [n_seq], scale float32 [n_seq]) of falcon_hip_context_get_guidance: -1 and 1 for a sequence without a guide"""
        gs, sc = np.zeros(self.n_seq, np.int32), np.zeros(self.n_seq, np.float32)
        if load().falcon_hip_context_get_guidance(self.ctx, gs.ctypes.data, sc.ctypes.data) != 0:
            raise RuntimeError("falcon_hip_context_get_guidance failed")
        return gs, sc

    def set_context_stop(self, on):
        """falcon_hip_context_set_context_stop for every sequence of this context (see FalconModel.set_context_stop)"""
        _set_context_stop(self.ctx, on)

    def resume(self, seq):
        """falcon_hip_context_resume of sequence seq"""
        _resume(self.ctx, seq)

    def context_swap(self, seq, n_past_new, regen, n_batch=512):
        """falcon_hip_context_swap of slot seq, in place: no other slot's cache or state is touched (the first call makes the plain
        context it evaluates in: one more cache of n_ctx rows)"""
        _context_swap(self.ctx, seq, n_past_new, regen, n_batch)

    def set_stop_poll(self, every_steps):
        load().falcon_hip_context_set_stop_poll(self.ctx, int(every_steps))

    def loop_steps(self):
        return load().falcon_hip_context_loop_steps(self.ctx)

    def save_session(self, seq, path, tokens, hparams=None, logits_all=False):
        """falcon_hip_session_save of sequence seq (see FalconModel.save_session)"""
        _save_session(self.ctx, seq, path, hparams or self.model.session_hparams(self.n_ctx), tokens, logits_all)

    def load_session(self, seq, path, hparams=None):
        """falcon_hip_session_load into slot seq: its rows and generator, no other slot; returns the file's tokens"""
        return _load_session(self.ctx, seq, path, hparams or self.model.session_hparams(self.n_ctx), self.n_ctx)

    def copy_state(self, seq, n_tokens, logits_all=False):
        return _copy_state(self.ctx, seq, n_tokens, logits_all)

    def set_state(self, seq, blob):
        return _set_state(self.ctx, seq, blob)

    def free(self):
        load().falcon_hip_context_free(self.ctx)


def graph_captures(obj):
    """falcon_hip_context_graph_captures of a FalconModel or SeqContext: hipGraph captures of its context so far (test and diagnostic hook)"""
    return load().falcon_hip_context_graph_captures(obj.ctx)


def copy_sampling(dst, dst_seq, src, src_seq):
    """falcon_hip_context_copy_sampling: the sampler row (parameters, window, generator state) of sequence src_seq of src -> sequence
    dst_seq of dst, each a FalconModel (sequence 0) or a SeqContext; the copy continues the source's stream. Returns 0, or 1 when refused."""
    return load().falcon_hip_context_copy_sampling(dst.ctx, int(dst_seq), src.ctx, int(src_seq))


def _set_stops(ctx, seq, st):
    if load().falcon_hip_context_set_stops(ctx, int(seq), C.byref(st) if st is not None else None) != 0:
        raise ValueError("falcon_hip_context_set_stops refused these stops")


def _stop_state(ctx, B):
    n, r = np.zeros(B, np.int32), np.zeros(B, np.int32)
    if load().falcon_hip_context_get_stops(ctx, n.ctypes.data, r.ctypes.data) != 0:
        raise RuntimeError("falcon_hip_context_get_stops failed")
    return n, r


def _set_stop_text(ctx, seq, st):
    if load().falcon_hip_context_set_stop_text(ctx, int(seq), C.byref(st) if st is not None else None) != 0:
        raise ValueError("falcon_hip_context_set_stop_text refused these stop strings")


def _stop_text_state(ctx, B):
    cut = np.zeros(B, np.int32)
    if load().falcon_hip_context_get_stop_text(ctx, cut.ctypes.data) != 0:
        raise RuntimeError("falcon_hip_context_get_stop_text failed")
    return cut


def _set_logprobs(obj, n_top):
    if load().falcon_hip_context_set_logprobs(obj.ctx, int(n_top)) != 0:
        raise ValueError("falcon_hip_context_set_logprobs refused n_top %d" % int(n_top))
    obj._lp_n_top, obj._lp_steps = int(n_top), 0


def _get_logprobs(obj, B):
    n_top, steps = getattr(obj, "_lp_n_top", -1), getattr(obj, "_lp_steps", 0)
    if n_top < 0 or steps < 1:
        raise RuntimeError("logprobs: set_logprobs is off, or no sample() / decode_sample() has run since")
    prob = np.zeros((steps, B), np.float32)
    ids, probs = np.zeros((steps, B, n_top), np.int32), np.zeros((steps, B, n_top), np.float32)
    if load().falcon_hip_get_logprobs(obj.ctx, prob.ctypes.data, ids.ctypes.data if n_top else None, probs.ctypes.data if n_top else None) != 0:
        raise RuntimeError("falcon_hip_get_logprobs failed")
    return prob, ids, probs


def logprob_rows(logits, row_stride, n_rows, n_vocab, chosen, n_top, prob, top_id=None, top_prob=None, max_out=None, sum_out=None):
    """ggml_hip_logprob_rows over DevBufs (stream-ordered, no sync): prob[r] = the soft-max probability of token chosen[r] in row r of
    logits, top_id / top_prob [r][n_top] the n_top most likely ids and theirs; returns 0, or 1 when refused (nothing launched)"""
    ptr = lambda b: b.ptr if b is not None else None
    return load().ggml_hip_logprob_rows(logits.ptr, int(row_stride), int(n_rows), int(n_vocab), chosen.ptr, int(n_top), prob.ptr,
                                        ptr(top_id), ptr(top_prob), ptr(max_out), ptr(sum_out))


def guide_rows(logits, row_stride, n_vocab, n_pairs, lead, guide, scale, mixed, mixed_stride, max_out=None, sum_out=None):
    """ggml_hip_guide_rows over DevBufs (stream-ordered, no sync): mixed[p] = the classifier-free-guidance mix (csrc/fq_guide.h) of logits rows
    lead[p] and guide[p] with scale[p]; pairs with lead[p] < 0 are skipped; max_out / sum_out [n_pairs][2]: the rows' maxima and double sums"""
    ptr = lambda b: b.ptr if b is not None else None
    load().ggml_hip_guide_rows(logits.ptr, int(row_stride), int(n_vocab), int(n_pairs), lead.ptr, guide.ptr, scale.ptr, mixed.ptr, int(mixed_stride),
                               ptr(max_out), ptr(sum_out))


def _set_sampling_ext(ctx, seq, params, history):
    h = np.ascontiguousarray(np.asarray(list(history), np.int32))
    rc = load().falcon_hip_context_set_sampling_ext(ctx, int(seq), C.byref(params), h.ctypes.data if h.size else None, int(h.size))
    if rc != 0:
        raise ValueError("falcon_hip_context_set_sampling_ext refused these parameters (%d)" % rc)


def _mirostat_mu(ctx, n):
    mu = np.zeros(n, np.float32)
    if load().falcon_hip_context_get_mirostat_mu(ctx, mu.ctypes.data) != 0:
        raise RuntimeError("falcon_hip_context_get_mirostat_mu failed")
    return mu


def _set_sampling(ctx, seq, params, history):
    h = np.ascontiguousarray(np.asarray(list(history), np.int32))
    rc = load().falcon_hip_context_set_sampling(ctx, int(seq), C.byref(params), h.ctypes.data if h.size else None, int(h.size))
    if rc != 0:
        raise ValueError("falcon_hip_context_set_sampling refused these parameters (%d)" % rc)


def copy_seq(dst, dst_seq, src, src_seq, n_tokens):
    """falcon_hip_context_copy_seq: K / V rows [0, n_tokens) of sequence src_seq of src -> sequence dst_seq of dst, each a
    FalconModel (its own context: sequence 0) or a SeqContext. Returns 0, or 1 when refused (nothing copied)."""
    return load().falcon_hip_context_copy_seq(dst.ctx, int(dst_seq), src.ctx, int(src_seq), int(n_tokens))


class Pipeline:
    """falcon_hip_pipeline_* (csrc/falcon_pipeline.hip): rank `rank` of a `world`-stage layer pipeline over `model` (a
    FalconModel holding that rank's blocks). unique_id: 128 bytes from Pipeline.unique_id() on rank 0 (RCCL transport), or
    local=True for the in-process transport (all ranks in this process, see run_local)."""

    def __init__(self, model, rank, world, n_groups, batch, n_ctx, unique_id=None, local=False):
        L = load()
        self.model, self.rank, self.world, self.G, self.B = model, rank, world, n_groups, batch
        if local:
            self.p = L.falcon_hip_pipeline_create_local(model.m, rank, world, n_groups, batch, n_ctx)
        else:
            self.p = L.falcon_hip_pipeline_create(model.m, rank, world, unique_id, n_groups, batch, n_ctx)
        if not self.p:
            raise RuntimeError("falcon_hip_pipeline_create failed")

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        if load().falcon_hip_pipeline_unique_id(buf) != 0:
            raise RuntimeError("RCCL is not available")
        return buf.raw

    def set_tokens(self, tokens):
        tok = np.ascontiguousarray(tokens, np.int32)
        assert tok.size == self.G * self.B
        if load().falcon_hip_pipeline_set_tokens(self.p, tok.ctypes.data) != 0:
            raise RuntimeError("falcon_hip_pipeline_set_tokens failed")

    def run(self, rounds, n_past0):
        if load().falcon_hip_pipeline_run(self.p, rounds, n_past0) != 0:
            raise RuntimeError("falcon_hip_pipeline_run failed")

    @staticmethod
    def run_local(ranks, rounds, n_past0):
        arr = (C.c_void_p * len(ranks))(*[r.p for r in ranks])
        if load().falcon_hip_pipeline_run_local(arr, len(ranks), rounds, n_past0) != 0:
            raise RuntimeError("falcon_hip_pipeline_run_local failed")

    @staticmethod
    def attach_rccl(ranks):
        """the local job's hand-offs through a one-rank RCCL communicator (self send / recv) instead of device copies"""
        arr = (C.c_void_p * len(ranks))(*[r.p for r in ranks])
        if load().falcon_hip_pipeline_local_attach_rccl(arr, len(ranks)) != 0:
            raise RuntimeError("falcon_hip_pipeline_local_attach_rccl failed (RCCL missing or refused)")

    def rccl_ranks(self):
        return load().falcon_hip_pipeline_rccl_ranks(self.p)

    TRANSPORTS = {0: "none (one stage)", 1: "rccl", 2: "local (device copies in one process)", 3: "local over a one-rank RCCL communicator", 4: "shm (host shared memory between processes)",
                  5: "ipc (device-to-device copies into the peer's IPC-exported mailboxes)"}

    def transport(self):
        return self.TRANSPORTS.get(load().falcon_hip_pipeline_transport(self.p), "?")

    def history(self, first_round, n_rounds):
        """[n_rounds][n_groups * batch] sampled tokens (last rank; waits for the device); None on other ranks"""
        out = np.zeros((n_rounds, self.G * self.B), np.int32)
        rc = load().falcon_hip_pipeline_get_history(self.p, out.ctypes.data, first_round, n_rounds)
        if rc == -1:
            return None
        if rc != 0:
            raise RuntimeError("falcon_hip_pipeline_get_history failed (%d)" % rc)
        return out

    def free(self):
        load().falcon_hip_pipeline_free(self.p)


def pipeline_schedule(rank, world, n_groups, rounds):
    """host only: the slots of one rank as [(exchange ops [(kind, group, peer)], computed group or None, round)], kinds
    'send_hidden' 'send_token' 'recv_hidden' 'recv_token'"""
    L = load()
    names = ("send_hidden", "send_token", "recv_hidden", "recv_token")
    out = (C.c_int * 9)()
    T = L.falcon_hip_pipeline_schedule(rank, world, n_groups, rounds, -1, out)
    slots = []
    for t in range(T):
        L.falcon_hip_pipeline_schedule(rank, world, n_groups, rounds, t, out)
        ops = [(names[out[1 + 3 * i]], out[2 + 3 * i], out[3 + 3 * i]) for i in range(out[0])]
        slots.append((ops, None if out[7] < 0 else out[7], out[8]))
    return slots


class Vocab:
    """the tokenizer of a GGCC v10 file (falcon_tokenize / falcon_token_to_str of the reference); host only"""

    def __init__(self, path):
        L = load()
        self.h = L.falcon_hip_vocab_load_ggcc(os.fsencode(path))
        err = L.falcon_hip_vocab_error(self.h)
        if err:
            L.falcon_hip_vocab_free(self.h)
            self.h = None
            raise ValueError("%s: %s" % (path, err.decode()))
        self.n_vocab, self.n_merges = L.falcon_hip_vocab_size(self.h), L.falcon_hip_vocab_merges(self.h)

    def tokenize(self, text, add_bos=False, n_max=None):
        """token ids (np.int32); with n_max: the C return value when the buffer is too small (minus the count)"""
        L = load()
        raw = text if isinstance(text, bytes) else text.encode("utf-8")
        cap = n_max if n_max is not None else 4 * len(raw) + 8
        buf = np.zeros(max(cap, 1), np.int32)
        n = L.falcon_hip_tokenize(self.h, raw, buf.ctypes.data, cap, 1 if add_bos else 0)
        if n < 0:
            return n
        return buf[:n].copy()

    def token_bytes(self, tid):
        p = C.c_char_p()
        n = load().falcon_hip_token_to_bytes(self.h, int(tid), C.byref(p))
        if n < 0:
            raise IndexError(tid)
        return C.string_at(p, n)

    def detokenize(self, ids):
        return b"".join(self.token_bytes(i) for i in ids)

    def free(self):
        if self.h:
            load().falcon_hip_vocab_free(self.h)
            self.h = None
