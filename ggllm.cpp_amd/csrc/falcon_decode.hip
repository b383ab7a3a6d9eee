// falcon_decode.hip -- generation on the device: the lock-step entries, the sampler / stop / stop-text / grammar / log-prob settings of a context, the
// decode loops, draft-and-verify decode and the pipeline step.
#include "falcon_ctx.h"
#include "fq_sample.h"
using namespace fq_drv;

// ------------------------------------------------------------------------------------------------ greedy decode
// argmax with first-maximum tie-break (std::max_element in llama_sample_token_greedy, libfalcon.cpp:3440-3450);
// also advances the device-side loop state: next token id, n_past + 1, output slot. `vals`/`idxs` are either the
// logits themselves (idxs == nullptr: candidate i has index i) or the per-workgroup candidates written by the
// lm_head kernel (fused decode path) -- the single-workgroup scan then covers 2032 instead of 65024 entries.
__global__ void __launch_bounds__(1024) k_argmax_advance(const float * __restrict__ vals, const int * __restrict__ idxs, int n,
                                                         int32_t * __restrict__ token, int * __restrict__ n_past, int32_t * __restrict__ out, int n_past0) {
    __shared__ float bv[16];
    __shared__ int   bi[16];
    float best = -INFINITY; int idx = 0x7FFFFFFF;
    for (int i0 = threadIdx.x; i0 < n; i0 += 4 * blockDim.x) {            // 4 independent loads per step
        float v[4]; int id[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = i0 + k * blockDim.x; const int ic = i < n ? i : n - 1; v[k] = vals[ic]; id[k] = idxs ? idxs[ic] : ic; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = i0 + k * blockDim.x; if (i < n && (v[k] > best || (v[k] == best && id[k] < idx))) { best = v[k]; idx = id[k]; } }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(idx, o);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { bv[wid] = best; bi[wid] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
        const int np = *n_past;
        out[n_past0 < 0 ? 0 : np - n_past0] = idx;              // (n_past0 < 0: a pipeline stage's captured step always uses slot 0)
        token[0] = idx;
        *n_past = np + 1;
    }
}

// the greedy pick of a single-stream step: from the fused lm_head's per-workgroup candidates where it wrote them, else from the logits row
static void launch_argmax_advance(falcon_hip_context * c, int32_t * token, int n_past0, hipStream_t st) {
    const int V = c->m->hp.n_vocab;
    if (stage_fused(c)) hipLaunchKernelGGL(k_argmax_advance, dim3(1), dim3(256), 0, st, c->argmax_val, c->argmax_idx, (V + 31) / 32, token, c->n_past_dev, c->out_tokens_dev, n_past0);
    else hipLaunchKernelGGL(k_argmax_advance, dim3(1), dim3(1024), 0, st, c->logits_dev, (const int *) nullptr, V, token, c->n_past_dev, c->out_tokens_dev, n_past0);
}

// ------------------------------------------------------------------------------------------------ pipeline step
__global__ void k_set_i32(int * p, int v) { *p = v; }
__global__ void k_copy_i32(int32_t * dst, const int32_t * src, int n = 1) { for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i]; }
// greedy sample of every row of a lock-step step: token[row] = argmax(logits[row]), lowest index on ties (as k_argmax_advance)
__global__ void __launch_bounds__(1024) k_argmax_rows(const float * __restrict__ logits, int n, int32_t * __restrict__ token) {
    __shared__ float bv[16];
    __shared__ int   bi[16];
    const float * vals = logits + (int64_t) blockIdx.x * n;
    float best = -INFINITY; int idx = 0x7FFFFFFF;
    if ((n & 3) == 0) {
        // four rows of 16 bytes in flight per thread (the scalar loop below was a chain of 64 dependent round trips: 25 us per step for 65024 logits)
        const float4 * v4 = (const float4 *) vals;
        const int n4 = n >> 2;
#pragma unroll 4
        for (int i = threadIdx.x; i < n4; i += blockDim.x) {
            const float4 v = v4[i];
            const float e[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 4; ++k) if (e[k] > best || (e[k] == best && 4 * i + k < idx)) { best = e[k]; idx = 4 * i + k; }
        }
    } else {
        for (int i = threadIdx.x; i < n; i += blockDim.x) { const float v = vals[i]; if (v > best || (v == best && i < idx)) { best = v; idx = i; } }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(idx, o);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
        token[blockIdx.x] = idx;
    }
}
__global__ void k_inc_i32(int * p) { *p = *p + 1; }

// One decode step of one pipeline stage, fully stream-ordered (no host synchronisation, no host memory): the token id
// (first stage) / residual row (other stages) are read from device memory, the residual row (inner stages) / the
// greedy-sampled next token (last stage) are written to device memory. The caller moves them between ranks (RCCL).
extern "C" int falcon_hip_stage_step(falcon_hip_context * c, const int32_t * token_dev, const float * hidden_in_dev, int n_past,
                                     float * hidden_out_dev, int32_t * next_token_dev) {
    hip_context & hc = fq_ctx();
    falcon_hip_model * m = c->m;
    hipStream_t st = hc.stream;
    if (n_past < 0 || n_past + 1 > c->n_ctx) { fprintf(stderr, "falcon-hip: stage step at n_past %d exceeds n_ctx %d\n", n_past, c->n_ctx); exit(1); }
    const keep_hidden_off no_hidden(c);
    // body of one step; n_past_base >= 0: position baked into the launch arguments (plain launches), < 0: the position is
    // whatever n_past_dev holds and the step leaves n_past_dev + 1 behind (captured form, replayable)
    const int B = c->n_seq > 0 ? c->n_seq : 1;                       // lock-step sequences: token_dev / next_token_dev hold B ids, the hidden rows are [B][n_embd]
    auto body = [&](int n_past_base, int max_kv) {
        if (m->first_stage()) hipLaunchKernelGGL(k_copy_i32, dim3(1), dim3(64), 0, st, c->tokens_dev, token_dev, B);
        else HIP_CHECK(hipMemcpyAsync(c->x, hidden_in_dev, (size_t) B * m->hp.n_embd * 4, hipMemcpyDeviceToDevice, st));
        launch_stage(c, B, max_kv, st);
        bool advanced = false;
        if (m->last_stage()) {
            if (next_token_dev) {
                // greedy sample; the loop-state outputs of k_argmax_advance go to scratch slots of this context
                if (B > 1)
                    hipLaunchKernelGGL(k_argmax_rows, dim3((unsigned) B), dim3(1024), 0, st, c->logits_dev, m->hp.n_vocab, next_token_dev);
                else
                    launch_argmax_advance(c, next_token_dev, n_past_base, st);
                advanced = B == 1;
            }
        } else if (hidden_out_dev) {
            HIP_CHECK(hipMemcpyAsync(hidden_out_dev, c->x, (size_t) B * m->hp.n_embd * 4, hipMemcpyDeviceToDevice, st));
        }
        if (n_past_base < 0 && !advanced) hipLaunchKernelGGL(k_inc_i32, dim3(1), dim3(1), 0, st, c->n_past_dev);
    };
    if (graph_ok_stage_step(c)) {
        // one hipGraph replay per step instead of ~70 launches from the host: a stage of a deep pipeline holds few blocks,
        // and the host side of a step would otherwise cost as much as its device side
        step_key key = step_key_of(c);
        key.entry[0] = key_ptr(token_dev); key.entry[1] = key_ptr(hidden_in_dev); key.entry[2] = key_ptr(hidden_out_dev); key.entry[3] = key_ptr(next_token_dev);
        if (!c->stage_step.holds(key)) c->step_next_n_past = -1;
        if (n_past != c->step_next_n_past) hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, st, c->n_past_dev, n_past);
        c->stage_step.replay(c, st, key, [&] { body(-1, c->n_ctx); });
        c->step_next_n_past = n_past + 1;
    } else {
        hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, st, c->n_past_dev, n_past);
        body(n_past, n_past + 1);
        c->step_next_n_past = -1;
    }
    return 0;
}

static int decode_loop(falcon_hip_context * c, bool ragged, bool sampled, const int32_t * first_tokens, const int32_t * n_past, int n_steps, int32_t * out_tokens, const char * where);

extern "C" int falcon_hip_decode_greedy(falcon_hip_context * c, int32_t first_token, int n_past, int n_steps, int32_t * out_tokens) {
    if (emb_refuses(c, "decode_greedy")) return 1;
    if (!c->m->first_stage() || !c->m->last_stage()) { fprintf(stderr, "falcon-hip: greedy decode needs the whole model in one process\n"); exit(1); }
    if (n_past + n_steps > c->n_ctx) { fprintf(stderr, "falcon-hip: decode past n_ctx\n"); exit(1); }
    return decode_loop(c, false, false, &first_token, &n_past, n_steps, out_tokens, "greedy decode");
}

// ------------------------------------------------------------------------------------------------ ragged lock-step steps
// Row t of a lock-step context at its own position pos[t] (falcon_hip_eval_seqs): the mat-muls are those of a uniform step of the same
// context (a row of them does not depend on the other rows), the RoPE row, KV append and keys [0, pos[t]] of the attention are row t's.
static int seqs_check(const falcon_hip_context * c, const char * what, const int32_t * tokens, const int32_t * n_past, int adv) {
    const falcon_hip_model * m = c->m;
    const int B = c->n_seq > 0 ? c->n_seq : 1;
    if (!m->first_stage() || !m->last_stage()) { fprintf(stderr, "falcon-hip: %s needs the whole model in one process\n", what); return 1; }
    for (int t = 0; t < B; ++t) if (n_past[t] < 0 || n_past[t] + adv > c->n_ctx) {
        fprintf(stderr, "falcon-hip: %s: sequence %d at n_past %d, %d step(s): needs 0 <= n_past and n_past + steps <= n_ctx (%d)\n", what, t, n_past[t], adv, c->n_ctx);
        return 1;
    }
    for (int t = 0; t < B; ++t) if (tokens[t] < 0 || tokens[t] >= m->hp.n_vocab) {
        fprintf(stderr, "falcon-hip: %s: token id %d of sequence %d is outside [0, %d)\n", what, tokens[t], t, m->hp.n_vocab);
        return 2;
    }
    if (c->sync_err_sticky) { fprintf(stderr, "falcon-hip: %s: an earlier step of this context lost an in-launch hand-off -- its KV cache is invalid, the context must be recreated\n", what); return 3; }
    return 0;
}

static void seqs_alloc(falcon_hip_context * c) {
    if (c->pos_dev) return;
    c->pos_dev       = (int *) dev_alloc(c->allocs, (size_t) c->n_seq * 4 + 256);
    c->seq_steps_dev = (int *) dev_alloc(c->allocs, (size_t) c->n_seq * 4 + 256);
}

extern "C" int falcon_hip_eval_seqs(falcon_hip_context * c, const int32_t * tokens, const int32_t * n_past) {
    if (const int rc = seqs_check(c, "eval_seqs", tokens, n_past, 1)) return rc;
    if (c->n_seq == 0) return falcon_hip_eval_stage(c, tokens, nullptr, 1, n_past[0], 1, nullptr);     // a context of one sequence
    seqs_alloc(c);
    hip_context & hc = fq_ctx();
    falcon_hip_model * m = c->m;
    const int B = c->n_seq;
    hipStream_t st = hc.stream;
    int max_pos = 0;
    for (int t = 0; t < B; ++t) max_pos = n_past[t] > max_pos ? n_past[t] : max_pos;
    c->logits_pending = false;
    c->logits_last = nullptr;
    c->logits_none = false;
    HIP_CHECK(hipMemcpyAsync(c->pos_dev, n_past, (size_t) B * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->tokens_dev, tokens, (size_t) B * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));        // (the arrays may live on the caller's stack)
    launch_stage(c, B, max_pos + 1, st, 1);     // LDS for the longest row
    const int64_t V = m->hp.n_vocab;
    c->logits_host.resize((size_t) B * V);
    HIP_CHECK(hipMemcpyAsync(c->logits_host.data(), c->logits_dev, (size_t) B * V * 4, hipMemcpyDeviceToHost, st));
    fetch_sync_error(c, st);
    HIP_CHECK(hipStreamSynchronize(st));
    c->logits_fresh = true;
    return report_sync_error(c, "eval_seqs");
}

// greedy sample of every row of a ragged step (k_argmax_rows' scan: lowest index on ties), then the row's loop state: next token, out[steps[t]][t], pos[t] + 1.
// Per-row step counters (one workgroup owns each): one captured step serves any positions and any number of steps.
__global__ void __launch_bounds__(1024) k_argmax_rows_step(const float * __restrict__ logits, int n, int32_t * __restrict__ token, int * __restrict__ pos,
                                                           int * __restrict__ steps, int32_t * __restrict__ out, int n_seq) {
    __shared__ float bv[16];
    __shared__ int   bi[16];
    const float * vals = logits + (int64_t) blockIdx.x * n;
    float best = -INFINITY; int idx = 0x7FFFFFFF;
    if ((n & 3) == 0) {
        const float4 * v4 = (const float4 *) vals;
        const int n4 = n >> 2;
#pragma unroll 4
        for (int i = threadIdx.x; i < n4; i += blockDim.x) {
            const float4 v = v4[i];
            const float e[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 4; ++k) if (e[k] > best || (e[k] == best && 4 * i + k < idx)) { best = e[k]; idx = 4 * i + k; }
        }
    } else {
        for (int i = threadIdx.x; i < n; i += blockDim.x) { const float v = vals[i]; if (v > best || (v == best && i < idx)) { best = v; idx = i; } }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(idx, o);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
        const int t = blockIdx.x, s = steps[t];
        out[(int64_t) s * n_seq + t] = idx;
        token[t] = idx;
        pos[t] = pos[t] + 1;
        steps[t] = s + 1;
    }
}

extern "C" int falcon_hip_decode_greedy_seqs(falcon_hip_context * c, const int32_t * first_tokens, const int32_t * n_past, int n_steps, int32_t * out_tokens) {
    if (n_steps < 1) { fprintf(stderr, "falcon-hip: decode_greedy_seqs: n_steps %d < 1\n", n_steps); return 1; }
    if (const int rc = seqs_check(c, "decode_greedy_seqs", first_tokens, n_past, n_steps)) return rc;
    if (c->n_seq == 0) return falcon_hip_decode_greedy(c, first_tokens[0], n_past[0], n_steps, out_tokens);     // a context of one sequence
    return decode_loop(c, true, false, first_tokens, n_past, n_steps, out_tokens, "decode_greedy_seqs");
}
// ------------------------------------------------------------------------------------------------ sampled decode
// falcon_main's default sampler chain (kernels_sample.hip) in place of the argmax: one sampler row per sequence, its
// parameters, window and generator in device memory, so the loops below are the greedy ones with k_sample_rows as the
// step's last launch (one replay per step with falcon_hip_context_use_graph).
static ggml_hip_sampler * ctx_sampler(falcon_hip_context * c) {
    if (!c->sampler) c->sampler = ggml_hip_sampler_create(ctx_rows(c), c->m->hp.n_vocab, c->n_ctx);
    if (c->sampler && c->m->vb_pool) fq_sampler_share_vocab_bytes(c->sampler, c->m->vb_pool, c->m->vb_offs);      // (the model's vocabulary may have come after the sampler)
    return c->sampler;
}
// What every entry that sets or reads a sampler row asks first: the context's sampler, made now if need be -- or null and the entry's return in *rc: 1 behind
// the message (no lm_head; no sampler could be made), and with `off` -- the call turns a thing off -- on a context that never sampled 0, or 1 for a bad
// sequence: nothing to turn off, and no sampler is made for it
static ggml_hip_sampler * entry_sampler(falcon_hip_context * c, const char * who, int * rc, bool off = false, int seq = 0) {
    *rc = 1;
    if (!has_head(c, who)) return nullptr;
    if (off && !c->sampler) {
        if (seq < 0 || seq >= ctx_rows(c)) fprintf(stderr, "falcon-hip: %s: bad sequence %d\n", who, seq); else *rc = 0;
        return nullptr;
    }
    return ctx_sampler(c);
}
// a getter on a context that never sampled: every row reads `v`, and no sampler is made to say so
static void fill_rows(const falcon_hip_context * c, int32_t * out, int32_t v) { if (out) for (int t = 0; t < ctx_rows(c); ++t) out[t] = v; }

// the generator a loaded session left for this sequence before its row existed (falcon_hip_set_state) replaces the seeded one, once
static int take_kept_rng(falcon_hip_context * c, ggml_hip_sampler * s, int seq) {
    for (size_t i = 0; i < c->rng_kept.size(); ++i) if ((int) c->rng_kept[i][0] == seq) {
        const int rc = ggml_hip_sampler_set_rng(s, seq, c->rng_kept[i].data() + 1, (int32_t) c->rng_kept[i][1 + FQ_MT_N]);
        c->rng_kept.erase(c->rng_kept.begin() + (long) i);
        return rc;
    }
    return 0;
}

extern "C" int falcon_hip_context_set_sampling(falcon_hip_context * c, int seq, const ggml_hip_sampling * params, const int32_t * history, int n_history) {
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "set_sampling", &rc);
    if (s) rc = ggml_hip_sampler_set_row(s, seq, params, history, n_history);
    return rc ? rc : take_kept_rng(c, s, seq);
}

extern "C" int falcon_hip_context_set_sampling_ext(falcon_hip_context * c, int seq, const ggml_hip_sampling_ext * params, const int32_t * history, int n_history) {
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "set_sampling_ext", &rc);
    if (s) rc = ggml_hip_sampler_set_row_ext(s, seq, params, history, n_history);
    return rc ? rc : take_kept_rng(c, s, seq);
}
extern "C" int falcon_hip_context_get_mirostat_mu(falcon_hip_context * c, float * mu_out) {
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "get_mirostat_mu", &rc);
    return s ? ggml_hip_sampler_get_mu(s, mu_out) : rc;
}

extern "C" int falcon_hip_context_copy_sampling(falcon_hip_context * dst, int dst_seq, falcon_hip_context * src, int src_seq) {
    if (!dst || !src || !dst->m->last_stage() || !src->m->last_stage()) { fprintf(stderr, "falcon-hip: copy_sampling: a context without an lm_head\n"); return 1; }
    ggml_hip_sampler * d = ctx_sampler(dst), * s = ctx_sampler(src);
    return d && s ? ggml_hip_sampler_copy_row(d, dst_seq, s, src_seq) : 1;
}

// ---- stops (fq_stop.h): the rows' sequences, budgets and state belong to the sampler; the loop's early exit is decode_loop's
extern "C" int falcon_hip_context_set_stops(falcon_hip_context * c, int seq, const ggml_hip_stops * stops) {
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "set_stops", &rc, !stops, seq);
    return s ? ggml_hip_sampler_set_stops(s, seq, stops) : rc;
}
extern "C" int falcon_hip_context_get_stops(falcon_hip_context * c, int32_t * n_drawn_out, int32_t * reason_out) {
    if (!has_head(c, "get_stops")) return 1;
    if (!c->sampler) { fill_rows(c, n_drawn_out, 0); fill_rows(c, reason_out, FQ_STOP_RUNNING); return 0; }      // every sequence running with nothing drawn
    return ggml_hip_sampler_get_stops(ctx_sampler(c), n_drawn_out, reason_out);
}
extern "C" int falcon_hip_context_set_stop_text(falcon_hip_context * c, int seq, const ggml_hip_stop_text * text) {
    // (a model without an lm_head takes no vocabulary either: that refusal is entry_sampler's)
    if (text && c->m->last_stage() && !c->m->vb_pool) { fprintf(stderr, "falcon-hip: set_stop_text: the model has no vocabulary (falcon_hip_model_set_vocab)\n"); return 1; }
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "set_stop_text", &rc, !text, seq);
    return s ? ggml_hip_sampler_set_stop_text(s, seq, text) : rc;
}
extern "C" int falcon_hip_context_get_stop_text(falcon_hip_context * c, int32_t * cut_bytes_out) {
    if (!has_head(c, "get_stop_text") || !cut_bytes_out) return 1;
    if (!c->sampler) { fill_rows(c, cut_bytes_out, 0); return 0; }      // no sequence has ended by text
    return ggml_hip_sampler_get_stop_text(c->sampler, cut_bytes_out);
}
extern "C" int falcon_hip_context_set_grammar(falcon_hip_context * c, int seq, ggml_hip_grammar * g, int state) {
    // (spec_K > 0: a whole model, so the context holds an lm_head)
    if (g && c->spec_K > 0) { fprintf(stderr, "falcon-hip: set_grammar: draft-and-verify decode is on (falcon_hip_context_set_spec) and applies no grammar: turn it off first\n"); return 1; }
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "set_grammar", &rc, !g, seq);
    return s ? ggml_hip_sampler_set_grammar(s, seq, g, state) : rc;
}
extern "C" int falcon_hip_context_get_grammar_state(falcon_hip_context * c, int32_t * states_out) {
    if (!has_head(c, "get_grammar_state") || !states_out) return 1;
    if (!c->sampler) { fill_rows(c, states_out, -1); return 0; }      // no sequence holds a grammar
    return ggml_hip_sampler_get_grammar_state(c->sampler, states_out);
}
// ---- guidance (fq_guide.h): the pairs belong to the sampler; fq_launch_sample puts the mix in front of its launch, decode_loop's early exit counts a guide row as its leader
extern "C" int falcon_hip_context_set_guidance(falcon_hip_context * c, int seq, int guide_seq, float scale) {
    if (c->n_seq == 0) { fprintf(stderr, "falcon-hip: set_guidance: a context of one sequence has no row for a negative prompt: make a lock-step context (falcon_hip_context_create_seqs)\n"); return 1; }
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "set_guidance", &rc, guide_seq < 0, seq);
    return s ? ggml_hip_sampler_set_guidance(s, seq, guide_seq, scale) : rc;
}
extern "C" int falcon_hip_context_get_guidance(falcon_hip_context * c, int32_t * guide_seq_out, float * scale_out) {
    if (!has_head(c, "get_guidance")) return 1;
    if (!c->sampler) {                                      // no sequence has a guide
        fill_rows(c, guide_seq_out, -1);
        if (scale_out) for (int t = 0; t < ctx_rows(c); ++t) scale_out[t] = 1.0f;
        return 0;
    }
    return ggml_hip_sampler_get_guidance(c->sampler, guide_seq_out, scale_out);
}
extern "C" void falcon_hip_context_set_stop_poll(falcon_hip_context * c, int every_steps) { c->stop_poll = every_steps < 1 ? 1 : every_steps; }
extern "C" int falcon_hip_context_loop_steps(const falcon_hip_context * c) { return c->loop_steps; }

// ---- log-probabilities (kernels_logprob.hip): one launch behind the sampler's, which has written the chosen tokens and advanced the step counters
static void lp_drop(falcon_hip_context * c) {               // frees the record buffers (the sampled loops' slots carry the addresses in their keys)
    HIP_CHECK(hipStreamSynchronize(fq_ctx().stream));
    c->lp_prob.reset(0); c->lp_top_id.reset(0); c->lp_top_prob.reset(0);
    c->lp_cap = 0; c->lp_steps = c->lp_rows = 0;
}
static void lp_reserve(falcon_hip_context * c, int64_t records) {      // (outside any capture)
    if (c->lp_n_top < 0 || records <= c->lp_cap) return;
    const int n_top = c->lp_n_top;
    lp_drop(c);
    c->lp_cap = records;
    c->lp_prob.reset((size_t) records);
    if (n_top > 0) { c->lp_top_id.reset((size_t) records * n_top); c->lp_top_prob.reset((size_t) records * n_top); }
}
// the log-prob part of a sampled step's key: the record buffers, and lp_n_top and lp_cap, arguments of the record launch (no launch while lp_n_top < 0)
static void lp_step_key(const falcon_hip_context * c, int64_t key[5]) {
    key[0] = key_ptr(c->lp_prob.get()); key[1] = key_ptr(c->lp_top_id.get()); key[2] = key_ptr(c->lp_top_prob.get()); key[3] = c->lp_n_top; key[4] = c->lp_cap;
}
// rows' records at step (steps[r] - 1) of a loop whose sampler launch has just advanced steps, or (steps == nullptr) at step 0
// (a row the sampler's launch skipped because it had ended keeps the records it has: the launch gets the sampler's skip words)
static void lp_launch(falcon_hip_context * c, int n_rows, const float * logits, const int32_t * chosen, const int * steps, hipStream_t st) {
    fq_launch_logprob(logits, c->m->hp.n_vocab, n_rows, c->m->hp.n_vocab, chosen, c->lp_n_top, steps, -1, n_rows, c->lp_cap,
                      c->lp_prob.get(), c->lp_top_id.get(), c->lp_top_prob.get(), nullptr, nullptr, st, fq_sampler_stop_skip(c->sampler));
}

extern "C" int falcon_hip_context_set_logprobs(falcon_hip_context * c, int n_top) {
    if (!has_head(c, "set_logprobs")) return 1;
    if (n_top < -1 || n_top > GGML_HIP_LOGPROB_MAX_TOP || n_top > c->m->hp.n_vocab) {
        fprintf(stderr, "falcon-hip: set_logprobs: n_top %d is outside [-1, min(%d, n_vocab)]\n", n_top, GGML_HIP_LOGPROB_MAX_TOP);
        return 1;
    }
    if (n_top >= 0 && c->spec_K > 0) { fprintf(stderr, "falcon-hip: set_logprobs: draft-and-verify decode is on (falcon_hip_context_set_spec) and records no log-probabilities: turn it off first\n"); return 1; }
    if (n_top == c->lp_n_top) return 0;
    lp_drop(c);                                             // (lp_n_top is in the sampled slots' keys: they hold or lack the launch)
    c->lp_n_top = n_top;
    return 0;
}

extern "C" int falcon_hip_get_logprobs(falcon_hip_context * c, float * prob_out, int32_t * top_id_out, float * top_prob_out) {
    if (c->lp_n_top < 0 || c->lp_steps < 1 || !prob_out) return 1;
    const size_t n = (size_t) c->lp_steps * c->lp_rows;
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemcpyAsync(prob_out, c->lp_prob.get(), n * 4, hipMemcpyDeviceToHost, st));
    if (c->lp_n_top > 0 && top_id_out) HIP_CHECK(hipMemcpyAsync(top_id_out, c->lp_top_id.get(), n * c->lp_n_top * 4, hipMemcpyDeviceToHost, st));
    if (c->lp_n_top > 0 && top_prob_out) HIP_CHECK(hipMemcpyAsync(top_prob_out, c->lp_top_prob.get(), n * c->lp_n_top * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int falcon_hip_sample(falcon_hip_context * c, int32_t * out) {
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "sample", &rc);
    if (!s) return rc;
    hipStream_t st = fq_ctx().stream;
    const int64_t V = c->m->hp.n_vocab;
    const int B = ctx_rows(c);
    const float * lg = c->n_seq > 0 ? c->logits_dev : c->logits_dev + (int64_t)(c->last_rows - 1) * V;
    lp_reserve(c, B);
    fq_launch_sample(s, B, lg, V, fq_sampler_tokens(s), nullptr, nullptr, nullptr, 0, st);
    if (c->lp_n_top >= 0) { lp_launch(c, B, lg, fq_sampler_tokens(s), nullptr, st); c->lp_steps = 1; c->lp_rows = B; }
    HIP_CHECK(hipMemcpyAsync(out, fq_sampler_tokens(s), (size_t) B * 4, hipMemcpyDeviceToHost, st));
    std::vector<int> skipped;                               // stops: a sequence that had ended drew nothing -- -1, as in the loops' output
    if (const int * skip = fq_sampler_stop_skip(s)) { skipped.resize(B); HIP_CHECK(hipMemcpyAsync(skipped.data(), skip, (size_t) B * 4, hipMemcpyDeviceToHost, st)); }
    HIP_CHECK(hipStreamSynchronize(st));
    for (size_t t = 0; t < skipped.size(); ++t) if (skipped[t]) out[t] = -1;
    return 0;
}

// The polled loop of the device-side decode loops (decode_loop: the rows' stops; falcon_hip_decode_spec: the draft-and-verify state): n steps, or fewer once
// ended(image) says so. The steps run in chunks of E = stop_poll; behind chunk j the device state is copied into the page-locked image j & 1 and an
// event is recorded, between two replays, never inside the captured step. Chunk j + 2 is enqueued only after chunk j's event has passed and ended(j & 1) is
// false for its image, so the device always has a chunk queued while the host waits, and a loop that ends at step k (0-based) launches at most
// (k / E + 2) * E steps: at most two intervals past the end. An event waited for was always recorded by THIS call: the wait at step s = (j + 2) * E < n
// is for chunk j's record, made at step (j + 1) * E - 1 under the condition (j + 1) * E < n, which s < n implies -- never one left over from an
// earlier call. Returns the steps launched.
template <class T, class Step, class Ended>
static int run_polled(int n, int E, bool poll, polled_images<T> & im, const T * state_dev, hipStream_t st, Step && step, Ended && ended) {
    int s = 0;
    for (; s < n; ++s) {
        if (poll && s % E == 0 && s >= 2 * E) {
            const int img = (s / E) & 1;
            HIP_CHECK(hipEventSynchronize(im.ev[img]));
            if (ended(im.image(img))) break;
        }
        step();
        if (poll && (s + 1) % E == 0 && s + 1 < n) {
            const int img = (s / E) & 1;
            HIP_CHECK(hipMemcpyAsync(im.image(img), state_dev, sizeof(T) * im.rows, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipEventRecord(im.ev[img], st));
        }
    }
    return s;
}

// ------------------------------------------------------------------------------------------------ the decode loops
// THE loop behind falcon_hip_decode_greedy / _sample / _greedy_seqs / _sample_seqs, which keep their own argument checks: n_steps times launch_stage and
// the step's last launch, which picks every row's next token and advances the loop state in device memory -- one replay per step where the entry point's
// predicate holds. ragged: the B rows of a lock-step context, row t at pos_dev[t] with its step counter, output seq_out_dev [step][B]; else one row at
// n_past_dev, output out_tokens_dev. sampled: the last launch is the sampler's, plus the records' while lp_n_top >= 0; else the argmax.
static int decode_loop(falcon_hip_context * c, bool ragged, bool sampled, const int32_t * first_tokens, const int32_t * n_past, int n_steps, int32_t * out_tokens, const char * where) {
    falcon_hip_model * m = c->m;
    hipStream_t st = fq_ctx().stream;
    const int B = ragged ? c->n_seq : 1;
    ggml_hip_sampler * sm = nullptr;
    if (emb_refuses(c, where)) return 1;
    if (ragged) seqs_alloc(c);
    if (sampled && !(sm = ctx_sampler(c))) return 1;
    c->logits_fresh = false;
    // (under a context stop no call runs more than n_ctx steps and the calls' lengths follow the slots' positions: sized for n_ctx once, the buffer -- and the
    // captured step that holds its address -- stays through the swaps)
    const int64_t out_need = (int64_t)(sampled && fq_sampler_ctx_limit(sm) > 0 && n_steps < c->n_ctx ? c->n_ctx : n_steps) * B;
    if (ragged && out_need > c->seq_out_cap) {                      // (grows outside any capture; seq_out_dev is in both lock-step slots' keys, and the new
        HIP_CHECK(hipStreamSynchronize(st));                        // buffer exists before the old one goes: always another address, always a re-capture)
        c->seq_out_cap = out_need;
        c->seq_out_dev.reset((size_t) out_need);
    }
    if (sampled) lp_reserve(c, ragged ? (int64_t) n_steps * B : c->n_ctx);      // (single stream: as out_tokens_dev, any n_steps of this context)
    int * pos = ragged ? c->pos_dev : c->n_past_dev;
    int * steps = ragged ? c->seq_steps_dev : sampled ? fq_sampler_steps(sm) : nullptr;
    int32_t * out_dev = ragged ? c->seq_out_dev.get() : c->out_tokens_dev;
    int max_pos = 0;
    for (int t = 0; t < B; ++t) max_pos = n_past[t] > max_pos ? n_past[t] : max_pos;
    HIP_CHECK(hipMemcpyAsync(pos, n_past, (size_t) B * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->tokens_dev, first_tokens, (size_t) B * 4, hipMemcpyHostToDevice, st));
    if (steps) HIP_CHECK(hipMemsetAsync(steps, 0, (size_t) B * 4, st));
    // stops: with any row of the context holding some, a row that ends writes nothing more (its output reads -1 from there on) and rides the pass frozen:
    // its token is evaluated again at its position, which rewrites the same K / V row. Once EVERY row holds stops the loop may end early -- poll.
    // A guide row (fq_guide.h) ends with its leader and has no stops of its own that count: every DRAWING row holds stops.
    const int stop_rows = sampled ? fq_sampler_stop_rows(sm) : 0;
    const int pairs = sampled ? fq_sampler_guide_pairs(sm) : 0;
    const int * lead_of = pairs > 0 ? fq_sampler_lead_of(sm) : nullptr;
    const bool poll = pairs > 0 ? fq_sampler_drawing_stop_rows(sm) == B - pairs : stop_rows == B;
    if (stop_rows > 0) HIP_CHECK(hipMemsetAsync(out_dev, 0xff, (size_t) n_steps * B * 4, st));
    if (poll) c->stop_poll_img.make((size_t) B);
    HIP_CHECK(hipStreamSynchronize(st));        // (the arrays may live on the caller's stack)
    const keep_hidden_off no_hidden(c);
    auto one_step = [&](int max_kv) {
        launch_stage(c, B, max_kv, st, ragged ? 1 : 0);
        if (sampled) {
            fq_launch_sample(sm, B, c->logits_dev, m->hp.n_vocab, c->tokens_dev, pos, steps, out_dev, B, st);
            // (the next step's lm_head is ordered behind it; under a context stop a row that ends at the end of its cache keeps its tokens_dev entry: the draws are the sampler's)
            if (c->lp_n_top >= 0) lp_launch(c, B, c->logits_dev, fq_sampler_ctx_limit(sm) > 0 ? fq_sampler_tokens(sm) : c->tokens_dev, steps, st);
        } else if (ragged)
            hipLaunchKernelGGL(k_argmax_rows_step, dim3((unsigned) B), dim3(1024), 0, st, c->logits_dev, m->hp.n_vocab, c->tokens_dev, pos, steps, out_dev, B);
        else
            launch_argmax_advance(c, c->tokens_dev, n_past[0], st);      // (pos = n_past_dev, out_dev = out_tokens_dev)
    };
    // n_steps steps, or fewer when every row has ended (run_polled). (The whole 40-byte states are copied, not the reason words alone: one contiguous copy, and
    // the same bytes get_stops reads.)
    auto run_steps = [&](auto && step) {
        c->loop_steps = run_polled(n_steps, c->stop_poll, poll, c->stop_poll_img, sampled ? fq_sampler_stop_state(sm) : nullptr, st, step,
            [&](const fq_stop_state * rows) { bool running = false; for (int t = 0; t < B; ++t) running |= !(lead_of && lead_of[t] >= 0) && !fq_stop_finished(&rows[t]); return !running; });
    };
    if (ragged ? graph_ok_seqs(c) : graph_ok_loop(c)) {
        // positions, output slots and the sampler's state are read from device memory, so one capture, sized for the whole context, serves any call -- but
        // for the single-stream argmax, whose k_argmax_advance takes the base position as an argument
        step_key key = step_key_of(c);
        key.entry[0] = ragged ? key_ptr(out_dev) : sampled ? 0 : n_past[0];
        if (sampled) { lp_step_key(c, key.lp); fq_sampler_step_key(sm, key.sampler); }
        step_slot & slot = ragged ? (sampled ? c->sample_seqs_step : c->seqs_step) : (sampled ? c->sample_step : c->decode_step);
        run_steps([&] { slot.replay(c, st, key, [&] { one_step(c->n_ctx); }); });
    } else {
        run_steps([&] { one_step(max_pos + n_steps < c->n_ctx ? max_pos + n_steps : c->n_ctx); });      // (beyond n_ctx only under a context stop: no row gets there)
    }
    HIP_CHECK(hipMemcpyAsync(out_tokens, out_dev, (size_t) n_steps * B * 4, hipMemcpyDeviceToHost, st));
    fetch_sync_error(c, st);
    HIP_CHECK(hipStreamSynchronize(st));
    if (!ragged) c->last_rows = 1;              // (falcon_hip_sample: the last step's row)
    if (!sampled) c->lp_steps = 0;              // (the greedy loops record no log-probabilities)
    else if (c->lp_n_top >= 0) { c->lp_steps = n_steps; c->lp_rows = B; }
    return report_sync_error(c, where);
}

// the context stop (falcon_hip_context_set_context_stop) is on: the sampled loops take any n_steps, a row ends at the end of its cache
static bool context_stop_on(const falcon_hip_context * c) { return c->sampler && fq_sampler_ctx_limit(c->sampler) > 0; }
// ... and every row has ended after n_run steps at the latest: the steps behind that would find the rows frozen and write -1. Their output is filled here, and
// the steps to run come back
static int context_stop_truncate(int n_steps, int n_run, int B, int32_t * out_tokens) {
    if (n_steps <= n_run) return n_steps;
    for (int64_t i = (int64_t) n_run * B; i < (int64_t) n_steps * B; ++i) out_tokens[i] = -1;
    return n_run;
}

extern "C" int falcon_hip_decode_sample(falcon_hip_context * c, int32_t first_token, int n_past, int n_steps, int32_t * out_tokens) {
    if (emb_refuses(c, "decode_sample")) return 1;
    if (!c->m->first_stage() || !c->m->last_stage()) { fprintf(stderr, "falcon-hip: sampled decode needs the whole model in one process\n"); exit(1); }
    if (context_stop_on(c) && n_past >= 0 && n_past < c->n_ctx) n_steps = context_stop_truncate(n_steps, c->n_ctx - n_past, 1, out_tokens);
    if (n_past + n_steps > c->n_ctx) { fprintf(stderr, "falcon-hip: decode past n_ctx\n"); exit(1); }
    return decode_loop(c, false, true, &first_token, &n_past, n_steps, out_tokens, "sampled decode");
}

extern "C" int falcon_hip_decode_sample_seqs(falcon_hip_context * c, const int32_t * first_tokens, const int32_t * n_past, int n_steps, int32_t * out_tokens) {
    if (n_steps < 1) { fprintf(stderr, "falcon-hip: decode_sample_seqs: n_steps %d < 1\n", n_steps); return 1; }
    if (context_stop_on(c)) {
        // every sequence needs room for ONE step; each ends at the end of its own cache at the latest, so the steps behind the last such end are all -1
        if (const int rc = seqs_check(c, "decode_sample_seqs", first_tokens, n_past, 1)) return rc;
        int n_run = 1;
        for (int t = 0; t < ctx_rows(c); ++t) n_run = c->n_ctx - n_past[t] > n_run ? c->n_ctx - n_past[t] : n_run;
        n_steps = context_stop_truncate(n_steps, n_run, ctx_rows(c), out_tokens);
    } else if (const int rc = seqs_check(c, "decode_sample_seqs", first_tokens, n_past, n_steps)) return rc;
    if (c->n_seq == 0) return falcon_hip_decode_sample(c, first_tokens[0], n_past[0], n_steps, out_tokens);     // a context of one sequence
    return decode_loop(c, true, true, first_tokens, n_past, n_steps, out_tokens, "decode_sample_seqs");
}

// ------------------------------------------------------------------------------------------------ draft-and-verify decode (fq_spec.h)
// A pass evaluates the pending token and spec_K drafts as spec_K + 1 consecutive positions of the one cache (launch_stage's verify form), then ONE launch runs the
// sampler over the logits rows in order while each draw is the next row's draft, advances the position by the draws it made, and leaves the next pass's tokens.
static fq_spec_launch spec_launch_args(const falcon_hip_context * c) {
    return fq_spec_launch{ c->spec_state, c->spec_hist, c->n_ctx + 1, c->spec_guess, c->spec_drafts, c->tokens_dev, c->spec_K + 1, c->spec_source, c->spec_gmin, c->spec_gmax, c->n_ctx };
}
// the spec part of a pass's key: the settings among those arguments, and the first two of the buffers (all four are made at once and stay)
static void spec_step_key(const falcon_hip_context * c, int64_t key[3]) {
    key[0] = (int64_t) c->spec_K | ((int64_t) c->spec_source << 8) | ((int64_t) c->spec_gmin << 16) | ((int64_t) c->spec_gmax << 24);
    key[1] = key_ptr(c->spec_state); key[2] = key_ptr(c->spec_hist);
}
extern "C" int falcon_hip_context_set_spec(falcon_hip_context * c, int n_draft, int source, int ngram_min, int ngram_max, const int32_t * history, int n_history) {
    if (!c) return 1;
    hipStream_t st = fq_ctx().stream;
    if (n_draft == 0) {                                     // off: every entry launches what it launched before
        HIP_CHECK(hipStreamSynchronize(st));
        c->spec_step.drop();
        c->spec_K = 0;
        return 0;
    }
    if (c->n_seq > 0) { fprintf(stderr, "falcon-hip: set_spec: a lock-step context (%d sequences) has no draft-and-verify decode\n", c->n_seq); return 1; }
    if (!c->m->first_stage() || !c->m->last_stage()) { fprintf(stderr, "falcon-hip: set_spec: draft-and-verify decode needs the whole model in one process\n"); return 1; }
    if (n_draft < 1 || n_draft > FQ_SPEC_MAX_DRAFT) { fprintf(stderr, "falcon-hip: set_spec: %d drafts per pass (0: off, 1..%d)\n", n_draft, FQ_SPEC_MAX_DRAFT); return 1; }
    if (n_draft + 1 > c->n_batch) { fprintf(stderr, "falcon-hip: set_spec: a pass of %d rows does not fit n_batch %d\n", n_draft + 1, c->n_batch); return 1; }
    if (source != FQ_SPEC_LOOKUP && source != FQ_SPEC_GIVEN) { fprintf(stderr, "falcon-hip: set_spec: source %d (%d: lookup, %d: given)\n", source, FQ_SPEC_LOOKUP, FQ_SPEC_GIVEN); return 1; }
    if (source == FQ_SPEC_LOOKUP && (ngram_min < 1 || ngram_max < ngram_min || ngram_max > FQ_SPEC_MAX_NGRAM)) {
        fprintf(stderr, "falcon-hip: set_spec: n-grams %d..%d (1 <= min <= max <= %d)\n", ngram_min, ngram_max, FQ_SPEC_MAX_NGRAM);
        return 1;
    }
    if (n_history < 0 || n_history > c->n_ctx || (n_history > 0 && !history)) { fprintf(stderr, "falcon-hip: set_spec: a history of %d tokens (0..n_ctx %d)\n", n_history, c->n_ctx); return 1; }
    for (int i = 0; i < n_history; ++i) if (history[i] < 0 || history[i] >= c->m->hp.n_vocab) { fprintf(stderr, "falcon-hip: set_spec: history token %d is outside [0, %d)\n", history[i], c->m->hp.n_vocab); return 1; }
    if (c->sampler && fq_sampler_grammar_rows(c->sampler) > 0) { fprintf(stderr, "falcon-hip: set_spec: the sequence holds a grammar (falcon_hip_context_set_grammar) and a verify pass applies none: take it off first\n"); return 1; }
    if (c->lp_n_top >= 0) { fprintf(stderr, "falcon-hip: set_spec: log-probability records are on (falcon_hip_context_set_logprobs) and a verify pass records none: turn them off first\n"); return 1; }
    if (!fq_verify_attention_fits(c->n_ctx)) { fprintf(stderr, "falcon-hip: set_spec: n_ctx %d does not fit the verify attention's score row\n", c->n_ctx); return 1; }
    ggml_hip_sampler * sm = ctx_sampler(c);
    if (!sm) return 1;
    HIP_CHECK(hipStreamSynchronize(st));                    // (outside any capture; nothing in flight reads what follows)
    fq_sampler_spec_prepare(sm);
    if (!c->spec_state) {
        c->spec_state  = (fq_spec_state *) dev_alloc(c->allocs, sizeof(fq_spec_state) + 256);
        c->spec_hist   = (int32_t *) dev_alloc(c->allocs, ((size_t) c->n_ctx + 1) * 4 + 256);
        c->spec_guess  = (int32_t *) dev_alloc(c->allocs, (size_t) c->n_ctx * 4 + 256);
        c->spec_drafts = (int32_t *) dev_alloc(c->allocs, FQ_SPEC_MAX_DRAFT * 4 + 256);
        c->spec_poll_img.make(1);
    }
    fq_spec_state fresh;
    fq_spec_reset(&fresh);
    fresh.n_hist = source == FQ_SPEC_LOOKUP ? n_history : 0;
    HIP_CHECK(hipMemcpyAsync(c->spec_state, &fresh, sizeof fresh, hipMemcpyHostToDevice, st));
    if (fresh.n_hist > 0) HIP_CHECK(hipMemcpyAsync(c->spec_hist, history, (size_t) n_history * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(c->spec_drafts, 0xff, FQ_SPEC_MAX_DRAFT * 4, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (fresh is a local, the history the caller's)
    c->spec_K = n_draft; c->spec_source = source;
    c->spec_gmin = source == FQ_SPEC_LOOKUP ? ngram_min : 1; c->spec_gmax = source == FQ_SPEC_LOOKUP ? ngram_max : 1;
    return 0;
}

extern "C" int falcon_hip_context_set_spec_guess(falcon_hip_context * c, const int32_t * tokens, int n) {
    if (!c || c->spec_K < 1 || c->spec_source != FQ_SPEC_GIVEN) { fprintf(stderr, "falcon-hip: set_spec_guess: draft-and-verify decode with the given source is not on (falcon_hip_context_set_spec)\n"); return 1; }
    if (n < 0 || n > c->n_ctx || (n > 0 && !tokens)) { fprintf(stderr, "falcon-hip: set_spec_guess: a guess of %d tokens (0..n_ctx %d)\n", n, c->n_ctx); return 1; }
    for (int i = 0; i < n; ++i) if (tokens[i] < -1 || tokens[i] >= c->m->hp.n_vocab) { fprintf(stderr, "falcon-hip: set_spec_guess: token %d is outside [-1, %d)\n", tokens[i], c->m->hp.n_vocab); return 1; }
    hipStream_t st = fq_ctx().stream;
    const int32_t w[2] = { n, 0 };                          // n_guess, given_at: draw number 0 is the next one
    static_assert(offsetof(fq_spec_state, n_guess) == 4 && offsetof(fq_spec_state, given_at) == 8, "the guess's length and the draw's number are written as two words");
    if (n > 0) HIP_CHECK(hipMemcpyAsync(c->spec_guess, tokens, (size_t) n * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(&c->spec_state->n_guess, w, 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int falcon_hip_context_get_spec_stats(falcon_hip_context * c, int64_t * passes_out, int64_t * draws_out, int64_t * hist_out) {
    if (!c || !c->spec_state) { fprintf(stderr, "falcon-hip: get_spec_stats: draft-and-verify decode was never on\n"); return 1; }
    fq_spec_state h;
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemcpyAsync(&h, c->spec_state, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (passes_out) *passes_out = h.passes;
    if (draws_out) *draws_out = h.draws;
    if (hist_out) for (int i = 0; i <= FQ_SPEC_MAX_DRAFT; ++i) hist_out[i] = h.hist[i];
    return 0;
}

extern "C" int falcon_hip_decode_spec(falcon_hip_context * c, int32_t first_token, int n_past, int n_tokens, int32_t * out_tokens, int * n_out) {
    if (!c || c->spec_K < 1) { fprintf(stderr, "falcon-hip: decode_spec: draft-and-verify decode is not on (falcon_hip_context_set_spec)\n"); return 1; }
    falcon_hip_model * m = c->m;
    if (emb_refuses(c, "decode_spec")) return 1;
    if (!out_tokens || n_tokens < 1 || n_past < 0 || n_past >= c->n_ctx || first_token < 0 || first_token >= m->hp.n_vocab) {
        fprintf(stderr, "falcon-hip: decode_spec: token %d at n_past %d, %d tokens: needs a token of the vocabulary, 0 <= n_past < n_ctx (%d), n_tokens >= 1\n", first_token, n_past, n_tokens, c->n_ctx);
        return 1;
    }
    if (c->sync_err_sticky) { fprintf(stderr, "falcon-hip: decode_spec: an earlier step of this context lost an in-launch hand-off -- the context must be recreated\n"); return 3; }
    if (context_stop_on(c)) n_tokens = context_stop_truncate(n_tokens, c->n_ctx - n_past, 1, out_tokens);
    if (n_past + n_tokens > c->n_ctx) { fprintf(stderr, "falcon-hip: decode_spec: %d tokens from n_past %d run past n_ctx %d (falcon_hip_context_set_context_stop ends the row there instead)\n", n_tokens, n_past, c->n_ctx); return 1; }
    ggml_hip_sampler * sm = ctx_sampler(c);
    if (!sm) return 1;
    hipStream_t st = fq_ctx().stream;
    const int K = c->spec_K;
    int * steps = fq_sampler_steps(sm);
    int32_t * out_dev = c->out_tokens_dev;                   // [n_ctx]
    c->logits_fresh = false;
    const int32_t lw[2] = { n_tokens, 0 };                  // left, ended
    static_assert(offsetof(fq_spec_state, left) == 12 && offsetof(fq_spec_state, ended) == 16, "the call's budget and the end flag are written as two words");
    HIP_CHECK(hipMemcpyAsync(c->n_past_dev, &n_past, 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->tokens_dev, &first_token, 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(&c->spec_state->left, lw, 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(steps, 0, 4, st));
    HIP_CHECK(hipMemsetAsync(out_dev, 0xff, (size_t) n_tokens * 4, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (the words may live on the caller's stack)
    const fq_spec_launch sp = spec_launch_args(c);
    fq_launch_spec_draft(sp, st);                           // the first pass's drafts, from the history / the guess as they stand
    const keep_hidden_off no_hidden(c);
    auto one_pass = [&] {
        launch_stage(c, K + 1, c->n_ctx, st, 0, c->n_ctx);
        fq_launch_verify(sm, sp, c->logits_dev, m->hp.n_vocab, c->tokens_dev, c->n_past_dev, steps, out_dev, st);
    };
    step_key key = step_key_of(c);
    spec_step_key(c, key.spec);
    fq_sampler_step_key(sm, key.sampler);                   // (its grammar word is 0 here: set_spec and set_grammar refuse one another)
    const bool graph = c->use_graph && graph_ok_strict();
    // at most n_tokens passes (one draw each), fewer when the budget is spent or the row's stops end it: the state is polled as decode_loop polls the rows' stops
    // (run_polled), so at most two intervals of passes run past the end (they draw nothing: the verify launch leaves a row without budget, or ended, as it is)
    c->loop_steps = run_polled(n_tokens, c->stop_poll, true, c->spec_poll_img, (const fq_spec_state *) c->spec_state, st,
        [&] { if (graph) c->spec_step.replay(c, st, key, one_pass); else one_pass(); },
        [&](const fq_spec_state * s) { return s->left == 0 || s->ended != 0; });
    int drawn = 0;
    HIP_CHECK(hipMemcpyAsync(out_tokens, out_dev, (size_t) n_tokens * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&drawn, steps, 4, hipMemcpyDeviceToHost, st));
    fetch_sync_error(c, st);
    HIP_CHECK(hipStreamSynchronize(st));
    if (n_out) *n_out = drawn;
    c->last_rows = 1;
    c->lp_steps = 0;
    return report_sync_error(c, "decode_spec");
}
extern "C" int falcon_hip_context_set_context_stop(falcon_hip_context * c, int on) {
    int rc;
    ggml_hip_sampler * s = entry_sampler(c, "set_context_stop", &rc, !on);
    return s ? ggml_hip_sampler_set_context_stop(s, on ? c->n_ctx : 0) : rc;
}
extern "C" int falcon_hip_context_resume(falcon_hip_context * c, int seq) {
    if (!has_head(c, "resume")) return 1;
    if (!c->sampler) { fprintf(stderr, "falcon-hip: resume: sequence %d did not end at the end of its cache (the context never sampled)\n", seq); return 1; }
    return ggml_hip_sampler_resume(c->sampler, seq);
}
