// falcon_hip.hip -- device-resident Falcon decoder stack (include/falcon-hip.h).
//
// Op sequence = falcon_eval_internal (libfalcon.cpp:2115-2466), one launch list per block:
//   LN(x) [+ LN2(x) on 40B]  -> Q8 activations        (ggml_norm/mul/add 2166-2188; mul_mat INIT ggml.c:11462)
//   QKV = Wqkv . a                                     (2192)
//   RoPE(Q,K) neox + KV append                         (2229-2280)
//   att = softmax(mask(K.Q/8)) V, heads merged         (2285-2366)
//   wo  = Wo . q8(att)                                 (2370)
//   up  = gelu(Wup . a)                                (2389-2392)
//   x   = (Wdown . q8(up) + wo) + x                    (2394-2400)
// then ln_f + lm_head (2421-2440). Everything runs on the library stream; a decode step (N = 1) reads its token id
// and n_past from device memory, so one captured hipGraph is replayed for every generated token.
// This unit: the context, capture and replay, the mode switches, the eval entries, embeddings, logits and perplexity (falcon_ctx.h names the others).
#include "falcon_ctx.h"
#include <atomic>
#include <cmath>
using namespace fq_drv;

// k_attn_out hands the attention output from workgroup to workgroup with a BOUNDED spin; a time-out sets sync_words[1] and
// the launch carries on with whatever the granules hold. Wherever the host waits for the stream anyway the word comes
// along, and a set word fails the call (callers of the purely stream-ordered falcon_hip_stage_step poll
// falcon_hip_context_sync_error themselves).
void fq_drv::fetch_sync_error(falcon_hip_context * c, hipStream_t st) {
    HIP_CHECK(hipMemcpyAsync(&c->sync_err_host, c->sync_words + 1, 4, hipMemcpyDeviceToHost, st));
}
int fq_drv::report_sync_error(falcon_hip_context * c, const char * where) {
    if (!c->sync_err_host) return 0;
    c->sync_err_sticky = true;
    fprintf(stderr, "falcon-hip: %s: an in-launch hand-off timed out (sync word %u) -- the results of this call are invalid\n", where, c->sync_err_host);
    return 3;
}
// what every entry that reads logits or samples asks first (a pipeline stage other than the last holds no head)
bool fq_drv::has_head(const falcon_hip_context * c, const char * who) {
    if (c->m->last_stage()) return true;
    fprintf(stderr, "falcon-hip: %s: this context holds no lm_head\n", who);
    return false;
}

static void drop_graphs(falcon_hip_context * c) {             // every captured graph of the context
    for (step_slot * s : { &c->decode_step, &c->sample_step, &c->seqs_step, &c->sample_seqs_step, &c->token_step, &c->token_step_emb, &c->stage_step, &c->spec_step }) s->drop();
    for (step_slot & s : c->batch_steps) s.drop();
    c->batch_steps.clear();
}
extern "C" int falcon_hip_context_graph_captures(const falcon_hip_context * c) { return c->n_captures; }

static size_t act_col_bytes_max(int64_t K, bool f16 = false) {
    size_t b = fq_act_col_bytes(FQ_Q8_1, K), b0 = fq_act_col_bytes(FQ_Q8_0, K), bk = fq_act_col_bytes(FQ_Q8_K, K);
    if (b0 > b) b = b0;
    if (bk > b) b = bk;
    if (f16 && fq_f16_col_bytes(K) > b) b = fq_f16_col_bytes(K);      // (the fp16 image of F16 consumers: 2 bytes per element)
    return b;
}
static std::atomic<int> g_live_contexts{0};       // the ring forms' schedule tables are shared by every context of the process and released with the last one
// the ring forms' per-shape schedules (device tables) must exist before any launch is captured into a graph: legacy formats kernels_ring.hip, k-quants kernels_ringk.hip
// (one schedule per distinct (format, shape) of the stage's blocks -- not only block 0's: launchers look plans up without creating them, and a block of another format
// would silently take the register-streaming kernel)
static bool ring_prepare_any(const falcon_hip_model * m) {
    bool any = false; int seen[32]; int n_seen = 0;
    for (const layer_weights & L : m->layers) {
        const fq_weight & q = L.qkv;
        bool dup = false;
        for (int i = 0; i < n_seen; ++i) dup = dup || seen[i] == q.type;
        if (dup) continue;
        if (n_seen < 32) seen[n_seen++] = q.type;
        const bool ok = fq_ring_prepare(q.type, m->hp.n_embd, m->hp.n_ff, q.M, fq_ctx().n_cu) || fq_ringk_prepare(q.type, m->hp.n_embd, m->hp.n_ff, q.M, fq_ctx().n_cu);
        any = any || ok;
    }
    return any;
}

// the ring form of the unmerged output mat-vec launch (k_ring_out, one wave per row in chunks): measured on Falcon-40B against k_gemv_out with the fast k-quant
// dots -- Q2_K 234 -> 246 tok/s, Q3_K 188.5 -> 192, but Q4_K 198 -> 181, Q5_K 157 -> 146, Q6_K 153 -> 142: on by default for the two formats
// with 64-element units only
static bool ring_out_auto(const falcon_hip_model * m) {
    if (const char * e = getenv("FALCON_HIP_RING_OUT")) return atoi(e) != 0;
    if (m->layers.empty()) return false;
    const int t = m->layers[0].down.type;
    return t == FQ_Q2_K || t == FQ_Q3_K;
}

static falcon_hip_context * context_create(falcon_hip_model * m, int n_ctx, int n_batch, int rope_n_ctx, int n_seq) {
    const falcon_hip_hparams & hp = m->hp;
    for (size_t i = 0; i < m->layers.size(); ++i) {
        const layer_weights & L = m->layers[i];
        if (!L.qkv.plane[0] || !L.wo.plane[0] || !L.up.plane[0] || !L.down.plane[0] || !L.ln_w || !L.ln_b || (hp.two_norms && (!L.ln2_w || !L.ln2_b))) {
            fprintf(stderr, "falcon-hip: layer %d is missing tensors\n", hp.layer_begin + (int) i); exit(1);
        }
    }
    if (m->first_stage() && !m->tok_emb.plane[0]) { fprintf(stderr, "falcon-hip: missing word_embeddings\n"); exit(1); }
    if (m->last_stage() && (!m->lm_head.plane[0] || !m->out_norm_w || !m->out_norm_b)) { fprintf(stderr, "falcon-hip: missing ln_f / lm_head\n"); exit(1); }

    falcon_hip_context * c = new falcon_hip_context();
    c->m = m; c->n_ctx = n_ctx; c->n_batch = n_batch; c->rope_n_ctx = rope_n_ctx > 0 ? rope_n_ctx : n_ctx; c->n_seq = n_seq;
    const int64_t E = hp.n_embd, D = 64, QKV = (int64_t)(hp.n_head + 2 * hp.n_head_kv) * D, FF = hp.n_ff, B = n_batch;
    const int64_t nl = (int64_t) m->layers.size();
    c->x      = (float *) dev_alloc(c->allocs, (size_t) B * E * 4);
    c->ln     = (float *) dev_alloc(c->allocs, (size_t) B * E * 4);
    c->ln2    = (float *) dev_alloc(c->allocs, (size_t) B * E * 4);
    c->qkv    = (float *) dev_alloc(c->allocs, (size_t) B * QKV * 4);
    c->att    = (float *) dev_alloc(c->allocs, (size_t) B * E * 4);
    // score rows of the long-prompt attention forms, owned here and sized once (kernels.h): no launch of this context allocates
    c->att_scratch.bytes = n_seq > 0 ? 0 : fq_attention_scratch_need(n_batch, hp.n_head, n_ctx, hp.n_head_kv);
    c->att_scratch.p     = c->att_scratch.bytes ? (float *) dev_alloc(c->allocs, c->att_scratch.bytes) : nullptr;
    c->wo_out = (float *) dev_alloc(c->allocs, (size_t) B * E * 4);
    c->up     = (float *) dev_alloc(c->allocs, (size_t) B * FF * 4);
    if (m->last_stage()) c->logits_dev = (float *) dev_alloc(c->allocs, (size_t) B * hp.n_vocab * 4);
    const bool f16 = stage_has_f16(m);                               // (only then: a quantized model keeps the sizes it had)
    c->buf_e   = (uint8_t *) dev_alloc(c->allocs, act_col_bytes_max(E, f16) * (size_t) B + 256);
    c->buf_e2  = (uint8_t *) dev_alloc(c->allocs, act_col_bytes_max(E, f16) * (size_t) B + 256);
    c->buf_att = (uint8_t *) dev_alloc(c->allocs, act_col_bytes_max(E, f16) * (size_t) B + 256);
    c->buf_ff  = (uint8_t *) dev_alloc(c->allocs, act_col_bytes_max(FF, f16) * (size_t) B + 256);
    const size_t kvb = (size_t) nl * (n_seq > 0 ? n_seq : 1) * n_ctx * hp.n_head_kv * D * 4;
    c->k_cache = (float *) dev_alloc(c->allocs, kvb);
    c->v_cache = (float *) dev_alloc(c->allocs, kvb);
    HIP_CHECK(hipMemset(c->k_cache, 0, kvb ? kvb : 16));
    HIP_CHECK(hipMemset(c->v_cache, 0, kvb ? kvb : 16));
    {
        std::vector<float> cs = fq_rope_table_host((int) D, n_ctx, c->rope_n_ctx);
        c->rope_cs = (float *) dev_alloc(c->allocs, cs.size() * 4);
        HIP_CHECK(hipMemcpy(c->rope_cs, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
    }
    c->n_past_dev     = (int *) dev_alloc(c->allocs, 256);
    c->tokens_dev     = (int32_t *) dev_alloc(c->allocs, (size_t) B * 4 + 256);
    c->out_tokens_dev = (int32_t *) dev_alloc(c->allocs, (size_t) n_ctx * 4 + 256);
    HIP_CHECK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    c->ev_fork.resize((size_t) nl); c->ev_join.resize((size_t) nl); c->ev_attn.resize((size_t) nl);
    for (int64_t i = 0; i < nl; ++i) { HIP_CHECK(hipEventCreateWithFlags(&c->ev_fork[i], hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&c->ev_attn[i], hipEventDisableTiming)); }
    if (const char * e = getenv("FALCON_HIP_PAR2_MAX_N")) c->par2_max_n = atoi(e);
    if (const char * e = getenv("FALCON_HIP_DUAL")) c->dual_stream = atoi(e) != 0;
    c->argmax_val     = (float *) dev_alloc(c->allocs, (size_t)(hp.n_vocab / 32 + 8) * 4);
    c->argmax_idx     = (int *) dev_alloc(c->allocs, (size_t)(hp.n_vocab / 32 + 8) * 4);
    c->sync_words     = (unsigned *) dev_alloc(c->allocs, 64 + 256);        // + the rope table row of the current position
    HIP_CHECK(hipMemset(c->sync_words, 0, 64 + 256));
    c->att_gran       = (unsigned long long *) dev_alloc(c->allocs, (size_t) hp.n_embd * 8 + 64);
    HIP_CHECK(hipMemset(c->att_gran, 0, (size_t) hp.n_embd * 8 + 64));
    c->x_gran         = (unsigned long long *) dev_alloc(c->allocs, (size_t) hp.n_embd * 8 + 64);
    HIP_CHECK(hipMemset(c->x_gran, 0, (size_t) hp.n_embd * 8 + 64));
    if (const char * e = getenv("FALCON_HIP_TWO_PHASE")) c->two_phase = atoi(e) != 0;
    if (const char * e = getenv("FALCON_HIP_STAGE_GRAPH")) c->stage_graph = atoi(e) != 0;
    c->ring_ln = !(getenv("FALCON_HIP_RING") && atoi(getenv("FALCON_HIP_RING")) == 0);      // (default on: a context starts in mode 2)
    if (const char * e = getenv("FALCON_HIP_PREFILL_GRAPH")) c->prefill_graph = atoi(e) != 0;
    ++g_live_contexts;
    if (c->ring_ln && nl > 0) c->ring_ln = ring_prepare_any(m);
    c->ring_out = ring_out_auto(m);
    if (const char * e = getenv("FALCON_HIP_MERGED")) c->merged_attn_out = atoi(e) != 0;
    return c;
}

extern "C" falcon_hip_context * falcon_hip_context_create(falcon_hip_model * m, int n_ctx, int n_batch, int rope_n_ctx) {
    return context_create(m, n_ctx, n_batch, rope_n_ctx, 0);
}
extern "C" falcon_hip_context * falcon_hip_context_create_seqs(falcon_hip_model * m, int n_ctx, int n_seq, int rope_n_ctx) {
    if (n_seq < 1 || n_seq > 256) { fprintf(stderr, "falcon-hip: a lock-step context holds 1..256 sequences, not %d\n", n_seq); return nullptr; }
    return context_create(m, n_ctx, n_seq, rope_n_ctx, n_seq > 1 ? n_seq : 0);
}
extern "C" int falcon_hip_context_n_seq(const falcon_hip_context * c) { return c->n_seq > 0 ? c->n_seq : 1; }

extern "C" void falcon_hip_context_free(falcon_hip_context * c) {
    if (!c) return;
    if (c->swap_ctx) { falcon_hip_context_free(c->swap_ctx); c->swap_ctx = nullptr; }
    if (--g_live_contexts == 0) { HIP_CHECK(hipStreamSynchronize(fq_ctx().stream)); fq_ring_free_plans(); fq_ringk_free_plans(); }
    drop_graphs(c);
    if (c->sampler) ggml_hip_sampler_free(c->sampler);
    for (hipEvent_t e : c->ev_fork) HIP_CHECK(hipEventDestroy(e));
    for (hipEvent_t e : c->ev_join) HIP_CHECK(hipEventDestroy(e));
    for (hipEvent_t e : c->ev_attn) HIP_CHECK(hipEventDestroy(e));
    if (c->side) HIP_CHECK(hipStreamDestroy(c->side));
    for (void * p : c->allocs) HIP_CHECK(hipFree(p));
    delete c;                                               // (what later calls made -- dev_buf, pinned_buf, polled_images -- goes with it)
}

extern "C" void falcon_hip_context_keep_hidden(falcon_hip_context * c, int keep) {
    c->keep_hidden = keep != 0;
    if (keep && !c->hidden_dev)
        c->hidden_dev = (float *) dev_alloc(c->allocs, (size_t)(c->m->layers.size() + 1) * c->n_batch * c->m->hp.n_embd * 4);
}
extern "C" void falcon_hip_get_hidden(falcon_hip_context * c, float * dst) {
    HIP_CHECK(hipStreamSynchronize(fq_ctx().stream));
    HIP_CHECK(hipMemcpy(dst, c->hidden_dev, (size_t)(c->m->layers.size() + 1) * c->hidden_tokens * c->m->hp.n_embd * 4, hipMemcpyDeviceToHost));
}
extern "C" void falcon_hip_context_use_graph(falcon_hip_context * c, int enable) { c->use_graph = enable != 0; }
extern "C" int falcon_hip_context_sync_error(falcon_hip_context * c) {      // 1 if a k_attn_out poll ever timed out (results invalid)
    unsigned w[2] = {0, 0};
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(w, c->sync_words, sizeof w, hipMemcpyDeviceToHost));
    return (int) w[1];
}
extern "C" void falcon_hip_context_set_fused(falcon_hip_context * c, int mode) {      // 0 op list, 1 three launches per block, 2 two (default), 3 one (two-phase), 5 two with the ring form forced; 4 was the persistent engine (removed in round 6, NOTEBOOK section 4): now the default form
    drop_graphs(c);
    c->fused_decode = mode != 0;
    c->merged_attn_out = mode >= 2;
    if (mode == 4) mode = 2;
    c->two_phase = mode == 3;
    // the LayerNorm mat-vec launch in the ring form (kernels_ring.hip): mode 5 always, mode 2 unless FALCON_HIP_RING=0 (measured +1.6 % on
    // Falcon-7B Q4_0; legacy formats only, other models keep k_gemv_ln)
    static const bool ring_default = !(getenv("FALCON_HIP_RING") && atoi(getenv("FALCON_HIP_RING")) == 0);
    c->ring_ln = (mode == 5 || (mode == 2 && ring_default)) && !c->m->layers.empty() && ring_prepare_any(c->m);
    c->ring_out = mode == 5 || (mode == 2 && ring_out_auto(c->m));
}

// the context's own modes that select a launch list: the first word of every step_key (a step_slot re-captures when it differs)
static int graph_signature(const falcon_hip_context * c) {
    return (stage_fused(c) ? 1 : 0) | (fq_reference_order() ? 2 : 0) | (fq_attn_f64() ? 4 : 0) | (c->merged_attn_out ? 8 : 0) |
           (c->two_phase ? 16 : 0) | (c->dual_stream ? 32 : 0) | (stage_fused_ref(c) ? 128 : 0) |
           (c->emb_mode << 16) | (c->emb_mode && c->emb_no_head ? 1 << 18 : 0);      // (embeddings off: the value it always had)
}
// ... and the whole key: the signature alone is the same in reference orders 1 and 2 and before and after ggml_hip_debug_force_gemv /
// ggml_hip_debug_gemm_mode, whose launch lists differ -- the epoch moves with every such switch
step_key fq_drv::step_key_of(const falcon_hip_context * c) {
    step_key k;
    k.sig = graph_signature(c); k.epoch = fq_config_epoch();
    return k;
}

// ---- which calls replay a captured step (side by side; the differences are historical and kept as they are)
// the decode attention keeps a score row of max_n_kv floats in LDS; a captured step is sized for the whole context (its position is read
// from device memory), so contexts longer than that buffer allows run their single-token steps as plain launches sized for n_past + 1
static bool fused_graph_fits(const falcon_hip_context * c) { return fq_attn_decode_lds_bytes(c->n_ctx) <= 160 * 1024; }
// no replay under the profiler's brackets or the phase stamps, nor in reference order 1
bool fq_drv::graph_ok_strict() { return !fq_prof_active() && !fq_ctx().dbg_stamps && (!fq_reference_order() || fq_reference_fast()); }
// falcon_hip_decode_greedy / _sample: NOT strict -- they replay under the profiler, the stamps and order 1 whenever the caller asked for the graph.
// Neither NOTEBOOK nor the commit history records a reason for the difference; it is kept, not endorsed
bool fq_drv::graph_ok_loop(const falcon_hip_context * c)    { return c->use_graph && fused_graph_fits(c); }
bool fq_drv::graph_ok_seqs(const falcon_hip_context * c)    { return c->use_graph && fused_graph_fits(c) && graph_ok_strict(); }      // falcon_hip_decode_greedy_seqs / _sample_seqs
static bool graph_ok_token(const falcon_hip_context * c)      { return stage_fused(c) && fused_graph_fits(c) && graph_ok_strict(); }     // falcon_hip_eval_token: no opt-in, fused steps only
bool fq_drv::graph_ok_stage_step(const falcon_hip_context * c) { return c->stage_graph && !fq_prof_active() && !fq_ctx().dbg_stamps && fused_graph_fits(c); }      // falcon_hip_stage_step: order 1 replays too
static bool graph_ok_batch(const falcon_hip_context * c, int N) {                                                                        // eval_stage_impl's batches (FALCON_HIP_PREFILL_GRAPH=1)
    return c->prefill_graph && N > 4 && c->n_seq == 0 && !fq_tl_collecting() && graph_ok_strict();
}

// ------------------------------------------------------------------------------------------------ one eval
// score_targets (falcon_hip_eval_score): the logits stay on the device, score_out[r] = the soft-max probability of score_targets[r] >= 0
static int eval_stage_impl(falcon_hip_context * c, const int32_t * tokens, const float * hidden_in_dev, int N,
                           int n_past, int logits_all, float * hidden_out_dev, const int32_t * score_targets, float * score_out) {
    hip_context & hc = fq_ctx();
    falcon_hip_model * m = c->m;
    const int adv = c->n_seq > 0 ? 1 : N;                            // lock-step sequences: N rows = one position of each of N sequences
    if (N < 1 || N > c->n_batch || n_past < 0 || n_past + adv > c->n_ctx || (m->first_stage() && !tokens) || (!m->first_stage() && !hidden_in_dev)) {
        fprintf(stderr, "falcon-hip: eval of %d tokens at n_past %d: needs 1 <= n_tokens <= n_batch (%d), n_past + n_tokens <= n_ctx (%d) and its input\n", N, n_past, c->n_batch, c->n_ctx);
        return 1;                                                    // (falcon_eval's convention: non-zero = failed to eval, libfalcon.cpp:4588-4591)
    }
    if (m->first_stage()) {
        for (int i = 0; i < N; ++i) if (tokens[i] < 0 || tokens[i] >= m->hp.n_vocab) {
            fprintf(stderr, "falcon-hip: token id %d at position %d is outside [0, %d)\n", tokens[i], i, m->hp.n_vocab);
            return 2;
        }
    }
    if (c->sync_err_sticky) { fprintf(stderr, "falcon-hip: eval: an earlier step of this context lost an in-launch hand-off -- its KV cache is invalid, the context must be recreated\n"); return 3; }
    hipStream_t st = hc.stream;
    c->logits_pending = false;
    c->logits_last = nullptr;
    c->logits_none = score_targets != nullptr;
    c->logits_fresh = false;
    HIP_CHECK(hipMemcpyAsync(c->n_past_dev, &n_past, 4, hipMemcpyHostToDevice, st));
    if (score_targets) {
        if (!c->score_tgt.get()) { c->score_tgt.reset((size_t) c->n_batch); c->score_prob.reset((size_t) c->n_batch); }
        HIP_CHECK(hipMemcpyAsync(c->score_tgt.get(), score_targets, (size_t) N * 4, hipMemcpyHostToDevice, st));
    }
    if (m->first_stage()) HIP_CHECK(hipMemcpyAsync(c->tokens_dev, tokens, (size_t) N * 4, hipMemcpyHostToDevice, st));
    else                  HIP_CHECK(hipMemcpyAsync(c->x, hidden_in_dev, (size_t) N * m->hp.n_embd * 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));        // n_past / tokens may live on the caller's stack
    // batches: one hipGraph replay per (size, keys) instead of ~10 launches and 3 cross-stream joins per block from the host
    if (graph_ok_batch(c, N)) {
        step_key key = step_key_of(c);
        key.batch = { N, n_past + adv, c->keep_hidden };
        step_slot * slot = nullptr;
        for (step_slot & s : c->batch_steps) if (s.holds(key)) slot = &s;
        if (!slot) {                                                // a new shape: its own slot, the oldest of 8 makes room
            if (c->batch_steps.size() >= 8) { c->batch_steps.front().drop(); c->batch_steps.erase(c->batch_steps.begin()); }
            c->batch_steps.emplace_back();
            slot = &c->batch_steps.back();
        }
        slot->replay(c, st, key, [&] { launch_stage(c, N, n_past + adv, st); });
        if (c->keep_hidden) c->hidden_tokens = N;                  // (host-side state that launch_stage sets when it runs)
    } else {
        launch_stage(c, N, n_past + adv, st);
    }
    if (c->emb_mode) { c->emb_have = true; c->emb_host_fresh = false; }
    if (c->emb_mode && c->emb_no_head) {                             // falcon_hip_embed: no lm_head ran, no logits exist
        c->logits_none = true;
        fetch_sync_error(c, st);
        HIP_CHECK(hipStreamSynchronize(st));
        return report_sync_error(c, "embed");
    }
    if (m->last_stage()) {
        const int64_t V = m->hp.n_vocab;
        c->last_rows = N;
        if (score_targets) {                                                             // n_tokens floats come back, no logits
            fq_launch_score(c->logits_dev, V, N, (int) V, c->score_tgt.get(), c->score_prob.get(), nullptr, nullptr, st);
            c->score_host.resize((size_t) N);
            HIP_CHECK(hipMemcpyAsync(c->score_host.data(), c->score_prob.get(), (size_t) N * 4, hipMemcpyDeviceToHost, st));
        } else if (logits_all) {
            c->logits_host.resize((size_t) N * V);
            HIP_CHECK(hipMemcpyAsync(c->logits_host.data(), c->logits_dev, (size_t) N * V * 4, hipMemcpyDeviceToHost, st));
        } else {                                                                         // libfalcon.cpp:2545-2547
            c->logits_host.resize((size_t) V);
            HIP_CHECK(hipMemcpyAsync(c->logits_host.data(), c->logits_dev + (size_t)(N - 1) * V, (size_t) V * 4, hipMemcpyDeviceToHost, st));
        }
        fetch_sync_error(c, st);
        HIP_CHECK(hipStreamSynchronize(st));
        c->logits_fresh = !score_targets;
        if (score_targets) for (int r = 0; r < N; ++r) if (score_targets[r] >= 0) score_out[r] = c->score_host[r];
        return report_sync_error(c, "eval");
    } else if (hidden_out_dev) {
        HIP_CHECK(hipMemcpyAsync(hidden_out_dev, c->x, (size_t) N * m->hp.n_embd * 4, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

extern "C" int falcon_hip_eval_stage(falcon_hip_context * c, const int32_t * tokens, const float * hidden_in_dev, int N,
                                     int n_past, int logits_all, float * hidden_out_dev) {
    return eval_stage_impl(c, tokens, hidden_in_dev, N, n_past, logits_all, hidden_out_dev, nullptr, nullptr);
}

extern "C" int falcon_hip_eval(falcon_hip_context * c, const int32_t * tokens, int n_tokens, int n_past, int logits_all) {
    if (!c->m->first_stage() || !c->m->last_stage()) { fprintf(stderr, "falcon-hip: falcon_hip_eval needs the whole model in one process\n"); exit(1); }
    return falcon_hip_eval_stage(c, tokens, nullptr, n_tokens, n_past, logits_all, nullptr);
}

// falcon_hip_eval with the per-launch timing table printed on stderr afterwards (kernels.h fq_tl_*): the resident path's counterpart of the reference's
// --debug-timings node table (libfalcon.cpp:2506-2520 -> ggml_graph_print_impl, ggml.c:18266-18360). Plain launches (no graph replay), one synchronisation at the end.
extern "C" int falcon_hip_eval_debug_timings(falcon_hip_context * c, const int32_t * tokens, int n_tokens, int n_past, int logits_all) {
    fq_tl_begin();
    const int rc = falcon_hip_eval(c, tokens, n_tokens, n_past, logits_all);
    char title[160];
    snprintf(title, sizeof(title), "falcon-hip: launches of this eval (%d token%s at n_past %d; device-resident path, no ggml graph: one line per launch site)", n_tokens, n_tokens == 1 ? "" : "s", n_past);
    fq_tl_end(stderr, title);
    return rc;
}

// falcon_hip_eval with the reference's scoring arithmetic (falcon_perplexity.cpp:12-27, csrc/fq_score.h) as the call's last launch: every row's logits
// stay in HBM, n_tokens probabilities come back. What the host would compute from falcon_hip_eval(..., 1) + falcon_hip_get_logits, bit for bit.
extern "C" int falcon_hip_eval_score(falcon_hip_context * c, const int32_t * tokens, int n_tokens, int n_past, const int32_t * targets, float * probs_out) {
    if (!has_head(c, "eval_score")) return 1;
    if (!c->m->first_stage() || c->n_seq > 0) { fprintf(stderr, "falcon-hip: eval_score needs the whole model in one process and a single sequence\n"); return 1; }
    if (!targets || !probs_out) { fprintf(stderr, "falcon-hip: eval_score: needs targets and probs_out\n"); return 1; }
    for (int i = 0; i < n_tokens; ++i) if (targets[i] >= c->m->hp.n_vocab) {
        fprintf(stderr, "falcon-hip: eval_score: target id %d at position %d is outside [0, %d)\n", targets[i], i, c->m->hp.n_vocab);
        return 2;
    }
    return eval_stage_impl(c, tokens, nullptr, n_tokens, n_past, 1, nullptr, targets, probs_out);
}

// ------------------------------------------------------------------------------------------------ embeddings (include/falcon-hip.h)
// The reference keeps the ln_f row of the last evaluated token when its context was made with params.embedding (libfalcon.cpp:2409-2435, 2551-2557). The
// row exists in every eval here as well -- the head's LayerNorm launch computes it on the way to lm_head's activation image -- and a set mode makes
// launch_stage keep it. Mode 0: not one launch, buffer or graph key differs from a context that never heard of embeddings.
static bool model_row_split(const falcon_hip_model * m) {
    if (m->lm_head.form_M > 0) return true;
    for (const layer_weights & L : m->layers) if (L.qkv.form_M > 0 || L.wo.form_M > 0 || L.up.form_M > 0 || L.down.form_M > 0) return true;
    return false;
}
extern "C" int falcon_hip_context_set_embedding(falcon_hip_context * c, int mode) {
    falcon_hip_model * m = c->m;
    if (mode & ~(FALCON_HIP_EMBED_LAST | FALCON_HIP_EMBED_POOL)) { fprintf(stderr, "falcon-hip: set_embedding: mode %d has bits other than 1 (last row) and 2 (pool)\n", mode); return 1; }
    if (mode && c->n_seq > 0) { fprintf(stderr, "falcon-hip: set_embedding: a lock-step context of %d sequences keeps no embedding (a plain context does)\n", c->n_seq); return 1; }
    if (mode && (!m->first_stage() || !m->last_stage())) { fprintf(stderr, "falcon-hip: set_embedding: a pipeline stage holds part of the layers; the embedding needs all of them and ln_f\n"); return 1; }
    if (mode && model_row_split(m)) { fprintf(stderr, "falcon-hip: set_embedding: row-split models keep no embedding\n"); return 1; }
    if (mode && !c->emb) {
        const size_t E = (size_t) m->hp.n_embd;
        c->emb_rows   = (float *) dev_alloc(c->allocs, (size_t) c->n_batch * E * 4);
        c->emb        = (float *) dev_alloc(c->allocs, E * 4);
        c->pool_acc   = (double *) dev_alloc(c->allocs, (E + 1) * 8);
        c->pool_count = (long long *) dev_alloc(c->allocs, 8);
        c->pool_out   = (float *) dev_alloc(c->allocs, E * 4);
        HIP_CHECK(hipMemset(c->pool_acc, 0, (E + 1) * 8));
        HIP_CHECK(hipMemset(c->pool_count, 0, 8));
    }
    if (mode && !c->emb_mode) {                                      // switched on: the reference's vector before its first eval, n_embd zeros, and no row to hand out
        HIP_CHECK(hipMemsetAsync(c->emb, 0, (size_t) m->hp.n_embd * 4, fq_ctx().stream));
        c->emb_have = false; c->emb_host_fresh = false;
    }
    c->emb_mode = mode;                                              // (the captured steps carry the mode in their keys: nothing to drop)
    return 0;
}
bool fq_drv::emb_refuses(const falcon_hip_context * c, const char * what) {
    if (!c || !c->emb_mode) return false;
    fprintf(stderr, "falcon-hip: %s: refused while an embedding mode is set (falcon_hip_context_set_embedding(c, 0) first): only falcon_hip_eval, _eval_score and _embed keep the row\n", what);
    return true;
}
extern "C" const float * falcon_hip_get_embeddings(falcon_hip_context * c) {
    if (!(c->emb_mode & FALCON_HIP_EMBED_LAST) || !c->emb_have) return nullptr;
    if (!c->emb_host_fresh) {
        hipStream_t st = fq_ctx().stream;
        c->emb_host.resize((size_t) c->m->hp.n_embd);
        HIP_CHECK(hipMemcpyAsync(c->emb_host.data(), c->emb, c->emb_host.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        c->emb_host_fresh = true;
    }
    return c->emb_host.data();
}
extern "C" int falcon_hip_embed(falcon_hip_context * c, const int32_t * tokens, int n_tokens, int n_past) {
    if (!c->emb_mode) { fprintf(stderr, "falcon-hip: embed: no embedding mode is set (falcon_hip_context_set_embedding)\n"); return 1; }
    c->emb_no_head = true;
    const int rc = eval_stage_impl(c, tokens, nullptr, n_tokens, n_past, 0, nullptr, nullptr, nullptr);
    c->emb_no_head = false;
    return rc;
}
extern "C" int falcon_hip_embedding_pool_reset(falcon_hip_context * c) {
    if (!c->pool_acc) return 0;                                      // (nothing was ever pooled)
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemsetAsync(c->pool_acc, 0, ((size_t) c->m->hp.n_embd + 1) * 8, st));
    HIP_CHECK(hipMemsetAsync(c->pool_count, 0, 8, st));
    return 0;
}
extern "C" int64_t falcon_hip_embedding_pool_count(const falcon_hip_context * c) {
    if (!c->pool_count) return 0;
    long long n = 0;
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemcpyAsync(&n, c->pool_count, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return (int64_t) n;
}
extern "C" int falcon_hip_get_embedding_pooled(falcon_hip_context * c, int normalize, float * out) {
    if (!(c->emb_mode & FALCON_HIP_EMBED_POOL) || !out) { fprintf(stderr, "falcon-hip: get_embedding_pooled: pooling is not on (falcon_hip_context_set_embedding with bit 1), or no destination\n"); return 3; }
    hipStream_t st = fq_ctx().stream;
    const int E = c->m->hp.n_embd;
    if (const int rc = fq_embed_pool_finish_checked(c->pool_acc, c->pool_count, E, normalize, c->pool_out, c->pool_acc + E, st)) return rc;
    HIP_CHECK(hipMemcpyAsync(out, c->pool_out, (size_t) E * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" const float * falcon_hip_get_logits(falcon_hip_context * c) {
    if (c->logits_none) return nullptr;
    if (c->logits_pending) {                                         // the last falcon_hip_eval_token's row copy (page-locked memory) is in flight behind its launches
        // (polled, not slept on: the caller samples the moment the row is there, and a blocking wait's wake-up costs tens of microseconds of a ~1 ms step)
        hipStream_t st = fq_ctx().stream;
        // bounded: ~20 ms of polling (a step is ~1 ms), then a blocking wait -- a stream that hangs must not burn a host core for ever
        bool done = false;
        for (int spin = 0; spin < 200000 && !done; ++spin) {
            const hipError_t e = hipStreamQuery(st);
            if (e == hipSuccess) done = true; else if (e != hipErrorNotReady) HIP_CHECK(e); else __builtin_ia32_pause();
        }
        if (!done) HIP_CHECK(hipStreamSynchronize(st));
        c->sync_err_host = *(const unsigned *)(c->logits_pinned.get() + c->m->hp.n_vocab);
        c->logits_pending = false;
        (void) report_sync_error(c, "eval");                        // sticky: falcon_hip_context_last_error / the next eval report it (this call cannot)
    }
    return c->logits_last ? c->logits_last : c->logits_host.data();
}
// 0, or 3 when a step of this context lost an in-launch hand-off (every result since is invalid). Host state only: callers of
// falcon_hip_get_logits, which cannot fail, ask here after it.
extern "C" int falcon_hip_context_last_error(const falcon_hip_context * c) { return c->sync_err_sticky ? 3 : 0; }

__global__ void k_set2_i32(int * p, int v, int * q, int w) { *p = v; *q = w; }
// One token at n_past (falcon_eval with n_tokens = 1, libfalcon.cpp:4566), asynchronous: the fused decode launches are replayed
// from a hipGraph (captured on first use, position read from device memory) and the logits row's copy into page-locked host memory is
// enqueued right behind them; the host does not wait -- falcon_hip_get_logits does, when (and only when) the caller asks for the row.
// Returns 0, 1 / 2 as falcon_hip_eval, or 3 once an earlier asynchronous step of this context has lost a hand-off.
extern "C" int falcon_hip_eval_token(falcon_hip_context * c, int32_t token, int n_past) {
    hip_context & hc = fq_ctx();
    falcon_hip_model * m = c->m;
    if (!m->first_stage() || !m->last_stage() || c->n_seq > 0) { fprintf(stderr, "falcon-hip: falcon_hip_eval_token needs the whole model in one process and a single sequence\n"); exit(1); }
    if (c->sync_err_sticky) { fprintf(stderr, "falcon-hip: eval: an earlier step of this context lost an in-launch hand-off -- its KV cache is invalid, the context must be recreated\n"); return 3; }
    if (n_past < 0 || n_past + 1 > c->n_ctx) { fprintf(stderr, "falcon-hip: eval of one token at n_past %d exceeds n_ctx %d\n", n_past, c->n_ctx); return 1; }
    if (token < 0 || token >= m->hp.n_vocab) { fprintf(stderr, "falcon-hip: token id %d is outside [0, %d)\n", token, m->hp.n_vocab); return 2; }
    hipStream_t st = hc.stream;
    if (c->logits_pending) {                                         // a row nobody asked for: its copy must land before the next one is enqueued into the same buffer
        HIP_CHECK(hipStreamSynchronize(st));
        c->sync_err_host = *(const unsigned *)(c->logits_pinned.get() + m->hp.n_vocab);
        c->logits_pending = false;
        if (report_sync_error(c, "eval")) return 3;
    }
    if (!c->logits_pinned.get()) c->logits_pinned.reset((size_t) m->hp.n_vocab + 16);      // (+ the hand-off error word: a copy into pageable memory would make this call wait for the whole step)
    hipLaunchKernelGGL(k_set2_i32, dim3(1), dim3(1), 0, st, c->n_past_dev, n_past, (int *) c->tokens_dev, (int) token);
    const keep_hidden_off no_hidden(c);
    if (graph_ok_token(c)) {
        (c->emb_mode ? c->token_step_emb : c->token_step).replay(c, st, step_key_of(c), [&] { launch_stage(c, 1, c->n_ctx, st); });
    } else {
        launch_stage(c, 1, n_past + 1, st);
    }
    if (c->emb_mode) { c->emb_have = true; c->emb_host_fresh = false; }
    HIP_CHECK(hipMemcpyAsync(c->logits_pinned.get(), c->logits_dev, (size_t) m->hp.n_vocab * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(c->logits_pinned.get() + m->hp.n_vocab, c->sync_words + 1, 4, hipMemcpyDeviceToHost, st));
    c->logits_last = c->logits_pinned.get();
    c->logits_none = false;
    c->logits_pending = true;
    c->logits_fresh = true;
    c->last_rows = 1;
    return 0;
}

// The n_ctx handed to ggml_rope may change from call to call (falcon_evaluation_config::n_max_real_ctx, libfalcon.cpp:2229-2230):
// the NTK factor only depends on n_ctx / 2048 (ggml.c:12880-12887), so the table is rebuilt -- in place, after the stream has
// drained -- only when that bucket changes.
extern "C" void falcon_hip_context_set_rope_n_ctx(falcon_hip_context * c, int rope_n_ctx) {
    if (rope_n_ctx <= 0) rope_n_ctx = c->n_ctx;
    const int old_b = c->rope_n_ctx >= 2048 ? c->rope_n_ctx / 2048 : 0, new_b = rope_n_ctx >= 2048 ? rope_n_ctx / 2048 : 0;
    c->rope_n_ctx = rope_n_ctx;
    if (old_b == new_b || !c->rope_cs) return;
    HIP_CHECK(hipStreamSynchronize(fq_ctx().stream));
    const std::vector<float> cs = fq_rope_table_host(64, c->n_ctx, rope_n_ctx);
    HIP_CHECK(hipMemcpy(c->rope_cs, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
}

// ------------------------------------------------------------------------------------------------ perplexity
// The reference's perplexity loop (examples/falcon_perplexity/falcon_perplexity.cpp:28-124), same chunking and the same
// host arithmetic: the token stream is cut into chunks of n_ctx tokens, each chunk is evaluated from an empty context in
// batches of n_batch (logits of every position), and the negative log-likelihood of token j+1 is added for
// j in [min(512, n_ctx/2), n_ctx-1) with soft_max as in :12-27 (float expf of logit - max, double sum, float division).
// Returns the number of scored tokens; *nll_out = their summed NLL (perplexity = exp(nll / count)).
extern "C" int falcon_hip_perplexity(falcon_hip_context * c, const int32_t * tokens, int64_t n_tokens, int n_ctx, int n_batch, double * nll_out) {
    if (emb_refuses(c, "perplexity")) return -1;
    if (n_ctx < 2 || n_ctx > c->n_ctx || n_batch < 1 || n_batch > c->n_batch) {
        fprintf(stderr, "falcon-hip: perplexity: n_ctx %d / n_batch %d exceed the context's (%d / %d)\n", n_ctx, n_batch, c->n_ctx, c->n_batch); exit(1);
    }
    const int64_t n_chunk = n_tokens / n_ctx;
    const int V = c->m->hp.n_vocab;
    for (int64_t i = 0; i < n_chunk * n_ctx; ++i) if (tokens[i] < 0 || tokens[i] >= V) {
        fprintf(stderr, "falcon-hip: perplexity: token id %d at position %lld is outside [0, %d)\n", tokens[i], (long long) i, V);
        return -1;
    }
    double nll = 0.0; int count = 0;
    const int first = 512 < n_ctx / 2 ? 512 : n_ctx / 2;              // positions [first, n_ctx - 1) of a chunk are scored
    std::vector<int32_t> targets((size_t) n_batch);
    std::vector<float> probs((size_t) n_batch);
    for (int64_t i = 0; i < n_chunk; ++i) {
        const int64_t start = i * n_ctx, end = start + n_ctx;
        const int num_batches = (n_ctx + n_batch - 1) / n_batch;
        for (int j = 0; j < num_batches; ++j) {
            const int64_t batch_start = start + (int64_t) j * n_batch;
            const int batch_size = (int)(end - batch_start < n_batch ? end - batch_start : n_batch);
            for (int r = 0; r < batch_size; ++r) {
                const int pos = j * n_batch + r;
                targets[r] = pos >= first && pos < n_ctx - 1 ? tokens[start + pos + 1] : -1;
            }
            if (falcon_hip_eval_score(c, tokens + batch_start, batch_size, j * n_batch, targets.data(), probs.data())) return -1;
            for (int r = 0; r < batch_size; ++r) if (targets[r] >= 0) { nll += -std::log(probs[r]); ++count; }      // position order
        }
    }
    if (nll_out) *nll_out = nll;
    return count;
}

