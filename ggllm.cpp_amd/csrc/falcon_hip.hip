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
#include "fq_device.h"
#include "kernels.h"
#include "hip_context.h"
#include "fq_f16.h"
#include "fq_stop.h"
#include "fq_spec.h"
#include "fq_ctx_swap.h"
#include "fq_sample.h"
#include "fq_session.h"
#include "fq_lora.h"
#include "fq_lora_base.h"
#include "../../include/falcon-hip.h"
#include <cmath>
#include <cstring>

#include <string>
#include <string.h>
#include <vector>
#include <atomic>

struct layer_weights {
    fq_weight qkv{}, wo{}, up{}, down{};
    float * ln_w = nullptr, * ln_b = nullptr, * ln2_w = nullptr, * ln2_b = nullptr;
};

struct falcon_hip_model {
    falcon_hip_hparams hp{};
    fq_weight tok_emb{}, lm_head{};
    float * out_norm_w = nullptr, * out_norm_b = nullptr;
    std::vector<layer_weights> layers;        // local layers only
    std::vector<void *> allocs;
    // Weight ARENA: every matrix of the stage is carved out of a few very large allocations instead of one hipMalloc per
    // tensor. Measured on MI355X (Falcon-7B Q4_0, the persistent engine's loader alone, round 3): 131
    // separate allocations 2680 us per token (1.45 TB/s), one arena 695 us (5.6 TB/s) -- the driver maps a large allocation
    // with large page fragments, and a wave that streams 1 KiB pieces lives or dies by the translation reach.
    uint8_t * arena_cur = nullptr; size_t arena_left = 0;
    size_t weight_bytes = 0;                   // quantized bytes streamed per decoded token (local layers [+ lm_head])
    uint8_t * vb_pool = nullptr; int32_t * vb_offs = nullptr;      // the vocabulary's bytes for stop strings (falcon_hip_model_set_vocab; in allocs), shared by the contexts' samplers
    bool first_stage() const { return hp.layer_begin == 0; }
    bool last_stage()  const { return hp.layer_end == hp.n_layer; }
};

// ---- captured steps. Every entry point that replays a hipGraph keeps ONE slot: the exec and the key it was captured under. The key
// is everything the captured launch list depends on -- a changed key re-captures, and nothing else invalidates a slot except
// drop_graphs (context free, set_fused). capture_step / step_slot::replay / drop_graphs below hold all of the mechanism.
struct falcon_hip_context;
struct step_key {
    int sig = -1;                              // graph_signature(): the context's own modes
    int epoch = -1;                            // fq_config_epoch(): the process-wide switches that change a launch list
    int64_t baked[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };    // what the body writes into launch arguments besides the context's fixed buffers: addresses of buffers that move, baked integers
    bool operator==(const step_key & o) const { return sig == o.sig && epoch == o.epoch && !memcmp(baked, o.baked, sizeof baked); }
};
struct step_slot {
    hipGraphExec_t exec = nullptr;
    step_key key;                              // of exec
    bool holds(const step_key & k) const { return exec && key == k; }
    template <class Body> void replay(falcon_hip_context * c, hipStream_t st, const step_key & k, Body && body);      // re-captures body() when k differs, then launches
    void drop() { if (exec) { HIP_CHECK(hipGraphExecDestroy(exec)); exec = nullptr; } }
};

struct falcon_hip_context {
    falcon_hip_model * m = nullptr;
    int n_ctx = 0, n_batch = 0, rope_n_ctx = 0;
    // n_seq > 0: a context of n_seq independent sequences that advance in lock step (falcon_hip_context_create_seqs): every
    // step evaluates one token of each, row t of the activations belongs to sequence t and attends to its own KV cache
    // ([layer][seq][n_ctx][HKV][D]) -- one pass over the stage's weights serves n_seq tokens
    int n_seq = 0;
    float * x = nullptr, * ln = nullptr, * ln2 = nullptr, * qkv = nullptr, * att = nullptr, * wo_out = nullptr, * up = nullptr;
    fq_att_scratch att_scratch{nullptr, 0};
    float * logits_dev = nullptr;
    // quantized-activation images. Each buffer holds the LARGEST image of its length (Q8_1: 1.25 bytes per element) and is
    // typed per use from the weight that consumes it (ggml.c:1627-1718 vec_dot_type), so that a file which mixes weight
    // formats between tensors or blocks never writes an image into a buffer sized for another family.
    uint8_t * buf_e = nullptr, * buf_e2 = nullptr, * buf_att = nullptr, * buf_ff = nullptr;
    float * k_cache = nullptr, * v_cache = nullptr;
    float * rope_cs = nullptr;
    int * n_past_dev = nullptr;
    // ragged steps (falcon_hip_eval_seqs / falcon_hip_decode_greedy_seqs): row t at position pos_dev[t]; the device loop's per-row step counters and its
    // [step][seq] output. Apart from n_past_dev, which every uniform launch reads and k_set2_i32 / k_inc_i32 write; allocated by the first ragged call
    // (a context that never takes one keeps the parent layout of its buffers).
    int * pos_dev = nullptr, * seq_steps_dev = nullptr;
    int32_t * seq_out_dev = nullptr; int64_t seq_out_cap = 0;
    int32_t * tokens_dev = nullptr, * out_tokens_dev = nullptr;
    float * hidden_dev = nullptr;
    float * argmax_val = nullptr;              // per-workgroup greedy candidates written by the lm_head kernel
    int   * argmax_idx = nullptr;
    bool keep_hidden = false;
    int  hidden_tokens = 0;
    std::vector<float> logits_host;
    float * logits_pinned = nullptr;           // one row of page-locked host memory: falcon_hip_eval_token's copy is enqueued behind the graph replay
    const float * logits_last = nullptr;       // what falcon_hip_get_logits returns: logits_host.data() or logits_pinned
    bool logits_none = false;                  // the last eval was falcon_hip_eval_score: no logits were copied, falcon_hip_get_logits returns NULL
    int32_t * score_tgt = nullptr;             // falcon_hip_eval_score: [n_batch] targets and [n_batch] probabilities in device memory, made by the first call
    float * score_prob = nullptr;
    std::vector<float> score_host;
    bool logits_fresh = false;                 // the host rows are those of the LAST call (falcon_hip_eval, eval_token, eval_seqs); a decode loop or eval_score leaves none (falcon_hip_copy_state writes them)
    bool logits_pending = false;               // falcon_hip_eval_token: the row's copy is in flight (falcon_hip_get_logits waits for it)
    bool sync_err_sticky = false;              // an in-launch hand-off timed out in an asynchronous step: every later eval of this context fails (3)
    std::vector<void *> allocs;
    bool use_graph = false;
    // the captured steps, one slot per entry point (baked: what its key holds besides signature and epoch)
    step_slot decode_step;                     // falcon_hip_decode_greedy (baked: the base position, an argument of k_argmax_advance)
    step_slot sample_step;                     // falcon_hip_decode_sample (baked: the lp_* buffers, lp_n_top, lp_cap, the sampler's stop arrays -- 0 while no row has stops)
    step_slot seqs_step;                       // falcon_hip_decode_greedy_seqs (baked: seq_out_dev)
    step_slot sample_seqs_step;                // falcon_hip_decode_sample_seqs (baked: seq_out_dev, the lp_* buffers, lp_n_top, lp_cap, the sampler's stop arrays)
    step_slot token_step;                      // falcon_hip_eval_token (baked: nothing)
    step_slot token_step_emb;                  // ... while an embedding mode is set: a slot of its own, so that switching the mode on and off again finds token_step as it was
    step_slot stage_step;                      // falcon_hip_stage_step (baked: its four device pointers; the position lives on the device)
    int step_next_n_past = -1;                 // ... and what n_past_dev holds after stage_step's last replay (-1: unknown)
    int n_captures = 0;                        // captures of this context so far, batch graphs included (falcon_hip_context_graph_captures)
    // fused decode: MLP-up GEMV on a side stream, concurrent with QKV GEMV + attention. Measured on MI355X (Falcon-7B
    // Q4_0, hipGraph): 555 tok/s with the fork/join vs 674 tok/s in stream order -- the cross-stream dependencies cost
    // more than the ~8 us of attention they hide, so it is OFF by default (FALCON_HIP_DUAL=1 turns it on).
    bool dual_stream = false;
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev_fork, ev_join, ev_attn;  // per local layer (dual-stream decode; two-branch prefill: fork, MLP branch done, attention branch done)
    int  par2_max_n = 1 << 30;                  // batches of 17 .. par2_max_n tokens (lock-step passes: from 33 sequences; FALCON_HIP_PAR2_MIN_N) run a block's attention and MLP branches on two streams (FALCON_HIP_PAR2_MAX_N; 0: never). Below that the streaming mat-mul fills every CU by itself (16 tokens: 4.14 ms in stream order against 4.63 forked)
    bool fused_decode = true;                  // N == 1: k_gemv_ln / k_attn_decode / k_gemv_out instead of the op-by-op list
    bool merged_attn_out = true;               // ... with attention and the output mat-vec in one launch (k_attn_out) when the grid fits the chip
    // ... and the next block's k_gemv_ln as a second phase of that launch (k_attn_out_ln): one launch per block. Measured on
    // MI355X (Falcon-7B Q4_0): 867 tok/s against 934 with two launches -- the second phase starts 4.3 us after the last
    // residual value is published (every workgroup sweeps the 36 KB row out of the hand-off buffer, the early finishers
    // keep polling it) and the launch boundary it removes costs less than that. OFF by default; set_fused(3) /
    // FALCON_HIP_TWO_PHASE=1 turn it on.
    bool two_phase = false;
    unsigned long long * x_gran = nullptr;     // hand-off granules of the residual row between the two phases
    unsigned * sync_words = nullptr;           // [0] hand-off epoch of k_attn_out, [1] its time-out flag, [16..80) rope row of the position
    unsigned long long * att_gran = nullptr;   // hand-off granules of k_attn_out: one per 32-bit word of the attention image / row
    bool stage_graph = true;                   // FALCON_HIP_STAGE_GRAPH=0: plain launches
    bool ring_ln = false;                      // k_gemv_ln's launches in the ring form (kernels_ring.hip; k-quants: kernels_ringk.hip); FALCON_HIP_RING=0: never
    bool ring_out = false;                     // the unmerged k_gemv_out launches in the ring form (kernels_ringk.hip): FALCON_HIP_RING_OUT=1 always, 0 never, unset: where it measured faster (ring_out_auto)
    // batched evaluation replayed from hipGraphs (FALCON_HIP_PREFILL_GRAPH=1; default: plain launches): the ~320 launches and 96 cross-stream joins of a
    // prompt batch are then scheduled by the graph instead of the host (the joins cost ~12 us of idle device each as stream events: 11 % of a
    // 128-token Falcon-7B prompt). Keyed by (tokens, keys, mode signature, keep_hidden); the position and the token ids are read from device memory.
    struct batch_graph { int N, max_kv; int64_t sig; hipGraphExec_t exec; };      // sig: the signature (embedding mode included) and keep_hidden low, the epoch high
    std::vector<batch_graph> batch_graphs;
    bool prefill_graph = false;                // (off by default: a replay saves 1-2 % of a batch, capturing a new (tokens, keys) shape costs ~5 ms once)
    // sampled decode (falcon_hip_context_set_sampling / falcon_hip_sample / falcon_hip_decode_sample[_seqs], kernels_sample.hip): one sampler
    // row per sequence, created by the first call that needs it and kept until the context is freed
    ggml_hip_sampler * sampler = nullptr;
    int  last_rows = 1;                         // rows of the last eval's logits (falcon_hip_sample draws from the last of them)
    // log-probabilities of the sampled loops (falcon_hip_context_set_logprobs, kernels_logprob.hip): nothing exists while lp_n_top < 0. The record buffers hold
    // lp_cap records of the current lp_n_top; the captured sampled steps bake all of these in and carry them in their keys
    int  lp_n_top = -1;
    float * lp_prob = nullptr, * lp_top_prob = nullptr; int32_t * lp_top_id = nullptr; int64_t lp_cap = 0;
    int  lp_steps = 0, lp_rows = 0;             // shape of the last recorded call (0: none)
    unsigned sync_err_host = 0;                // copy of sync_words[1], fetched wherever the host synchronises anyway
    // stops of the sampled loops (falcon_hip_context_set_stops; the rows' configuration and state live in the sampler). The loop polls the rows' states
    // every stop_poll steps: two page-locked images of them, each behind its own event, made by the first loop that polls.
    // The default of 16 began as a guess. Measured since (scripts/gpu_stop.py, profiles/stop_7b.json: Falcon-7B Q4_0, 128 steps through the graph, 1.085 ms per
    // step with stops off): +2.0 us per step at 4, +1.3 at 16, +0.9 at 64, next to an A/A spread of 0.4 -- the wait costs nothing that shows, so the interval only
    // trades steps launched past the end (at most 2 x interval - 1) against copies; 16 stays.
    int  stop_poll = 16;
    fq_stop_state * stop_host = nullptr;       // [2][rows]
    hipEvent_t stop_ev[2] = { nullptr, nullptr };
    int  loop_steps = 0;                       // steps the last decode loop launched (falcon_hip_context_loop_steps)
    // generators a loaded session left for sequences whose sampler row did not exist yet (falcon_hip_set_state): [seq, 624 words, position] each; the next
    // set_sampling / set_sampling_ext of the sequence takes its entry over instead of seeding
    std::vector<std::vector<uint32_t>> rng_kept;
    // context swap (falcon_hip_context_swap): the plain context a lock-step context evaluates a slot's regenerated tokens in, made by its first swap
    // (one more cache of n_ctx rows) and freed with it
    falcon_hip_context * swap_ctx = nullptr;
    // draft-and-verify decode (falcon_hip_context_set_spec, fq_spec.h; plain contexts only): spec_K drafts per pass (0: off). The buffers are made by the first
    // set_spec, sized for the context (history n_ctx + 1 tokens, guess n_ctx), and stay: a new history or guess keeps the captured pass, turning spec off drops it
    int  spec_K = 0, spec_source = 0, spec_gmin = 1, spec_gmax = 1;
    fq_spec_state * spec_state = nullptr;
    int32_t * spec_hist = nullptr, * spec_guess = nullptr, * spec_drafts = nullptr;
    fq_spec_state * spec_host = nullptr;       // [2]: page-locked images of the state, each behind its own event (the loop's poll, as stop_host)
    hipEvent_t spec_ev[2] = { nullptr, nullptr };
    step_slot spec_step;                       // falcon_hip_decode_spec (baked: K, source and n-gram bounds, the spec buffers, and what sample_step bakes of the sampler)
    // embeddings (falcon_hip_context_set_embedding; plain single-process contexts only): emb_mode 0 = off, nothing below exists or is launched. Bit 0: the ln_f
    // rows of an eval go to emb_rows and the last of them to emb; bit 1: k_embed_pool_accum adds them to pool_acc / pool_count (kernels_embed.hip). The buffers
    // are made by the first set_embedding and stay; every captured step carries the mode in its key
    int  emb_mode = 0;
    bool emb_no_head = false;                  // falcon_hip_embed: this launch_stage ends after ln_f
    float * emb_rows = nullptr, * emb = nullptr;
    double * pool_acc = nullptr;               // [n_embd], then the finishing launch's sum of squares
    long long * pool_count = nullptr;
    float * pool_out = nullptr;
    int64_t pool_count_host = 0;               // what *pool_count holds (the host knows every eval's N)
    std::vector<float> emb_host;
    bool emb_have = false, emb_host_fresh = false;      // emb holds a row (an eval or a loaded state); emb_host is its copy
};

// k_attn_out hands the attention output from workgroup to workgroup with a BOUNDED spin; a time-out sets sync_words[1] and
// the launch carries on with whatever the granules hold. Wherever the host waits for the stream anyway the word comes
// along, and a set word fails the call (callers of the purely stream-ordered falcon_hip_stage_step poll
// falcon_hip_context_sync_error themselves).
static void fetch_sync_error(falcon_hip_context * c, hipStream_t st) {
    HIP_CHECK(hipMemcpyAsync(&c->sync_err_host, c->sync_words + 1, 4, hipMemcpyDeviceToHost, st));
}
static int report_sync_error(falcon_hip_context * c, const char * where) {
    if (!c->sync_err_host) return 0;
    c->sync_err_sticky = true;
    fprintf(stderr, "falcon-hip: %s: an in-launch hand-off timed out (sync word %u) -- the results of this call are invalid\n", where, c->sync_err_host);
    return 3;
}

// THE capture: body() enqueues one step on st; returns the instantiated graph
template <class Body> static hipGraphExec_t capture_step(falcon_hip_context * c, hipStream_t st, Body && body) {
    hipGraph_t g;
    hipGraphExec_t exec = nullptr;
    HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    body();
    HIP_CHECK(hipStreamEndCapture(st, &g));
    HIP_CHECK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphDestroy(g));
    ++c->n_captures;
    return exec;
}
template <class Body> void step_slot::replay(falcon_hip_context * c, hipStream_t st, const step_key & k, Body && body) {
    if (!holds(k)) { drop(); exec = capture_step(c, st, body); key = k; }
    HIP_CHECK(hipGraphLaunch(exec, st));
}
static void drop_graphs(falcon_hip_context * c) {             // every captured graph of the context
    for (step_slot * s : { &c->decode_step, &c->sample_step, &c->seqs_step, &c->sample_seqs_step, &c->token_step, &c->token_step_emb, &c->stage_step, &c->spec_step }) s->drop();
    for (auto & bg : c->batch_graphs) HIP_CHECK(hipGraphExecDestroy(bg.exec));
    c->batch_graphs.clear();
}
extern "C" int falcon_hip_context_graph_captures(const falcon_hip_context * c) { return c->n_captures; }

static void * dev_alloc(std::vector<void *> & keep, size_t bytes) {
    void * p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
    keep.push_back(p);
    return p;
}

extern "C" falcon_hip_model * falcon_hip_model_create(const falcon_hip_hparams * hp) {
    fq_ctx();
    falcon_hip_model * m = new falcon_hip_model();
    m->hp = *hp;
    if (m->hp.layer_end <= 0 || m->hp.layer_end > hp->n_layer) m->hp.layer_end = hp->n_layer;
    if (m->hp.layer_begin < 0) m->hp.layer_begin = 0;
    if (hp->n_embd % hp->n_head || hp->n_embd / hp->n_head != 64 || hp->n_head % hp->n_head_kv) {
        fprintf(stderr, "falcon-hip: unsupported head geometry (n_embd %d, n_head %d, n_head_kv %d)\n", hp->n_embd, hp->n_head, hp->n_head_kv);
        exit(1);
    }
    m->layers.resize((size_t)(m->hp.layer_end - m->hp.layer_begin));
    return m;
}

extern "C" void falcon_hip_model_free(falcon_hip_model * m) {
    if (!m) return;
    for (void * p : m->allocs) HIP_CHECK(hipFree(p));
    delete m;
}

static uint8_t * arena_alloc(falcon_hip_model * m, size_t bytes) {
    bytes = (bytes + 2048 + 65535) & ~(size_t) 65535;            // slack for clamped tail loads / the engine's last DMA piece; 64 KiB granules
    if (bytes > m->arena_left) {
        size_t chunk = (size_t) 1 << 30;
        if (const char * e = getenv("FALCON_HIP_ARENA_MB")) chunk = (size_t) atoll(e) << 20;
        if (chunk < bytes) chunk = bytes;
        void * p = nullptr;
        HIP_CHECK(hipMalloc(&p, chunk));
        m->allocs.push_back(p);
        m->arena_cur = (uint8_t *) p; m->arena_left = chunk;
    }
    uint8_t * r = m->arena_cur;
    m->arena_cur += bytes; m->arena_left -= bytes;
    return r;
}

static fq_weight upload_weight(falcon_hip_model * m, int type, const void * data, int64_t K, int64_t M) {
    hip_context & c = fq_ctx();
    if (type == FQ_F16) {                                         // row-major fp16 as in the file: 2 bytes per weight, no re-layout (kernels_f16.hip)
        if (!fq_f16_row_ok(K)) { fprintf(stderr, "falcon-hip: F16 weights with K=%lld unsupported (the row length must be a multiple of %d)\n", (long long) K, FQ_F16_K_MULTIPLE); exit(1); }
        const fq_weight w = fq_f16_weight_view(arena_alloc(m, (size_t) M * (size_t) K * 2), K, M);
        HIP_CHECK(hipMemcpyAsync(w.plane[0], data, w.bytes, hipMemcpyHostToDevice, c.stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        return w;
    }
    const fq_type_desc d = fq_desc(type);
    if (d.blck == 0 || K % d.blck != 0) { fprintf(stderr, "falcon-hip: weight type %d with K=%lld unsupported\n", type, (long long) K); exit(1); }
    fq_weight w{};
    w.type = type; w.K = K; w.M = M; w.nblk = K / d.blck;
    w.bytes = (size_t) M * w.nblk * d.tsize;
    w.row_stride = fq_il_row_stride(d, w.nblk);
    uint8_t * slab = arena_alloc(m, (size_t) M * w.row_stride);
    for (int p = 0; p < d.nplanes; ++p) w.plane[p] = slab;
    const size_t row_bytes = (size_t) w.nblk * d.tsize;
    int64_t rows_per_chunk = (int64_t)((256u << 20) / row_bytes);
    if (rows_per_chunk < 1) rows_per_chunk = 1;
    if (rows_per_chunk > M) rows_per_chunk = M;
    uint8_t * stage = nullptr;
    HIP_CHECK(hipMalloc((void **) &stage, (size_t) rows_per_chunk * row_bytes));
    for (int64_t r0 = 0; r0 < M; r0 += rows_per_chunk) {
        const int64_t nr = (M - r0 < rows_per_chunk) ? M - r0 : rows_per_chunk;
        HIP_CHECK(hipMemcpyAsync(stage, (const uint8_t *) data + (size_t) r0 * row_bytes, (size_t) nr * row_bytes, hipMemcpyHostToDevice, c.stream));
        fq_weight sub = w;
        sub.M = nr;
        for (int p = 0; p < d.nplanes; ++p)
            sub.plane[p] = w.plane[0] + (size_t) r0 * w.row_stride;
        fq_launch_retile(stage, sub, c.stream);
        HIP_CHECK(hipStreamSynchronize(c.stream));
    }
    HIP_CHECK(hipFree(stage));
    return w;
}

static float * upload_f32(falcon_hip_model * m, const void * data, int64_t n) {
    float * p = (float *) dev_alloc(m->allocs, (size_t) n * 4);
    HIP_CHECK(hipMemcpy(p, data, (size_t) n * 4, hipMemcpyHostToDevice));
    return p;
}

extern "C" int falcon_hip_model_set_tensor(falcon_hip_model * m, const char * name_c, int type, const void * data, int64_t ne0, int64_t ne1) {
    const std::string name(name_c);
    const falcon_hip_hparams & hp = m->hp;
    auto want2d = [&](int64_t k, int64_t rows) {
        if (ne0 != k || ne1 != rows) { fprintf(stderr, "falcon-hip: %s has shape [%lld,%lld], expected [%lld,%lld]\n", name_c, (long long) ne0, (long long) ne1, (long long) k, (long long) rows); exit(1); }
    };
    auto want_f32 = [&]() { if (type != FQ_F32 || ne0 != hp.n_embd) { fprintf(stderr, "falcon-hip: %s must be f32[%d]\n", name_c, hp.n_embd); exit(1); } };
    const int64_t E = hp.n_embd, D = 64, QKV = (int64_t)(hp.n_head + 2 * hp.n_head_kv) * D;
    if (name == "transformer.word_embeddings.weight") {
        if (!m->first_stage()) return -1;
        want2d(E, hp.n_vocab); m->tok_emb = upload_weight(m, type, data, E, hp.n_vocab); return 0;
    }
    if (name == "lm_head.weight") {
        if (!m->last_stage()) return -1;
        want2d(E, hp.n_vocab); m->lm_head = upload_weight(m, type, data, E, hp.n_vocab); m->weight_bytes += m->lm_head.bytes; return 0;
    }
    if (name == "transformer.ln_f.weight") { if (!m->last_stage()) return -1; want_f32(); m->out_norm_w = upload_f32(m, data, E); return 0; }
    if (name == "transformer.ln_f.bias")   { if (!m->last_stage()) return -1; want_f32(); m->out_norm_b = upload_f32(m, data, E); return 0; }
    const std::string pre = "transformer.h.";
    if (name.compare(0, pre.size(), pre) != 0) return -1;
    const size_t dot = name.find('.', pre.size());
    if (dot == std::string::npos) return -1;
    const int il = atoi(name.substr(pre.size(), dot - pre.size()).c_str());
    if (il < hp.layer_begin || il >= hp.layer_end) return -1;
    layer_weights & L = m->layers[(size_t)(il - hp.layer_begin)];
    const std::string leaf = name.substr(dot + 1);
    if (leaf == "self_attention.query_key_value.weight") { want2d(E, QKV);     L.qkv  = upload_weight(m, type, data, E, QKV);      m->weight_bytes += L.qkv.bytes;  return 0; }
    if (leaf == "self_attention.dense.weight")           { want2d(E, E);       L.wo   = upload_weight(m, type, data, E, E);        m->weight_bytes += L.wo.bytes;   return 0; }
    if (leaf == "mlp.dense_h_to_4h.weight")              { want2d(E, hp.n_ff); L.up   = upload_weight(m, type, data, E, hp.n_ff);  m->weight_bytes += L.up.bytes;   return 0; }
    if (leaf == "mlp.dense_4h_to_h.weight")              { want2d(hp.n_ff, E); L.down = upload_weight(m, type, data, hp.n_ff, E);  m->weight_bytes += L.down.bytes; return 0; }
    // norms: 7B has input_layernorm (shared); 40B/180B have ln_mlp (-> MLP input) and ln_attn (-> QKV input), libfalcon.cpp:1845-1855
    if (leaf == "input_layernorm.weight" || leaf == "ln_mlp.weight") { want_f32(); L.ln_w  = upload_f32(m, data, E); return 0; }
    if (leaf == "input_layernorm.bias"   || leaf == "ln_mlp.bias")   { want_f32(); L.ln_b  = upload_f32(m, data, E); return 0; }
    if (leaf == "ln_attn.weight") { want_f32(); L.ln2_w = upload_f32(m, data, E); return 0; }
    if (leaf == "ln_attn.bias")   { want_f32(); L.ln2_b = upload_f32(m, data, E); return 0; }
    return -1;
}

extern "C" void falcon_hip_model_get_hparams(const falcon_hip_model * m, falcon_hip_hparams * hp_out) { *hp_out = m->hp; }
extern "C" size_t falcon_hip_model_weight_bytes(const falcon_hip_model * m) { return m->weight_bytes; }

static size_t act_col_bytes_max(int64_t K, bool f16 = false) {
    size_t b = fq_act_col_bytes(FQ_Q8_1, K), b0 = fq_act_col_bytes(FQ_Q8_0, K), bk = fq_act_col_bytes(FQ_Q8_K, K);
    if (b0 > b) b = b0;
    if (bk > b) b = bk;
    if (f16 && fq_f16_col_bytes(K) > b) b = fq_f16_col_bytes(K);      // (the fp16 image of F16 consumers: 2 bytes per element)
    return b;
}
// F16 matrices (kernels_f16.hip): blocks that hold one, and stages whose lm_head is one, run the op-by-op list -- the fused launches are per quantized format
static bool layer_has_f16(const layer_weights & L) { return L.qkv.type == FQ_F16 || L.wo.type == FQ_F16 || L.up.type == FQ_F16 || L.down.type == FQ_F16; }
static bool stage_has_f16(const falcon_hip_model * m) {
    for (const layer_weights & L : m->layers) if (layer_has_f16(L)) return true;
    return m->last_stage() && m->lm_head.type == FQ_F16;
}
// the image view of `buf` for the activations that weight `w` consumes
static fq_act act_for(uint8_t * buf, const fq_weight & w, int64_t cols) {
    fq_act a{}; a.type = w.type == FQ_F16 ? (int) FQ_F16 : fq_desc(w.type).act_type; a.K = w.K; a.ncols = cols; a.base = buf; return a;
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
    if (c->seq_out_dev) HIP_CHECK(hipFree(c->seq_out_dev));
    if (c->logits_pinned) HIP_CHECK(hipHostFree(c->logits_pinned));
    if (c->score_tgt) HIP_CHECK(hipFree(c->score_tgt));
    if (c->score_prob) HIP_CHECK(hipFree(c->score_prob));
    for (void * p : { (void *) c->lp_prob, (void *) c->lp_top_id, (void *) c->lp_top_prob }) if (p) HIP_CHECK(hipFree(p));
    if (c->stop_host) HIP_CHECK(hipHostFree(c->stop_host));
    for (hipEvent_t e : c->stop_ev) if (e) HIP_CHECK(hipEventDestroy(e));
    if (c->spec_host) HIP_CHECK(hipHostFree(c->spec_host));
    for (hipEvent_t e : c->spec_ev) if (e) HIP_CHECK(hipEventDestroy(e));
    delete c;
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

static bool stage_uniform(const falcon_hip_model * m) {
    for (const layer_weights & L : m->layers) if (L.qkv.type != L.up.type || L.down.type != L.wo.type) return false;
    return true;
}
// THE predicate for "an N = 1 step of this context runs the fused decode kernels" -- launch_stage, the greedy sampler and
// the pipeline step all ask here, so the sampler reads the per-workgroup argmax candidates exactly when the fused lm_head
// wrote them. The fused kernels are instantiated per weight format (a model that mixes formats inside a block takes the
// op list) and implement the default summation order only (ggml_hip_reference_order -> op list).
// Round 6: the FAST reference order (ggml_hip_reference_order(2)) has the fused launches too, for stages of one legacy format (fq_ref_chain.h).
static bool stage_legacy(const falcon_hip_model * m) {
    auto leg = [](int t) { return t == FQ_Q4_0 || t == FQ_Q4_1 || t == FQ_Q5_0 || t == FQ_Q5_1 || t == FQ_Q8_0; };
    if (m->layers.empty() || m->hp.n_embd % 32 || m->hp.n_ff % 32) return false;
    const int t = m->layers[0].qkv.type;
    for (const layer_weights & L : m->layers) if (L.qkv.type != t || L.up.type != t || L.down.type != t || L.wo.type != t) return false;
    if (m->last_stage() && !leg(m->lm_head.type)) return false;
    return leg(t);
}
static bool stage_fused_ref(const falcon_hip_context * c) {        // N = 1 steps run the fused launches in the reference's association
    return c->fused_decode && fq_reference_fast() && stage_legacy(c->m) && !c->two_phase && !c->dual_stream;
}
static bool stage_fused(const falcon_hip_context * c) {
    if (stage_fused_ref(c)) return true;
    return c->fused_decode && stage_uniform(c->m) && !stage_has_f16(c->m) && !fq_reference_order() && !fq_attn_f64();
}
// the context's own modes that select a launch list: the first word of every step_key (a step_slot re-captures when it differs)
static int graph_signature(const falcon_hip_context * c) {
    return (stage_fused(c) ? 1 : 0) | (fq_reference_order() ? 2 : 0) | (fq_attn_f64() ? 4 : 0) | (c->merged_attn_out ? 8 : 0) |
           (c->two_phase ? 16 : 0) | (c->dual_stream ? 32 : 0) | (stage_fused_ref(c) ? 128 : 0) |
           (c->emb_mode << 16) | (c->emb_mode && c->emb_no_head ? 1 << 18 : 0);      // (bit 8: keep_hidden in the batch key; embeddings off: the value it always had)
}
// ... and the whole key: the signature alone is the same in reference orders 1 and 2 and before and after ggml_hip_debug_force_gemv /
// ggml_hip_debug_gemm_mode, whose launch lists differ -- the epoch moves with every such switch
static int64_t key_ptr(const void * p) { return (int64_t)(intptr_t) p; }
static step_key step_key_of(const falcon_hip_context * c, std::initializer_list<int64_t> baked = {}) {
    step_key k;
    k.sig = graph_signature(c); k.epoch = fq_config_epoch();
    int i = 0;
    for (int64_t v : baked) k.baked[i++] = v;
    return k;
}

// ---- which calls replay a captured step (side by side; the differences are historical and kept as they are)
// the decode attention keeps a score row of max_n_kv floats in LDS; a captured step is sized for the whole context (its position is read
// from device memory), so contexts longer than that buffer allows run their single-token steps as plain launches sized for n_past + 1
static bool fused_graph_fits(const falcon_hip_context * c) { return fq_attn_decode_lds_bytes(c->n_ctx) <= 160 * 1024; }
// no replay under the profiler's brackets or the phase stamps, nor in reference order 1
static bool graph_ok_strict() { return !fq_prof_active() && !fq_ctx().dbg_stamps && (!fq_reference_order() || fq_reference_fast()); }
// falcon_hip_decode_greedy / _sample: NOT strict -- they replay under the profiler, the stamps and order 1 whenever the caller asked for the graph.
// Neither NOTEBOOK nor the commit history records a reason for the difference; it is kept, not endorsed
static bool graph_ok_loop(const falcon_hip_context * c)       { return c->use_graph && fused_graph_fits(c); }
static bool graph_ok_seqs(const falcon_hip_context * c)       { return c->use_graph && fused_graph_fits(c) && graph_ok_strict(); }      // falcon_hip_decode_greedy_seqs / _sample_seqs
static bool graph_ok_token(const falcon_hip_context * c)      { return stage_fused(c) && fused_graph_fits(c) && graph_ok_strict(); }     // falcon_hip_eval_token: no opt-in, fused steps only
static bool graph_ok_stage_step(const falcon_hip_context * c) { return c->stage_graph && !fq_prof_active() && !fq_ctx().dbg_stamps && fused_graph_fits(c); }      // falcon_hip_stage_step: order 1 replays too
static bool graph_ok_batch(const falcon_hip_context * c, int N) {                                                                        // eval_stage_impl's batches (FALCON_HIP_PREFILL_GRAPH=1)
    return c->prefill_graph && N > 4 && c->n_seq == 0 && !fq_tl_collecting() && graph_ok_strict();
}

// ------------------------------------------------------------------------------------------------ one eval
// Launches every kernel of this stage for N tokens. Inputs already in place: tokens_dev (first stage) or x, and
// n_past_dev. max_n_kv bounds n_past + N for LDS sizing. pos_stride 1 (lock-step contexts only): a ragged step, row t at
// position pos_dev[t] (max_n_kv > every one of them); 0: every row at n_past_dev.
// verify_limit > 0 (plain contexts, 2 <= N <= 16: a draft-and-verify pass, falcon_hip_decode_spec): the N rows are the positions n_past_dev + t of the one cache, as
// in a prompt batch, but a row whose position would be >= verify_limit (n_ctx) appends nothing and is not attended for (kernels_block.hip: the verify launches);
// and 2..4 rows take the column mat-vec launches a lock-step context of as many sequences takes -- one pass over the weights, every row the bits of the single row.
// lock-step contexts (and verify passes) of up to this many rows run the column mat-vec kernels in chunks of 4: fq_mm_cols_max_n (fq_mm_forms.h), from the model's first Wqkv
static int cols_max_n(const falcon_hip_model * m) { return m->layers.empty() ? 4 : fq_mm_cols_max_n(fq_mm_mat_of(m->layers[0].qkv), fq_mm_sw()); }
// ---- the fused single-token path of launch_stage
static void launch_stage_token(falcon_hip_context * c, int max_n_kv, hipStream_t st) {
    falcon_hip_model * m = c->m;
    const falcon_hip_hparams & hp = m->hp;
    hip_context & hc = fq_ctx();
    const int64_t E = hp.n_embd, D = 64, H = hp.n_head, HKV = hp.n_head_kv, FF = hp.n_ff;
    const int64_t n_caches = c->n_seq > 0 ? c->n_seq : 1;
    // ---- fused single-token path (kernels_decode.hip), bit-identical to the op list below. Per block, by mode:
    //   3 launches  k_gemv_ln | k_attn_decode | k_gemv_out
    //   2 launches  k_gemv_ln | k_attn_out                        (attention inside the output mat-vec launch)
    //   1 launch    k_attn_out_ln = k_attn_out of block l + k_gemv_ln of block l+1 (or ln_f + lm_head) as a second phase
    const bool prof = fq_prof_active();
    const bool dual = c->dual_stream && !prof;
    const bool ref = stage_fused_ref(c);                    // the reference's association on the same launches (fq_ref_chain.h)
    auto ln_args = [&](size_t li) {
        const layer_weights & L = m->layers[li];
        const int ff_act = fq_desc(L.down.type).act_type;
        const bool quant_epi = (ff_act == FQ_Q8_0 || ff_act == FQ_Q8_1);
        fq_gemv_ln_args ga{};
        ga.x = c->x; ga.E = E; ga.nseg = 2; ga.gelu_table = hc.gelu_table; ga.dbg = hc.dbg_stamps;
        ga.epoch_word = c->merged_attn_out ? c->sync_words : nullptr;
        if (c->merged_attn_out) { ga.n_past_ptr = c->n_past_dev; ga.rope_cs = c->rope_cs; ga.rope_cur = (float *)(c->sync_words + 16); }
        ga.seg[0] = { L.qkv, hp.two_norms ? L.ln2_w : L.ln_w, hp.two_norms ? L.ln2_b : L.ln_b, FQ_LNEPI_STORE, c->qkv, nullptr, 0, 0 };
        ga.seg[1] = { L.up, L.ln_w, L.ln_b, quant_epi ? FQ_LNEPI_GELU_QUANT : FQ_LNEPI_GELU_STORE, c->up, c->buf_ff, ff_act, 0 };
        return ga;
    };
    auto head_args = [&]() {
        fq_gemv_ln_args ga{};
        ga.x = c->x; ga.E = E; ga.nseg = 1; ga.gelu_table = hc.gelu_table;
        ga.epoch_word = c->merged_attn_out ? c->sync_words : nullptr;
        ga.seg[0] = { m->lm_head, m->out_norm_w, m->out_norm_b, FQ_LNEPI_STORE, c->logits_dev, nullptr, 0, 0 };
        ga.argmax_val = c->argmax_val; ga.argmax_idx = c->argmax_idx;
        return ga;
    };
    bool ln_done = false;                                   // this block's k_gemv_ln already ran as the previous launch's second phase
    bool head_done = false;
    for (size_t li = 0; li < m->layers.size(); ++li) {
        const layer_weights & L = m->layers[li];
        if (c->keep_hidden) HIP_CHECK(hipMemcpyAsync(c->hidden_dev + li * (size_t) E, c->x, (size_t) E * 4, hipMemcpyDeviceToDevice, st));
        const int ff_act = fq_desc(L.down.type).act_type;
        const bool quant_epi = (ff_act == FQ_Q8_0 || ff_act == FQ_Q8_1);
        const fq_gemv_ln_args ga = ln_args(li);
        if (dual) {
            // the MLP-up mat-vec only needs x: run it on the side stream while QKV + attention run on the main one
            fq_gemv_ln_args gu = ga; gu.nseg = 1; gu.seg[0] = ga.seg[1]; gu.seg[0].block_begin = 0;
            fq_gemv_ln_args gq = ga; gq.nseg = 1;
            HIP_CHECK(hipEventRecord(c->ev_fork[li], st));
            HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_fork[li], 0));
            fq_launch_gemv_ln(gu, hc.n_cu, c->side);
            if (!quant_epi) fq_launch_quantize_act(c->up, FF, act_for(c->buf_ff, L.down, 1), c->side);
            HIP_CHECK(hipEventRecord(c->ev_join[li], c->side));
            fq_launch_gemv_ln(gq, hc.n_cu, st);
        } else if (!ln_done) {
            if (prof) fq_prof_open(st);
            bool ring = false;
            if (c->ring_ln && quant_epi) ring = fq_launch_gemv_ln_ring(ga, c->sync_words + 1, hc.n_cu, st, ref);
            else if (c->ring_ln && !ref) ring = fq_launch_ringk_ln(ga, c->sync_words + 1, hc.n_cu, st);      // k-quants: GELU stored as f32
            if (!ring) fq_launch_gemv_ln(ga, hc.n_cu, st, ref);
            if (prof) fq_prof_close(st, (double)(L.qkv.bytes + L.up.bytes));
        }
        ln_done = false;
        float * kc = c->k_cache + li * (size_t) n_caches * c->n_ctx * HKV * D;
        float * vc = c->v_cache + li * (size_t) n_caches * c->n_ctx * HKV * D;
        const int att_act = fq_desc(L.wo.type).act_type;
        const bool att_q = (att_act == FQ_Q8_0 || att_act == FQ_Q8_1);      // the head's 64 outputs = two 32-blocks
        fq_gemv_out_args go{ L.down, L.wo, c->buf_ff, c->att, att_q ? c->buf_att : nullptr, c->x, c->x,
                             hc.dbg_stamps ? hc.dbg_stamps + 4096 * 8 : nullptr };
        if (dual) HIP_CHECK(hipStreamWaitEvent(st, c->ev_join[li], 0));
        // the merged attention + output launch: in the reference's association (ref), or with the next block's k_gemv_ln / the head as a second phase (next)
        auto attn_out = [&](bool in_ref_order, const fq_gemv_ln_args * next) {
            if (in_ref_order) return fq_launch_attn_out_ref(go, c->qkv, (int) H, (int) HKV, c->n_past_dev, max_n_kv, c->rope_cs, (const float *)(c->sync_words + 16),
                                                            kc, vc, hc.exp_table_attn, att_act, c->att_gran, c->sync_words, c->sync_words + 1, hc.n_cu, st);
            return fq_launch_attn_out(go, c->qkv, (int) H, (int) HKV, c->n_past_dev, max_n_kv, c->rope_cs, (const float *)(c->sync_words + 16),
                                      kc, vc, hc.exp_table_attn, att_act, c->att_gran, c->sync_words, c->sync_words + 1, hc.n_cu, st, next, next ? c->x_gran : nullptr);
        };
        // gelu(up) still f32 (k-quant consumers: a Q8_K block spans 256 rows, i.e. several workgroups of the launch above): quantized by its own launch
        // ahead of the merged form, or by extra workgroups of the attention launch (the rider) in the three-launch form
        bool ff_pending = !quant_epi && !dual;
        bool merged = false;
        if (ref && c->merged_attn_out) {
            // the merged launch in the reference's association; where its grid does not fit the chip: attention (f64 dots) + output launch below
            if (prof) fq_prof_open(st);
            merged = attn_out(true, nullptr);
            if (prof) { if (merged) fq_prof_close(st, (double)(L.down.bytes + L.wo.bytes)); else fq_prof_cancel(); }
        }
        const bool will_merge = !ref && c->merged_attn_out && !dual && fq_attn_out_fits(go, (int) H, max_n_kv, hc.n_cu);
        if (ff_pending && will_merge) { fq_launch_quantize_act(c->up, FF, act_for(c->buf_ff, L.down, 1), st); ff_pending = false; }
        if (will_merge) {
            // second phase: the next block's k_gemv_ln (its GELU output must be quantized in its epilogue: a separate
            // quantizer launch cannot sit between the phases), or ln_f + lm_head after the last block
            fq_gemv_ln_args next{}; bool have_next = false; double next_bytes = 0.0;
            if (c->two_phase && !c->keep_hidden) {
                if (li + 1 < m->layers.size()) {
                    const layer_weights & Ln = m->layers[li + 1];
                    const int a2 = fq_desc(Ln.down.type).act_type;
                    if (a2 == FQ_Q8_0 || a2 == FQ_Q8_1) { next = ln_args(li + 1); have_next = true; next_bytes = (double)(Ln.qkv.bytes + Ln.up.bytes); }
                } else if (m->last_stage() && !c->emb_mode) { next = head_args(); have_next = true; next_bytes = (double) m->lm_head.bytes; }      // (embeddings: the head stays a launch of its own, which falcon_hip_embed leaves out -- keep_hidden's precedent, for the last block only; c->x is whole behind either launch)
            }
            if (prof) fq_prof_open(st);
            if (have_next) {
                merged = attn_out(false, &next);
                if (merged) {
                    if (li + 1 < m->layers.size()) ln_done = true; else head_done = true;
                    if (prof) { fq_prof_close(st, (double)(L.down.bytes + L.wo.bytes) + next_bytes); }
                }
            }
            if (!merged) {
                merged = attn_out(false, nullptr);
                if (merged && prof) fq_prof_close(st, (double)(L.down.bytes + L.wo.bytes));
            }
            if (!merged && prof) fq_prof_cancel();
            if (!merged) { fprintf(stderr, "falcon-hip: the merged attention + output launch refused a shape fq_attn_out_fits accepted\n"); exit(1); }
        }
        if (!merged) {
            const fq_act a_ff1 = act_for(c->buf_ff, L.down, 1);
            if (ff_pending && fq_mm_sw().quant_rider && a_ff1.type == FQ_Q8_K && FF % 256 == 0) {
                // attention of the one sequence + the rider: k_attn_decode's code (k_attn_decode_seqs at one sequence), gelu(up)'s Q8_K image by extra workgroups
                fq_launch_attn_decode_seqs(c->qkv, 1, (int) H, (int) HKV, c->n_past_dev, max_n_kv, c->rope_cs, kc, vc, 0, hc.exp_table_attn,
                                           att_q ? nullptr : c->att, att_q ? c->buf_att : nullptr, att_act, (int64_t) fq_act_col_bytes(att_act, E), st, c->up, FF, &a_ff1);
                ff_pending = false;
            } else {
                if (ff_pending) { fq_launch_quantize_act(c->up, FF, a_ff1, st); ff_pending = false; }
                fq_launch_attn_decode(c->qkv, (int) H, (int) HKV, c->n_past_dev, max_n_kv, c->rope_cs, kc, vc, hc.exp_table_attn,
                                      att_q ? nullptr : c->att, att_q ? c->buf_att : nullptr, att_act, st, ref);
            }
            if (prof) fq_prof_open(st);
            if (ref) fq_launch_gemv_out(go, hc.n_cu, st, true);
            else if (!(c->ring_out && fq_launch_ring_out(go, c->sync_words + 1, hc.n_cu, st))) fq_launch_gemv_out(go, hc.n_cu, st);
            if (prof) fq_prof_close(st, (double)(L.down.bytes + L.wo.bytes));
        }
    }
    if (c->keep_hidden) {
        HIP_CHECK(hipMemcpyAsync(c->hidden_dev + m->layers.size() * (size_t) E, c->x, (size_t) E * 4, hipMemcpyDeviceToDevice, st));
        c->hidden_tokens = 1;
    }
    if (m->last_stage() && c->emb_mode) {                        // the ln_f row the fused head normalises for itself and drops
        fq_launch_layer_norm(c->x, E, 1, m->out_norm_w, m->out_norm_b, c->emb, st);
        if (c->emb_mode & FALCON_HIP_EMBED_POOL) fq_launch_embed_pool_accum(c->emb, 1, (int) E, c->pool_acc, c->pool_count, st);
        if (c->emb_no_head) return;
    }
    if (m->last_stage() && !head_done) {
        const fq_gemv_ln_args ga = head_args();
        if (prof) fq_prof_open(st);
        fq_launch_gemv_ln(ga, hc.n_cu, st, ref);
        if (prof) fq_prof_close(st, (double) m->lm_head.bytes);
    }
}

// ---- the batched path of launch_stage: one block
// what every launch of a block reads: its weights and caches, the four activation images, the rows and where they stand
struct stage_block {
    const layer_weights & L; size_t li; bool f16;      // f16: some matrix of the block is F16 -- the generic launches only: every fused / paired / two-stream form is per quantized format
    float * kc, * vc;
    fq_act a_qkv, a_up, a_att, a_ff;
    int N, max_n_kv;
    const int * seq_pos; int64_t seq_stride; int pos_stride, verify_limit;      // (launch_stage's header)
    hipStream_t st;
    const fq_mm_mode & md;                              // the process modes as of this launch_stage call (the form rules' input)
};
enum block_form { BLOCK_COLUMNS, BLOCK_TWO_STREAMS, BLOCK_GENERIC };
static fq_gemv_epi epi_store() { return fq_gemv_epi{ FQ_EPI_STORE, fq_ctx().gelu_table, nullptr, nullptr, 0 }; }
static fq_gemv_epi epi_gelu()  { return fq_gemv_epi{ FQ_EPI_GELU, fq_ctx().gelu_table, nullptr, nullptr, 0 }; }
static int64_t n_qkv(const falcon_hip_hparams & hp) { return ((int64_t) hp.n_head + 2 * hp.n_head_kv) * 64; }

// one mat-mul of a block (lock-step contexts: the k-quants' streaming forms from 3 sequences up, fq_mul_mat_q_acts_from3)
static void mm(const stage_block & b, const fq_weight & w, const fq_act & a, float * dst, int64_t ldd, const fq_gemv_epi & ep, hipStream_t st) {
    if (b.seq_stride) fq_mul_mat_q_acts_from3(w, a, b.N, dst, ldd, ep, st); else fq_mul_mat_q_acts(w, a, b.N, dst, ldd, ep, st);
}
// RoPE, KV append, attention and the image Wo takes, of all N rows.
//   lock-step sequences: one launch of the decode attention (k_attn_decode's code: the same bits as the three launches of a prompt), which also writes the
//     image for Q8_0 / Q8_1 consumers; ride: gelu(up)'s quantizer rides on that launch (Wup's GELU output exists already when Wqkv and Wup went in one launch)
//   a draft-and-verify pass: the verify launches (rows at or beyond verify_limit append nothing)
//   a prompt batch: rope + KV store, attention, quantize
static void block_attention(falcon_hip_context * c, const stage_block & b, bool ride) {
    const falcon_hip_hparams & hp = c->m->hp;
    hip_context & hc = fq_ctx();
    const int64_t E = hp.n_embd, FF = hp.n_ff;
    const int H = hp.n_head, HKV = hp.n_head_kv, D = 64;
    hipStream_t st = b.st;
    if (b.seq_stride && !fq_reference_order() && !fq_attn_f64()) {
        const bool att_q = (b.a_att.type == FQ_Q8_0 || b.a_att.type == FQ_Q8_1);
        fq_launch_attn_decode_seqs(c->qkv, b.N, H, HKV, b.seq_pos, b.max_n_kv, c->rope_cs, b.kc, b.vc, b.seq_stride, hc.exp_table_attn,
                                   att_q ? nullptr : c->att, att_q ? c->buf_att : nullptr, b.a_att.type, (int64_t) fq_act_col_bytes(b.a_att.type, E), st,
                                   ride ? c->up : nullptr, FF, ride ? &b.a_ff : nullptr, b.pos_stride);
        if (!att_q) fq_launch_quantize_act(c->att, E, b.a_att, st);
    } else if (b.verify_limit) {
        fq_launch_rope_kv_verify(c->qkv, b.N, H, HKV, D, c->n_past_dev, b.verify_limit, c->rope_cs, b.kc, b.vc, st);
        fq_launch_attention_verify(c->qkv, b.N, H, HKV, D, c->n_past_dev, b.verify_limit, b.kc, b.vc, hc.exp_table_attn, c->att, st);
        fq_launch_quantize_act(c->att, E, b.a_att, st);
    } else {
        fq_launch_rope_kv(c->qkv, b.N, H, HKV, D, b.seq_pos, c->rope_cs, b.kc, b.vc, st, b.seq_stride, b.pos_stride);
        fq_launch_attention(c->qkv, b.N, H, HKV, D, b.seq_pos, b.max_n_kv, b.kc, b.vc, hc.exp_table_attn, c->att, st, b.seq_stride, &c->att_scratch, b.pos_stride);
        fq_launch_quantize_act(c->att, E, b.a_att, st);
    }
}
// The LayerNorm(s) in front of a block (and the output norm) come out of the PREVIOUS block's residual-sum launch where that is a launch of its own (the short prompts'
// two-stream form): next_norm(li) = what block li (li == #blocks: the head) needs; false: no such launch for it
static bool next_norm(falcon_hip_context * c, size_t li, int N, fq_next_norm & nn) {
    falcon_hip_model * m = c->m;
    const int64_t E = m->hp.n_embd;
    nn = fq_next_norm{};
    if (li == m->layers.size()) {
        if (!m->last_stage()) return false;
        nn.w0 = m->out_norm_w; nn.b0 = m->out_norm_b; nn.a0 = act_for(c->buf_e, m->lm_head, N);
        return fq_add2_ln_ok(nn, E);
    }
    const layer_weights & Ln = m->layers[li];
    nn.w0 = Ln.ln_w; nn.b0 = Ln.ln_b; nn.a0 = act_for(c->buf_e, Ln.up, N);
    if (m->hp.two_norms) { nn.w1 = Ln.ln2_w; nn.b1 = Ln.ln2_b; nn.a1 = act_for(c->buf_e2, Ln.qkv, N); return fq_add2_ln_ok(nn, E); }
    return fq_desc(Ln.qkv.type).act_type == nn.a0.type && fq_add2_ln_ok(nn, E);      // (one norm, two activation families: two images of it -- launch_stage's own launches)
}

// Which form a block takes, decided up front from the form rules (fq_mm_forms.h) and the context's modes.
//   BLOCK_COLUMNS: 2..cols_max_n(m) lock-step sequences (or rows of a verify pass): the block's weights in TWO launches that serve every column (kernels_cols.hip),
//     the decode attention of all sequences in one launch between them -- same bits as the generic launches. In chunks of 4 columns; beyond cols_max_n one pass of
//     the streaming small-batch mat-mul (kernels_gemm_skinny.hip, N <= 16) is cheaper: measured on Falcon-7B Q4_0 3.6 ms per pass of 8 in two chunks, 4.0 ms for 12
//     and 4.1 ms for 16 in one pass (the 128-token tile GEMM beyond 16: 8.3-9.2 ms for any N up to 64)
//   BLOCK_TWO_STREAMS: batched evaluation (N > 4): a block's two branches -- {Wqkv, RoPE, attention, Wo} and {Wup + GELU, Wdown} -- only meet in
//     the residual sum, and three of the four mat-muls of a short prompt launch fewer workgroups than the chip has CUs (142
//     for a 4544-row matrix and 128 tokens). They run on two streams: the MLP branch on the side stream, its Wdown (whose
//     epilogue adds Wo's result and the residual) after the attention branch. Same kernels, same bits. Measured in one
//     process on the same resident Falcon-7B Q4_0 (scripts/gpu_par2_ab.py), one stream -> two branches: 16 tokens 8.66 -> 7.83
//     ms, 32: 9.17 -> 8.13, 128: 9.41 -> 8.82, 512: 26.75 -> 24.59, 1024: 49.3 -> 47.3, 2048: 104.9 -> 101.7.
//     (not where the mat-muls are passes of the k-quants' small-batch forms: they fill the chip and share one partial-sum scratch -- nor where a legacy K-share
//     mat-mul of each branch would write that scratch at once: fq_mm_par2_scratch_clash)
//     (round 6: lock-step passes of more than 32 sequences as well -- the same launches of ~50-100 us each, the decode attention of all sequences in the attention branch;
//     FALCON_HIP_PAR2_SEQS=0: those in stream order, as before)
//     (from 17 tokens for prompts -- 32 tokens 4.86 -> 4.70 ms, 20: 4.70 -> 4.62 --, from 33 sequences for lock-step passes, whose launches sit in the step's hipGraph:
//     32 per pass 4.78 -> 5.0 ms with it; profiles/r06zu_ab_par2_min_n.txt. FALCON_HIP_PAR2_MIN_N=n: both from n)
static int cols_out_width(const stage_block & b) {      // columns per output launch of the column form (Falcon-40B width: 2), 0: none
    return b.L.down.type == b.L.wo.type ? fq_gemv_out_cols_width(b.L.wo.type, b.L.down.K, b.L.wo.K) : 0;
}
static block_form block_form_of(const falcon_hip_context * c, const stage_block & b) {
    const fq_mm_switches & sw = fq_mm_sw();
    const layer_weights & L = b.L;
    const int N = b.N;
    if ((b.seq_stride || b.verify_limit) && N >= 2 && N <= cols_max_n(c->m) && c->fused_decode && !fq_reference_order() && !fq_attn_f64() &&
        L.qkv.type == L.up.type && cols_out_width(b) > 0 && !b.f16) return BLOCK_COLUMNS;
    const int par2_min_n = sw.par2_min_n ? sw.par2_min_n : (b.seq_stride ? 33 : 17);
    if (!b.verify_limit && !b.f16 && (!b.seq_stride || sw.par2_seqs) && N >= par2_min_n && N <= c->par2_max_n && !fq_prof_active() && !fq_ctx().dbg_stamps &&
        !fq_mm_par2_scratch_clash(fq_mm_mat_of(L.qkv), fq_mm_mat_of(L.wo), fq_mm_mat_of(L.up), fq_mm_mat_of(L.down), N, fq_ctx().n_cu, b.md, sw)) return BLOCK_TWO_STREAMS;
    return BLOCK_GENERIC;
}

// x = (Wdown a_ff + Wo a_att) + x, in stream order: the column form's output launches (cw_out > 0), the paired K-share / fused sum launch (5..16 columns, or
// passes of it), or Wo into its own matrix and Wdown with the residual epilogue
static void block_output(falcon_hip_context * c, const stage_block & b, int cw_out) {
    const layer_weights & L = b.L;
    const int64_t E = c->m->hp.n_embd;
    const int n_cu = fq_ctx().n_cu;
    hipStream_t st = b.st;
    if (cw_out > 0 && fq_col_passes(b.N, cw_out, false, "column output mat-vec", [&](const fq_col_window & cw) {
            const fq_gemv_out_cols_args go{ L.down, L.wo, cw.act(b.a_ff).base, cw.act(b.a_att).base, cw.dst(c->x, E), cw.dst(c->x, E), E, (int) cw.n };
            return fq_launch_gemv_out_cols(go, n_cu, st); })) return;
    const int min_cols = b.seq_stride ? 3 : 5;                             // (lock-step contexts: the k-quant small-batch forms from 3 sequences up)
    if (!b.f16 && fq_mul_mat_q_acts_out2(L.wo, b.a_att, L.down, b.a_ff, b.N, c->x, E, st, min_cols)) return;
    const fq_gemv_epi resid{ FQ_EPI_ADD2, fq_ctx().gelu_table, c->wo_out, c->x, E };          // x = (down + wo) + x, in place
    mm(b, L.wo, b.a_att, c->wo_out, E, epi_store(), st);
    mm(b, L.down, b.a_ff, c->x, E, resid, st);
}
// the generic form, in stream order: Wqkv [+ Wup in the same launch], attention, Wup + GELU, its image, the output
static void block_generic(falcon_hip_context * c, const stage_block & b, int cw_out = 0) {
    const layer_weights & L = b.L;
    const falcon_hip_hparams & hp = c->m->hp;
    const int64_t QKV = n_qkv(hp), FF = hp.n_ff;
    hipStream_t st = b.st;
    // Wqkv and Wup behind the same LayerNorm image (one-norm blocks): one launch of the small-batch mat-mul for both (5..32 columns)
    const bool pair_done = !b.f16 && b.a_qkv.base == b.a_up.base && b.a_qkv.type == b.a_up.type &&
                           fq_mul_mat_q_acts_pair(L.qkv, L.up, b.a_up, b.N, c->qkv, QKV, epi_store(), c->up, FF, epi_gelu(), st);
    if (!pair_done) mm(b, L.qkv, b.a_qkv, c->qkv, QKV, epi_store(), st);
    const bool ride = b.seq_stride && !fq_reference_order() && !fq_attn_f64() && fq_mm_sw().quant_rider && pair_done && (b.a_ff.type == FQ_Q8_0 || b.a_ff.type == FQ_Q8_1);
    block_attention(c, b, ride);
    bool ff_quantized = ride;
    // (k-quants, 5..16 columns or passes of them: GELU and Wdown's Q8_K image come out of the small-batch form's sum launch)
    if (!pair_done) {
        const int min_cols = b.seq_stride ? 3 : 5;
        if (!b.f16 && fq_mul_mat_q_acts_gelu_q8k(L.up, b.a_up, b.N, c->up, FF, b.a_ff, st, min_cols)) ff_quantized = true;
        else mm(b, L.up, b.a_up, c->up, FF, epi_gelu(), st);
    }
    if (!ff_quantized) fq_launch_quantize_act(c->up, FF, b.a_ff, st);
    block_output(c, b, cw_out);
}
// the column form (block_form_of). A first launch that refuses the shape (its LDS) leaves the block to the generic launches, which still try the column output launch
static void block_columns(falcon_hip_context * c, const stage_block & b) {
    const layer_weights & L = b.L;
    const falcon_hip_hparams & hp = c->m->hp;
    const int64_t QKV = n_qkv(hp), FF = hp.n_ff;
    const int n_cu = fq_ctx().n_cu, cw_out = cols_out_width(b);
    const bool quant_epi = (b.a_ff.type == FQ_Q8_0 || b.a_ff.type == FQ_Q8_1) && FF % 32 == 0;
    if (!fq_col_passes(b.N, 4, false, "column mat-vec", [&](const fq_col_window & cw) {
            fq_gemv_cols_args ga{};
            ga.nseg = 2; ga.ncols = (int) cw.n; ga.gelu_table = fq_ctx().gelu_table;
            ga.seg[0] = { L.qkv, cw.act(b.a_qkv).base, FQ_LNEPI_STORE, cw.dst(c->qkv, QKV), QKV, nullptr, 0, 0 };
            ga.seg[1] = { L.up, cw.act(b.a_up).base, quant_epi ? FQ_LNEPI_GELU_QUANT : FQ_LNEPI_GELU_STORE, cw.dst(c->up, FF), FF, cw.act(b.a_ff).base, b.a_ff.type, 0 };
            return fq_launch_gemv_cols(ga, n_cu, b.st); })) { block_generic(c, b, cw_out); return; }
    block_attention(c, b, false);
    if (!quant_epi) fq_launch_quantize_act(c->up, FF, b.a_ff, b.st);
    block_output(c, b, cw_out);
}
// the two-stream form (block_form_of): the MLP branch on the side stream. true: the residual sum was a launch of its own and carried the next block's LayerNorm(s)
static bool block_two_streams(falcon_hip_context * c, const stage_block & b) {
    const layer_weights & L = b.L;
    const falcon_hip_hparams & hp = c->m->hp;
    hip_context & hc = fq_ctx();
    const int64_t E = hp.n_embd, QKV = n_qkv(hp), FF = hp.n_ff;
    const int N = b.N;
    const size_t li = b.li;
    hipStream_t st = b.st;
    HIP_CHECK(hipEventRecord(c->ev_fork[li], st));
    HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_fork[li], 0));
    mm(b, L.up, b.a_up, c->up, FF, epi_gelu(), c->side);
    fq_launch_quantize_act(c->up, FF, b.a_ff, c->side);
    mm(b, L.qkv, b.a_qkv, c->qkv, QKV, epi_store(), st);
    block_attention(c, b, false);
    // (round 6) Short prompts: neither branch waits for the other to carry the residual sum in an epilogue. Wdown -- the long launch of a short prompt (K = 4 n_embd,
    // 142 workgroups on 256 CUs at 128 tokens) -- follows Wup on the side stream and leaves its result in the (free again) f32 Wup matrix, Wo leaves its own, and
    // x = (down + wo) + x (libfalcon.cpp:2399-2400, the same additions in the same order) is a small launch behind the join.
    // Measured on MI355X, Falcon-7B Q4_0, epilogue form -> this (scripts/gpu_prompt_lengths.py, A/B/A/B on one box, profiles/r06zm_*): 40 tokens 6.80 -> 6.25 ms,
    // 64: 6.88 -> 6.40, 128: 8.17 -> 7.03 (18.2 k tok/s), 256: 14.3 -> 12.2, 512: 23.08 -> 23.00, 1024: 42.1 -> 41.6 -- but 384: 17.5 -> 18.2: Wdown's 426 workgroups
    // are 1.7 rounds of the chip there and the attention branch beside them only stretches the second. Hence: Wdown's launch at most 1.25 rounds or at least 2.
    // FALCON_HIP_PAR2_DOWN_FIRST=0: never (the epilogue form below), 2: always
    const int down_first = fq_mm_sw().par2_down_first;
    const int64_t down_wgs = fq_mm_gemm_wgs(fq_mm_mat_of(L.down), N, hc.n_cu, b.md, fq_mm_sw());      // (of the launch fq_launch_gemm will make: the same rules)
    if ((E & 3) == 0 && (down_first == 2 || (down_first == 1 && (4 * down_wgs <= 5 * (int64_t) hc.n_cu || down_wgs >= 2 * (int64_t) hc.n_cu)))) {
        mm(b, L.down, b.a_ff, c->up, E, epi_store(), c->side);
        HIP_CHECK(hipEventRecord(c->ev_join[li], c->side));
        mm(b, L.wo, b.a_att, c->wo_out, E, epi_store(), st);
        HIP_CHECK(hipStreamWaitEvent(st, c->ev_join[li], 0));
        fq_next_norm nn;
        if (next_norm(c, li + 1, N, nn)) { fq_launch_add2_ln(c->x, c->up, c->wo_out, E, N, nn, st); return true; }
        fq_launch_add2_inplace(c->x, c->up, c->wo_out, (int64_t) N * E, st);
        return false;
    }
    mm(b, L.wo, b.a_att, c->wo_out, E, epi_store(), st);
    HIP_CHECK(hipEventRecord(c->ev_attn[li], st));
    HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_attn[li], 0));
    const fq_gemv_epi resid{ FQ_EPI_ADD2, hc.gelu_table, c->wo_out, c->x, E };          // x = (down + wo) + x, in place
    mm(b, L.down, b.a_ff, c->x, E, resid, c->side);
    HIP_CHECK(hipEventRecord(c->ev_join[li], c->side));
    HIP_CHECK(hipStreamWaitEvent(st, c->ev_join[li], 0));
    return false;
}

static void launch_stage(falcon_hip_context * c, int N, int max_n_kv, hipStream_t st, int pos_stride = 0, int verify_limit = 0) {
    falcon_hip_model * m = c->m;
    const falcon_hip_hparams & hp = m->hp;
    const int64_t E = hp.n_embd, D = 64, HKV = hp.n_head_kv;

    if (m->first_stage()) fq_launch_dequant_rows(m->tok_emb, c->tokens_dev, N, c->x, st);    // ggml_get_rows, libfalcon.cpp:2120

    const int64_t seq_stride = c->n_seq > 0 ? (int64_t) c->n_ctx * HKV * D : 0;             // lock-step sequences: one KV cache per row
    const int64_t n_caches = c->n_seq > 0 ? c->n_seq : 1;
    if (c->n_seq > 0 && N != c->n_seq) { fprintf(stderr, "falcon-hip: a context of %d lock-step sequences evaluates %d rows per step, not %d\n", c->n_seq, c->n_seq, N); exit(1); }
    const int * seq_pos = pos_stride ? c->pos_dev : c->n_past_dev;                         // what the lock-step attention launches read
    if (pos_stride && !seq_stride) { fprintf(stderr, "falcon-hip: per-row positions need a lock-step context\n"); exit(1); }
    // the fused kernels are instantiated per weight format: a model that mixes formats inside a block (e.g. the reference's
    // Q4_K_M for Falcon-7B: only the 18176-wide Wdown can hold 256-element super-blocks) takes the op list
    if (N == 1 && stage_fused(c)) { launch_stage_token(c, max_n_kv, st); return; }
    // LayerNorm of x + the image its consumer takes. An F16 consumer (ggml_compute_forward_mul_mat_f16_f32's INIT phase, ggml.c:11176-11196): the f32 rows of
    // ggml_norm, mul, add, then their fp16 image (kernels_f16.hip)
    auto ln_image = [&](const float * w, const float * b, const fq_act & a, float * y = nullptr) {
        if (a.type == FQ_F16) { fq_launch_layer_norm(c->x, E, N, w, b, c->ln, st); fq_launch_quantize_act(c->ln, E, a, st); }
        else fq_launch_layer_norm_quant(c->x, E, N, w, b, y, a, st);                         // (y: the f32 rows, needed by the embeddings only)
    };
    bool ln_done = false;                                   // this block's LayerNorm image(s) came out of the previous block's residual-sum launch
    const fq_mm_mode md = fq_mm_mode_now();
    for (size_t li = 0; li < m->layers.size(); ++li) {
        const layer_weights & L = m->layers[li];
        if (c->keep_hidden) HIP_CHECK(hipMemcpyAsync(c->hidden_dev + li * (size_t) N * E, c->x, (size_t) N * E * 4, hipMemcpyDeviceToDevice, st));
        const fq_act a_up = act_for(c->buf_e, L.up, N);
        fq_act a_qkv = a_up;
        if (hp.two_norms) {                                                              // ln_mlp and ln_attn: one launch when both images are of one type
            a_qkv = act_for(c->buf_e2, L.qkv, N);
            if (ln_done) {
            } else if (a_up.type == FQ_F16 || a_qkv.type == FQ_F16 || !fq_launch_layer_norm_quant2(c->x, E, N, L.ln_w, L.ln_b, a_up, L.ln2_w, L.ln2_b, a_qkv, st)) {
                ln_image(L.ln_w, L.ln_b, a_up);
                ln_image(L.ln2_w, L.ln2_b, a_qkv);
            }
        } else if (!ln_done) ln_image(L.ln_w, L.ln_b, a_up);
        ln_done = false;
        if (hp.two_norms) {
        } else if (act_for(c->buf_e2, L.qkv, N).type != a_up.type) {                     // same norm, the other activation family
            a_qkv = act_for(c->buf_e2, L.qkv, N);
            ln_image(L.ln_w, L.ln_b, a_qkv);
        }
        const size_t cache_off = li * (size_t) n_caches * c->n_ctx * HKV * D;
        const stage_block b{ L, li, layer_has_f16(L), c->k_cache + cache_off, c->v_cache + cache_off, a_qkv, a_up, act_for(c->buf_att, L.wo, N), act_for(c->buf_ff, L.down, N),
                             N, max_n_kv, seq_pos, seq_stride, pos_stride, verify_limit, st, md };
        switch (block_form_of(c, b)) {
            case BLOCK_COLUMNS:     block_columns(c, b); break;
            case BLOCK_TWO_STREAMS: ln_done = block_two_streams(c, b); break;
            case BLOCK_GENERIC:     block_generic(c, b); break;
        }
    }
    if (c->keep_hidden) {
        HIP_CHECK(hipMemcpyAsync(c->hidden_dev + m->layers.size() * (size_t) N * E, c->x, (size_t) N * E * 4, hipMemcpyDeviceToDevice, st));
        c->hidden_tokens = N;
    }
    if (m->last_stage()) {
        const fq_act a_head = act_for(c->buf_e, m->lm_head, N);
        if (!ln_done) ln_image(m->out_norm_w, m->out_norm_b, a_head, c->emb_mode ? c->emb_rows : nullptr);
        if (c->emb_mode) {
            // the ln_f rows: out of the launch above (an F16 head's are in c->ln), or -- the last block's residual-sum launch made the head's image -- by one plain LayerNorm
            const float * rows = !ln_done && a_head.type == FQ_F16 ? c->ln : c->emb_rows;
            if (ln_done) fq_launch_layer_norm(c->x, E, N, m->out_norm_w, m->out_norm_b, c->emb_rows, st);
            HIP_CHECK(hipMemcpyAsync(c->emb, rows + (size_t)(N - 1) * E, (size_t) E * 4, hipMemcpyDeviceToDevice, st));      // libfalcon.cpp:2551-2557: the last token's
            if (c->emb_mode & FALCON_HIP_EMBED_POOL) fq_launch_embed_pool_accum(rows, N, (int) E, c->pool_acc, c->pool_count, st);
            if (c->emb_no_head) return;
        }
        // (2..cols_max_n rows of a lock-step context or a verify pass: the column mat-vec launch, as the blocks)
        if ((seq_stride || verify_limit) && N >= 2 && N <= cols_max_n(m) && c->fused_decode && !fq_reference_order() && m->lm_head.type != FQ_F16 &&
            fq_col_passes(N, 4, false, "column mat-vec (lm_head)", [&](const fq_col_window & cw) {
                fq_gemv_cols_args ga{};
                ga.nseg = 1; ga.ncols = (int) cw.n; ga.gelu_table = fq_ctx().gelu_table;
                ga.seg[0] = { m->lm_head, cw.act(a_head).base, FQ_LNEPI_STORE, cw.dst(c->logits_dev, hp.n_vocab), hp.n_vocab, nullptr, 0, 0 };
                return fq_launch_gemv_cols(ga, fq_ctx().n_cu, st); })) return;
        if (seq_stride) fq_mul_mat_q_acts_from3(m->lm_head, a_head, N, c->logits_dev, hp.n_vocab, epi_store(), st);      // all N rows, libfalcon.cpp:2440
        else fq_mul_mat_q_acts(m->lm_head, a_head, N, c->logits_dev, hp.n_vocab, epi_store(), st);
    }
}

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
        if (!c->score_tgt) {
            HIP_CHECK(hipMalloc((void **) &c->score_tgt, (size_t) c->n_batch * 4));
            HIP_CHECK(hipMalloc((void **) &c->score_prob, (size_t) c->n_batch * 4));
        }
        HIP_CHECK(hipMemcpyAsync(c->score_tgt, score_targets, (size_t) N * 4, hipMemcpyHostToDevice, st));
    }
    if (m->first_stage()) HIP_CHECK(hipMemcpyAsync(c->tokens_dev, tokens, (size_t) N * 4, hipMemcpyHostToDevice, st));
    else                  HIP_CHECK(hipMemcpyAsync(c->x, hidden_in_dev, (size_t) N * m->hp.n_embd * 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));        // n_past / tokens may live on the caller's stack
    // batches: one hipGraph replay per (size, keys) instead of ~10 launches and 3 cross-stream joins per block from the host
    if (graph_ok_batch(c, N)) {
        const int64_t sig = (int64_t)(graph_signature(c) | (c->keep_hidden ? 256 : 0)) + ((int64_t) fq_config_epoch() << 32);
        hipGraphExec_t exec = nullptr;
        for (const auto & bg : c->batch_graphs) if (bg.N == N && bg.max_kv == n_past + adv && bg.sig == sig) { exec = bg.exec; break; }
        if (!exec) {
            exec = capture_step(c, st, [&] { launch_stage(c, N, n_past + adv, st); });
            if (c->batch_graphs.size() >= 8) { HIP_CHECK(hipGraphExecDestroy(c->batch_graphs.front().exec)); c->batch_graphs.erase(c->batch_graphs.begin()); }
            c->batch_graphs.push_back({ N, n_past + adv, sig, exec });
        }
        HIP_CHECK(hipGraphLaunch(exec, st));
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
            fq_launch_score(c->logits_dev, V, N, (int) V, c->score_tgt, c->score_prob, nullptr, nullptr, st);
            c->score_host.resize((size_t) N);
            HIP_CHECK(hipMemcpyAsync(c->score_host.data(), c->score_prob, (size_t) N * 4, hipMemcpyDeviceToHost, st));
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
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: eval_score: this context holds no lm_head\n"); return 1; }
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
static bool emb_refuses(const falcon_hip_context * c, const char * what) {
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
        c->sync_err_host = *(const unsigned *)(c->logits_pinned + c->m->hp.n_vocab);
        c->logits_pending = false;
        (void) report_sync_error(c, "eval");                        // sticky: falcon_hip_context_last_error / the next eval report it (this call cannot)
    }
    return c->logits_last ? c->logits_last : c->logits_host.data();
}
// 0, or 3 when a step of this context lost an in-launch hand-off (every result since is invalid). Host state only: callers of
// falcon_hip_get_logits, which cannot fail, ask here after it.
extern "C" int falcon_hip_context_last_error(const falcon_hip_context * c) { return c->sync_err_sticky ? 3 : 0; }

__global__ void k_set_i32(int * p, int v);
__global__ void k_set2_i32(int * p, int v, int * q, int w);
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
        c->sync_err_host = *(const unsigned *)(c->logits_pinned + m->hp.n_vocab);
        c->logits_pending = false;
        if (report_sync_error(c, "eval")) return 3;
    }
    if (!c->logits_pinned) HIP_CHECK(hipHostMalloc((void **) &c->logits_pinned, (size_t) m->hp.n_vocab * 4 + 64, hipHostMallocDefault));      // (+ the hand-off error word: a copy into pageable memory would make this call wait for the whole step)
    hipLaunchKernelGGL(k_set2_i32, dim3(1), dim3(1), 0, st, c->n_past_dev, n_past, (int *) c->tokens_dev, (int) token);
    const bool was_keep = c->keep_hidden;
    c->keep_hidden = false;
    if (graph_ok_token(c)) {
        (c->emb_mode ? c->token_step_emb : c->token_step).replay(c, st, step_key_of(c), [&] { launch_stage(c, 1, c->n_ctx, st); });
    } else {
        launch_stage(c, 1, n_past + 1, st);
    }
    c->keep_hidden = was_keep;
    if (c->emb_mode) { c->emb_have = true; c->emb_host_fresh = false; }
    HIP_CHECK(hipMemcpyAsync(c->logits_pinned, c->logits_dev, (size_t) m->hp.n_vocab * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(c->logits_pinned + m->hp.n_vocab, c->sync_words + 1, 4, hipMemcpyDeviceToHost, st));
    c->logits_last = c->logits_pinned;
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

// ------------------------------------------------------------------------------------------------ pipeline step
__global__ void k_set_i32(int * p, int v) { *p = v; }
__global__ void k_set2_i32(int * p, int v, int * q, int w) { *p = v; *q = w; }
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
    const bool was_keep = c->keep_hidden;
    c->keep_hidden = false;
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
                else if (stage_fused(c))
                    hipLaunchKernelGGL(k_argmax_advance, dim3(1), dim3(256), 0, st, c->argmax_val, c->argmax_idx, (m->hp.n_vocab + 31) / 32, next_token_dev, c->n_past_dev, c->out_tokens_dev, n_past_base);
                else
                    hipLaunchKernelGGL(k_argmax_advance, dim3(1), dim3(1024), 0, st, c->logits_dev, (const int *) nullptr, m->hp.n_vocab, next_token_dev, c->n_past_dev, c->out_tokens_dev, n_past_base);
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
        const step_key key = step_key_of(c, { key_ptr(token_dev), key_ptr(hidden_in_dev), key_ptr(hidden_out_dev), key_ptr(next_token_dev) });
        if (!c->stage_step.holds(key)) c->step_next_n_past = -1;
        if (n_past != c->step_next_n_past) hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, st, c->n_past_dev, n_past);
        c->stage_step.replay(c, st, key, [&] { body(-1, c->n_ctx); });
        c->step_next_n_past = n_past + 1;
    } else {
        hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, st, c->n_past_dev, n_past);
        body(n_past, n_past + 1);
        c->step_next_n_past = -1;
    }
    c->keep_hidden = was_keep;
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

// K and V rows [0, n_tokens) of every local layer from one sequence's cache to another's. Lock-step caches are [layer][seq][n_ctx][HKV][64],
// plain ones [layer][n_ctx][HKV][64]: blockIdx.z = K / V, blockIdx.y = layer, n4 float4 per layer starting at the sequence's slot
// (one launch: a slot's layers lie up to n_seq x n_ctx rows apart, a pitch beyond what a 2-D memcpy is sure to take)
__global__ void __launch_bounds__(256) k_copy_seq_kv(float4 * __restrict__ dk, float4 * __restrict__ dv, int64_t d_layer4, const float4 * __restrict__ sk,
                                                     const float4 * __restrict__ sv, int64_t s_layer4, int64_t n4) {
    float4 * d = (blockIdx.z ? dv : dk) + (int64_t) blockIdx.y * d_layer4;
    const float4 * s = (blockIdx.z ? sv : sk) + (int64_t) blockIdx.y * s_layer4;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t) gridDim.x * blockDim.x) d[i] = s[i];
}
static int rope_table_key(const falcon_hip_context * c) { const int b = c->rope_n_ctx / 2048; return b > 1 ? b : 1; }      // (buckets 0 and 1: the same table)
extern "C" int falcon_hip_context_copy_seq(falcon_hip_context * dst, int dst_seq, const falcon_hip_context * src, int src_seq, int n_tokens) {
    if (!dst || !src || dst->m != src->m) { fprintf(stderr, "falcon-hip: copy_seq: the contexts hold different models\n"); return 1; }
    if (rope_table_key(dst) != rope_table_key(src)) { fprintf(stderr, "falcon-hip: copy_seq: the contexts rotate with different RoPE tables (rope_n_ctx %d / %d)\n", dst->rope_n_ctx, src->rope_n_ctx); return 1; }
    const int dn = dst->n_seq > 0 ? dst->n_seq : 1, sn = src->n_seq > 0 ? src->n_seq : 1;
    if (dst_seq < 0 || dst_seq >= dn || src_seq < 0 || src_seq >= sn) { fprintf(stderr, "falcon-hip: copy_seq: sequence %d of %d -> %d of %d is out of range\n", src_seq, sn, dst_seq, dn); return 1; }
    if (n_tokens < 0 || n_tokens > dst->n_ctx || n_tokens > src->n_ctx) { fprintf(stderr, "falcon-hip: copy_seq: %d rows exceed n_ctx (%d -> %d)\n", n_tokens, src->n_ctx, dst->n_ctx); return 1; }
    const int64_t nl = (int64_t) dst->m->layers.size(), row4 = (int64_t) dst->m->hp.n_head_kv * 16;      // float4 per cache row (HKV x 64 floats)
    if (n_tokens == 0 || nl == 0 || (dst == src && dst_seq == src_seq)) return 0;
    const int64_t dslot = (int64_t) dst->n_ctx * row4, sslot = (int64_t) src->n_ctx * row4;     // one sequence's cache of one layer
    const int64_t n4 = (int64_t) n_tokens * row4;
    const unsigned gx = (unsigned)((n4 + 255) / 256 < 1024 ? (n4 + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_copy_seq_kv, dim3(gx, (unsigned) nl, 2), dim3(256), 0, fq_ctx().stream,
                       (float4 *) dst->k_cache + dst_seq * dslot, (float4 *) dst->v_cache + dst_seq * dslot, dslot * dn,
                       (const float4 *) src->k_cache + src_seq * sslot, (const float4 *) src->v_cache + src_seq * sslot, sslot * sn, n4);
    return 0;
}

// ------------------------------------------------------------------------------------------------ sampled decode
// falcon_main's default sampler chain (kernels_sample.hip) in place of the argmax: one sampler row per sequence, its
// parameters, window and generator in device memory, so the loops below are the greedy ones with k_sample_rows as the
// step's last launch (one replay per step with falcon_hip_context_use_graph).
static ggml_hip_sampler * ctx_sampler(falcon_hip_context * c) {
    if (!c->sampler) c->sampler = ggml_hip_sampler_create(c->n_seq > 0 ? c->n_seq : 1, c->m->hp.n_vocab, c->n_ctx);
    if (c->sampler && c->m->vb_pool) fq_sampler_share_vocab_bytes(c->sampler, c->m->vb_pool, c->m->vb_offs);      // (the model's vocabulary may have come after the sampler)
    return c->sampler;
}

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
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: set_sampling: this context holds no lm_head\n"); return 1; }
    ggml_hip_sampler * s = ctx_sampler(c);
    const int rc = s ? ggml_hip_sampler_set_row(s, seq, params, history, n_history) : 1;
    return rc ? rc : take_kept_rng(c, s, seq);
}

extern "C" int falcon_hip_context_set_sampling_ext(falcon_hip_context * c, int seq, const ggml_hip_sampling_ext * params, const int32_t * history, int n_history) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: set_sampling_ext: this context holds no lm_head\n"); return 1; }
    ggml_hip_sampler * s = ctx_sampler(c);
    const int rc = s ? ggml_hip_sampler_set_row_ext(s, seq, params, history, n_history) : 1;
    return rc ? rc : take_kept_rng(c, s, seq);
}
extern "C" int falcon_hip_context_get_mirostat_mu(falcon_hip_context * c, float * mu_out) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: get_mirostat_mu: this context holds no lm_head\n"); return 1; }
    ggml_hip_sampler * s = ctx_sampler(c);
    return s ? ggml_hip_sampler_get_mu(s, mu_out) : 1;
}

extern "C" int falcon_hip_context_copy_sampling(falcon_hip_context * dst, int dst_seq, falcon_hip_context * src, int src_seq) {
    if (!dst || !src || !dst->m->last_stage() || !src->m->last_stage()) { fprintf(stderr, "falcon-hip: copy_sampling: a context without an lm_head\n"); return 1; }
    ggml_hip_sampler * d = ctx_sampler(dst), * s = ctx_sampler(src);
    return d && s ? ggml_hip_sampler_copy_row(d, dst_seq, s, src_seq) : 1;
}

// ---- stops (fq_stop.h): the rows' sequences, budgets and state belong to the sampler; the loop's early exit is decode_loop's
extern "C" int falcon_hip_context_set_stops(falcon_hip_context * c, int seq, const ggml_hip_stops * stops) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: set_stops: this context holds no lm_head\n"); return 1; }
    const int n_rows = c->n_seq > 0 ? c->n_seq : 1;
    if (!stops && !c->sampler) {                            // off on a context that never sampled: nothing to turn off, and no sampler is made for it
        if (seq < 0 || seq >= n_rows) { fprintf(stderr, "falcon-hip: set_stops: bad sequence %d\n", seq); return 1; }
        return 0;
    }
    ggml_hip_sampler * s = ctx_sampler(c);
    return s ? ggml_hip_sampler_set_stops(s, seq, stops) : 1;
}
extern "C" int falcon_hip_context_get_stops(falcon_hip_context * c, int32_t * n_drawn_out, int32_t * reason_out) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: get_stops: this context holds no lm_head\n"); return 1; }
    if (!c->sampler) {                                      // never sampled: every sequence running with nothing drawn (no sampler is made to say so)
        for (int t = 0; t < (c->n_seq > 0 ? c->n_seq : 1); ++t) { if (n_drawn_out) n_drawn_out[t] = 0; if (reason_out) reason_out[t] = FQ_STOP_RUNNING; }
        return 0;
    }
    ggml_hip_sampler * s = ctx_sampler(c);
    return s ? ggml_hip_sampler_get_stops(s, n_drawn_out, reason_out) : 1;
}
// ---- stop strings (fq_stop_text.h): the vocabulary's bytes belong to the model, the rows' strings and rings to the sampler
extern "C" int falcon_hip_model_set_vocab(falcon_hip_model * m, const falcon_hip_vocab * v) {
    if (!m || !v) return 1;
    if (!m->last_stage()) { fprintf(stderr, "falcon-hip: model_set_vocab: this model holds no lm_head\n"); return 1; }
    const int n = falcon_hip_vocab_size(v);
    if (n != m->hp.n_vocab) { fprintf(stderr, "falcon-hip: model_set_vocab: a vocabulary of %d tokens for a model with n_vocab %d\n", n, m->hp.n_vocab); return 1; }
    std::vector<int32_t> offs((size_t) n + 1, 0);
    std::vector<uint8_t> pool;
    for (int t = 0; t < n; ++t) {
        const char * b = nullptr;
        const int l = falcon_hip_token_to_bytes(v, t, &b);
        if ((int64_t) pool.size() + l > INT32_MAX) { fprintf(stderr, "falcon-hip: model_set_vocab: the tokens' bytes do not fit 32-bit offsets\n"); return 1; }
        pool.insert(pool.end(), (const uint8_t *) b, (const uint8_t *) b + l);
        offs[(size_t) t + 1] = (int32_t) pool.size();
    }
    uint8_t * pd = nullptr; int32_t * od = nullptr;
    if (fq_vocab_bytes_upload("falcon-hip: model_set_vocab", pool.data(), offs.data(), n, &pd, &od)) return 1;
    m->allocs.push_back(pd); m->allocs.push_back(od);       // (arrays this call replaces stay until the model goes: a context's sampler may still hold them)
    m->vb_pool = pd; m->vb_offs = od;
    return 0;
}
extern "C" int falcon_hip_context_set_stop_text(falcon_hip_context * c, int seq, const ggml_hip_stop_text * text) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: set_stop_text: this context holds no lm_head\n"); return 1; }
    const int n_rows = c->n_seq > 0 ? c->n_seq : 1;
    if (!text && !c->sampler) {                             // off on a context that never sampled: nothing to turn off, and no sampler is made for it
        if (seq < 0 || seq >= n_rows) { fprintf(stderr, "falcon-hip: set_stop_text: bad sequence %d\n", seq); return 1; }
        return 0;
    }
    if (text && !c->m->vb_pool) { fprintf(stderr, "falcon-hip: set_stop_text: the model has no vocabulary (falcon_hip_model_set_vocab)\n"); return 1; }
    ggml_hip_sampler * s = ctx_sampler(c);
    return s ? ggml_hip_sampler_set_stop_text(s, seq, text) : 1;
}
extern "C" int falcon_hip_context_get_stop_text(falcon_hip_context * c, int32_t * cut_bytes_out) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: get_stop_text: this context holds no lm_head\n"); return 1; }
    if (!cut_bytes_out) return 1;
    if (!c->sampler) {                                      // never sampled: no sequence has ended by text
        for (int t = 0; t < (c->n_seq > 0 ? c->n_seq : 1); ++t) cut_bytes_out[t] = 0;
        return 0;
    }
    return ggml_hip_sampler_get_stop_text(c->sampler, cut_bytes_out);
}
// ---- grammars (fq_grammar.h): a grammar is indexed with the model's vocabulary and keeps its own copy; the rows' bindings and states belong to the sampler
extern "C" ggml_hip_grammar * falcon_hip_grammar_create(falcon_hip_model * m, const ggml_hip_dfa * dfa, int eos_id, int * bad_state) {
    if (bad_state) *bad_state = -1;
    if (!m || !m->vb_pool) { fprintf(stderr, "falcon-hip: grammar_create: the model has no vocabulary (falcon_hip_model_set_vocab)\n"); return nullptr; }
    return fq_grammar_make("falcon-hip: grammar_create", m->hp.n_vocab, m->vb_pool, m->vb_offs, true, dfa, eos_id, bad_state);
}
extern "C" int falcon_hip_grammar_free(ggml_hip_grammar * g) { return ggml_hip_grammar_free(g); }
extern "C" int falcon_hip_context_set_grammar(falcon_hip_context * c, int seq, ggml_hip_grammar * g, int state) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: set_grammar: this context holds no lm_head\n"); return 1; }
    const int n_rows = c->n_seq > 0 ? c->n_seq : 1;
    if (!g && !c->sampler) {                                // off on a context that never sampled: nothing to turn off, and no sampler is made for it
        if (seq < 0 || seq >= n_rows) { fprintf(stderr, "falcon-hip: set_grammar: bad sequence %d\n", seq); return 1; }
        return 0;
    }
    if (g && c->spec_K > 0) { fprintf(stderr, "falcon-hip: set_grammar: draft-and-verify decode is on (falcon_hip_context_set_spec) and applies no grammar: turn it off first\n"); return 1; }
    ggml_hip_sampler * s = ctx_sampler(c);
    return s ? ggml_hip_sampler_set_grammar(s, seq, g, state) : 1;
}
extern "C" int falcon_hip_context_get_grammar_state(falcon_hip_context * c, int32_t * states_out) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: get_grammar_state: this context holds no lm_head\n"); return 1; }
    if (!states_out) return 1;
    if (!c->sampler) {                                      // never sampled: no sequence holds a grammar
        for (int t = 0; t < (c->n_seq > 0 ? c->n_seq : 1); ++t) states_out[t] = -1;
        return 0;
    }
    return ggml_hip_sampler_get_grammar_state(c->sampler, states_out);
}
extern "C" void falcon_hip_context_set_stop_poll(falcon_hip_context * c, int every_steps) { c->stop_poll = every_steps < 1 ? 1 : every_steps; }
extern "C" int falcon_hip_context_loop_steps(const falcon_hip_context * c) { return c->loop_steps; }

// ---- log-probabilities (kernels_logprob.hip): one launch behind the sampler's, which has written the chosen tokens and advanced the step counters
static void lp_drop(falcon_hip_context * c) {               // frees the record buffers (the sampled loops' slots carry the addresses in their keys)
    HIP_CHECK(hipStreamSynchronize(fq_ctx().stream));
    for (void * p : { (void *) c->lp_prob, (void *) c->lp_top_id, (void *) c->lp_top_prob }) if (p) HIP_CHECK(hipFree(p));
    c->lp_prob = c->lp_top_prob = nullptr; c->lp_top_id = nullptr;
    c->lp_cap = 0; c->lp_steps = c->lp_rows = 0;
}
static void lp_reserve(falcon_hip_context * c, int64_t records) {      // (outside any capture)
    if (c->lp_n_top < 0 || records <= c->lp_cap) return;
    const int n_top = c->lp_n_top;
    lp_drop(c);
    c->lp_cap = records;
    HIP_CHECK(hipMalloc((void **) &c->lp_prob, (size_t) records * 4));
    if (n_top > 0) {
        HIP_CHECK(hipMalloc((void **) &c->lp_top_id, (size_t) records * n_top * 4));
        HIP_CHECK(hipMalloc((void **) &c->lp_top_prob, (size_t) records * n_top * 4));
    }
}
// rows' records at step (steps[r] - 1) of a loop whose sampler launch has just advanced steps, or (steps == nullptr) at step 0
// (a row the sampler's launch skipped because it had ended keeps the records it has: the launch gets the sampler's skip words)
static void lp_launch(falcon_hip_context * c, int n_rows, const float * logits, const int32_t * chosen, const int * steps, hipStream_t st) {
    fq_launch_logprob(logits, c->m->hp.n_vocab, n_rows, c->m->hp.n_vocab, chosen, c->lp_n_top, steps, -1, n_rows, c->lp_cap,
                      c->lp_prob, c->lp_top_id, c->lp_top_prob, nullptr, nullptr, st, fq_sampler_stop_skip(c->sampler));
}

extern "C" int falcon_hip_context_set_logprobs(falcon_hip_context * c, int n_top) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: set_logprobs: this context holds no lm_head\n"); return 1; }
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
    HIP_CHECK(hipMemcpyAsync(prob_out, c->lp_prob, n * 4, hipMemcpyDeviceToHost, st));
    if (c->lp_n_top > 0 && top_id_out) HIP_CHECK(hipMemcpyAsync(top_id_out, c->lp_top_id, n * c->lp_n_top * 4, hipMemcpyDeviceToHost, st));
    if (c->lp_n_top > 0 && top_prob_out) HIP_CHECK(hipMemcpyAsync(top_prob_out, c->lp_top_prob, n * c->lp_n_top * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int falcon_hip_sample(falcon_hip_context * c, int32_t * out) {
    falcon_hip_model * m = c->m;
    if (!m->last_stage()) { fprintf(stderr, "falcon-hip: sample: this context holds no lm_head\n"); return 1; }
    ggml_hip_sampler * s = ctx_sampler(c);
    if (!s) return 1;
    hipStream_t st = fq_ctx().stream;
    const int64_t V = m->hp.n_vocab;
    const int B = c->n_seq > 0 ? c->n_seq : 1;
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
// ended() says so. The steps run in chunks of E = stop_poll; behind chunk j copy_state(j & 1) copies the device state into the page-locked image j & 1 and an
// event is recorded, between two replays, never inside the captured step. Chunk j + 2 is enqueued only after chunk j's event has passed and ended(j & 1) is
// false for its image, so the device always has a chunk queued while the host waits, and a loop that ends at step k (0-based) launches at most
// (k / E + 2) * E steps: at most two intervals past the end. An event waited for was always recorded by THIS call: the wait at step s = (j + 2) * E < n
// is for chunk j's record, made at step (j + 1) * E - 1 under the condition (j + 1) * E < n, which s < n implies -- never one left over from an
// earlier call. Returns the steps launched.
template <class Step, class Copy, class Ended>
static int run_polled(int n, int E, bool poll, hipEvent_t * ev, hipStream_t st, Step && step, Copy && copy_state, Ended && ended) {
    int s = 0;
    for (; s < n; ++s) {
        if (poll && s % E == 0 && s >= 2 * E) {
            const int img = (s / E) & 1;
            HIP_CHECK(hipEventSynchronize(ev[img]));
            if (ended(img)) break;
        }
        step();
        if (poll && (s + 1) % E == 0 && s + 1 < n) {
            const int img = (s / E) & 1;
            copy_state(img);
            HIP_CHECK(hipEventRecord(ev[img], st));
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
        int32_t * old = c->seq_out_dev;
        c->seq_out_cap = out_need;
        HIP_CHECK(hipMalloc((void **) &c->seq_out_dev, (size_t) c->seq_out_cap * 4));
        if (old) HIP_CHECK(hipFree(old));
    }
    if (sampled) lp_reserve(c, ragged ? (int64_t) n_steps * B : c->n_ctx);      // (single stream: as out_tokens_dev, any n_steps of this context)
    int * pos = ragged ? c->pos_dev : c->n_past_dev;
    int * steps = ragged ? c->seq_steps_dev : sampled ? fq_sampler_steps(sm) : nullptr;
    int32_t * out_dev = ragged ? c->seq_out_dev : c->out_tokens_dev;
    int max_pos = 0;
    for (int t = 0; t < B; ++t) max_pos = n_past[t] > max_pos ? n_past[t] : max_pos;
    HIP_CHECK(hipMemcpyAsync(pos, n_past, (size_t) B * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->tokens_dev, first_tokens, (size_t) B * 4, hipMemcpyHostToDevice, st));
    if (steps) HIP_CHECK(hipMemsetAsync(steps, 0, (size_t) B * 4, st));
    // stops: with any row of the context holding some, a row that ends writes nothing more (its output reads -1 from there on) and rides the pass frozen:
    // its token is evaluated again at its position, which rewrites the same K / V row. Once EVERY row holds stops the loop may end early -- poll.
    const int stop_rows = sampled ? fq_sampler_stop_rows(sm) : 0;
    const bool poll = stop_rows == B;
    if (stop_rows > 0) HIP_CHECK(hipMemsetAsync(out_dev, 0xff, (size_t) n_steps * B * 4, st));
    if (poll && !c->stop_host) {
        HIP_CHECK(hipHostMalloc((void **) &c->stop_host, sizeof(fq_stop_state) * 2 * B, hipHostMallocDefault));
        for (hipEvent_t & e : c->stop_ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIP_CHECK(hipStreamSynchronize(st));        // (the arrays may live on the caller's stack)
    const bool was_keep = c->keep_hidden;
    c->keep_hidden = false;
    auto one_step = [&](int max_kv) {
        launch_stage(c, B, max_kv, st, ragged ? 1 : 0);
        if (sampled) {
            fq_launch_sample(sm, B, c->logits_dev, m->hp.n_vocab, c->tokens_dev, pos, steps, out_dev, B, st);
            // (the next step's lm_head is ordered behind it; under a context stop a row that ends at the end of its cache keeps its tokens_dev entry: the draws are the sampler's)
            if (c->lp_n_top >= 0) lp_launch(c, B, c->logits_dev, fq_sampler_ctx_limit(sm) > 0 ? fq_sampler_tokens(sm) : c->tokens_dev, steps, st);
        } else if (ragged)
            hipLaunchKernelGGL(k_argmax_rows_step, dim3((unsigned) B), dim3(1024), 0, st, c->logits_dev, m->hp.n_vocab, c->tokens_dev, pos, steps, out_dev, B);
        else if (stage_fused(c))
            hipLaunchKernelGGL(k_argmax_advance, dim3(1), dim3(256), 0, st, c->argmax_val, c->argmax_idx, (m->hp.n_vocab + 31) / 32, c->tokens_dev, pos, out_dev, n_past[0]);
        else
            hipLaunchKernelGGL(k_argmax_advance, dim3(1), dim3(1024), 0, st, c->logits_dev, (const int *) nullptr, m->hp.n_vocab, c->tokens_dev, pos, out_dev, n_past[0]);
    };
    // n_steps steps, or fewer when every row has ended (run_polled). (The whole 40-byte states are copied, not the reason words alone: one contiguous copy, and
    // the same bytes get_stops reads.)
    auto run_steps = [&](auto && step) {
        c->loop_steps = run_polled(n_steps, c->stop_poll, poll, c->stop_ev, st, step,
            [&](int img) { HIP_CHECK(hipMemcpyAsync(c->stop_host + img * B, fq_sampler_stop_state(sm), sizeof(fq_stop_state) * B, hipMemcpyDeviceToHost, st)); },
            [&](int img) { bool running = false; for (int t = 0; t < B; ++t) running |= !fq_stop_finished(&c->stop_host[img * B + t]); return !running; });
    };
    if (ragged ? graph_ok_seqs(c) : graph_ok_loop(c)) {
        // positions, output slots and the sampler's state are read from device memory, so one capture, sized for the whole context, serves any call -- but
        // for the single-stream argmax, whose k_argmax_advance takes the base position as an argument
        step_key key = step_key_of(c, { ragged ? key_ptr(out_dev) : sampled ? 0 : n_past[0] });
        if (sampled) { key.baked[1] = key_ptr(c->lp_prob); key.baked[2] = key_ptr(c->lp_top_id); key.baked[3] = key_ptr(c->lp_top_prob); key.baked[4] = c->lp_n_top; key.baked[5] = c->lp_cap; }      // (lp_cap: an argument of the record launch)
        if (sampled) { key.baked[6] = key_ptr(fq_sampler_stop_cfg(sm)); key.baked[7] = key_ptr(fq_sampler_stop_state(sm)); key.baked[8] = key_ptr(fq_sampler_stop_skip(sm)); }      // (0 while no row has stops: turning them on or off re-captures; a row's sequences and budget are device data)
        if (sampled) key.baked[9] = fq_sampler_ext_rows(sm) > 0;      // (which instantiation of the sampler's kernel the step holds)
        if (sampled) fq_sampler_stop_text_key(sm, key.baked + 10);    // (stop strings: the rows' strings and rings, the vocabulary's bytes; 0 while no row has any -- the instantiation again)
        if (sampled) key.baked[14] = fq_sampler_ctx_limit(sm);        // (the context stop: an argument of the sampler's launch, 0 while off)
        if (sampled) key.baked[15] = key_ptr(fq_sampler_grammar_key(sm));      // (grammars: the rows' bindings, 0 while no row has one -- the instantiation again; a row's grammar and state are device data)
        step_slot & slot = ragged ? (sampled ? c->sample_seqs_step : c->seqs_step) : (sampled ? c->sample_step : c->decode_step);
        run_steps([&] { slot.replay(c, st, key, [&] { one_step(c->n_ctx); }); });
    } else {
        run_steps([&] { one_step(max_pos + n_steps < c->n_ctx ? max_pos + n_steps : c->n_ctx); });      // (beyond n_ctx only under a context stop: no row gets there)
    }
    HIP_CHECK(hipMemcpyAsync(out_tokens, out_dev, (size_t) n_steps * B * 4, hipMemcpyDeviceToHost, st));
    fetch_sync_error(c, st);
    HIP_CHECK(hipStreamSynchronize(st));
    c->keep_hidden = was_keep;
    if (!ragged) c->last_rows = 1;              // (falcon_hip_sample: the last step's row)
    if (!sampled) c->lp_steps = 0;              // (the greedy loops record no log-probabilities)
    else if (c->lp_n_top >= 0) { c->lp_steps = n_steps; c->lp_rows = B; }
    return report_sync_error(c, where);
}

// the context stop (falcon_hip_context_set_context_stop) is on: the sampled loops take any n_steps, a row ends at the end of its cache
static bool context_stop_on(const falcon_hip_context * c) { return c->sampler && fq_sampler_ctx_limit(c->sampler) > 0; }

extern "C" int falcon_hip_decode_sample(falcon_hip_context * c, int32_t first_token, int n_past, int n_steps, int32_t * out_tokens) {
    if (emb_refuses(c, "decode_sample")) return 1;
    if (!c->m->first_stage() || !c->m->last_stage()) { fprintf(stderr, "falcon-hip: sampled decode needs the whole model in one process\n"); exit(1); }
    if (context_stop_on(c) && n_past >= 0 && n_past < c->n_ctx && n_steps > c->n_ctx - n_past) {
        // the row ends at the end of its cache at the latest: the steps behind that would find it frozen and write -1
        const int n_run = c->n_ctx - n_past;
        for (int i = n_run; i < n_steps; ++i) out_tokens[i] = -1;
        n_steps = n_run;
    }
    if (n_past + n_steps > c->n_ctx) { fprintf(stderr, "falcon-hip: decode past n_ctx\n"); exit(1); }
    return decode_loop(c, false, true, &first_token, &n_past, n_steps, out_tokens, "sampled decode");
}

extern "C" int falcon_hip_decode_sample_seqs(falcon_hip_context * c, const int32_t * first_tokens, const int32_t * n_past, int n_steps, int32_t * out_tokens) {
    if (n_steps < 1) { fprintf(stderr, "falcon-hip: decode_sample_seqs: n_steps %d < 1\n", n_steps); return 1; }
    if (context_stop_on(c)) {
        // every sequence needs room for ONE step; each ends at the end of its own cache at the latest, so the steps behind the last such end are all -1
        if (const int rc = seqs_check(c, "decode_sample_seqs", first_tokens, n_past, 1)) return rc;
        const int B = c->n_seq > 0 ? c->n_seq : 1;
        int n_run = 1;
        for (int t = 0; t < B; ++t) n_run = c->n_ctx - n_past[t] > n_run ? c->n_ctx - n_past[t] : n_run;
        if (n_steps > n_run) {
            for (int64_t i = (int64_t) n_run * B; i < (int64_t) n_steps * B; ++i) out_tokens[i] = -1;
            n_steps = n_run;
        }
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
        HIP_CHECK(hipHostMalloc((void **) &c->spec_host, sizeof(fq_spec_state) * 2, hipHostMallocDefault));
        for (hipEvent_t & e : c->spec_ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
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
    if (context_stop_on(c) && n_tokens > c->n_ctx - n_past) {
        // the row ends at the end of its cache at the latest: nothing is drawn behind that
        for (int i = c->n_ctx - n_past; i < n_tokens; ++i) out_tokens[i] = -1;
        n_tokens = c->n_ctx - n_past;
    }
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
    const bool was_keep = c->keep_hidden;
    c->keep_hidden = false;
    auto one_pass = [&] {
        launch_stage(c, K + 1, c->n_ctx, st, 0, c->n_ctx);
        fq_launch_verify(sm, sp, c->logits_dev, m->hp.n_vocab, c->tokens_dev, c->n_past_dev, steps, out_dev, st);
    };
    step_key key = step_key_of(c, { (int64_t) K | ((int64_t) c->spec_source << 8) | ((int64_t) c->spec_gmin << 16) | ((int64_t) c->spec_gmax << 24), key_ptr(c->spec_state), key_ptr(c->spec_hist) });
    key.baked[6] = key_ptr(fq_sampler_stop_cfg(sm)); key.baked[7] = key_ptr(fq_sampler_stop_state(sm)); key.baked[8] = key_ptr(fq_sampler_stop_skip(sm));
    key.baked[9] = fq_sampler_ext_rows(sm) > 0;
    fq_sampler_stop_text_key(sm, key.baked + 10);
    key.baked[14] = fq_sampler_ctx_limit(sm);
    const bool graph = c->use_graph && graph_ok_strict();
    // at most n_tokens passes (one draw each), fewer when the budget is spent or the row's stops end it: the state is polled as decode_loop polls the rows' stops
    // (run_polled), so at most two intervals of passes run past the end (they draw nothing: the verify launch leaves a row without budget, or ended, as it is)
    c->loop_steps = run_polled(n_tokens, c->stop_poll, true, c->spec_ev, st, [&] { if (graph) c->spec_step.replay(c, st, key, one_pass); else one_pass(); },
        [&](int img) { HIP_CHECK(hipMemcpyAsync(c->spec_host + img, c->spec_state, sizeof(fq_spec_state), hipMemcpyDeviceToHost, st)); },
        [&](int img) { return c->spec_host[img].left == 0 || c->spec_host[img].ended != 0; });
    int drawn = 0;
    HIP_CHECK(hipMemcpyAsync(out_tokens, out_dev, (size_t) n_tokens * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&drawn, steps, 4, hipMemcpyDeviceToHost, st));
    fetch_sync_error(c, st);
    HIP_CHECK(hipStreamSynchronize(st));
    if (n_out) *n_out = drawn;
    c->keep_hidden = was_keep;
    c->last_rows = 1;
    c->lp_steps = 0;
    return report_sync_error(c, "decode_spec");
}

// ------------------------------------------------------------------------------------------------ context swap (fq_ctx_swap.h)
// falcon_main's way past n_ctx (falcon_main.cpp:694-751): the planner is host arithmetic; the context stop ends a row at the end of its cache inside the
// sampler's launch (kernels_sample.hip); the swap evaluates the regenerated tokens through the prefill path and lets the row run again.
static_assert(sizeof(falcon_hip_swap_cfg) == sizeof(fq_swap_cfg) && offsetof(falcon_hip_swap_cfg, prompt_size) == offsetof(fq_swap_cfg, prompt_size), "include/falcon-hip.h restates csrc/fq_ctx_swap.h's configuration");
extern "C" int falcon_hip_swap_plan(const falcon_hip_swap_cfg * cfg, int n_history, int n_pending, int * n_past_new, int * n_regen) {
    return fq_swap_plan((const fq_swap_cfg *) cfg, n_history, n_pending, n_past_new, n_regen);
}
extern "C" int falcon_hip_swap_history(const int32_t * prompt, int n_prompt, int n_batch, int32_t * history_out) {
    return fq_swap_history(prompt, n_prompt, n_batch, history_out);
}

extern "C" int falcon_hip_context_set_context_stop(falcon_hip_context * c, int on) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: set_context_stop: this context holds no lm_head\n"); return 1; }
    if (!on && !c->sampler) return 0;                       // off on a context that never sampled: nothing to turn off, and no sampler is made for it
    ggml_hip_sampler * s = ctx_sampler(c);
    return s ? ggml_hip_sampler_set_context_stop(s, on ? c->n_ctx : 0) : 1;
}
extern "C" int falcon_hip_context_resume(falcon_hip_context * c, int seq) {
    if (!c->m->last_stage()) { fprintf(stderr, "falcon-hip: resume: this context holds no lm_head\n"); return 1; }
    if (!c->sampler) { fprintf(stderr, "falcon-hip: resume: sequence %d did not end at the end of its cache (the context never sampled)\n", seq); return 1; }
    return ggml_hip_sampler_resume(c->sampler, seq);
}

// What the reference does to the V rows it "keeps" (libfalcon.cpp:2255-2281). It stores V transposed and packed to the CURRENT length: element (t, hd) of a
// layer -- hd = head * 64 + d -- lies at hd * (n_past + N) + t, and every eval re-packs the rows before it, read as a view of stride n_past, behind the new
// stride. That view is right while n_past is what the last eval left. After a swap it is not: the buffer is packed for n_ctx positions and is read with stride
// nk, so "kept" element (t, hd), t < nk, becomes element number hd * nk + t of the packed buffer -- position (hd * nk + t) % n_ctx of feature
// (hd * nk + t) / n_ctx. K is stored by position and is kept as it is. In the reference orders the library computes what the reference computes, so the swap
// re-packs V the same way there, once, before anything is evaluated: gather into a buffer of the call, then write rows [0, nk). (The sources span the whole
// slot, the destinations are its first nk rows; nk <= n_ctx keeps (hd * nk + t) / n_ctx below the row's width.)
__global__ void __launch_bounds__(256) k_swap_v_gather(float * __restrict__ tmp, const float * __restrict__ v, int64_t layer_stride, int nk, int n_ctx, int row) {
    const float * src = v + (int64_t) blockIdx.y * layer_stride;
    float * dst = tmp + (int64_t) blockIdx.y * nk * row;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nk * row; i += gridDim.x * blockDim.x) {
        const int t = i / row, hd = i % row, f = hd * nk + t;
        dst[i] = src[(int64_t)(f % n_ctx) * row + f / n_ctx];
    }
}
__global__ void __launch_bounds__(256) k_swap_v_put(float * __restrict__ v, const float * __restrict__ tmp, int64_t layer_stride, int n) {
    float * dst = v + (int64_t) blockIdx.y * layer_stride;
    const float * src = tmp + (int64_t) blockIdx.y * n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
}
static void swap_v_repack(falcon_hip_context * c, int seq, int nk) {
    const int nl = (int) c->m->layers.size(), row = c->m->hp.n_head_kv * 64, B = c->n_seq > 0 ? c->n_seq : 1;
    if (nl == 0 || nk <= 0) return;
    hipStream_t st = fq_ctx().stream;
    const int64_t slot = (int64_t) c->n_ctx * row;
    float * tmp = nullptr;
    HIP_CHECK(hipMalloc((void **) &tmp, (size_t) nl * nk * row * 4));
    const unsigned gx = (unsigned)(((int64_t) nk * row + 255) / 256 < 256 ? ((int64_t) nk * row + 255) / 256 : 256);
    hipLaunchKernelGGL(k_swap_v_gather, dim3(gx, (unsigned) nl), dim3(256), 0, st, tmp, c->v_cache + seq * slot, slot * B, nk, c->n_ctx, row);
    hipLaunchKernelGGL(k_swap_v_put, dim3(gx, (unsigned) nl), dim3(256), 0, st, c->v_cache + seq * slot, tmp, slot * B, nk * row);
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipFree(tmp));
}

extern "C" int falcon_hip_context_swap(falcon_hip_context * c, int seq, int n_past_new, const int32_t * regen, int n_regen, int n_batch) {
    falcon_hip_model * m = c->m;
    const int B = c->n_seq > 0 ? c->n_seq : 1;
    if (emb_refuses(c, "context_swap")) return 1;
    if (!m->first_stage() || !m->last_stage()) { fprintf(stderr, "falcon-hip: context_swap: a pipeline stage holds part of the layers; a swap evaluates through all of them\n"); return 1; }
    if (seq < 0 || seq >= B) { fprintf(stderr, "falcon-hip: context_swap: sequence %d of %d is out of range\n", seq, B); return 1; }
    if (n_past_new < 0 || n_regen < 0 || n_batch < 1 || (n_regen > 0 && !regen) || (int64_t) n_past_new + n_regen + 1 > c->n_ctx) {
        fprintf(stderr, "falcon-hip: context_swap: %d kept rows + %d regenerated tokens + the waiting one need 0 <= both, n_batch (%d) >= 1 and their sum <= n_ctx (%d)\n", n_past_new, n_regen, n_batch, c->n_ctx);
        return 1;
    }
    for (int i = 0; i < n_regen; ++i) if (regen[i] < 0 || regen[i] >= m->hp.n_vocab) { fprintf(stderr, "falcon-hip: context_swap: token id %d at %d is outside [0, %d)\n", regen[i], i, m->hp.n_vocab); return 2; }
    if (c->sync_err_sticky) { fprintf(stderr, "falcon-hip: context_swap: an earlier step of this context lost an in-launch hand-off -- its KV cache is invalid, the context must be recreated\n"); return 3; }
    int32_t reason[256];
    if (falcon_hip_context_get_stops(c, nullptr, reason)) return 1;
    if (reason[seq] != FQ_STOP_CONTEXT) { fprintf(stderr, "falcon-hip: context_swap: sequence %d did not end at the end of its cache (reason %d)\n", seq, reason[seq]); return 1; }
    if (fq_reference_order()) swap_v_repack(c, seq, n_past_new);      // (the reference's kept V rows are not the rows it had: above)
    // the context that evaluates: this one, or for a lock-step context a plain one of the same length that borrows the slot's rows
    falcon_hip_context * e = c;
    if (c->n_seq > 0) {
        if (c->swap_ctx && c->swap_ctx->n_batch < n_batch) { falcon_hip_context_free(c->swap_ctx); c->swap_ctx = nullptr; }
        if (!c->swap_ctx) c->swap_ctx = context_create(m, c->n_ctx, n_batch, c->rope_n_ctx, 0);
        e = c->swap_ctx;
        if (e->rope_n_ctx != c->rope_n_ctx) falcon_hip_context_set_rope_n_ctx(e, c->rope_n_ctx);
    }
    const int nb = n_batch < e->n_batch ? n_batch : e->n_batch;
    if (e != c && n_regen > 0 && n_past_new > 0) if (const int rc = falcon_hip_context_copy_seq(e, 0, c, seq, n_past_new)) return rc;
    for (int i = 0; i < n_regen; i += nb) {
        const int n = n_regen - i < nb ? n_regen - i : nb;
        if (const int rc = falcon_hip_eval(e, regen + i, n, n_past_new + i, 0)) return rc;
    }
    if (e != c && n_regen > 0) {                            // rows [n_past_new, n_past_new + n_regen) back into the slot, those before them untouched
        const int64_t nl = (int64_t) m->layers.size(), row4 = (int64_t) m->hp.n_head_kv * 16, slot = (int64_t) c->n_ctx * row4, n4 = (int64_t) n_regen * row4;
        const unsigned gx = (unsigned)((n4 + 255) / 256 < 1024 ? (n4 + 255) / 256 : 1024);
        if (nl > 0) hipLaunchKernelGGL(k_copy_seq_kv, dim3(gx, (unsigned) nl, 2), dim3(256), 0, fq_ctx().stream,
                                       (float4 *) c->k_cache + seq * slot + n_past_new * row4, (float4 *) c->v_cache + seq * slot + n_past_new * row4, slot * B,
                                       (const float4 *) e->k_cache + n_past_new * row4, (const float4 *) e->v_cache + n_past_new * row4, slot, n4);
    }
    return falcon_hip_context_resume(c, seq);
}

// ------------------------------------------------------------------------------------------------ sessions (fq_session.h, kernels_session.hip)
// The reference's state blob and session file for one sequence of a context: generator, last logits, K and V rows [0, n_tokens). The rows travel through a
// staging buffer in the file's layout (V transposed), allocated for the call and freed after it, one transfer to or from the host; no standing buffer of the
// context moves, so its captured steps stay valid.
static fq_session_dims session_dims(const falcon_hip_context * c) {
    return fq_session_dims{ c->n_ctx, c->m->hp.n_layer, c->m->hp.n_head_kv * 64 };
}
static size_t session_logits_cap(const falcon_hip_context * c, int logits_all) {
    return (size_t) c->m->hp.n_vocab * (logits_all ? (size_t) c->n_ctx : 1);
}
// the embedding section this context writes and takes: the kept row, or nothing (fq_session.h)
static size_t session_emb_size(const falcon_hip_context * c) { return c->emb_mode & FALCON_HIP_EMBED_LAST ? (size_t) c->m->hp.n_embd : 0; }
// what every entry refuses first: 0, or the code
static int session_check(const falcon_hip_context * c, int seq, const char * what) {
    if (!c) return FALCON_HIP_SESSION_E_ARG;
    if (!c->m->first_stage() || !c->m->last_stage()) { fprintf(stderr, "falcon-hip: %s: a pipeline stage holds part of the layers; a session spans all of them\n", what); return FALCON_HIP_SESSION_E_STAGE; }
    if (seq < 0 || seq >= (c->n_seq > 0 ? c->n_seq : 1)) { fprintf(stderr, "falcon-hip: %s: sequence %d of %d is out of range\n", what, seq, c->n_seq > 0 ? c->n_seq : 1); return FALCON_HIP_SESSION_E_SEQ; }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(fq_ctx().stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { fprintf(stderr, "falcon-hip: %s: the stream is capturing\n", what); return FALCON_HIP_SESSION_E_CAPTURE; }
    return 0;
}

extern "C" size_t falcon_hip_state_size(const falcon_hip_context * c, int n_tokens, int logits_all) {
    if (!c || n_tokens < 0 || n_tokens > c->n_ctx) return 0;
    return fq_state_bytes(session_dims(c), session_logits_cap(c, logits_all), n_tokens, session_emb_size(c));
}

extern "C" int falcon_hip_copy_state(falcon_hip_context * c, int seq, int n_tokens, int logits_all, void * dst) {
    if (const int rc = session_check(c, seq, "copy_state")) return rc;
    if (!dst || n_tokens < 0 || n_tokens > c->n_ctx) { fprintf(stderr, "falcon-hip: copy_state: %d rows of a cache of %d\n", n_tokens, c->n_ctx); return FALCON_HIP_SESSION_E_ARG; }
    const fq_session_dims d = session_dims(c);
    hipStream_t st = fq_ctx().stream;
    const size_t V = (size_t) c->m->hp.n_vocab, cap = session_logits_cap(c, logits_all), kvb = fq_session_kv_bytes(d, n_tokens);
    float * stage = nullptr;
    if (kvb && hipMalloc((void **) &stage, 2 * kvb) != hipSuccess) {
        (void) hipGetLastError();
        fprintf(stderr, "falcon-hip: copy_state: cannot allocate %zu staging bytes\n", 2 * kvb);
        return FALCON_HIP_SESSION_E_ALLOC;
    }
    // the generator: the sequence's sampler row, or what a loaded session left for it, or a fresh std::mt19937(1) -- the reference context's when nothing drew from it
    uint32_t mt[FQ_MT_N];
    int32_t mti = 0;
    bool have = false;
    if (c->sampler) have = ggml_hip_sampler_get_rng(c->sampler, seq, mt, &mti) == 0;
    for (const auto & k : c->rng_kept) if (!have && (int) k[0] == seq) { memcpy(mt, k.data() + 1, sizeof mt); mti = (int32_t) k[1 + FQ_MT_N]; have = true; }
    if (!have) { int i; fq_mt_seed(mt, &i, 1u); mti = i; }
    // the logits the last eval left on the host: every row it kept when the capacity holds them, else its last row; a lock-step context: the sequence's row
    const float * lg = nullptr;
    size_t lg_n = 0;
    if (c->logits_fresh && !c->logits_none) {
        lg = falcon_hip_get_logits(c);                              // (waits for eval_token's row)
        const size_t rows = c->logits_last == c->logits_pinned && c->logits_last ? 1 : c->logits_host.size() / V;
        if (c->n_seq > 0) { lg += (size_t) seq * V; lg_n = V; }
        else if (rows * V <= cap) lg_n = rows * V;
        else { lg += (rows - 1) * V; lg_n = V; }
    }
    uint8_t * kv_host = nullptr;
    // the kept row (zeros before the first eval, as the reference's freshly sized vector)
    const size_t emb_n = session_emb_size(c);
    std::vector<float> emb(emb_n);
    if (emb_n) HIP_CHECK(hipMemcpyAsync(emb.data(), c->emb, emb_n * 4, hipMemcpyDeviceToHost, st));
    if (emb_n) HIP_CHECK(hipStreamSynchronize(st));
    fq_state_write((uint8_t *) dst, d, mt, mti, cap, lg, lg_n, n_tokens, &kv_host, emb_n, emb.data());
    if (kvb) {
        const int n_seq = c->n_seq > 0 ? c->n_seq : 1;
        fq_launch_session_pack(c->k_cache, c->v_cache, stage, d.n_layer, c->m->hp.n_head_kv, n_tokens, (int64_t) n_seq * c->n_ctx, (int64_t) seq * c->n_ctx, st);
        HIP_CHECK(hipMemcpyAsync(kv_host, stage, 2 * kvb, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (stage) HIP_CHECK(hipFree(stage));
    return 0;
}

// the parsed state into the context; nothing of the context is touched before every refusal is behind
static int session_apply(falcon_hip_context * c, int seq, const fq_state_view & v) {
    const fq_session_dims d = session_dims(c);
    hipStream_t st = fq_ctx().stream;
    const size_t V = (size_t) c->m->hp.n_vocab, kvb = fq_session_kv_bytes(d, v.kv_ntok);
    float * stage = nullptr;
    if (kvb && hipMalloc((void **) &stage, 2 * kvb) != hipSuccess) {
        (void) hipGetLastError();
        fprintf(stderr, "falcon-hip: set_state: cannot allocate %zu staging bytes\n", 2 * kvb);
        return FALCON_HIP_SESSION_E_ALLOC;
    }
    HIP_CHECK(hipStreamSynchronize(st));                             // (a pending eval_token row must land before its buffer is given up)
    if (kvb) {
        const int n_seq = c->n_seq > 0 ? c->n_seq : 1;
        HIP_CHECK(hipMemcpyAsync(stage, v.k, 2 * kvb, hipMemcpyHostToDevice, st));      // (K and V lie back to back in the blob)
        fq_launch_session_unpack(c->k_cache, c->v_cache, stage, d.n_layer, c->m->hp.n_head_kv, v.kv_ntok, (int64_t) n_seq * c->n_ctx, (int64_t) seq * c->n_ctx, st);
    }
    // logits: whole rows of a single-sequence context go back into the buffer falcon_hip_get_logits returns, and the last of them onto the device, where
    // falcon_hip_sample draws from it (a lock-step context's rows belong to all its sequences at once: left as they are)
    if (c->n_seq == 0 && v.logits_size >= V && v.logits_size % V == 0 && v.logits_size / V <= (size_t) c->n_ctx) {
        c->logits_host.resize(v.logits_size);
        memcpy(c->logits_host.data(), v.logits, v.logits_size * 4);
        c->logits_pending = false; c->logits_last = nullptr; c->logits_none = false; c->logits_fresh = true;
        HIP_CHECK(hipMemcpyAsync(c->logits_dev, c->logits_host.data() + (v.logits_size - V), V * 4, hipMemcpyHostToDevice, st));
        c->last_rows = 1;
    }
    if (v.emb_size) {                                                // (the parser took the size this context expects: n_embd)
        HIP_CHECK(hipMemcpyAsync(c->emb, v.emb, v.emb_size * 4, hipMemcpyHostToDevice, st));
        c->emb_have = true; c->emb_host_fresh = false;
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (stage) HIP_CHECK(hipFree(stage));
    // the generator: into the row if there is one, else kept for the set_sampling that makes it
    for (size_t i = 0; i < c->rng_kept.size(); ++i) if ((int) c->rng_kept[i][0] == seq) { c->rng_kept.erase(c->rng_kept.begin() + (long) i); break; }
    if (c->sampler) return ggml_hip_sampler_set_rng(c->sampler, seq, v.mt, v.mti) ? FALCON_HIP_SESSION_E_ARG : 0;
    std::vector<uint32_t> k(2 + FQ_MT_N);
    k[0] = (uint32_t) seq; memcpy(k.data() + 1, v.mt, sizeof v.mt); k[1 + FQ_MT_N] = (uint32_t) v.mti;
    c->rng_kept.push_back(std::move(k));
    return 0;
}

extern "C" int falcon_hip_set_state(falcon_hip_context * c, int seq, const void * src, size_t n_bytes, int * n_tokens_out) {
    if (const int rc = session_check(c, seq, "set_state")) return rc;
    if (!src) return FALCON_HIP_SESSION_E_ARG;
    fq_state_view v;
    if (const int rc = fq_state_parse((const uint8_t *) src, n_bytes, session_dims(c), &v, session_emb_size(c))) { fprintf(stderr, "falcon-hip: set_state: refused (code %d, fq_session.h)\n", rc); return rc; }
    if (const int rc = session_apply(c, seq, v)) return rc;
    if (n_tokens_out) *n_tokens_out = v.kv_ntok;
    return 0;
}

static fq_session_hparams session_record(const falcon_hip_session_hparams * hp) {
    fq_session_hparams r;
    static_assert(sizeof(falcon_hip_session_hparams) == sizeof(fq_session_hparams), "the same nine int32");
    memcpy(&r, hp, sizeof r);
    return r;
}

extern "C" int falcon_hip_session_save(falcon_hip_context * c, int seq, const char * path, const falcon_hip_session_hparams * hparams, const int32_t * tokens,
                                       int n_tokens, int logits_all) {
    if (const int rc = session_check(c, seq, "session_save")) return rc;
    if (!path || !hparams || n_tokens < 0 || n_tokens > c->n_ctx || (n_tokens > 0 && !tokens)) { fprintf(stderr, "falcon-hip: session_save: %d tokens of a cache of %d, or missing arguments\n", n_tokens, c->n_ctx); return FALCON_HIP_SESSION_E_ARG; }
    const size_t head = fq_session_header_bytes((size_t) n_tokens), body = falcon_hip_state_size(c, n_tokens, logits_all);
    std::vector<uint8_t> buf(head + body);
    fq_session_write_header(buf.data(), session_record(hparams), tokens, (uint32_t) n_tokens);
    if (const int rc = falcon_hip_copy_state(c, seq, n_tokens, logits_all, buf.data() + head)) return rc;
    FILE * f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "falcon-hip: session_save: cannot write %s\n", path); return FALCON_HIP_SESSION_E_IO; }
    const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0 || !ok) { fprintf(stderr, "falcon-hip: session_save: short write to %s\n", path); remove(path); return FALCON_HIP_SESSION_E_IO; }
    return 0;
}

extern "C" int falcon_hip_session_load(falcon_hip_context * c, int seq, const char * path, const falcon_hip_session_hparams * hparams, int32_t * tokens_out,
                                       int capacity, int * n_out) {
    if (const int rc = session_check(c, seq, "session_load")) return rc;
    if (!path || !hparams || capacity < 0 || (capacity > 0 && !tokens_out)) return FALCON_HIP_SESSION_E_ARG;
    FILE * f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "falcon-hip: session_load: cannot read %s\n", path); return FALCON_HIP_SESSION_E_IO; }
    std::vector<uint8_t> buf;
    if (fseek(f, 0, SEEK_END) == 0) { const long n = ftell(f); if (n > 0) buf.resize((size_t) n); }
    rewind(f);
    const bool ok = buf.empty() || fread(buf.data(), 1, buf.size(), f) == buf.size();
    fclose(f);
    if (!ok) { fprintf(stderr, "falcon-hip: session_load: short read from %s\n", path); return FALCON_HIP_SESSION_E_IO; }
    fq_session_view s;
    if (const int rc = fq_session_parse(buf.data(), buf.size(), session_record(hparams), (size_t) capacity, session_dims(c), &s, session_emb_size(c))) {
        fprintf(stderr, "falcon-hip: session_load: %s refused (code %d, fq_session.h)\n", path, rc);
        return rc;
    }
    if (const int rc = session_apply(c, seq, s.st)) return rc;
    if (s.n_tokens) memcpy(tokens_out, s.tokens, (size_t) s.n_tokens * 4);
    if (n_out) *n_out = (int) s.n_tokens;
    return 0;
}

// ------------------------------------------------------------------------------------------------ LoRA adapters, tensor read-back
// llama_apply_lora_from_file (libfalcon.h:187-191, libfalcon.cpp:3927-4170) on the device-resident weights: fq_lora.h reads and checks the whole adapter, then every
// pair patches its matrix in row chunks -- dequantize (or the base file's rows) -> k_lora_add (kernels_lora.hip) -> the reference's quantizer -> re-tile into
// the matrix's own storage. Addresses, row_stride, bytes and weight_bytes stay: captured steps and ring schedules remain valid. Everything that can refuse does
// so before the first write.
static_assert(FALCON_HIP_LORA_E_IO == FQ_LORA_E_IO && FALCON_HIP_LORA_E_TRUNCATED == FQ_LORA_E_TRUNCATED && FALCON_HIP_LORA_E_TYPE_PAIR == FQ_LORA_E_TYPE_PAIR,
              "the reader's codes are the C ABI's");

// the model's matrix `name`: 0 and *w, 1 a matrix of another pipeline stage (skipped), -1 not a matrix of this model
static int model_matrix(falcon_hip_model * m, const std::string & name, fq_weight ** w) {
    const falcon_hip_hparams & hp = m->hp;
    if (name == "transformer.word_embeddings.weight") { if (!m->first_stage()) return 1; *w = &m->tok_emb; return 0; }
    if (name == "lm_head.weight")                     { if (!m->last_stage())  return 1; *w = &m->lm_head; return 0; }
    const fq_lora_hparams lh{ hp.n_vocab, hp.n_embd, hp.n_head, hp.n_head_kv, hp.n_layer, hp.n_ff };
    int64_t K = 0, M = 0;
    if (!fq_lora_matrix_shape(lh, name, &K, &M)) return -1;
    const int il = atoi(name.c_str() + strlen("transformer.h."));
    if (il < hp.layer_begin || il >= hp.layer_end) return 1;
    layer_weights & L = m->layers[(size_t)(il - hp.layer_begin)];
    const std::string leaf = name.substr(name.find('.', strlen("transformer.h.")) + 1);
    *w = leaf == "self_attention.query_key_value.weight" ? &L.qkv : leaf == "self_attention.dense.weight" ? &L.wo : leaf == "mlp.dense_h_to_4h.weight" ? &L.up : &L.down;
    return 0;
}

static bool lora_not_capturing(const char * what) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(fq_ctx().stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) return true;
    fprintf(stderr, "falcon-hip: %s: the stream is capturing\n", what);
    return false;
}

namespace {
struct lora_job { const fq_lora_pair * p; fq_weight * w; fq_lora_base_tensor base; };
struct lora_bufs {                                                 // allocated once per call, for the largest matrix of the adapter
    float * a = nullptr, * b = nullptr, * stage = nullptr; uint16_t * h16 = nullptr; uint8_t * q = nullptr;
    ~lora_bufs() { for (void * p : { (void *) a, (void *) b, (void *) stage, (void *) h16, (void *) q }) if (p) (void) hipFree(p); }
};
bool lora_alloc(void ** p, size_t n) {
    if (!n) return true;
    if (hipMalloc(p, n) == hipSuccess) return true;
    (void) hipGetLastError();
    fprintf(stderr, "falcon-hip: apply_lora: cannot allocate %zu staging bytes\n", n);
    return false;
}
}   // namespace

int fq_model_apply_lora(falcon_hip_model * m, const char * path_lora, fq_lora_base_fn base, void * user) {
    if (!m || !path_lora) { fprintf(stderr, "falcon-hip: apply_lora: missing argument\n"); return FALCON_HIP_LORA_E_ARG; }
    if (!lora_not_capturing("apply_lora")) return FALCON_HIP_LORA_E_CAPTURE;
    const falcon_hip_hparams & hp = m->hp;
    const fq_lora_hparams lh{ hp.n_vocab, hp.n_embd, hp.n_head, hp.n_head_kv, hp.n_layer, hp.n_ff };
    std::vector<uint8_t> file;
    fq_lora_view v;
    char msg[1400];
    if (const int rc = fq_lora_read(path_lora, lh, &file, &v, msg, sizeof msg)) { fprintf(stderr, "falcon-hip: apply_lora: %s: %s\n", path_lora, msg); return rc; }
    // ---- every refusal of the model level, and the sizes of the staging buffers
    std::vector<lora_job> jobs;
    int64_t rows_cap = (int64_t) 1 << 40;
    if (const char * e = getenv("FALCON_HIP_LORA_ROWS")) { const long long x = atoll(e); if (x > 0) rows_cap = x; }      // rows per chunk (tests; read per call)
    size_t a_max = 0, b_max = 0, stage_max = 0, h16_max = 0, q_max = 0;
    auto chunk_rows = [&](const fq_weight & w) {
        int64_t n = (int64_t)((256u << 20) / ((size_t) w.K * 4));      // 256 MB of f32 staging, as upload_weight stages its blocks
        if (n > rows_cap) n = rows_cap;
        return n < 1 ? (int64_t) 1 : (n > w.M ? w.M : n);
    };
    for (const fq_lora_pair & p : v.pairs) {
        fq_weight * w = nullptr;
        const int found = model_matrix(m, p.name, &w);
        if (found > 0) continue;                                        // another stage's
        if (found < 0 || !w->plane[0] || w->K != p.K || w->M != p.M) { fprintf(stderr, "falcon-hip: apply_lora: %s is not a loaded matrix of this model\n", p.name.c_str()); return FQ_LORA_E_UNKNOWN; }
        if (w->form_M > 0) { fprintf(stderr, "falcon-hip: apply_lora: %s is a row range of a split matrix; adapters are not applied to row-split models\n", p.name.c_str()); return FALCON_HIP_LORA_E_ROW_SPLIT; }
        if (p.r >= ((int64_t) 1 << 24)) { fprintf(stderr, "falcon-hip: apply_lora: %s: r = %lld\n", p.name.c_str(), (long long) p.r); return FQ_LORA_E_INNER; }
        lora_job j{ &p, w, fq_lora_base_tensor{ false, 0, 0, 0, 0, nullptr } };
        if (base) {
            j.base = base(user, p.name.c_str());
            if (!j.base.found) { fprintf(stderr, "falcon-hip: apply_lora: tensor '%s' not found in base model\n", p.name.c_str()); return FALCON_HIP_LORA_E_BASE_TENSOR; }
            if (j.base.n_dims != 2 || j.base.ne0 != p.K || j.base.ne1 != p.M || (j.base.type != FQ_F32 && j.base.type != FQ_F16)) {
                fprintf(stderr, "falcon-hip: apply_lora: base tensor '%s' is [%lld x %lld] of type %d; it must be [%lld x %lld] F16 or F32\n", p.name.c_str(), (long long) j.base.ne0,
                        (long long) j.base.ne1, j.base.type, (long long) p.K, (long long) p.M);
                return FALCON_HIP_LORA_E_BASE_TENSOR;
            }
            if (w->type == FQ_F16) { fprintf(stderr, "falcon-hip: apply_lora: %s is F16 on the device; a base file with an F16 destination is not pinned against the reference and refused\n", p.name.c_str()); return FALCON_HIP_LORA_E_BASE_F16_DST; }
        }
        const size_t nr = (size_t) chunk_rows(*w), K = (size_t) p.K;
        const size_t ab = K * (size_t) p.r * 4, bb = (size_t) p.M * (size_t) p.r * 4;
        a_max = ab > a_max ? ab : a_max; b_max = bb > b_max ? bb : b_max;
        if (p.a.ftype == 1) { const size_t hb = (K > (size_t) p.M ? K : (size_t) p.M) * (size_t) p.r * 2; h16_max = hb > h16_max ? hb : h16_max; }
        if (w->type != FQ_F16) {
            stage_max = nr * K * 4 > stage_max ? nr * K * 4 : stage_max;
            const size_t qb = nr * (size_t) w->nblk * fq_desc(w->type).tsize;
            q_max = qb > q_max ? qb : q_max;
            if (j.base.found && j.base.type == FQ_F16) h16_max = nr * K * 2 > h16_max ? nr * K * 2 : h16_max;
        }
        jobs.push_back(j);
    }
    if (jobs.empty()) return 0;
    lora_bufs buf;
    if (!lora_alloc((void **) &buf.a, a_max) || !lora_alloc((void **) &buf.b, b_max) || !lora_alloc((void **) &buf.stage, stage_max) ||
        !lora_alloc((void **) &buf.h16, h16_max) || !lora_alloc((void **) &buf.q, q_max)) return FALCON_HIP_LORA_E_ALLOC;
    // ---- the merge. No eval of any context may read a half-patched matrix: the device is idle before the first write and after the last
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipDeviceSynchronize());
    const float scaling = (float) v.alpha / (float) v.r;              // libfalcon.cpp:3961
    for (const lora_job & j : jobs) {
        const fq_lora_pair & p = *j.p;
        const fq_weight & w = *j.w;
        const int r = (int) p.r;
        const int64_t K = p.K, M = p.M;
        // loraA [K][r] and loraB [M][r] as f32, once per matrix. F16 loraA: ggml_compute_forward_mul_mat_f16_f32 rounds loraB to fp16 first (ggml.c:11243-11256)
        if (p.a.ftype == 1) {
            HIP_CHECK(hipMemcpyAsync(buf.h16, file.data() + p.a.offset, p.a.bytes, hipMemcpyHostToDevice, st));
            fq_launch_f16_to_f32(buf.h16, buf.a, K * r, st);
            HIP_CHECK(hipMemcpyAsync(buf.b, file.data() + p.b.offset, p.b.bytes, hipMemcpyHostToDevice, st));
            fq_launch_f32_to_f16(buf.b, buf.h16, M * r, st);
            fq_launch_f16_to_f32(buf.h16, buf.b, M * r, st);
        } else {
            HIP_CHECK(hipMemcpyAsync(buf.a, file.data() + p.a.offset, p.a.bytes, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(buf.b, file.data() + p.b.offset, p.b.bytes, hipMemcpyHostToDevice, st));
        }
        if (w.type == FQ_F16) {                                       // W = fp16(fp32(W) + ba), in place (ggml.c:8457-8459); no staging, so no chunks
            fq_launch_lora_add(buf.a, buf.b, r, K, M, scaling, w.plane[0], K, true, st);
            HIP_CHECK(hipStreamSynchronize(st));                      // (the next matrix reuses buf.a / buf.b / file-backed copies)
            continue;
        }
        const int64_t per = chunk_rows(w);
        for (int64_t r0 = 0; r0 < M; r0 += per) {
            const int64_t nr = M - r0 < per ? M - r0 : per;
            fq_weight sub = w;
            sub.M = nr;
            for (int pl = 0; pl < FQ_MAX_PLANES; ++pl) sub.plane[pl] = w.plane[0] + (size_t) r0 * w.row_stride;
            if (!j.base.found) fq_launch_dequant_rows(sub, nullptr, nr, buf.stage, st);                       // x = dequantize_row(W)    (ggml.c:8612)
            else if (j.base.type == FQ_F32) HIP_CHECK(hipMemcpyAsync(buf.stage, j.base.data + (size_t) r0 * K * 4, (size_t) nr * K * 4, hipMemcpyHostToDevice, st));
            else HIP_CHECK(hipMemcpyAsync(buf.h16, j.base.data + (size_t) r0 * K * 2, (size_t) nr * K * 2, hipMemcpyHostToDevice, st));
            if (j.base.found && j.base.type == FQ_F16) {
                // add(base F16, BA) is an F16 tensor: t = fp16(fp32(base) + ba), and cpy quantizes fp32(t) -- the extra rounding is the reference's
                fq_launch_lora_add(buf.a, buf.b + (size_t) r0 * r, r, K, nr, scaling, buf.h16, K, true, st);
                fq_launch_f16_to_f32(buf.h16, buf.stage, nr * K, st);
            } else {
                fq_launch_lora_add(buf.a, buf.b + (size_t) r0 * r, r, K, nr, scaling, buf.stage, K, false, st);      // y = x + ba
            }
            fq_launch_wquant(w.type, buf.stage, nr * K, buf.q, nullptr, st);                                  // W = quantize_row(y): the _reference quantizers
            fq_launch_retile(buf.q, sub, st);
            HIP_CHECK(hipStreamSynchronize(st));                      // (the host-side source of the next chunk's copy is pageable memory; one chunk in flight)
        }
    }
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

extern "C" int64_t falcon_hip_model_get_tensor(falcon_hip_model * m, const char * name, void * dst, size_t cap) {
    if (!m || !name) return -1;
    fq_weight * w = nullptr;
    if (model_matrix(m, name, &w) != 0 || !w->plane[0]) { fprintf(stderr, "falcon-hip: get_tensor: %s is not a matrix this model holds\n", name); return -1; }
    if (!dst) return (int64_t) w->bytes;
    if (cap < w->bytes) { fprintf(stderr, "falcon-hip: get_tensor: %s needs %zu bytes, the buffer holds %zu\n", name, w->bytes, cap); return -1; }
    if (!lora_not_capturing("get_tensor")) return -1;
    hipStream_t st = fq_ctx().stream;
    if (w->type == FQ_F16) {
        HIP_CHECK(hipMemcpyAsync(dst, w->plane[0], w->bytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return (int64_t) w->bytes;
    }
    uint8_t * q = nullptr;
    if (!lora_alloc((void **) &q, w->bytes)) return -1;
    fq_launch_untile(*w, q, st);
    HIP_CHECK(hipMemcpyAsync(dst, q, w->bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipFree(q));
    return (int64_t) w->bytes;
}

// host only: reads and checks an adapter against hparams (fq_lora.h); returns its code, and on 0 r, alpha and the number of pairs it would apply
extern "C" int falcon_hip_lora_scan(const char * path, const falcon_hip_hparams * hp, int * r_out, int * alpha_out, int * n_tensors_out) {
    if (!path || !hp) return FALCON_HIP_LORA_E_ARG;
    const fq_lora_hparams lh{ hp->n_vocab, hp->n_embd, hp->n_head, hp->n_head_kv, hp->n_layer, hp->n_ff };
    std::vector<uint8_t> file;
    fq_lora_view v;
    char msg[1400];
    if (const int rc = fq_lora_read(path, lh, &file, &v, msg, sizeof msg)) { fprintf(stderr, "falcon-hip: lora_scan: %s: %s\n", path, msg); return rc; }
    if (r_out) *r_out = v.r;
    if (alpha_out) *alpha_out = v.alpha;
    if (n_tensors_out) *n_tensors_out = (int) v.pairs.size();
    return 0;
}
