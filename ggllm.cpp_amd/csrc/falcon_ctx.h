// falcon_ctx.h -- what the units of the Falcon driver share: the model, the context, the captured-step key and slot, and the few helpers
// more than one unit calls. Private to csrc/ (never installed, never included from include/). The units, one duty each:
//   falcon_model.hip   model, weight arena, tensors in and out, vocabulary bytes, LoRA merge
//   falcon_hip.hip     context, capture / replay, modes, the eval entries, embeddings, logits, perplexity
//   falcon_stage.hip   launch_stage: the launch list of one eval
//   falcon_decode.hip  lock-step entries, sampler / stop / grammar / log-prob settings, the decode loops, draft-and-verify, the pipeline step
//   falcon_state.hip   KV slot copies, context swap, state blobs and session files
#pragma once
#include "fq_device.h"
#include "kernels.h"
#include "hip_context.h"
#include "fq_f16.h"
#include "fq_stop.h"
#include "fq_spec.h"
#include "../../include/falcon-hip.h"
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <vector>

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
// The key's parts are named, and each is filled by the code that owns the launches it describes (addresses of buffers that move, baked integers); a step
// leaves the parts of what it does not launch at zero. All zero by default, no padding: compared bytewise.
struct step_key {
    int64_t sig = 0;                           // graph_signature(): the context's own modes
    int64_t epoch = 0;                         // fq_config_epoch(): the process-wide switches that change a launch list
    int64_t entry[4] = {};                     // what the entry itself bakes: decode_greedy's base position, the lock-step loops' output buffer, stage_step's four pointers
    int64_t lp[5] = {};                        // the log-prob records of a sampled step (lp_step_key, falcon_decode.hip)
    int64_t sampler[FQ_SAMPLER_KEY_WORDS] = {};      // what the sampler's launch takes (fq_sampler_step_key, kernels_sample.hip); a greedy step's: all zero
    int64_t spec[3] = {};                      // a draft-and-verify pass (spec_step_key, falcon_decode.hip)
    struct { int64_t N, max_kv, keep_hidden; } batch = { 0, 0, 0 };      // a captured batch (eval_stage_impl, falcon_hip.hip)
    bool operator==(const step_key & o) const { return !memcmp(this, &o, sizeof *this); }
};
static_assert(std::has_unique_object_representations_v<step_key>, "step_key is compared with memcmp: no padding");
struct step_slot {
    hipGraphExec_t exec = nullptr;
    step_key key;                              // of exec
    bool holds(const step_key & k) const { return exec && key == k; }
    template <class Body> void replay(falcon_hip_context * c, hipStream_t st, const step_key & k, Body && body);      // re-captures body() when k differs, then launches
    void drop() { if (exec) { HIP_CHECK(hipGraphExecDestroy(exec)); exec = nullptr; } }
};

// ---- what a context makes after its creation, on the first call that needs it, releases itself when the context goes
// n elements of device (or page-locked host) memory. reset(n) makes the new buffer before it frees the old one: a buffer that grows always moves, and
// with it the key of every captured step that holds its address
template <class T, bool pinned> struct owned_buf {
    T * p = nullptr;
    owned_buf() = default;
    owned_buf(const owned_buf &) = delete;
    owned_buf & operator=(const owned_buf &) = delete;
    ~owned_buf() { reset(0); }
    T * get() const { return p; }
    void reset(size_t n) {
        T * old = p;
        p = nullptr;
        if (n && pinned) HIP_CHECK(hipHostMalloc((void **) &p, n * sizeof(T), hipHostMallocDefault));
        if (n && !pinned) HIP_CHECK(hipMalloc((void **) &p, n * sizeof(T)));
        if (old) HIP_CHECK(pinned ? hipHostFree(old) : hipFree(old));
    }
};
template <class T> using dev_buf = owned_buf<T, false>;
template <class T> using pinned_buf = owned_buf<T, true>;
// what run_polled (falcon_decode.hip) polls: two page-locked images of `rows` T each, each behind its own event
template <class T> struct polled_images {
    pinned_buf<T> host;
    hipEvent_t ev[2] = { nullptr, nullptr };
    size_t rows = 0;
    ~polled_images() { for (hipEvent_t e : ev) if (e) HIP_CHECK(hipEventDestroy(e)); }
    void make(size_t n_rows) {                 // (once: a context's rows do not change)
        if (host.get()) return;
        rows = n_rows;
        host.reset(2 * rows);
        for (hipEvent_t & e : ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    T * image(int i) const { return host.get() + (size_t) i * rows; }
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
    dev_buf<int32_t> seq_out_dev; int64_t seq_out_cap = 0;
    int32_t * tokens_dev = nullptr, * out_tokens_dev = nullptr;
    float * hidden_dev = nullptr;
    float * argmax_val = nullptr;              // per-workgroup greedy candidates written by the lm_head kernel
    int   * argmax_idx = nullptr;
    bool keep_hidden = false;
    int  hidden_tokens = 0;
    std::vector<float> logits_host;
    pinned_buf<float> logits_pinned;           // one row of page-locked host memory: falcon_hip_eval_token's copy is enqueued behind the graph replay
    const float * logits_last = nullptr;       // what falcon_hip_get_logits returns: logits_host.data() or logits_pinned
    bool logits_none = false;                  // the last eval was falcon_hip_eval_score: no logits were copied, falcon_hip_get_logits returns NULL
    dev_buf<int32_t> score_tgt;                // falcon_hip_eval_score: [n_batch] targets and [n_batch] probabilities in device memory, made by the first call
    dev_buf<float> score_prob;
    std::vector<float> score_host;
    bool logits_fresh = false;                 // the host rows are those of the LAST call (falcon_hip_eval, eval_token, eval_seqs); a decode loop or eval_score leaves none (falcon_hip_copy_state writes them)
    bool logits_pending = false;               // falcon_hip_eval_token: the row's copy is in flight (falcon_hip_get_logits waits for it)
    bool sync_err_sticky = false;              // an in-launch hand-off timed out in an asynchronous step: every later eval of this context fails (3)
    std::vector<void *> allocs;
    bool use_graph = false;
    // the captured steps, one slot per entry point (in brackets: the parts of its key besides signature and epoch)
    step_slot decode_step;                     // falcon_hip_decode_greedy (entry: the base position, an argument of k_argmax_advance)
    step_slot sample_step;                     // falcon_hip_decode_sample (lp, sampler)
    step_slot seqs_step;                       // falcon_hip_decode_greedy_seqs (entry: seq_out_dev)
    step_slot sample_seqs_step;                // falcon_hip_decode_sample_seqs (entry: seq_out_dev; lp, sampler)
    step_slot token_step;                      // falcon_hip_eval_token (nothing)
    step_slot token_step_emb;                  // ... while an embedding mode is set: a slot of its own, so that switching the mode on and off again finds token_step as it was
    step_slot stage_step;                      // falcon_hip_stage_step (entry: its four device pointers; the position lives on the device)
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
    std::vector<step_slot> batch_steps;        // at most 8, the oldest goes first; each keyed by step_key_of plus the batch part
    bool prefill_graph = false;                // (off by default: a replay saves 1-2 % of a batch, capturing a new (tokens, keys) shape costs ~5 ms once)
    // sampled decode (falcon_hip_context_set_sampling / falcon_hip_sample / falcon_hip_decode_sample[_seqs], kernels_sample.hip): one sampler
    // row per sequence, created by the first call that needs it and kept until the context is freed
    ggml_hip_sampler * sampler = nullptr;
    int  last_rows = 1;                         // rows of the last eval's logits (falcon_hip_sample draws from the last of them)
    // log-probabilities of the sampled loops (falcon_hip_context_set_logprobs, kernels_logprob.hip): nothing exists while lp_n_top < 0. The record buffers hold
    // lp_cap records of the current lp_n_top; the captured sampled steps bake all of these in and carry them in their keys' lp part
    int  lp_n_top = -1;
    dev_buf<float> lp_prob, lp_top_prob; dev_buf<int32_t> lp_top_id; int64_t lp_cap = 0;
    int  lp_steps = 0, lp_rows = 0;             // shape of the last recorded call (0: none)
    unsigned sync_err_host = 0;                // copy of sync_words[1], fetched wherever the host synchronises anyway
    // stops of the sampled loops (falcon_hip_context_set_stops; the rows' configuration and state live in the sampler). The loop polls the rows' states
    // every stop_poll steps: two page-locked images of them, each behind its own event, made by the first loop that polls.
    // The default of 16 began as a guess. Measured since (scripts/gpu_stop.py, profiles/stop_7b.json: Falcon-7B Q4_0, 128 steps through the graph, 1.085 ms per
    // step with stops off): +2.0 us per step at 4, +1.3 at 16, +0.9 at 64, next to an A/A spread of 0.4 -- the wait costs nothing that shows, so the interval only
    // trades steps launched past the end (at most 2 x interval - 1) against copies; 16 stays.
    int  stop_poll = 16;
    polled_images<fq_stop_state> stop_poll_img;      // [2][rows]
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
    polled_images<fq_spec_state> spec_poll_img;      // [2][1]: the state's images (the loop's poll, as stop_poll_img)
    step_slot spec_step;                       // falcon_hip_decode_spec (spec, sampler)
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

// THE capture and replay: body() enqueues one step on st; captured again when k differs from the key the slot holds, then launched
template <class Body> void step_slot::replay(falcon_hip_context * c, hipStream_t st, const step_key & k, Body && body) {
    if (!holds(k)) {
        drop();
        hipGraph_t g;
        HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        body();
        HIP_CHECK(hipStreamEndCapture(st, &g));
        HIP_CHECK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
        HIP_CHECK(hipGraphDestroy(g));
        ++c->n_captures;
        key = k;
    }
    HIP_CHECK(hipGraphLaunch(exec, st));
}
// sets keep_hidden aside for a scope: single-token steps, the loops and the passes keep no hidden rows
struct keep_hidden_off {
    falcon_hip_context * c; bool was;
    explicit keep_hidden_off(falcon_hip_context * ctx) : c(ctx), was(ctx->keep_hidden) { c->keep_hidden = false; }
    ~keep_hidden_off() { c->keep_hidden = was; }
};

// ---- the helpers more than one unit calls (C++ symbols of the library: a namespace of their own, apart from the kernel side's fq_*)
namespace fq_drv {
inline void * dev_alloc(std::vector<void *> & keep, size_t bytes) {
    void * p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
    keep.push_back(p);
    return p;
}
inline int ctx_rows(const falcon_hip_context * c) { return c->n_seq > 0 ? c->n_seq : 1; }      // sequences of the context = rows of its sampler
inline int64_t key_ptr(const void * p) { return (int64_t)(intptr_t) p; }
// F16 matrices (kernels_f16.hip): blocks that hold one, and stages whose lm_head is one, run the op-by-op list -- the fused launches are per quantized format
inline bool layer_has_f16(const layer_weights & L) { return L.qkv.type == FQ_F16 || L.wo.type == FQ_F16 || L.up.type == FQ_F16 || L.down.type == FQ_F16; }
inline bool stage_has_f16(const falcon_hip_model * m) {
    for (const layer_weights & L : m->layers) if (layer_has_f16(L)) return true;
    return m->last_stage() && m->lm_head.type == FQ_F16;
}
// falcon_stage.hip
bool stage_fused_ref(const falcon_hip_context * c);
bool stage_fused(const falcon_hip_context * c);
void launch_stage(falcon_hip_context * c, int N, int max_n_kv, hipStream_t st, int pos_stride = 0, int verify_limit = 0);
// falcon_hip.hip
void fetch_sync_error(falcon_hip_context * c, hipStream_t st);
int  report_sync_error(falcon_hip_context * c, const char * where);
bool has_head(const falcon_hip_context * c, const char * who);
bool emb_refuses(const falcon_hip_context * c, const char * what);
step_key step_key_of(const falcon_hip_context * c);
bool graph_ok_strict();
bool graph_ok_loop(const falcon_hip_context * c);
bool graph_ok_seqs(const falcon_hip_context * c);
bool graph_ok_stage_step(const falcon_hip_context * c);
}   // namespace fq_drv
