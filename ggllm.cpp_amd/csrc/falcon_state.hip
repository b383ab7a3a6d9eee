// falcon_state.hip -- what moves a sequence's state: KV slot copies, the context swap, state blobs and session files.
#include "falcon_ctx.h"
#include "fq_ctx_swap.h"
#include "fq_sample.h"
#include "fq_session.h"
using namespace fq_drv;

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
    if (c->sampler && fq_sampler_guide_pairs(c->sampler) > 0 && (fq_sampler_lead_of(c->sampler)[seq] >= 0 || fq_sampler_guide_of(c->sampler)[seq] >= 0)) {
        fprintf(stderr, "falcon-hip: context_swap: sequence %d leads or guides a pair (falcon_hip_context_set_guidance): a swap moves one slot, a pair moves together\n", seq);
        return 1;
    }
    int32_t reason[256];
    if (falcon_hip_context_get_stops(c, nullptr, reason)) return 1;
    if (reason[seq] != FQ_STOP_CONTEXT) { fprintf(stderr, "falcon-hip: context_swap: sequence %d did not end at the end of its cache (reason %d)\n", seq, reason[seq]); return 1; }
    if (fq_reference_order()) swap_v_repack(c, seq, n_past_new);      // (the reference's kept V rows are not the rows it had: above)
    // the context that evaluates: this one, or for a lock-step context a plain one of the same length that borrows the slot's rows
    falcon_hip_context * e = c;
    if (c->n_seq > 0) {
        if (c->swap_ctx && c->swap_ctx->n_batch < n_batch) { falcon_hip_context_free(c->swap_ctx); c->swap_ctx = nullptr; }
        if (!c->swap_ctx) c->swap_ctx = falcon_hip_context_create(m, c->n_ctx, n_batch, c->rope_n_ctx);
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
        const size_t rows = c->logits_last == c->logits_pinned.get() && c->logits_last ? 1 : c->logits_host.size() / V;
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
