// falcon_model.hip -- the model of the Falcon driver: creation, the weight arena, tensors in and out, the vocabulary's bytes, the LoRA merge.
#include "falcon_ctx.h"
#include "fq_lora.h"
#include "fq_lora_base.h"
#include <string>
using namespace fq_drv;

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
// ---- grammars (fq_grammar.h): a grammar is indexed with the model's vocabulary and keeps its own copy; the rows' bindings and states belong to the sampler
extern "C" ggml_hip_grammar * falcon_hip_grammar_create(falcon_hip_model * m, const ggml_hip_dfa * dfa, int eos_id, int * bad_state) {
    if (bad_state) *bad_state = -1;
    if (!m || !m->vb_pool) { fprintf(stderr, "falcon-hip: grammar_create: the model has no vocabulary (falcon_hip_model_set_vocab)\n"); return nullptr; }
    return fq_grammar_make("falcon-hip: grammar_create", m->hp.n_vocab, m->vb_pool, m->vb_offs, true, dfa, eos_id, bad_state);
}
extern "C" int falcon_hip_grammar_free(ggml_hip_grammar * g) { return ggml_hip_grammar_free(g); }
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
