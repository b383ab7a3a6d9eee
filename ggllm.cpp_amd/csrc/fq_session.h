// fq_session.h -- the reference's session file and state blob (llama_save_session_file / llama_load_session_file, falcon_copy_state_data /
// falcon_set_state_data, libfalcon.cpp:4185-4564), restated for the host: plain C++, no HIP, so that tests/test_session_cpu.py compiles it with g++
// (tests/host/session_harness.cpp) next to the library (falcon_state.hip), which adds the device side (kernels_session.hip).
//
//   file   u32 magic 'ggsn', u32 version 1, the nine int32 of falcon_hparams (libfalcon.cpp:146-155; compared by memcmp on load),
//          u32 n_tokens, n_tokens x i32, then the state blob up to the end of the file
//   state  size_t rng_size, 64 KiB zero-padded: the text libstdc++ streams for std::mt19937 (624 words and the position, decimal, one space between)
//          size_t logits_capacity, size_t logits_size, capacity floats of which size are set (capacity: n_vocab, or n_ctx * n_vocab with logits_all)
//          size_t embedding_size, then as many floats: 0, or n_embd and ctx->embedding (the ln_f row of the last evaluated token) when the context was made
//          with params.embedding. The reference asserts capacity() == embedding_size on load (libfalcon.cpp:4385-4395), so the size a context expects is the
//          only one it takes, in both directions (emb_expect below: 0 by default, as before embeddings existed here)
//          size_t kv_size, int kv_ntok
//          K  f32 [n_layer][kv_ntok][n_head_kv * 64]
//          V  f32 [n_layer][n_head_kv * 64][kv_ntok]        (transposed: the reference's build without FALCON_NO_KV_UPGRADE)
// kv_size is the reference's MEM_REQ_KV_SELF (libfalcon.cpp:162-175): ggml_tensor_overhead() + 3 * (ggml_tensor_overhead() + ne * 4) with
// ne = n_head_kv * 64 * n_layer * n_ctx; the reference asserts equality on load. Everything is little-endian with the widths of the x86-64 / LP64 host
// the reference runs on (size_t 8 bytes, int 4). Parsers return a code, never assert or exit, and write their outputs only on success.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define FQ_SESSION_MAGIC 0x6767736eu                 // 'ggsn' (libfalcon.h:34, 41)
#define FQ_SESSION_VERSION 1u
#define FQ_SESSION_RNG_BYTES 65536                   // LLAMA_MAX_RNG_STATE
#define FQ_SESSION_MT_N 624
// ggml_tensor_overhead() of the reference's build: not spelled out in its sources (object header + tensor struct + alignment slack). Taken from the
// kv_size field of the golden files (tests/golden/session.npz, written by the reference itself: scripts/gen_session_golden.py), where
// kv_size = 4 * overhead + 3 * 4 * ne holds for both models (n_ctx 32: ne 4096 -> 50816, ne 8192 -> 99968).
#define FQ_SESSION_TENSOR_OVERHEAD 416

enum {
    FQ_SESSION_OK = 0,
    FQ_SESSION_E_MAGIC = 1,          // wrong magic or version
    FQ_SESSION_E_HPARAMS = 2,        // the hparams record differs from the caller's
    FQ_SESSION_E_CAPACITY = 3,       // more tokens than the caller's buffer holds
    FQ_SESSION_E_TRUNCATED = 4,      // shorter than its own fields say
    FQ_SESSION_E_NTOK = 5,           // kv_ntok < 0 or above n_ctx
    FQ_SESSION_E_KV_SIZE = 6,        // kv_size is not this context's
    FQ_SESSION_E_EMBEDDING = 7,      // embedding size not the expected one (0, or n_embd for a context that keeps the row)
    FQ_SESSION_E_RNG = 8,            // the generator text does not parse to 624 words and a position in 0..624
    FQ_SESSION_E_LOGITS = 9,         // logits size above its capacity
    // (the model level adds its own, include/falcon-hip.h: 16..)
};

struct fq_session_hparams {          // falcon_hparams, in the reference's order
    int32_t n_vocab, n_ctx, n_embd, n_head, n_head_kv, n_layer, n_falcon_type, n_bpe_merges, ftype;
};
static_assert(sizeof(fq_session_hparams) == 36, "nine int32, no padding");

struct fq_session_dims {             // what the state's layout depends on
    int n_ctx, n_layer, row;         // row: n_head_kv * 64 floats per cached position
};

struct fq_state_view {               // a parsed state blob; the pointers point into it (unaligned: copy with memcpy)
    uint32_t mt[FQ_SESSION_MT_N];
    int mti;
    size_t logits_cap, logits_size;
    const uint8_t * logits;          // logits_size floats
    int kv_ntok;
    const uint8_t * k, * v;          // n_layer * kv_ntok * row floats each
    size_t n_bytes;                  // of the blob
    size_t emb_size;                 // 0 or n_embd
    const uint8_t * emb;             // emb_size floats
};

struct fq_session_view {
    fq_session_hparams hp;
    uint32_t n_tokens;
    const uint8_t * tokens;          // n_tokens i32
    size_t state_off;                // where the blob begins
    fq_state_view st;
};

static inline size_t fq_session_kv_size(const fq_session_dims & d) {
    return (size_t) 4 * FQ_SESSION_TENSOR_OVERHEAD + (size_t) 3 * 4 * ((size_t) d.row * d.n_layer * d.n_ctx);
}
static inline size_t fq_session_kv_bytes(const fq_session_dims & d, int kv_ntok) {      // K, or V
    return (size_t) d.n_layer * (size_t) kv_ntok * d.row * 4;
}
static inline size_t fq_state_bytes(const fq_session_dims & d, size_t logits_cap, int kv_ntok, size_t emb_size = 0) {
    return 8 + FQ_SESSION_RNG_BYTES + 16 + logits_cap * 4 + 8 + emb_size * 4 + 8 + 4 + 2 * fq_session_kv_bytes(d, kv_ntok);
}
static inline size_t fq_session_header_bytes(size_t n_tokens) { return 8 + sizeof(fq_session_hparams) + 4 + n_tokens * 4; }

// ---- the generator's text: operator<< of std::mersenne_twister_engine (bits/random.tcc): every state word, then the position, decimal, separated by one space
static inline size_t fq_session_rng_format(const uint32_t * mt, int mti, char * dst /* FQ_SESSION_RNG_BYTES */) {
    size_t n = 0;
    for (int i = 0; i <= FQ_SESSION_MT_N; ++i) {
        uint32_t v = i < FQ_SESSION_MT_N ? mt[i] : (uint32_t) mti;
        char d[10];
        int k = 0;
        do { d[k++] = (char) ('0' + v % 10); v /= 10; } while (v);
        while (k) dst[n++] = d[--k];
        if (i < FQ_SESSION_MT_N) dst[n++] = ' ';
    }
    return n;                        // at most 625 * 11 bytes
}
// operator>>: 625 whitespace-separated decimal numbers; a word beyond 32 bits, a position beyond 624, a missing number or anything else in the text is refused
static inline int fq_session_rng_parse(const char * s, size_t n, uint32_t * mt, int * mti) {
    uint32_t w[FQ_SESSION_MT_N + 1];
    size_t i = 0;
    for (int k = 0; k <= FQ_SESSION_MT_N; ++k) {
        while (i < n && (s[i] == ' ' || s[i] == '\n' || s[i] == '\t' || s[i] == '\r')) ++i;
        if (i >= n || s[i] < '0' || s[i] > '9') return FQ_SESSION_E_RNG;
        uint64_t v = 0;
        while (i < n && s[i] >= '0' && s[i] <= '9') { v = v * 10 + (uint64_t)(s[i] - '0'); if (v > 0xffffffffull) return FQ_SESSION_E_RNG; ++i; }
        w[k] = (uint32_t) v;
    }
    while (i < n && (s[i] == ' ' || s[i] == '\n' || s[i] == '\t' || s[i] == '\r')) ++i;
    if (i != n || w[FQ_SESSION_MT_N] > FQ_SESSION_MT_N) return FQ_SESSION_E_RNG;
    memcpy(mt, w, sizeof(uint32_t) * FQ_SESSION_MT_N);
    *mti = (int) w[FQ_SESSION_MT_N];
    return FQ_SESSION_OK;
}

// ---- state blob
// Writes everything but the K and V rows into dst (fq_state_bytes(d, logits_cap, kv_ntok) bytes) and returns where they go: K at *kv_out, V right behind it
// (fq_session_kv_bytes each) -- the device side copies both there in one transfer. logits_size <= logits_cap; the unset capacity is zeros.
// emb_size floats of emb make the embedding section (0: an empty one).
static inline size_t fq_state_write(uint8_t * dst, const fq_session_dims & d, const uint32_t * mt, int mti, size_t logits_cap, const float * logits,
                                    size_t logits_size, int kv_ntok, uint8_t ** kv_out, size_t emb_size = 0, const float * emb = nullptr) {
    uint8_t * o = dst;
    auto put = [&](const void * p, size_t n) { memcpy(o, p, n); o += n; };
    auto put_sz = [&](size_t v) { const uint64_t x = v; put(&x, 8); };
    memset(o + 8, 0, FQ_SESSION_RNG_BYTES);
    put_sz(fq_session_rng_format(mt, mti, (char *) o + 8));
    o += FQ_SESSION_RNG_BYTES;
    put_sz(logits_cap);
    put_sz(logits_size);
    memset(o, 0, logits_cap * 4);
    if (logits_size) memcpy(o, logits, logits_size * 4);
    o += logits_cap * 4;
    put_sz(emb_size);                                              // embedding
    if (emb_size) put(emb, emb_size * 4);
    put_sz(fq_session_kv_size(d));
    const int32_t nt = kv_ntok;
    put(&nt, 4);
    if (kv_out) *kv_out = o;
    o += 2 * fq_session_kv_bytes(d, kv_ntok);
    return (size_t)(o - dst);
}

static inline int fq_state_parse(const uint8_t * src, size_t n, const fq_session_dims & d, fq_state_view * out, size_t emb_expect = 0) {
    fq_state_view v;
    size_t pos = 0;
    auto need = [&](size_t k) { return k <= n - pos; };              // (pos <= n always)
    auto get_sz = [&](uint64_t & x) { if (!need(8)) return false; memcpy(&x, src + pos, 8); pos += 8; return true; };
    uint64_t rng_size = 0, cap = 0, size = 0, emb = 0, kv_size = 0;
    if (!get_sz(rng_size) || !need(FQ_SESSION_RNG_BYTES)) return FQ_SESSION_E_TRUNCATED;
    if (rng_size > FQ_SESSION_RNG_BYTES) return FQ_SESSION_E_RNG;
    if (const int rc = fq_session_rng_parse((const char *) src + pos, (size_t) rng_size, v.mt, &v.mti)) return rc;
    pos += FQ_SESSION_RNG_BYTES;
    if (!get_sz(cap) || !get_sz(size)) return FQ_SESSION_E_TRUNCATED;
    if (cap > (n - pos) / 4) return FQ_SESSION_E_TRUNCATED;
    if (size > cap) return FQ_SESSION_E_LOGITS;
    v.logits_cap = (size_t) cap; v.logits_size = (size_t) size; v.logits = src + pos;
    pos += (size_t) cap * 4;
    if (!get_sz(emb)) return FQ_SESSION_E_TRUNCATED;
    if (emb != emb_expect) return FQ_SESSION_E_EMBEDDING;
    if (emb > (n - pos) / 4) return FQ_SESSION_E_TRUNCATED;
    v.emb_size = (size_t) emb; v.emb = src + pos;
    pos += (size_t) emb * 4;
    int32_t nt = 0;
    if (!get_sz(kv_size) || !need(4)) return FQ_SESSION_E_TRUNCATED;
    memcpy(&nt, src + pos, 4); pos += 4;
    if (nt < 0 || nt > d.n_ctx) return FQ_SESSION_E_NTOK;
    if (kv_size != fq_session_kv_size(d)) return FQ_SESSION_E_KV_SIZE;
    const size_t kvb = fq_session_kv_bytes(d, nt);
    if (!need(kvb) || !(kvb <= n - pos - kvb)) return FQ_SESSION_E_TRUNCATED;
    v.kv_ntok = nt; v.k = src + pos; v.v = src + pos + kvb;
    pos += 2 * kvb;
    v.n_bytes = pos;
    *out = v;
    return FQ_SESSION_OK;
}

// ---- file
static inline size_t fq_session_write_header(uint8_t * dst, const fq_session_hparams & hp, const int32_t * tokens, uint32_t n_tokens) {
    const uint32_t head[2] = { FQ_SESSION_MAGIC, FQ_SESSION_VERSION };
    uint8_t * o = dst;
    memcpy(o, head, 8); o += 8;
    memcpy(o, &hp, sizeof hp); o += sizeof hp;
    memcpy(o, &n_tokens, 4); o += 4;
    if (n_tokens) memcpy(o, tokens, (size_t) n_tokens * 4);
    o += (size_t) n_tokens * 4;
    return (size_t)(o - dst);
}

// want: the caller's hparams record; token_capacity: of the caller's buffer; d: the context's dimensions (d.n_ctx bounds kv_ntok)
static inline int fq_session_parse(const uint8_t * p, size_t n, const fq_session_hparams & want, size_t token_capacity, const fq_session_dims & d,
                                   fq_session_view * out, size_t emb_expect = 0) {
    fq_session_view s;
    if (n < 8) return FQ_SESSION_E_TRUNCATED;
    uint32_t head[2];
    memcpy(head, p, 8);
    if (head[0] != FQ_SESSION_MAGIC || head[1] != FQ_SESSION_VERSION) return FQ_SESSION_E_MAGIC;
    if (n < 8 + sizeof(fq_session_hparams)) return FQ_SESSION_E_TRUNCATED;
    memcpy(&s.hp, p + 8, sizeof s.hp);
    if (memcmp(&s.hp, &want, sizeof want)) return FQ_SESSION_E_HPARAMS;
    size_t pos = 8 + sizeof(fq_session_hparams);
    if (n - pos < 4) return FQ_SESSION_E_TRUNCATED;
    memcpy(&s.n_tokens, p + pos, 4); pos += 4;
    if (s.n_tokens > token_capacity) return FQ_SESSION_E_CAPACITY;
    if ((n - pos) / 4 < s.n_tokens) return FQ_SESSION_E_TRUNCATED;
    s.tokens = p + pos;
    pos += (size_t) s.n_tokens * 4;
    s.state_off = pos;
    if (const int rc = fq_state_parse(p + pos, n - pos, d, &s.st, emb_expect)) return rc;
    *out = s;
    return FQ_SESSION_OK;
}
