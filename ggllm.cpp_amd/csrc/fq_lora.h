// fq_lora.h -- the reference's LoRA adapter file ('ggla', llama_apply_lora_from_file_internal, libfalcon.cpp:3927-4170), read and checked on the host:
// plain C++, no HIP, so that tests/test_lora_cpu.py compiles it with g++ (tests/host/lora_parse_main.cpp) next to the library (falcon_model.hip), which
// adds the device side (kernels_lora.hip).
//
//   file    u32 magic 0x67676c61 'ggla', u32 version 1, i32 r, i32 alpha
//   record  i32 n_dims (2), i32 name_len, i32 ftype (0 F32 | 1 F16), i32 ne[n_dims], the name, zero padding to a multiple of 32, the data
//   NAME.loraA  ne = [r, K]: K rows of r values          NAME.loraB  ne = [r, M]          K = ne0, M = ne1 of the model's matrix NAME
// The reference applies a name as soon as both halves have been read and then forgets every half it holds (lora_tensors.clear()); either half may come
// first and a name may come again. It checks as it goes and leaves earlier matrices patched when a later record is bad. This reader checks the WHOLE file
// against the model's hparams first and returns the pairs in file order: nothing is written unless everything is good. A half that is still waiting
// when another name is applied, or at the end of the file, is an error here (the reference drops it without a word).
// The parser returns a code, never asserts or exits, and writes one line into msg.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#define FQ_LORA_MAGIC 0x67676c61u                    // LLAMA_FILE_MAGIC_GGLA (libfalcon.h)
#define FQ_LORA_VERSION 1u
#define FQ_LORA_NAME_MAX 1024                        // the reference reads the name into char buf[1024]

enum {
    FQ_LORA_OK = 0,
    FQ_LORA_E_IO = 1,                // the file cannot be read
    FQ_LORA_E_MAGIC = 2,             // bad file magic
    FQ_LORA_E_VERSION = 3,           // a version other than 1
    FQ_LORA_E_RANK = 4,              // r <= 0 in the header
    FQ_LORA_E_TRUNCATED = 5,         // the header, a record or its data runs past the end of the file
    FQ_LORA_E_NOT_LORA = 6,          // a name that does not end in .loraA / .loraB
    FQ_LORA_E_UNKNOWN = 7,           // a name that is not a 2-D matrix of this model
    FQ_LORA_E_NDIMS = 8,             // n_dims != 2
    FQ_LORA_E_FTYPE = 9,             // a data type other than 0 (F32) and 1 (F16)
    FQ_LORA_E_SHAPE = 10,            // K != loraA.ne[1] or M != loraB.ne[1]: an adapter of another model
    FQ_LORA_E_INNER = 11,            // loraA.ne[0] != loraB.ne[0] (or not positive)
    FQ_LORA_E_UNPAIRED = 12,         // a half without its other half: at the end of the file, dropped by another name's pair, or given twice
    FQ_LORA_E_TYPE_PAIR = 13,        // a type pair other than (F32, F32) and (F16 loraA, F32 loraB)
    // (the model level adds its own, include/falcon-hip.h: 32..)
};

struct fq_lora_hparams { int32_t n_vocab, n_embd, n_head, n_head_kv, n_layer, n_ff; };

struct fq_lora_half { int ftype; int64_t ne0, ne1; size_t offset, bytes; };          // offset of the data in the file
struct fq_lora_pair { std::string name; int64_t K, M, r; fq_lora_half a, b; };     // r = the halves' ne0 (the header's r only scales)
struct fq_lora_view { int32_t r, alpha; std::vector<fq_lora_pair> pairs; };        // in file order of their second halves

// ne0 (K) and ne1 (M) of the 2-D matrix `name` of a model with these hparams; false: no such matrix
static inline bool fq_lora_matrix_shape(const fq_lora_hparams & hp, const std::string & name, int64_t * K, int64_t * M) {
    const int64_t E = hp.n_embd, QKV = (int64_t)(hp.n_head + 2 * hp.n_head_kv) * 64, FF = hp.n_ff, V = hp.n_vocab;
    if (name == "transformer.word_embeddings.weight" || name == "lm_head.weight") { *K = E; *M = V; return true; }
    const char pre[] = "transformer.h.";
    const size_t np = sizeof pre - 1;
    if (name.compare(0, np, pre) != 0) return false;
    size_t i = np;
    int64_t il = 0;
    while (i < name.size() && name[i] >= '0' && name[i] <= '9' && i - np < 9) il = il * 10 + (name[i++] - '0');
    if (i == np || i >= name.size() || name[i] != '.' || il >= hp.n_layer) return false;
    const std::string leaf = name.substr(i + 1);
    if (leaf == "self_attention.query_key_value.weight") { *K = E; *M = QKV; return true; }
    if (leaf == "self_attention.dense.weight")           { *K = E; *M = E;   return true; }
    if (leaf == "mlp.dense_h_to_4h.weight")              { *K = E; *M = FF;  return true; }
    if (leaf == "mlp.dense_4h_to_h.weight")              { *K = FF; *M = E;  return true; }
    return false;
}

static inline int fq_lora_parse(const uint8_t * p, size_t n, const fq_lora_hparams & hp, fq_lora_view * out, char * msg, size_t msg_cap) {
    auto fail = [&](int code, const char * what, const std::string & name) {
        if (msg && msg_cap) snprintf(msg, msg_cap, "%s%s%s%s", what, name.empty() ? "" : " '", name.c_str(), name.empty() ? "" : "'");
        return code;
    };
    size_t pos = 0;
    auto i32 = [&](int32_t & v) { if (n - pos < 4) return false; memcpy(&v, p + pos, 4); pos += 4; return true; };      // (pos <= n always)
    if (msg && msg_cap) msg[0] = 0;
    fq_lora_view v;
    int32_t magic = 0, version = 0;
    if (!i32(magic)) return fail(FQ_LORA_E_TRUNCATED, "truncated header", "");
    if ((uint32_t) magic != FQ_LORA_MAGIC) return fail(FQ_LORA_E_MAGIC, "bad file magic", "");
    if (!i32(version)) return fail(FQ_LORA_E_TRUNCATED, "truncated header", "");
    if ((uint32_t) version != FQ_LORA_VERSION) return fail(FQ_LORA_E_VERSION, "unsupported file version", "");
    if (!i32(v.r) || !i32(v.alpha)) return fail(FQ_LORA_E_TRUNCATED, "truncated header", "");
    if (v.r <= 0) return fail(FQ_LORA_E_RANK, "r is not positive", "");
    struct waiting { std::string base; int which; fq_lora_half h; };
    std::vector<waiting> held;                                       // the reference's lora_tensors
    while (pos < n) {
        int32_t n_dims = 0, len = 0, ftype = 0, ne[2] = { 1, 1 };
        if (!i32(n_dims) || !i32(len) || !i32(ftype)) return fail(FQ_LORA_E_TRUNCATED, "truncated tensor record", "");
        if (n_dims != 2) return fail(FQ_LORA_E_NDIMS, "unsupported tensor dimension", std::to_string(n_dims));
        if (!i32(ne[0]) || !i32(ne[1])) return fail(FQ_LORA_E_TRUNCATED, "truncated tensor record", "");
        if (len < 0 || len > FQ_LORA_NAME_MAX || (size_t) len > n - pos) return fail(FQ_LORA_E_TRUNCATED, "tensor name runs past the end of the file", "");
        const std::string name((const char *) p + pos, (size_t) len);
        pos += (size_t) len;
        const size_t suf = name.rfind(".lora");
        if (suf == std::string::npos) return fail(FQ_LORA_E_NOT_LORA, "not a lora tensor:", name);
        const std::string kind = name.substr(suf + 5), base = name.substr(0, suf);
        if (kind != "A" && kind != "B") return fail(FQ_LORA_E_NOT_LORA, "not a lora tensor:", name);
        int64_t K = 0, M = 0;
        if (!fq_lora_matrix_shape(hp, base, &K, &M)) return fail(FQ_LORA_E_UNKNOWN, "unknown tensor in lora adapter:", name);
        if (ftype != 0 && ftype != 1) return fail(FQ_LORA_E_FTYPE, "invalid tensor data type of", name);
        if (ne[0] <= 0 || ne[1] <= 0) return fail(FQ_LORA_E_INNER, "empty tensor", name);
        fq_lora_half h;
        h.ftype = ftype; h.ne0 = ne[0]; h.ne1 = ne[1];
        h.bytes = (size_t) ne[0] * (size_t) ne[1] * (ftype == 0 ? 4 : 2);      // (two positive int32: below 2^64)
        const size_t data = (pos + 31) & ~(size_t) 31;
        if (data > n || h.bytes > n - data) return fail(FQ_LORA_E_TRUNCATED, "data runs past the end of the file:", name);
        h.offset = data;
        pos = data + h.bytes;
        const int which = kind == "A" ? 0 : 1;
        int other = -1;
        for (size_t i = 0; i < held.size(); ++i) {
            if (held[i].base != base) continue;
            if (held[i].which == which) return fail(FQ_LORA_E_UNPAIRED, "given twice without its other half:", name);
            other = (int) i;
        }
        if (other < 0) { held.push_back(waiting{ base, which, h }); continue; }
        if (held.size() > 1) return fail(FQ_LORA_E_UNPAIRED, "a half of another tensor is dropped when this pair is applied:", name);
        fq_lora_pair pr;
        pr.name = base; pr.K = K; pr.M = M;
        pr.a = which == 0 ? h : held[(size_t) other].h;
        pr.b = which == 1 ? h : held[(size_t) other].h;
        held.clear();
        if (pr.a.ne1 != K || pr.b.ne1 != M) return fail(FQ_LORA_E_SHAPE, "incompatible tensor dimensions; is this adapter for this model?", base);
        if (pr.a.ne0 != pr.b.ne0) return fail(FQ_LORA_E_INNER, "loraA and loraB differ in their inner length:", base);
        if (pr.b.ftype != 0) return fail(FQ_LORA_E_TYPE_PAIR, "loraB must be F32 (loraA F32 or F16):", base);
        pr.r = pr.a.ne0;
        v.pairs.push_back(pr);
    }
    if (!held.empty()) return fail(FQ_LORA_E_UNPAIRED, "only one half at the end of the file:", held[0].base);
    *out = v;
    return FQ_LORA_OK;
}

// the whole file into buf, then fq_lora_parse
static inline int fq_lora_read(const char * path, const fq_lora_hparams & hp, std::vector<uint8_t> * buf, fq_lora_view * out, char * msg, size_t msg_cap) {
    FILE * f = path ? fopen(path, "rb") : nullptr;
    if (!f) { if (msg && msg_cap) snprintf(msg, msg_cap, "failed to open '%s'", path ? path : ""); return FQ_LORA_E_IO; }
    buf->clear();
    if (fseek(f, 0, SEEK_END) == 0) { const long n = ftell(f); if (n > 0) buf->resize((size_t) n); }
    rewind(f);
    const bool ok = buf->empty() || fread(buf->data(), 1, buf->size(), f) == buf->size();
    fclose(f);
    if (!ok) { if (msg && msg_cap) snprintf(msg, msg_cap, "short read from '%s'", path); return FQ_LORA_E_IO; }
    return fq_lora_parse(buf->data(), buf->size(), hp, out, msg, msg_cap);
}
