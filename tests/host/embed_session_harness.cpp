// embed_session_harness.cpp -- TEST INFRASTRUCTURE: the embedding section of csrc/fq_session.h (a context that keeps the ln_f row writes n_embd floats
// there and takes no other size; one that does not takes none) behind a C ABI for tests/test_embed_cpu.py (g++, host only), and -- with -DES_MAIN -- as a
// stand-alone program for a sanitizer build: every parse reads a heap buffer of exactly its size, so that a read past the end is a reported error.
//   embed_session_harness FILE N_CTX N_LAYER ROW N_EMBD      exit 0 when every case gave its expected code and the file re-composed to its own bytes
#include "fq_session.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

// parse p[0, n) expecting emb_expect floats in the embedding section. info: n_tokens, blob offset, logits capacity, logits size, logits offset, embedding
// size, embedding offset, kv_ntok, K offset, V offset, blob bytes, generator position. The outputs are written on success only.
static int es_parse_impl(const uint8_t * p, size_t n, const fq_session_dims & d, size_t emb_expect, int64_t * info, fq_session_view * view) {
    fq_session_hparams want{};
    if (n >= 8 + sizeof want) memcpy(&want, p + 8, sizeof want);
    fq_session_view s;
    memset(&s, 0x5a, sizeof s);
    const fq_session_view before = s;
    const int rc = fq_session_parse(p, n, want, (size_t) 1 << 20, d, &s, emb_expect);
    if (rc != FQ_SESSION_OK) return memcmp(&s, &before, sizeof s) ? -2 : rc;       // a refusal touches nothing
    if (info) {
        info[0] = s.n_tokens; info[1] = (int64_t) s.state_off; info[2] = (int64_t) s.st.logits_cap; info[3] = (int64_t) s.st.logits_size; info[4] = s.st.logits - p;
        info[5] = (int64_t) s.st.emb_size; info[6] = s.st.emb - p; info[7] = s.st.kv_ntok; info[8] = s.st.k - p; info[9] = s.st.v - p;
        info[10] = (int64_t) s.st.n_bytes; info[11] = s.st.mti;
    }
    if (view) *view = s;
    return rc;
}

// the parsed sections written again through the composer: the bytes of the file; returns their count, or minus the parser's code
static long es_recompose_impl(const uint8_t * p, size_t n, const fq_session_dims & d, size_t emb_expect, std::vector<uint8_t> & out) {
    fq_session_view s;
    const int rc = es_parse_impl(p, n, d, emb_expect, nullptr, &s);
    if (rc) return -(long) rc;
    std::vector<int32_t> tokens(s.n_tokens);
    if (s.n_tokens) memcpy(tokens.data(), s.tokens, (size_t) s.n_tokens * 4);
    std::vector<float> logits(s.st.logits_size), emb(s.st.emb_size);
    if (!logits.empty()) memcpy(logits.data(), s.st.logits, logits.size() * 4);
    if (!emb.empty()) memcpy(emb.data(), s.st.emb, emb.size() * 4);
    out.assign(fq_session_header_bytes(s.n_tokens) + fq_state_bytes(d, s.st.logits_cap, s.st.kv_ntok, s.st.emb_size), 0xEE);
    const size_t head = fq_session_write_header(out.data(), s.hp, tokens.data(), s.n_tokens);
    uint8_t * kv = nullptr;
    const size_t body = fq_state_write(out.data() + head, d, s.st.mt, s.st.mti, s.st.logits_cap, logits.data(), logits.size(), s.st.kv_ntok, &kv, emb.size(), emb.data());
    const size_t kvb = fq_session_kv_bytes(d, s.st.kv_ntok);
    if (kvb) { memcpy(kv, s.st.k, kvb); memcpy(kv + kvb, s.st.v, kvb); }
    return head + body == out.size() ? (long) out.size() : -100;
}

extern "C" {

int es_parse(const uint8_t * p, long n, const int32_t * dims, long emb_expect, int64_t * info) {
    return es_parse_impl(p, (size_t) n, fq_session_dims{ dims[0], dims[1], dims[2] }, (size_t) emb_expect, info, nullptr);
}
long es_state_bytes(const int32_t * dims, long logits_cap, int kv_ntok, long emb_size) {
    return (long) fq_state_bytes(fq_session_dims{ dims[0], dims[1], dims[2] }, (size_t) logits_cap, kv_ntok, (size_t) emb_size);
}
// dst: room for n bytes (the file's own size)
long es_recompose(const uint8_t * p, long n, const int32_t * dims, long emb_expect, uint8_t * dst) {
    std::vector<uint8_t> out;
    const long r = es_recompose_impl(p, (size_t) n, fq_session_dims{ dims[0], dims[1], dims[2] }, (size_t) emb_expect, out);
    if (r > 0 && r <= n) memcpy(dst, out.data(), (size_t) r);
    return r;
}

}

#ifdef ES_MAIN
static int parse_exact(const std::vector<uint8_t> & file, size_t n, const fq_session_dims & d, size_t emb_expect) {
    uint8_t * p = (uint8_t *) malloc(n ? n : 1);                    // exactly n bytes: the sanitizer sees every byte beyond
    memcpy(p, file.data(), n);
    fq_session_view s;
    const int rc = es_parse_impl(p, n, d, emb_expect, nullptr, &s);
    if (rc == FQ_SESSION_OK) {                                      // every byte of the row is inside the buffer: read them all
        unsigned sum = 0;
        for (size_t i = 0; i < s.st.emb_size * 4; ++i) sum += s.st.emb[i];
        printf("  (row checksum %u)\n", sum);
    }
    free(p);
    return rc;
}

int main(int argc, char ** argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s FILE N_CTX N_LAYER ROW N_EMBD\n", argv[0]); return 2; }
    FILE * f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<uint8_t> file;
    for (int c; (c = fgetc(f)) != EOF;) file.push_back((uint8_t) c);
    fclose(f);
    const fq_session_dims d{ atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) };
    const size_t E = (size_t) atoi(argv[5]);
    int bad = 0;
    auto expect = [&](const char * what, int rc, int want) { if (rc != want) { printf("%s: code %d (expected %d)\n", what, rc, want); ++bad; } };
    int64_t info[12];
    expect("whole file", es_parse_impl(file.data(), file.size(), d, E, info, nullptr), FQ_SESSION_OK);
    if (bad) return 1;
    expect("whole file, exact buffer", parse_exact(file, file.size(), d, E), FQ_SESSION_OK);
    expect("a context that keeps no row", parse_exact(file, file.size(), d, 0), FQ_SESSION_E_EMBEDDING);
    expect("a row one float shorter", parse_exact(file, file.size(), d, E - 1), FQ_SESSION_E_EMBEDDING);
    expect("a row one float longer", parse_exact(file, file.size(), d, E + 1), FQ_SESSION_E_EMBEDDING);
    const size_t sec = (size_t) info[6] - 8;                        // the section: its size field, then the row
    for (size_t n = sec; n < sec + 8 + 4 * E; ++n) expect("cut inside the embedding section", parse_exact(file, n, d, E), FQ_SESSION_E_TRUNCATED);
    std::vector<uint8_t> again;
    const long r = es_recompose_impl(file.data(), file.size(), d, E, again);
    if (r != (long) file.size() || memcmp(again.data(), file.data(), file.size())) { printf("re-composed file differs (%ld bytes of %zu)\n", r, file.size()); ++bad; }
    printf("%d unexpected result(s)\n", bad);
    return bad ? 1 : 0;
}
#endif
