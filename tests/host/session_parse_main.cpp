// session_parse_main.cpp -- TEST INFRASTRUCTURE: a stand-alone host program over csrc/fq_session.h for a sanitizer build (tests/test_session_cpu.py compiles
// it with -fsanitize=address,undefined where the compiler has the runtimes): parses a session file, three truncations of it and a copy whose kv_ntok is
// n_ctx + 1, each from a heap buffer of exactly its size, so that a read past the end is a reported error and not a quiet one.
//   session_parse_main FILE N_CTX N_LAYER ROW      exit 0 when every parse returned the expected code
#include "fq_session.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int parse(const std::vector<uint8_t> & file, size_t n, const fq_session_dims & d, int patch_ntok) {
    uint8_t * p = (uint8_t *) malloc(n ? n : 1);                    // exactly n bytes: the sanitizer sees every byte beyond
    memcpy(p, file.data(), n);
    fq_session_hparams want{};
    if (n >= 8 + sizeof want) memcpy(&want, p + 8, sizeof want);
    if (patch_ntok >= 0) {
        fq_session_view s;
        if (fq_session_parse(p, n, want, 1 << 20, d, &s) != FQ_SESSION_OK) { free(p); return -1; }
        const int32_t nt = patch_ntok;
        memcpy(p + (s.st.k - p) - 4, &nt, 4);                      // kv_ntok sits right before K
    }
    fq_session_view out;
    memset(&out, 0x5a, sizeof out);
    const fq_session_view before = out;
    const int rc = fq_session_parse(p, n, want, 1 << 20, d, &out);
    if (rc != FQ_SESSION_OK && memcmp(&out, &before, sizeof out)) { free(p); return -2; }      // a refusal touches nothing
    if (rc == FQ_SESSION_OK) {                                      // every byte the view points at is inside the buffer: read them all
        unsigned sum = 0;
        const size_t kvb = fq_session_kv_bytes(d, out.st.kv_ntok);
        for (size_t i = 0; i < out.n_tokens * 4u; ++i) sum += out.tokens[i];
        for (size_t i = 0; i < out.st.logits_size * 4; ++i) sum += out.st.logits[i];
        for (size_t i = 0; i < kvb; ++i) sum += out.st.k[i] + out.st.v[i];
        printf("  (checksum %u)\n", sum);
    }
    free(p);
    return rc;
}

int main(int argc, char ** argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s FILE N_CTX N_LAYER ROW\n", argv[0]); return 2; }
    FILE * f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<uint8_t> file;
    for (int c; (c = fgetc(f)) != EOF;) file.push_back((uint8_t) c);
    fclose(f);
    const fq_session_dims d{ atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) };
    uint32_t n_tokens = 0;
    if (file.size() >= 48) memcpy(&n_tokens, file.data() + 44, 4);
    const size_t head = fq_session_header_bytes(n_tokens);
    struct { const char * what; size_t n; int patch, want; } cases[] = {
        { "whole file", file.size(), -1, FQ_SESSION_OK },
        { "cut inside the hparams record", 20, -1, FQ_SESSION_E_TRUNCATED },
        { "cut inside the generator text", head + 100, -1, FQ_SESSION_E_TRUNCATED },
        { "one byte short", file.size() - 1, -1, FQ_SESSION_E_TRUNCATED },
        { "kv_ntok = n_ctx + 1", file.size(), d.n_ctx + 1, FQ_SESSION_E_NTOK },
    };
    int bad = 0;
    for (const auto & c : cases) {
        const int rc = parse(file, c.n, d, c.patch);
        printf("%s: code %d (expected %d)\n", c.what, rc, c.want);
        bad += rc != c.want;
    }
    return bad ? 1 : 0;
}
