// Host harness of csrc/fq_grammar.h for tests/test_grammar_cpu.py: the header the device compiles, behind a C interface (built as a shared
// library), and -- with GRAMMAR_HARNESS_MAIN -- a program of its own that replays a file of cases and compares every result with the ones
// recorded there (built with -fsanitize=address,undefined).
#include "fq_grammar.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" {
int gr_words(int n_vocab) { return fq_grammar_words(n_vocab); }
int gr_walk(const uint16_t * trans, int state, const uint8_t * b, int L) { return fq_grammar_walk(trans, state, b, L); }
int gr_allowed(const uint16_t * trans, const uint8_t * accept, int state, int token, int eos_id, const uint8_t * pool, const int32_t * offs) {
    return fq_grammar_allowed(trans, accept, state, token, eos_id, pool, offs) ? 1 : 0;
}
int gr_advance(const uint16_t * trans, int state, int token, int eos_id, const uint8_t * pool, const int32_t * offs) {
    return fq_grammar_advance(trans, state, token, eos_id, pool, offs);
}
// creation as the library does it: the table's check, the index (one word at a time), the per-state counts, their check.
// Returns the code; *bad the state to blame. index [n_states][words] and counts [n_states] are written only for a table that passed its check.
int gr_build(int n_states, int start, const uint16_t * trans, const uint8_t * accept, int n_vocab, int eos_id, const uint8_t * pool, const int32_t * offs,
             uint64_t * index, int32_t * counts, int * bad) {
    if (const int rc = fq_grammar_check_table(n_states, start, trans, accept, n_vocab, eos_id, bad)) return rc;
    const int W = fq_grammar_words(n_vocab);
    for (int s = 0; s < n_states; ++s) {
        counts[s] = 0;
        for (int w = 0; w < W; ++w) {
            const uint64_t word = fq_grammar_index_word(trans, accept, s, w, n_vocab, eos_id, pool, offs);
            index[(int64_t) s * W + w] = word;
            counts[s] += __builtin_popcountll(word);
        }
    }
    return fq_grammar_check_counts(n_states, counts, bad);
}
}

#ifdef GRAMMAR_HARNESS_MAIN
// the file: int64 words. Per case: n_states, start, n_vocab, eos_id, pool_len, trans [n_states * 256], accept [n_states], offs [n_vocab + 1],
// pool [pool_len], want_code, want_bad, have_index (0 / 1), index [n_states * words] if have_index, n_steps, then n_steps x (state, token, want_allowed, want_next)
int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE * f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int64_t> w;
    int64_t x;
    while (fread(&x, 8, 1, f) == 1) w.push_back(x);
    fclose(f);
    size_t i = 0;
    int n_cases = 0, n_steps_all = 0;
    auto next = [&]() -> int64_t { if (i >= w.size()) { fprintf(stderr, "the file ends inside a case\n"); exit(2); } return w[i++]; };
    while (i < w.size()) {
        const int n_states = (int) next(), start = (int) next(), n_vocab = (int) next(), eos_id = (int) next(), pool_len = (int) next();
        std::vector<uint16_t> trans((size_t) n_states * 256);
        std::vector<uint8_t> accept((size_t) n_states), pool((size_t) pool_len);       // (exact sizes: a read past an end is the sanitizer's to find)
        std::vector<int32_t> offs((size_t) n_vocab + 1);
        for (auto & v : trans) v = (uint16_t) next();
        for (auto & v : accept) v = (uint8_t) next();
        for (auto & v : offs) v = (int32_t) next();
        for (auto & v : pool) v = (uint8_t) next();
        const int want_code = (int) next(), want_bad = (int) next(), have_index = (int) next();
        const int W = fq_grammar_words(n_vocab);
        std::vector<uint64_t> index((size_t) n_states * W);
        std::vector<int32_t> counts((size_t) n_states);
        int bad = -7;
        const int code = gr_build(n_states, start, trans.data(), accept.data(), n_vocab, eos_id, pool.data(), offs.data(), index.data(), counts.data(), &bad);
        if (code != want_code || bad != want_bad) { fprintf(stderr, "case %d: code %d state %d, recorded %d / %d\n", n_cases, code, bad, want_code, want_bad); return 1; }
        if (have_index)
            for (size_t k = 0; k < index.size(); ++k)
                if (index[k] != (uint64_t) next()) { fprintf(stderr, "case %d: index word %zu differs\n", n_cases, k); return 1; }
        const int n_steps = (int) next();
        for (int k = 0; k < n_steps; ++k) {
            const int state = (int) next(), token = (int) next(), want_allowed = (int) next(), want_next = (int) next();
            const int a = gr_allowed(trans.data(), accept.data(), state, token, eos_id, pool.data(), offs.data());
            const int nx = gr_advance(trans.data(), state, token, eos_id, pool.data(), offs.data());
            if (a != want_allowed || nx != want_next) { fprintf(stderr, "case %d step %d: allowed %d next %d, recorded %d / %d\n", n_cases, k, a, nx, want_allowed, want_next); return 1; }
        }
        n_steps_all += n_steps;
        ++n_cases;
    }
    printf("grammar harness: %d cases, %d steps replayed\n", n_cases, n_steps_all);
    return 0;
}
#endif
