// host build of ggllm.cpp_amd/csrc/fq_stop_text.h (behind fq_stop.h) for tests/test_stop_text_cpu.py: one row driven draw by draw.
// Built twice: as a shared library the test calls, and with -DSTOP_TEXT_MAIN -fsanitize=address,undefined as a program of its
// own that replays the test's cases from a file of integers and compares every draw with the outcome recorded there.
#include "fq_stop_text.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct row {
    fq_stop_cfg ic; fq_stopt_cfg tc;
    fq_stop_state is; fq_stopt_state ts;
};
static void row_fresh(row * r) { fq_stop_reset(&r->is); fq_stopt_reset(&r->ts); }

extern "C" {
int row_bytes() { return (int) sizeof(row); }
void row_init(row * r) { memset(r, 0, sizeof *r); r->ic.on = 1; row_fresh(r); }
// either setter starts the whole shared state afresh (the strings / the id sequences of the other stay)
void row_set_text(row * r, int n, const int32_t * len, const uint8_t * bytes) {
    memset(&r->tc, 0, sizeof r->tc);
    r->tc.n = n;
    for (int k = 0; k < n; ++k) { r->tc.len[k] = len[k]; memcpy(r->tc.bytes[k], bytes + k * FQ_STOPT_MAX_LEN, (size_t) len[k]); }
    row_fresh(r);
}
void row_set_ids(row * r, int n_seqs, const int32_t * len, const int32_t * tok, int max_tokens) {
    memset(&r->ic, 0, sizeof r->ic);
    r->ic.on = 1; r->ic.n_seqs = n_seqs; r->ic.max_tokens = max_tokens;
    for (int k = 0; k < n_seqs; ++k) { r->ic.len[k] = len[k]; for (int j = 0; j < len[k]; ++j) r->ic.tok[k][j] = tok[k * FQ_STOP_MAX_LEN + j]; }
    row_fresh(r);
}
// one draw of `token` with bytes b[0..L): out = reason, n_drawn, cut_bytes afterwards; returns the reason
int row_draw(row * r, int token, const uint8_t * b, int L, int32_t * out) {
    fq_stop_draw(&r->ic, &r->is, token);
    const int reason = fq_stopt_draw(&r->tc, &r->ts, &r->is, b, L);
    out[0] = reason; out[1] = r->is.n_drawn; out[2] = r->ts.cut_bytes;
    return reason;
}
// as if `add` more bytes (a multiple of the ring's size, so every byte keeps its slot) had been drawn long ago: the way to the counter's end
void row_skip_bytes(row * r, int add) { r->ts.n_bytes = fq_stopt_count(r->ts.n_bytes, add); }
// a stream of draws over a vocabulary (pool, offs); out[i][3] as row_draw. Stops at the draw that ends the row and returns the draws taken
int row_run(row * r, const uint8_t * pool, const int32_t * offs, const int32_t * stream, int n, int32_t * out) {
    int i = 0;
    while (i < n && !fq_stop_finished(&r->is)) {
        row_draw(r, stream[i], pool + offs[stream[i]], offs[stream[i] + 1] - offs[stream[i]], out + 3 * i);
        ++i;
    }
    return i;
}
}

#ifdef STOP_TEXT_MAIN
// the file: integers. "0 n_vocab (len bytes...)*" the vocabulary; "1" a fresh row; "2 n (len bytes...)*" row_set_text; "3 n_seqs max_tokens (len toks...)*"
// row_set_ids; "4 token reason n_drawn cut_bytes" a draw and what it must give; "5 add" row_skip_bytes
int main(int argc, char ** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> pool; std::vector<int32_t> offs(1, 0);
    row * r = new row;                                      // (on the heap: the sanitizer sees every byte past its end)
    row_init(r);
    int op, draws = 0, bad = 0;
    auto rd = [&]() { int x = 0; if (fscanf(f, "%d", &x) != 1) { fprintf(stderr, "truncated case file\n"); exit(2); } return x; };
    while (fscanf(f, "%d", &op) == 1) {
        if (op == 0) {
            pool.clear(); offs.assign(1, 0);
            for (int n = rd(); n > 0; --n) { for (int l = rd(); l > 0; --l) pool.push_back((uint8_t) rd()); offs.push_back((int32_t) pool.size()); }
        } else if (op == 1) {
            row_init(r);
        } else if (op == 2) {
            const int n = rd();
            std::vector<int32_t> len((size_t) n + 1); std::vector<uint8_t> bytes((size_t) n * FQ_STOPT_MAX_LEN + 1);
            for (int k = 0; k < n; ++k) { len[k] = rd(); for (int j = 0; j < len[k]; ++j) bytes[(size_t) k * FQ_STOPT_MAX_LEN + j] = (uint8_t) rd(); }
            row_set_text(r, n, len.data(), bytes.data());
        } else if (op == 3) {
            const int n = rd(), max_tokens = rd();
            std::vector<int32_t> len((size_t) n + 1), tok((size_t) n * FQ_STOP_MAX_LEN + 1);
            for (int k = 0; k < n; ++k) { len[k] = rd(); for (int j = 0; j < len[k]; ++j) tok[(size_t) k * FQ_STOP_MAX_LEN + j] = rd(); }
            row_set_ids(r, n, len.data(), tok.data(), max_tokens);
        } else if (op == 4) {
            const int t = rd(), want[3] = { rd(), rd(), rd() };
            int32_t got[3];
            // the token's bytes in a buffer of exactly their length: a read past either end is the sanitizer's
            std::vector<uint8_t> b(pool.begin() + offs[t], pool.begin() + offs[t + 1]);
            row_draw(r, t, b.data(), (int) b.size(), got);
            ++draws;
            if (got[0] != want[0] || got[1] != want[1] || got[2] != want[2]) {
                if (++bad <= 10) fprintf(stderr, "draw %d (token %d): got %d %d %d, want %d %d %d\n", draws, t, got[0], got[1], got[2], want[0], want[1], want[2]);
            }
        } else if (op == 5) {
            row_skip_bytes(r, rd());
        } else { fprintf(stderr, "bad op %d\n", op); return 2; }
    }
    fclose(f);
    delete r;
    printf("%d draws, %d mismatches\n", draws, bad);
    return bad ? 1 : 0;
}
#endif
