// host build of ggllm.cpp_amd/csrc/fq_stop.h for tests/test_stop_cpu.py: one row's stops driven draw by draw
#include "fq_stop.h"

extern "C" {
// cfg: n_seqs, max_tokens, len[16], tok[16][8] (the layout of ggml_hip_stops without its order); state: n_drawn, reason, tail[8]
void stop_reset(int32_t * state) { fq_stop_reset((fq_stop_state *) state); }
int stop_draw(int n_seqs, const int32_t * len, const int32_t * tok, int max_tokens, int32_t * state, int token) {
    fq_stop_cfg c{};
    c.on = 1; c.n_seqs = n_seqs; c.max_tokens = max_tokens;
    for (int k = 0; k < n_seqs; ++k) { c.len[k] = len[k]; for (int j = 0; j < len[k]; ++j) c.tok[k][j] = tok[k * FQ_STOP_MAX_LEN + j]; }
    return fq_stop_draw(&c, (fq_stop_state *) state, token);
}
// a stream of draws; out[i]: the reason after draw i. Stops at the draw that ends the row (as the callers do) and returns the draws taken
int stop_run(int n_seqs, const int32_t * len, const int32_t * tok, int max_tokens, int32_t * state, const int32_t * stream, int n, int32_t * out) {
    int i = 0;
    while (i < n) {
        out[i] = stop_draw(n_seqs, len, tok, max_tokens, state, stream[i]);
        ++i;
        if (fq_stop_finished((const fq_stop_state *) state)) break;
    }
    return i;
}
int stop_state_words() { return (int)(sizeof(fq_stop_state) / 4); }
}
