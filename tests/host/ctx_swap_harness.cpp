// Host build of csrc/fq_ctx_swap.h (the context-swap planner) and of the context branch of csrc/fq_stop.h, for
// tests/test_ctx_swap_cpu.py: g++ compiles the very headers the library and the device sampler use.
#include "fq_ctx_swap.h"
#include "fq_stop.h"
#include "fq_stop_text.h"

extern "C" {

int swap_plan(int n_ctx, int n_system, int n_keep, int prompt_size, int n_history, int n_pending, int * n_past_new, int * n_regen) {
    const fq_swap_cfg c = { n_ctx, n_system, n_keep, prompt_size };
    return fq_swap_plan(&c, n_history, n_pending, n_past_new, n_regen);
}
// every history length 0 .. n_max of one configuration at once: out[2 * h] = n_past_new, out[2 * h + 1] = n_regen (-1, -1 where refused)
void swap_plan_all(int n_ctx, int n_system, int n_keep, int prompt_size, int n_pending, int n_max, int * out) {
    const fq_swap_cfg c = { n_ctx, n_system, n_keep, prompt_size };
    for (int h = 0; h <= n_max; ++h) {
        int a = -1, b = -1;
        if (fq_swap_plan(&c, h, n_pending, &a, &b)) a = b = -1;
        out[2 * h] = a; out[2 * h + 1] = b;
    }
}
int swap_history(const int32_t * prompt, int n_prompt, int n_batch, int32_t * out) { return fq_swap_history(prompt, n_prompt, n_batch, out); }

int stop_state_words() { return (int)(sizeof(fq_stop_state) / 4); }
int stop_context_reason() { return FQ_STOP_CONTEXT; }

// One row of the sampler's loop state on the host, in the order kernels_sample.hip runs the rules on a draw: fq_stop_draw, then (has_text) fq_stopt_draw, then
// fq_stop_context; the position and the next token move unless the last says the draw filled the cache. state: fq_stop_state; text_state: fq_stopt_state;
// loop[0] = position, loop[1] = next token. Returns the reason after the draw.
int ctx_draw(int n_seqs, const int32_t * len, const int32_t * tok, int max_tokens, int n_text, const int32_t * text_len, const uint8_t * text_bytes,
             void * state, void * text_state, int32_t * loop, int limit, int32_t token, const uint8_t * bytes, int n_bytes) {
    fq_stop_cfg c = {};
    c.on = 1; c.n_seqs = n_seqs; c.max_tokens = max_tokens;
    for (int k = 0; k < n_seqs; ++k) { c.len[k] = len[k]; for (int j = 0; j < FQ_STOP_MAX_LEN; ++j) c.tok[k][j] = tok[k * FQ_STOP_MAX_LEN + j]; }
    fq_stopt_cfg t = {};
    t.n = n_text;
    for (int k = 0; k < n_text; ++k) { t.len[k] = text_len[k]; for (int j = 0; j < FQ_STOPT_MAX_LEN; ++j) t.bytes[k][j] = text_bytes[k * FQ_STOPT_MAX_LEN + j]; }
    fq_stop_state * s = (fq_stop_state *) state;
    fq_stop_draw(&c, s, token);
    if (n_text > 0) fq_stopt_draw(&t, (fq_stopt_state *) text_state, s, bytes, n_bytes);
    if (!fq_stop_context(s, loop[0], limit)) { loop[0] += 1; loop[1] = token; }
    return s->reason;
}
int ctx_resume(void * state) { return fq_stop_resume((fq_stop_state *) state) ? 0 : 1; }
void ctx_reset(void * state, void * text_state) { fq_stop_reset((fq_stop_state *) state); fq_stopt_reset((fq_stopt_state *) text_state); }

}
