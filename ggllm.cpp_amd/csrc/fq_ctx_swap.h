// fq_ctx_swap.h -- what falcon_main does when the KV cache is full (examples/falcon/falcon_main.cpp:702-737), stated once
// for the library's planner (falcon_hip_swap_plan, falcon_hip_swap_history) and a host test (tests/test_ctx_swap_cpu.py
// compiles this header with g++ and checks it against tests/ctx_swap_ref.py). Plain C++: nothing here touches a device.
//
// The rule, quirks included. With the cache full and n_pending tokens waiting to be evaluated (1 while generating: the token
// just drawn), falcon_main keeps the first nk rows of the cache, evaluates the last n_regen tokens of its history again at
// positions nk .., and goes on with the pending token at nk + n_regen:
//   n_keep  := (n_keep < 0 || n_keep > prompt_size) ? prompt_size : n_keep                    (:524; prompt_size counts the system tokens)
//   nk      := n_system + ((n_keep > 0 && prompt_size > n_system) ? min(n_keep, prompt_size - n_system) : 0)
//   n_regen := nk < n_ctx / 2 ? n_ctx / 2 - nk : (nk < n_ctx - 10 ? 4 : 0)
//   n_regen := min(n_regen, n_history - n_pending)
//   regen   := history[n_history - n_pending - n_regen .. n_history - n_pending)
// The history is falcon_main's all_generation, NOT prompt + generation: the LAST token of every prompt batch of n_batch
// tokens (:1054-1055 pushes embd.back() once per loop turn), then every drawn token, the pending one included. With a long
// prompt and a short generation the clamp therefore pulls prompt-batch-last tokens into regen.
#pragma once
#include <stdint.h>

struct fq_swap_cfg {                // one generation's constants
    int32_t n_ctx;                  // the context's length
    int32_t n_system;               // tokens of the system prompt at the top of the prompt (0: none)
    int32_t n_keep;                 // falcon_main's --keep as given (negative: the whole prompt)
    int32_t prompt_size;            // tokens of the prompt, the system tokens included
};

// rows [0, nk) of the cache survive a swap
static inline int fq_swap_kept(const fq_swap_cfg * c) {
    const int n_keep = (c->n_keep < 0 || c->n_keep > c->prompt_size) ? c->prompt_size : c->n_keep;
    int nk = c->n_system;
    if (n_keep > 0 && c->prompt_size > c->n_system) nk += n_keep < c->prompt_size - c->n_system ? n_keep : c->prompt_size - c->n_system;
    return nk;
}

// the swap of a history of n_history tokens whose last n_pending are not evaluated yet: *n_past_new = nk, *n_regen as above
// (the regenerated tokens are history[n_history - n_pending - *n_regen .. n_history - n_pending)). 0, or 1 with nothing
// written for a configuration or history no generation has (n_ctx < 1, negative sizes, n_system > prompt_size,
// n_pending outside 0..n_history)
static inline int fq_swap_plan(const fq_swap_cfg * c, int n_history, int n_pending, int * n_past_new, int * n_regen) {
    if (!c || c->n_ctx < 1 || c->n_system < 0 || c->prompt_size < 0 || c->n_system > c->prompt_size || n_pending < 0 || n_history < n_pending) return 1;
    const int nk = fq_swap_kept(c);
    int r = 0;
    if (nk < c->n_ctx / 2) r = c->n_ctx / 2 - nk;
    else if (nk < c->n_ctx - 10) r = 4;
    if (r > n_history - n_pending) r = n_history - n_pending;
    if (n_past_new) *n_past_new = nk;
    if (n_regen) *n_regen = r;
    return 0;
}

// the history a prompt of n_prompt tokens leaves when it is consumed in batches of n_batch: the last token of every batch.
// Returns their number, (n_prompt + n_batch - 1) / n_batch, written to out unless it is null; 0 for n_batch < 1
static inline int fq_swap_history(const int32_t * prompt, int n_prompt, int n_batch, int32_t * out) {
    if (n_batch < 1 || n_prompt < 0) return 0;
    int n = 0;
    for (int i = 0; i < n_prompt; i += n_batch, ++n)
        if (out) out[n] = prompt[(i + n_batch < n_prompt ? i + n_batch : n_prompt) - 1];
    return n;
}
