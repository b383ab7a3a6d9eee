// fq_stop.h -- when a sampled row ends: stop sequences of token ids and a budget of drawn tokens, stated once for the
// device sampler (kernels_sample.hip runs fq_stop_draw on the lane that knows the drawn token) and a host test
// (tests/test_stop_cpu.py compiles this header with g++ and checks it against a restatement of the rule).
//
// The rule, per row, after every draw: n_drawn += 1 and the token enters the tail (the last FQ_STOP_MAX_LEN drawn tokens).
// The row then ends with reason k if stop sequence k equals the last len[k] drawn tokens -- the lowest such k; a sequence
// longer than n_drawn cannot match (the tail holds only tokens drawn since the stops were set). Otherwise it ends with
// FQ_STOP_BUDGET if max_tokens > 0 and n_drawn == max_tokens. A running row has FQ_STOP_RUNNING. A row that has ended is
// not drawn for again (the callers skip it) until fq_stop_reset.
//
// Unlike falcon_main (falcon_main.cpp:1024-1055), which looks at the generation before it pushes the new token -- one
// iteration late, across the prompt's tokens as well -- the row ends AT the draw that completes a sequence, and only drawn
// tokens count.
#pragma once
#include "fq_types.h"
#include <stdint.h>

#define FQ_STOP_MAX_SEQS 16
#define FQ_STOP_MAX_LEN 8           // a power of two: the tail is a ring indexed by the draw's number
#define FQ_STOP_RUNNING (-1)
#define FQ_STOP_BUDGET (-2)
#define FQ_STOP_CONTEXT (-3)        // the draw filled the row's cache (fq_stop_context)

struct fq_stop_cfg {                // a row's configuration (on == 0: the row has no stops and is never looked at)
    int32_t on, n_seqs, max_tokens;
    int32_t len[FQ_STOP_MAX_SEQS];
    int32_t tok[FQ_STOP_MAX_SEQS][FQ_STOP_MAX_LEN];
};
struct fq_stop_state {              // a row's state: draw d (0-based) sits in tail[d % FQ_STOP_MAX_LEN]
    int32_t n_drawn, reason;
    int32_t tail[FQ_STOP_MAX_LEN];
};

FQ_HD void fq_stop_reset(fq_stop_state * s) {
    s->n_drawn = 0; s->reason = FQ_STOP_RUNNING;
    for (int i = 0; i < FQ_STOP_MAX_LEN; ++i) s->tail[i] = -1;
}
FQ_HD bool fq_stop_finished(const fq_stop_state * s) { return s->reason != FQ_STOP_RUNNING; }

// the row drew `token`: returns (and stores) the row's reason afterwards
FQ_HD int fq_stop_draw(const fq_stop_cfg * c, fq_stop_state * s, int32_t token) {
    s->tail[s->n_drawn & (FQ_STOP_MAX_LEN - 1)] = token;
    const int n = ++s->n_drawn;
    int reason = FQ_STOP_RUNNING;
    for (int k = 0; k < c->n_seqs && reason == FQ_STOP_RUNNING; ++k) {
        const int l = c->len[k];
        if (l > n) continue;
        bool eq = true;
        for (int j = 0; j < l && eq; ++j) eq = c->tok[k][j] == s->tail[(n - l + j) & (FQ_STOP_MAX_LEN - 1)];
        if (eq) reason = k;
    }
    if (reason == FQ_STOP_RUNNING && c->max_tokens > 0 && n == c->max_tokens) reason = FQ_STOP_BUDGET;
    s->reason = reason;
    return reason;
}

// The end of the cache, the last thing looked at on a draw (behind fq_stop_draw and, where the row has strings, fq_stopt_end):
// a draw made at position pos -- the row's token was evaluated there, the draw would move it to pos + 1 -- fills the cache when
// pos + 1 reaches limit (the cache's length; 0: the rule is off). Returns whether it did. A row that is still running then ends
// with FQ_STOP_CONTEXT; a row that one of the other rules has just ended keeps that reason. Either way the caller leaves the
// row's position and next token as they were: the frozen row evaluates the same token at the same position again, and no
// position >= limit is ever evaluated. The drawn token has counted like any other (n_drawn, tail, ring).
FQ_HD bool fq_stop_context(fq_stop_state * s, int pos, int limit) {
    if (limit <= 0 || pos + 1 < limit) return false;
    if (s->reason == FQ_STOP_RUNNING) s->reason = FQ_STOP_CONTEXT;
    return true;
}
// a row that ended with FQ_STOP_CONTEXT runs again, nothing else of it changed; any other reason is refused (false)
FQ_HD bool fq_stop_resume(fq_stop_state * s) {
    if (s->reason != FQ_STOP_CONTEXT) return false;
    s->reason = FQ_STOP_RUNNING;
    return true;
}
