// fq_spec.h -- draft-and-verify decode: where a pass's drafts come from and when the verify loop goes on to the next row,
// stated once for the device (kernels_sample.hip: k_verify_rows, k_draft_lookup) and a host test (tests/test_spec_cpu.py
// compiles this header with g++ and checks it against tests/spec_ref.py).
//
// A pass evaluates the pending token t0 at position pos and K drafts d_1..d_K at pos + 1..pos + K in one weight pass. The
// verify loop then runs the row's sampler over logits row 0, 1, ... in order -- one generator, one window, one stop state --
// and goes on from row j to row j + 1 only while the draw of row j IS d_{j+1} (fq_spec_go_on). A draft is only ever a guess
// at what the sampler is about to draw: a wrong one costs a row of the pass, never a token.
//
// Source LOOKUP (prompt lookup): the history h[0..n) is prompt plus draws, h[n-1] the pending token. For g = ngram_max down
// to ngram_min take the LARGEST j <= n - g - 1 with h[j..j+g) == h[n-g..n); the first g that has such a j gives
// d_i = h[j + g + i - 1] for i = 1..K, and -1 where that index is >= n; no g: every draft is -1.
//   fq_spec_lookup_seq states that rule as it reads. The device does not loop over g: with e = j + g - 1 the end of the
//   earlier occurrence (e <= n - 2) and m(e) the length of the common suffix of h[0..e] and h[0..n-1], capped at ngram_max,
//   (g, j) matches exactly when m(e) >= g. So the first g with a match is G = max over e of m(e) (if >= ngram_min), and its
//   largest j is the largest e with m(e) == G: ONE max-reduction over the keys (m(e) << 32 | e) -- fq_spec_suffix_key.
//
// Source GIVEN: the caller's guess q[0..m) of the continuation, aligned by the draw's number since the guess was set: q[i]
// guesses draw number i. Row i of a pass stands where draw number s + i - 1 will stand (s the number of the pass's first
// draw), so the drafts of that pass are d_i = q[s + i - 1], i = 1..K, -1 beyond m. Row 0 holds the pending token: no guess.
#pragma once
#include "fq_types.h"
#include <stdint.h>

#define FQ_SPEC_MAX_DRAFT 15        // K: a pass has at most 16 rows
#define FQ_SPEC_MAX_NGRAM 32
#define FQ_SPEC_OFF 0               // (the operator-level verify: the caller's drafts, none made)
#define FQ_SPEC_LOOKUP 1
#define FQ_SPEC_GIVEN 2

struct fq_spec_state {              // a sequence's state, in device memory
    int32_t n_hist;                 // tokens in the history
    int32_t n_guess, given_at;      // GIVEN: the guess's length, draws since it was set
    int32_t left;                   // draws the call may still make (< 0: no limit)
    int32_t ended;                  // the row's stops ended it (as the launch saw it last)
    int32_t passes, draws;          // passes that drew, their draws
    int32_t hist[FQ_SPEC_MAX_DRAFT + 1];      // hist[d - 1]: passes that made d draws
};

FQ_HD void fq_spec_reset(fq_spec_state * s) {
    s->n_hist = 0; s->n_guess = 0; s->given_at = 0; s->left = -1; s->ended = 0; s->passes = 0; s->draws = 0;
    for (int i = 0; i <= FQ_SPEC_MAX_DRAFT; ++i) s->hist[i] = 0;
}

// the rule as it reads: drafts[i - 1] = d_i, i = 1..K. Returns the g that matched (0: none)
FQ_HD int fq_spec_lookup_seq(const int32_t * h, int n, int ngram_min, int ngram_max, int K, int32_t * drafts) {
    for (int i = 0; i < K; ++i) drafts[i] = -1;
    for (int g = ngram_max; g >= ngram_min && g >= 1; --g) {
        for (int j = n - g - 1; j >= 0; --j) {
            bool eq = true;
            for (int k = 0; k < g && eq; ++k) eq = h[j + k] == h[n - g + k];
            if (!eq) continue;
            for (int i = 1; i <= K; ++i) { const int at = j + g + i - 1; drafts[i - 1] = at < n ? h[at] : -1; }
            return g;
        }
    }
    return 0;
}

// the key of an earlier occurrence's end e (0 <= e <= n - 2): (common suffix length of h[0..e] and h[0..n-1], capped) << 32 | e
FQ_HD int64_t fq_spec_suffix_key(const int32_t * h, int n, int e, int ngram_max) {
    int m = 0;
    while (m < ngram_max && m <= e && h[e - m] == h[n - 1 - m]) ++m;
    return ((int64_t) m << 32) | (int64_t) e;
}
// draft i (1-based) behind the largest key of the history (-1: no e at all); -1 where there is none
FQ_HD int32_t fq_spec_lookup_draft(const int32_t * h, int n, int64_t best, int ngram_min, int i) {
    if (best < 0 || (int)(best >> 32) < ngram_min || (int)(best >> 32) < 1) return -1;
    const int at = (int)(best & 0xFFFFFFFF) + i;
    return at < n ? h[at] : -1;
}
// the same rule through the keys, one end after the other (what the device reduces in parallel)
FQ_HD void fq_spec_lookup_keys(const int32_t * h, int n, int ngram_min, int ngram_max, int K, int32_t * drafts) {
    int64_t best = -1;
    for (int e = 0; e <= n - 2; ++e) { const int64_t k = fq_spec_suffix_key(h, n, e, ngram_max); best = k > best ? k : best; }
    for (int i = 1; i <= K; ++i) drafts[i - 1] = fq_spec_lookup_draft(h, n, best, ngram_min, i);
}

// GIVEN: draft i (1-based) of a pass whose first draw is number s
FQ_HD int32_t fq_spec_given_draft(const int32_t * q, int m, int s, int i) { return s + i - 1 < m ? q[s + i - 1] : -1; }

// behind the draw of row j (0-based): does the loop go on to row j + 1? draft_next = d_{j+1} (-1: none), ended = a stop rule
// ended the row at this draw, next_pos = the position row j + 1 was evaluated at, n_ctx the cache's length (0: positions are
// not known, nothing to check), left = draws the call may still make behind this one (< 0: no limit)
FQ_HD bool fq_spec_go_on(int32_t draw, int32_t draft_next, bool ended, int j, int K, int next_pos, int n_ctx, int left) {
    return j < K && !ended && left != 0 && draft_next >= 0 && draw == draft_next && (n_ctx <= 0 || next_pos < n_ctx);
}
