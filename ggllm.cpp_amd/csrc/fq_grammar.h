// fq_grammar.h -- which tokens a constrained row may draw, stated once for the device (kernels_grammar.hip builds the index from it,
// kernels_sample_row.h's MASK instantiations advance a row's state through it) and a host test (tests/test_grammar_cpu.py compiles
// this header with g++ and checks it against tests/grammar_ref.py).
//
// The constraint is a deterministic automaton over BYTES: n_states states (1 <= n_states <= FQ_GRAMMAR_MAX_STATES), a table
// uint16_t trans[n_states][256], uint8_t accept[n_states] and a start state. State 0 is the dead state: all its transitions are 0 and
// it never accepts. The state after a token is the state after its bytes (fq_grammar_walk: 0 stays 0).
//
// Token t is allowed in state s:
//   t == eos_id (eos_id may be -1: no such token)   exactly when accept[s]; drawing it leaves the state as it is
//   a token without bytes                            never
//   any other token                                  exactly when walk(s, bytes(t)) != 0
// The index is uint64_t allow[n_states][n_words], n_words = ceil(n_vocab / 64): bit t % 64 of word t / 64 is set exactly when t is
// allowed in that state; bits at and beyond n_vocab are 0; state 0's row is all 0 (accept[0] is taken as 0 whatever the table says).
//
// A grammar in which some state other than 0 allows no token is refused (FQ_GRAMMAR_DEAD_END and the state's number: a row that
// got there could draw nothing), and so is a table with an entry >= n_states or a live transition out of state 0
// (FQ_GRAMMAR_BAD_TRANS and the state whose row holds it).
//
// At a draw a candidate that is not allowed in the row's state has the logit -inf, applied AFTER bias and penalties: what a -inf
// bias entry on every forbidden token gives for a repeat penalty > 0, without the 0 * inf a penalty of 0 would make of it. After the
// draw the row's state is fq_grammar_advance's.
#pragma once
#include "fq_types.h"
#include <stdint.h>

#define FQ_GRAMMAR_MAX_STATES 16384
#define FQ_GRAMMAR_OK 0
#define FQ_GRAMMAR_BAD_ARGS 1       // sizes, the start state, eos_id or a missing array
#define FQ_GRAMMAR_BAD_TRANS 2      // a transition >= n_states, or out of state 0
#define FQ_GRAMMAR_DEAD_END 3       // a state other than 0 that allows no token

// a row's binding, one entry per sampler row in device memory (trans == nullptr: the row is unconstrained). The grammar's arrays
// are device pointers; state is the row's state word, moved by the drawing lane.
struct fq_grammar_row {
    const uint16_t * trans;         // [n_states][256]
    const uint64_t * allow;         // [n_states][n_words]
    const uint8_t * pool;           // the vocabulary the index was built with: token t is pool[offs[t] .. offs[t + 1])
    const int32_t * offs;           // [n_vocab + 1]
    int32_t n_words, eos_id, state, n_states;
};

FQ_HD int fq_grammar_words(int n_vocab) { return (n_vocab + 63) / 64; }

// THE transition: one byte
FQ_HD int fq_grammar_step(const uint16_t * trans, int state, uint8_t byte) { return trans[(int64_t) state * 256 + byte]; }

// the state after bytes b[0..L) (0 once it is 0)
FQ_HD int fq_grammar_walk(const uint16_t * trans, int state, const uint8_t * b, int L) {
    for (int i = 0; i < L && state != 0; ++i) state = fq_grammar_step(trans, state, b[i]);
    return state;
}

// what a finished walk says about a token of L bytes (state_after: the walk's result from `state`)
FQ_HD bool fq_grammar_allowed_after(const uint8_t * accept, int state, int token, int eos_id, int L, int state_after) {
    if (state == 0) return false;
    if (token == eos_id) return accept[state] != 0;
    return L > 0 && state_after != 0;
}

FQ_HD bool fq_grammar_allowed(const uint16_t * trans, const uint8_t * accept, int state, int token, int eos_id, const uint8_t * pool, const int32_t * offs) {
    const int o0 = offs[token], L = offs[token + 1] - o0;
    return fq_grammar_allowed_after(accept, state, token, eos_id, L, token == eos_id ? state : fq_grammar_walk(trans, state, pool + o0, L));
}

// the row's state after it drew `token`
FQ_HD int fq_grammar_advance(const uint16_t * trans, int state, int token, int eos_id, const uint8_t * pool, const int32_t * offs) {
    if (token == eos_id) return state;
    const int o0 = offs[token];
    return fq_grammar_walk(trans, state, pool + o0, offs[token + 1] - o0);
}

// word w of state s's index row, one thread's form of what the device takes from a wave's ballot
FQ_HD uint64_t fq_grammar_index_word(const uint16_t * trans, const uint8_t * accept, int state, int w, int n_vocab, int eos_id, const uint8_t * pool, const int32_t * offs) {
    uint64_t word = 0;
    for (int j = 0; j < 64; ++j) {
        const int t = w * 64 + j;
        if (t < n_vocab && fq_grammar_allowed(trans, accept, state, t, eos_id, pool, offs)) word |= 1ull << j;
    }
    return word;
}

// the table's own check, before anything is made from it: FQ_GRAMMAR_OK, or the code and (BAD_TRANS) the state in *bad_state
FQ_HD int fq_grammar_check_table(int n_states, int start, const uint16_t * trans, const uint8_t * accept, int n_vocab, int eos_id, int * bad_state) {
    *bad_state = -1;
    if (n_states < 1 || n_states > FQ_GRAMMAR_MAX_STATES || start < 0 || start >= n_states || !trans || !accept || n_vocab < 1 || eos_id < -1 || eos_id >= n_vocab) return FQ_GRAMMAR_BAD_ARGS;
    for (int s = 0; s < n_states; ++s)
        for (int b = 0; b < 256; ++b) {
            const int to = trans[(int64_t) s * 256 + b];
            if (to >= n_states || (s == 0 && to != 0)) { *bad_state = s; return FQ_GRAMMAR_BAD_TRANS; }
        }
    return FQ_GRAMMAR_OK;
}

// the creation check on the per-state counts of allowed tokens: the lowest state other than 0 that allows none
FQ_HD int fq_grammar_check_counts(int n_states, const int32_t * counts, int * bad_state) {
    *bad_state = -1;
    for (int s = 1; s < n_states; ++s) if (counts[s] == 0) { *bad_state = s; return FQ_GRAMMAR_DEAD_END; }
    return FQ_GRAMMAR_OK;
}
