// fq_stop_text.h -- when a sampled row ends on TEXT: stop strings matched on the bytes of the drawn tokens, not on their ids,
// stated once for the device sampler (kernels_sample.hip: one wave, a lane per byte of the new token) and a host test
// (tests/test_stop_text_cpu.py compiles this header with g++ and checks it against bytes.find over the growing text).
//
// The drawn text of a row is the concatenation of the bytes of the tokens drawn since the row's stops were last set (what
// falcon_hip_token_to_bytes returns for them). After a draw of a token with bytes b[0..L) the row ends if some stop string
// is a suffix of the drawn text up to and including b[j], for a j in [0, L): the smallest such j wins, and among the
// strings that complete at that j the lowest index k. The reason is FQ_STOP_TEXT0 + k -- the first values an id sequence
// cannot produce, in the reason word of fq_stop.h's state -- and cut_bytes = len[k] + (L - 1 - j) counts the bytes from
// the first byte of the match to the end of the drawn text: dropping that many bytes from the end of the detokenised
// drawn tokens leaves the text before the stop string (the cut may reach into earlier tokens, or into the middle of one).
// A string longer than the drawn text cannot match; a token without bytes matches nothing; L may exceed the ring (a match
// may lie wholly inside one long token).
//
// Order on one draw: fq_stop_draw first (id sequences, then the budget). A text match replaces FQ_STOP_RUNNING and
// FQ_STOP_BUDGET, never an id match. The bytes enter the ring on every draw.
#pragma once
#include "fq_stop.h"

#define FQ_STOPT_MAX 16
#define FQ_STOPT_MAX_LEN 32         // a power of two: the ring is indexed by the byte's number in the drawn text
#define FQ_STOP_TEXT0 16            // == FQ_STOP_MAX_SEQS

struct fq_stopt_cfg {               // a row's strings (n == 0: none, the rule is not run)
    int32_t n;
    int32_t len[FQ_STOPT_MAX];
    uint8_t bytes[FQ_STOPT_MAX][FQ_STOPT_MAX_LEN];
};
struct fq_stopt_state {             // byte i of the drawn text sits in ring[i % FQ_STOPT_MAX_LEN]; the last FQ_STOPT_MAX_LEN - 1 are ever read
    int32_t n_bytes, cut_bytes;     // n_bytes: the drawn text's length, kept from overflowing by fq_stopt_count (only "at least a string's length" is asked of it)
    uint8_t ring[FQ_STOPT_MAX_LEN];
};

FQ_HD void fq_stopt_reset(fq_stopt_state * s) {
    s->n_bytes = 0; s->cut_bytes = 0;
    for (int i = 0; i < FQ_STOPT_MAX_LEN; ++i) s->ring[i] = 0;
}
// the text's length after L more bytes: exact below 2^30, then held in [2^29, 2^30] congruent mod FQ_STOPT_MAX_LEN (the ring's index stays right)
FQ_HD int32_t fq_stopt_count(int32_t n_bytes, int32_t L) {
    int64_t n = (int64_t) n_bytes + L;
    while (n > (1 << 30)) n -= 1 << 29;
    return (int32_t) n;
}

// THE rule at one byte: the lowest k whose string is a suffix of the drawn text up to and including that byte, or -1.
// have: the text's length up to and including the byte; back(i), 0 <= i < min(have, FQ_STOPT_MAX_LEN): the text's byte i places before it (back(0): itself)
template <class Back>
FQ_HD int fq_stopt_match_at(const fq_stopt_cfg * c, int64_t have, Back back) {
    for (int k = 0; k < c->n; ++k) {
        const int l = c->len[k];
        if (l > have) continue;
        bool eq = true;
        for (int i = 0; i < l && eq; ++i) eq = c->bytes[k][l - 1 - i] == back(i);
        if (eq) return k;
    }
    return -1;
}
// what a match of string k at byte j of an L-byte token does to a row whose fq_stop_draw said `reason`: the row's reason afterwards
FQ_HD int fq_stopt_end(const fq_stopt_cfg * c, fq_stopt_state * t, fq_stop_state * s, int reason, int j, int k, int L) {
    if (k >= 0 && (reason == FQ_STOP_RUNNING || reason == FQ_STOP_BUDGET)) {
        reason = FQ_STOP_TEXT0 + k;
        t->cut_bytes = c->len[k] + (L - 1 - j);
        s->reason = reason;
    }
    return reason;
}

// the row drew a token with bytes b[0..L), and fq_stop_draw has run for it (s->reason is its result): returns (and stores)
// the row's reason afterwards. One thread's form of what the device spreads over a wave.
FQ_HD int fq_stopt_draw(const fq_stopt_cfg * c, fq_stopt_state * t, fq_stop_state * s, const uint8_t * b, int L) {
    const int n0 = t->n_bytes;
    int j = 0, k = -1;
    for (; j < L; ++j) {
        k = fq_stopt_match_at(c, (int64_t) n0 + j + 1, [&](int i) { return i <= j ? b[j - i] : t->ring[(n0 + j - i) & (FQ_STOPT_MAX_LEN - 1)]; });
        if (k >= 0) break;
    }
    for (int i = L > FQ_STOPT_MAX_LEN ? L - FQ_STOPT_MAX_LEN : 0; i < L; ++i) t->ring[(n0 + i) & (FQ_STOPT_MAX_LEN - 1)] = b[i];
    t->n_bytes = fq_stopt_count(n0, L);
    return fq_stopt_end(c, t, s, s->reason, j, k, L);
}
