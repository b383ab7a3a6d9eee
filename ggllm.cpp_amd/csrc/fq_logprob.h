// fq_logprob.h -- what the model thought of a generated token: the soft-max probability of the chosen id and the n most
// likely ids of a logits row with theirs, stated once for the device (kernels_logprob.hip) and a host harness
// (tests/host/logprob_harness.cpp). For a row l[0..V):
//   max, sum  = fq_score_row's (fq_score.h): the float max scan, then the double sum of fq_expf(l[v] - max), v = 0, 1, ..., V-1
//               IN THAT ORDER;
//   prob(id)  = fq_score_prob(fq_score_term(l[id], max), sum) -- the float ggml_hip_score_rows returns for target id, bit for bit;
//   top-n     = the n ids with the largest fq_sort_key(l[id], id) (fq_sample.h), listed in descending key order: value
//               descending, ties by id ascending -- the sampler's documented candidate order. The order is on the bits:
//               +0 ranks above -0; -inf entries rank last and have probability 0. Keys are distinct, so the list is unique.
// The probabilities belong to the RAW row, the model's distribution: they are taken before the sampler's logit bias, penalties,
// temperature and truncation, exactly like FalconModel.score and falcon_hip_perplexity. NaN and +inf are outside the
// contract, as in fq_score.h.
#pragma once
#include "fq_score.h"

#define FQ_LOGPROB_MAX_TOP 32

// the largest key of the row below `below` (0: none; no key of a row inside the contract is 0)
FQ_HD uint64_t fq_logprob_next(const float * l, int n, uint64_t below) {
    uint64_t best = 0;
    for (int v = 0; v < n; ++v) {
        const uint64_t k = fq_sort_key(l[v], v);
        if (k < below && k > best) best = k;
    }
    return best;
}

// a whole row on one thread: the definition the kernel is checked against. chosen < 0: no chosen probability (NaN is
// returned), the top-n are still written. top_id / top_prob: n_top entries each (n_top <= V), may be NULL when n_top == 0.
FQ_HD float fq_logprob_row(const float * l, int n, int chosen, int n_top, int32_t * top_id, float * top_prob, float * max_out, double * sum_out) {
    float m; double sum;
    const float p0 = fq_score_row(l, n, chosen < 0 ? 0 : chosen, &m, &sum);
    if (max_out) *max_out = m;
    if (sum_out) *sum_out = sum;
    uint64_t below = ~(uint64_t) 0;
    for (int j = 0; j < n_top; ++j) {
        below = fq_logprob_next(l, n, below);
        const int id = fq_key_id(below);
        top_id[j] = id;
        top_prob[j] = fq_score_prob(fq_score_term(l[id], m), sum);
    }
    return chosen < 0 ? fq_u2f(0x7fc00000u) : p0;
}
