// fq_score.h -- the reference's soft-max probability of one token (examples/falcon_perplexity/falcon_perplexity.cpp:12-27,
// :107-117), restated once for the device (kernels_score.hip) and a host harness (tests/host/score_harness.cpp):
//   max  = the largest logit of the row (float);
//   e_v  = expf(l[v] - max): a float subtraction, then the host libm's expf (fq_expf, fq_sample.h);
//   sum  = a double that starts at 0 and takes (double) e_v for v = 0, 1, ..., V-1 IN THAT ORDER;
//   prob = (float)((double) e_t / sum).
// The order of the sum is the contract: any other association moves the double's last bits on almost every row of model
// width, and the rounded prob on a rare one. Rows are finite or -inf with at least one finite value (+inf and NaN give
// the reference NaN and are not covered).
#pragma once
#include "fq_sample.h"

// the reference's scan: starts at l[0], replaces on >
FQ_HD float fq_score_max(const float * l, int n) {
    float m = l[0];
    for (int v = 1; v < n; ++v) m = l[v] > m ? l[v] : m;
    return m;
}
FQ_HD float fq_score_term(float l, float max) { return fq_expf(l - max); }
FQ_HD double fq_score_step(double sum, float e) { return sum + (double) e; }             // one link of the chain
FQ_HD float fq_score_prob(float e_t, double sum) { return (float)((double) e_t / sum); }

// a whole row on one thread: the definition the kernel is checked against
FQ_HD float fq_score_row(const float * l, int n, int t, float * max_out, double * sum_out) {
    const float m = fq_score_max(l, n);
    double sum = 0.0;
    for (int v = 0; v < n; ++v) sum = fq_score_step(sum, fq_score_term(l[v], m));
    if (max_out) *max_out = m;
    if (sum_out) *sum_out = sum;
    return fq_score_prob(fq_score_term(l[t], m), sum);
}
