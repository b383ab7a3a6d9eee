// fq_guide.h -- classifier-free guidance (Sanchez et al. 2023, "Stay on topic with Classifier-Free Guidance"): the mix of a
// leader row x_b and a guide row x_g of V logits each, y[v] = lp_g[v] + scale * (lp_b[v] - lp_g[v]) over the rows'
// log-soft-maxes, stated once for the device (kernels_guide.hip) and a host harness (tests/host/guide_harness.cpp).
// For each row r of the two:
//   m_r     = fq_score_max(x_r, V) (fq_score.h);
//   e_r[v]  = fq_score_term(x_r[v], m_r): a float subtraction, then fq_expf;
//   S_r     = a double, summed IN THIS FIXED ORDER (there is no reference whose order had to be kept: this one is what a
//             workgroup of FQ_GUIDE_LANES lanes reading float4 sees, chosen for the machine and then pinned):
//               FQ_GUIDE_LANES partial sums q_0 .. q_255; q_j starts at 0.0 and takes (double) e_r[v] for every v with
//               (v / 4) % 256 == j, in increasing v (groups of four consecutive elements dealt round-robin to the lanes);
//               then for o = 1, 2, 4, ..., 128: q_j <- q_j + q_{j xor o} for every j at once (a butterfly: both partners of
//               an exchange hold the same bits afterwards, IEEE addition commutes); S_r = q_0;
//   L_r     = fq_logf((float) S_r) (fq_sample_chain.h). S_r >= 1 (the maximum's term is 1), so L_r >= 0;
//   lp_r[v] = (x_r[v] - m_r) - L_r: two float subtractions, in that order.
// The mix is a float subtraction, a multiplication and an addition, each rounded: no fused multiply-add.
// k_score_rows' single in-order chain (fq_score.h) is another association: the two sums differ in their last bits on almost
// every row of model width. Scoring keeps its order for the reference's sake; guidance pays for two rows in every decode step.
// Covered: rows of finite floats and a finite scale. Rows that hold +-inf or NaN are not.
#pragma once
#include "fq_score.h"
#include "fq_sample_chain.h"

#define FQ_GUIDE_LANES 256          // partial sums of a row == threads of k_guide_mix's workgroup
#define FQ_GUIDE_GROUP 4            // consecutive elements a lane takes at a time

FQ_HD double fq_guide_step(double q, float e) { return q + (double) e; }                  // one link of a lane's chain
FQ_HD float fq_guide_log_sum(double S) { return fq_logf((float) S); }
FQ_HD float fq_guide_lp(float x, float m, float L) { return (x - m) - L; }
FQ_HD float fq_guide_mix(float lp_b, float lp_g, float scale) {
    const float d = lp_b - lp_g;
    const float p = scale * d;
    return lp_g + p;
}

// a whole row's sum on one thread: the definition the kernel is checked against
FQ_HD double fq_guide_sum(const float * x, int n, float m) {
    double q[FQ_GUIDE_LANES];
    for (int j = 0; j < FQ_GUIDE_LANES; ++j) q[j] = 0.0;
    for (int v = 0; v < n; ++v) { const int j = (v / FQ_GUIDE_GROUP) % FQ_GUIDE_LANES; q[j] = fq_guide_step(q[j], fq_score_term(x[v], m)); }
    for (int o = 1; o < FQ_GUIDE_LANES; o <<= 1) {
        double t[FQ_GUIDE_LANES];
        for (int j = 0; j < FQ_GUIDE_LANES; ++j) t[j] = q[j] + q[j ^ o];
        for (int j = 0; j < FQ_GUIDE_LANES; ++j) q[j] = t[j];
    }
    return q[0];
}

// a whole pair on one thread. y: n floats (may be NULL); max_out / sum_out: {leader, guide} (may be NULL)
FQ_HD void fq_guide_pair(const float * xb, const float * xg, int n, float scale, float * y, float * max_out, double * sum_out) {
    const float mb = fq_score_max(xb, n), mg = fq_score_max(xg, n);
    const double Sb = fq_guide_sum(xb, n, mb), Sg = fq_guide_sum(xg, n, mg);
    const float Lb = fq_guide_log_sum(Sb), Lg = fq_guide_log_sum(Sg);
    if (y) for (int v = 0; v < n; ++v) y[v] = fq_guide_mix(fq_guide_lp(xb[v], mb, Lb), fq_guide_lp(xg[v], mg, Lg), scale);
    if (max_out) { max_out[0] = mb; max_out[1] = mg; }
    if (sum_out) { sum_out[0] = Sb; sum_out[1] = Sg; }
}
