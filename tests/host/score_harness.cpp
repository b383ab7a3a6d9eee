// Host-side statement of the scoring arithmetic, twice: score_fq is ggllm.cpp_amd/csrc/fq_score.h (the exact header the device
// kernel compiles), score_libm the reference's three lines (examples/falcon_perplexity/falcon_perplexity.cpp:12-27, :107-117)
// with <math.h> expf -- what the reference binary calls on this host. Both mirror ggml_hip_score_rows: row r at
// logits + r * row_stride, rows with targets[r] < 0 skipped (nothing written), max_out / sum_out / terms_out may be NULL
// (terms_out: [n_rows][n_vocab], the expf terms of the row, for the tests that re-associate the sum).
#include "fq_score.h"
#include <math.h>
#include <stdint.h>

extern "C" {

void score_fq(const float * logits, int64_t row_stride, int n_rows, int n_vocab, const int32_t * targets, float * prob, float * max_out,
              double * sum_out, float * terms_out) {
    for (int r = 0; r < n_rows; ++r) {
        if (targets[r] < 0) continue;
        const float * l = logits + r * row_stride;
        float m; double s;
        prob[r] = fq_score_row(l, n_vocab, targets[r], &m, &s);
        if (max_out) max_out[r] = m;
        if (sum_out) sum_out[r] = s;
        if (terms_out) for (int v = 0; v < n_vocab; ++v) terms_out[(int64_t) r * n_vocab + v] = fq_score_term(l[v], m);
    }
}

void score_libm(const float * logits, int64_t row_stride, int n_rows, int n_vocab, const int32_t * targets, float * prob, float * max_out,
                double * sum_out, float * terms_out) {
    for (int r = 0; r < n_rows; ++r) {
        if (targets[r] < 0) continue;
        const float * l = logits + r * row_stride;
        float max_logit = l[0];
        for (int v = 0; v < n_vocab; ++v) max_logit = l[v] > max_logit ? l[v] : max_logit;
        double sum_exp = 0.0;
        float e_t = 0.0f;
        for (int v = 0; v < n_vocab; ++v) {
            const float e = expf(l[v] - max_logit);
            sum_exp += e;
            if (v == targets[r]) e_t = e;
            if (terms_out) terms_out[(int64_t) r * n_vocab + v] = e;
        }
        prob[r] = (float)(e_t / sum_exp);
        if (max_out) max_out[r] = max_logit;
        if (sum_out) sum_out[r] = sum_exp;
    }
}

}
