// Host-side statement of the guidance arithmetic: ggllm.cpp_amd/csrc/fq_guide.h, the exact header the device kernel compiles.
// guide_rows mirrors ggml_hip_guide_rows: pair p mixes logits rows lead[p] and guide[p] (row r at logits + r * row_stride) with
// scale[p] into mixed + p * mixed_stride; pairs with lead[p] < 0 are skipped (nothing written); max_out / sum_out ([n_pairs][2],
// {leader, guide}) may be NULL. guide_expf / guide_logf: the header's two libm restatements, element-wise, for the tests'
// independent restatement of the order in numpy.
#include "fq_guide.h"
#include <stdint.h>

extern "C" {

void guide_rows(const float * logits, int64_t row_stride, int n_vocab, int n_pairs, const int32_t * lead, const int32_t * guide,
                const float * scale, float * mixed, int64_t mixed_stride, float * max_out, double * sum_out) {
    for (int p = 0; p < n_pairs; ++p) {
        if (lead[p] < 0) continue;
        fq_guide_pair(logits + lead[p] * row_stride, logits + guide[p] * row_stride, n_vocab, scale[p], mixed + p * mixed_stride,
                      max_out ? max_out + 2 * p : nullptr, sum_out ? sum_out + 2 * p : nullptr);
    }
}

void guide_expf(const float * x, float * out, int64_t n) { for (int64_t i = 0; i < n; ++i) out[i] = fq_expf(x[i]); }
void guide_logf(const float * x, float * out, int64_t n) { for (int64_t i = 0; i < n; ++i) out[i] = fq_logf(x[i]); }

}
