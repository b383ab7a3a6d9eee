// kernels_score.hip -- the reference's soft-max probability of a given token per logits row (examples/falcon_perplexity/
// falcon_perplexity.cpp:12-27, :107-117; the arithmetic is csrc/fq_score.h), so that scoring keeps the logits in HBM.
//
// The contract is the ORDER of the double sum: element 0 first, one addition per element. It is kept by construction: one
// workgroup owns a row, and ONE lane of it (thread 0) owns the row's sum and walks it through one dependent f64 add per
// element. What the other lanes share out is everything that is independent per element: the row's maximum (a float max does
// not depend on the order for the inputs covered: no NaN) and the terms expf(l[v] - max), computed from coalesced row reads and
// handed to the chain lane through LDS in tiles of FQ_SC_TILE floats, two buffers: waves 1..3 fill tile k+1 while the chain lane
// adds tile k. A row's result therefore depends on nothing but the row: not on n_rows, not on its place in the launch, not on
// ggml_hip_reference_order. The logits are read, never written.
#include "fq_device.h"
#include "hip_context.h"
#include "fq_score.h"
#include "../../include/ggml-hip-ops.h"

#include <math.h>

#define FQ_SC_THREADS 256
#define FQ_SC_TILE 4096             // terms per hand-off (2 x 16 KB of LDS)
#define FQ_SC_BLOCK 32              // terms the chain lane holds in registers at a time

// terms [base, base + cnt) of the row -> dst[0, cnt), by threads first, first + step, ...; the target's term also goes to *e_t
__device__ __forceinline__ void sc_fill(const float * __restrict__ x, int base, int cnt, float m, int t, float * __restrict__ dst,
                                        float * __restrict__ e_t, int first, int step) {
#pragma unroll 4
    for (int i = first; i < cnt; i += step) {
        const float e = fq_score_term(x[base + i], m);
        dst[i] = e;
        if (base + i == t) *e_t = e;
    }
}

__global__ void __launch_bounds__(FQ_SC_THREADS) k_score_rows(const float * __restrict__ logits, int64_t stride, int n,
        const int32_t * __restrict__ targets, float * __restrict__ prob, float * __restrict__ max_out, double * __restrict__ sum_out) {
    __shared__ __attribute__((aligned(16))) float term[2][FQ_SC_TILE];
    __shared__ float red[FQ_SC_THREADS / 64];
    __shared__ float sh_et;

    const int row = blockIdx.x, tid = threadIdx.x;
    const int t = targets[row];
    if (t < 0) return;                                      // (the whole workgroup: nothing is written for a skipped row)
    const float * x = logits + (int64_t) row * stride;

    float m = x[0];
    for (int i0 = tid; i0 < n; i0 += 8 * FQ_SC_THREADS) {
        float r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = i0 + u * FQ_SC_THREADS; r[u] = x[i < n ? i : 0]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) m = r[u] > m ? r[u] : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float v = __shfl_xor(m, o); m = v > m ? v : m; }
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < FQ_SC_THREADS / 64; ++w) m = red[w] > m ? red[w] : m;

    const int n_tiles = (n + FQ_SC_TILE - 1) / FQ_SC_TILE;
    sc_fill(x, 0, n < FQ_SC_TILE ? n : FQ_SC_TILE, m, t, term[0], &sh_et, tid, FQ_SC_THREADS);
    __syncthreads();
    double sum = 0.0;
    for (int k = 0; k < n_tiles; ++k) {
        if (tid >= 64) {
            if (k + 1 < n_tiles) {
                const int base = (k + 1) * FQ_SC_TILE;
                sc_fill(x, base, n - base < FQ_SC_TILE ? n - base : FQ_SC_TILE, m, t, term[(k + 1) & 1], &sh_et, tid - 64, FQ_SC_THREADS - 64);
            }
        } else if (tid == 0) {
            // THE chain: element k * FQ_SC_TILE + i is added after every element before it and before every element after it
            const float * e = term[k & 1];
            const int cnt = n - k * FQ_SC_TILE < FQ_SC_TILE ? n - k * FQ_SC_TILE : FQ_SC_TILE;
            // (blocks of FQ_SC_BLOCK terms, the next block's LDS reads issued before this block's additions: the reads' latency hides behind the chain)
            const int nb = cnt / FQ_SC_BLOCK;
            float4 cur[FQ_SC_BLOCK / 4], nxt[FQ_SC_BLOCK / 4];
            if (nb > 0) {
#pragma unroll
                for (int u = 0; u < FQ_SC_BLOCK / 4; ++u) cur[u] = *(const float4 *)(e + 4 * u);
            }
            for (int b = 0; b < nb; ++b) {
                const float * en = e + (b + 1 < nb ? b + 1 : b) * FQ_SC_BLOCK;
#pragma unroll
                for (int u = 0; u < FQ_SC_BLOCK / 4; ++u) nxt[u] = *(const float4 *)(en + 4 * u);
#pragma unroll
                for (int u = 0; u < FQ_SC_BLOCK / 4; ++u) {
                    sum = fq_score_step(sum, cur[u].x);
                    sum = fq_score_step(sum, cur[u].y);
                    sum = fq_score_step(sum, cur[u].z);
                    sum = fq_score_step(sum, cur[u].w);
                }
#pragma unroll
                for (int u = 0; u < FQ_SC_BLOCK / 4; ++u) cur[u] = nxt[u];
            }
            for (int i = nb * FQ_SC_BLOCK; i < cnt; ++i) sum = fq_score_step(sum, e[i]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        prob[row] = fq_score_prob(sh_et, sum);
        if (max_out) max_out[row] = m;
        if (sum_out) sum_out[row] = sum;
    }
}

void fq_launch_score(const float * logits, int64_t row_stride, int n_rows, int n_vocab, const int32_t * targets, float * prob,
                     float * max_out, double * sum_out, hipStream_t st) {
    if (n_rows < 1) return;
    hipLaunchKernelGGL(k_score_rows, dim3((unsigned) n_rows), dim3(FQ_SC_THREADS), 0, st, logits, row_stride, n_vocab, targets, prob, max_out, sum_out);
}

// ------------------------------------------------------------------------------------------------ C ABI (include/ggml-hip-ops.h)
extern "C" void ggml_hip_score_rows(const float * logits_dev, int64_t row_stride, int n_rows, int n_vocab, const int32_t * targets_dev,
                                    float * prob_dev, float * max_dev, double * sum_dev) {
    if (n_vocab < 1 || !logits_dev || !targets_dev || !prob_dev) { fprintf(stderr, "ggml-hip: score_rows(%d rows, n_vocab %d): needs n_vocab >= 1 and its pointers\n", n_rows, n_vocab); exit(1); }
    fq_launch_score(logits_dev, row_stride, n_rows, n_vocab, targets_dev, prob_dev, max_dev, sum_dev, fq_ctx().stream);
}
