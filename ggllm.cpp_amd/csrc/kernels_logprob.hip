// kernels_logprob.hip -- per logits row: the soft-max probability of the chosen token and the n_top most likely ids with
// theirs (the definition is csrc/fq_logprob.h), so that a decode loop can report what the model thought of its own output
// without copying logits to the host.
//
// The probabilities are fq_score.h's, so the ORDER of the double sum is the contract, kept by construction exactly as
// k_score_rows keeps it (kernels_score.hip; the chain is restated here rather than shared, so that not one instruction of
// that kernel moves): one workgroup owns a row, thread 0 owns the row's sum and walks it through one dependent f64 add per
// element, waves 1..3 compute the terms expf(l[v] - max) into two LDS tiles ahead of it.
//
// The top-n selection is exact and rides on the passes the row needs anyway. In the maximum's pass, thread t sees elements
// t, t + 256, ... and keeps the FQ_LP_KEEP largest 64-bit sort keys (fq_sort_key: value descending, id ascending) of them in
// registers. Then n_top rounds of a workgroup maximum over the threads' heads pick the winners in descending order; the
// owner of a winner pops it, and only when its short list runs dry does it rescan its own elements for the next
// FQ_LP_KEEP keys below the winner (rows whose leaders crowd into one residue class mod 256; at most n_top / FQ_LP_KEEP
// rescans of V / 256 elements each). Keys are distinct, so the result is unique: it does not depend on n_rows, on the row's
// place in the launch, or on ggml_hip_reference_order. The rounds run before the chain starts (a few microseconds next to
// the chain's V dependent additions). The logits are read, never written; every store is a vector store.
#include "fq_device.h"
#include "hip_context.h"
#include "fq_logprob.h"
#include "../../include/ggml-hip-ops.h"

#include <math.h>

#define FQ_LP_THREADS 256
#define FQ_LP_TILE 4096             // terms per hand-off (2 x 16 KB of LDS)
#define FQ_LP_BLOCK 32              // terms the chain lane holds in registers at a time
#define FQ_LP_KEEP 4                // keys a thread keeps between rescans

// c0 > c1 > c2 > c3 (0: empty) takes k if it is among the four largest
__device__ __forceinline__ void lp_push(uint64_t k, uint64_t & c0, uint64_t & c1, uint64_t & c2, uint64_t & c3) {
    if (k > c3) {
        uint64_t t = k, s;
        s = c0 > t ? c0 : t; t = c0 > t ? t : c0; c0 = s;
        s = c1 > t ? c1 : t; t = c1 > t ? t : c1; c1 = s;
        s = c2 > t ? c2 : t; t = c2 > t ? t : c2; c2 = s;
        c3 = t;
    }
}

__device__ __forceinline__ void lp_fill(const float * __restrict__ x, int base, int cnt, float m, float * __restrict__ dst, int first, int step) {
#pragma unroll 4
    for (int i = first; i < cnt; i += step) dst[i] = fq_score_term(x[base + i], m);
}

// rec_steps (optional): row r's record is (rec_steps[r] + rec_bias) * rec_stride + r, else r; a record outside [0, rec_cap) is not written.
// skip (optional): a row with skip[r] != 0 -- one the sampler's launch left alone because it had ended (fq_stop.h) -- writes nothing
__global__ void __launch_bounds__(FQ_LP_THREADS) k_logprob_rows(const float * __restrict__ logits, int64_t stride, int n,
        const int32_t * __restrict__ chosen, int n_top, const int * __restrict__ rec_steps, int rec_bias, int rec_stride, int64_t rec_cap,
        float * __restrict__ prob, int32_t * __restrict__ top_id, float * __restrict__ top_prob, float * __restrict__ max_out, double * __restrict__ sum_out,
        const int * __restrict__ skip) {
    __shared__ __attribute__((aligned(16))) float term[2][FQ_LP_TILE];
    __shared__ float red[FQ_LP_THREADS / 64];
    __shared__ uint64_t red_key[2][FQ_LP_THREADS / 64];
    __shared__ uint64_t win[FQ_LOGPROB_MAX_TOP];
    __shared__ double sh_sum;

    const int row = blockIdx.x, tid = threadIdx.x;
    if (skip && skip[row]) return;                          // (the whole workgroup)
    const float * x = logits + (int64_t) row * stride;
    const int64_t rec = rec_steps ? (int64_t)(rec_steps[row] + rec_bias) * rec_stride + row : row;
    if (rec < 0 || rec >= rec_cap) return;                  // (the whole workgroup)

    // the maximum (k_score_rows' scan) and, on the same loads, this thread's largest keys
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    float m = x[0];
    for (int i0 = tid; i0 < n; i0 += 8 * FQ_LP_THREADS) {
        float r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = i0 + u * FQ_LP_THREADS; r[u] = x[i < n ? i : 0]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) m = r[u] > m ? r[u] : m;
        if (n_top > 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int i = i0 + u * FQ_LP_THREADS; if (i < n) lp_push(fq_sort_key(r[u], i), c0, c1, c2, c3); }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float v = __shfl_xor(m, o); m = v > m ? v : m; }
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < FQ_LP_THREADS / 64; ++w) m = red[w] > m ? red[w] : m;

    // n_top rounds: the largest head wins, its owner moves on (n_top <= n: a round always finds a key)
    for (int j = 0; j < n_top; ++j) {
        uint64_t best = c0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint64_t v = __shfl_xor(best, o); best = v > best ? v : best; }
        if ((tid & 63) == 0) red_key[j & 1][tid >> 6] = best;
        __syncthreads();
        best = red_key[j & 1][0];
#pragma unroll
        for (int w = 1; w < FQ_LP_THREADS / 64; ++w) best = red_key[j & 1][w] > best ? red_key[j & 1][w] : best;
        if (best == 0) { if (tid == 0) win[j] = 0; continue; }      // (n_top > n: nothing left; the launchers refuse it)
        if (c0 == best) {                                   // (one thread: keys are distinct)
            win[j] = best;
            c0 = c1; c1 = c2; c2 = c3; c3 = 0;
            if (c0 == 0) {
                for (int i = tid; i < n; i += FQ_LP_THREADS) {
                    const uint64_t k = fq_sort_key(x[i], i);
                    if (k < best) lp_push(k, c0, c1, c2, c3);
                }
            }
        }
    }

    const int n_tiles = (n + FQ_LP_TILE - 1) / FQ_LP_TILE;
    lp_fill(x, 0, n < FQ_LP_TILE ? n : FQ_LP_TILE, m, term[0], tid, FQ_LP_THREADS);
    __syncthreads();
    double sum = 0.0;
    for (int k = 0; k < n_tiles; ++k) {
        if (tid >= 64) {
            if (k + 1 < n_tiles) {
                const int base = (k + 1) * FQ_LP_TILE;
                lp_fill(x, base, n - base < FQ_LP_TILE ? n - base : FQ_LP_TILE, m, term[(k + 1) & 1], tid - 64, FQ_LP_THREADS - 64);
            }
        } else if (tid == 0) {
            // THE chain: element k * FQ_LP_TILE + i is added after every element before it and before every element after it
            const float * e = term[k & 1];
            const int cnt = n - k * FQ_LP_TILE < FQ_LP_TILE ? n - k * FQ_LP_TILE : FQ_LP_TILE;
            const int nb = cnt / FQ_LP_BLOCK;
            float4 cur[FQ_LP_BLOCK / 4], nxt[FQ_LP_BLOCK / 4];
            if (nb > 0) {
#pragma unroll
                for (int u = 0; u < FQ_LP_BLOCK / 4; ++u) cur[u] = *(const float4 *)(e + 4 * u);
            }
            for (int b = 0; b < nb; ++b) {
                const float * en = e + (b + 1 < nb ? b + 1 : b) * FQ_LP_BLOCK;
#pragma unroll
                for (int u = 0; u < FQ_LP_BLOCK / 4; ++u) nxt[u] = *(const float4 *)(en + 4 * u);
#pragma unroll
                for (int u = 0; u < FQ_LP_BLOCK / 4; ++u) {
                    sum = fq_score_step(sum, cur[u].x);
                    sum = fq_score_step(sum, cur[u].y);
                    sum = fq_score_step(sum, cur[u].z);
                    sum = fq_score_step(sum, cur[u].w);
                }
#pragma unroll
                for (int u = 0; u < FQ_LP_BLOCK / 4; ++u) cur[u] = nxt[u];
            }
            for (int i = nb * FQ_LP_BLOCK; i < cnt; ++i) sum = fq_score_step(sum, e[i]);
            if (k + 1 == n_tiles) sh_sum = sum;
        }
        __syncthreads();
    }
    sum = sh_sum;
    if (tid < n_top) {
        const int id = win[tid] ? fq_key_id(win[tid]) : -1;
        top_id[rec * n_top + tid] = id;
        top_prob[rec * n_top + tid] = id >= 0 && id < n ? fq_score_prob(fq_score_term(x[id], m), sum) : fq_u2f(0x7fc00000u);
    }
    if (tid == 64) {
        const int ch = chosen[row];
        prob[rec] = ch >= 0 && ch < n ? fq_score_prob(fq_score_term(x[ch], m), sum) : fq_u2f(0x7fc00000u);
        if (max_out) max_out[rec] = m;
        if (sum_out) sum_out[rec] = sum;
    }
}

void fq_launch_logprob(const float * logits, int64_t row_stride, int n_rows, int n_vocab, const int32_t * chosen, int n_top,
                       const int * rec_steps, int rec_bias, int rec_stride, int64_t rec_cap, float * prob, int32_t * top_id, float * top_prob,
                       float * max_out, double * sum_out, hipStream_t st, const int * skip) {
    if (n_rows < 1) return;
    hipLaunchKernelGGL(k_logprob_rows, dim3((unsigned) n_rows), dim3(FQ_LP_THREADS), 0, st, logits, row_stride, n_vocab, chosen, n_top,
                       rec_steps, rec_bias, rec_stride, rec_cap, prob, top_id, top_prob, max_out, sum_out, skip);
}

// ------------------------------------------------------------------------------------------------ C ABI (include/ggml-hip-ops.h)
extern "C" int ggml_hip_logprob_rows(const float * logits_dev, int64_t row_stride, int n_rows, int n_vocab, const int32_t * chosen_dev, int n_top,
                                     float * prob_dev, int32_t * top_id_dev, float * top_prob_dev, float * max_dev, double * sum_dev) {
    if (n_vocab < 1 || n_top < 0 || n_top > GGML_HIP_LOGPROB_MAX_TOP || n_top > n_vocab || !logits_dev || !chosen_dev || !prob_dev ||
        (n_top > 0 && (!top_id_dev || !top_prob_dev))) {
        fprintf(stderr, "ggml-hip: logprob_rows(%d rows, n_vocab %d, n_top %d): needs n_vocab >= 1, 0 <= n_top <= min(%d, n_vocab) and its pointers\n",
                n_rows, n_vocab, n_top, GGML_HIP_LOGPROB_MAX_TOP);
        return 1;
    }
    fq_launch_logprob(logits_dev, row_stride, n_rows, n_vocab, chosen_dev, n_top, nullptr, 0, 0, n_rows, prob_dev, top_id_dev, top_prob_dev, max_dev, sum_dev, fq_ctx().stream);
    return 0;
}
