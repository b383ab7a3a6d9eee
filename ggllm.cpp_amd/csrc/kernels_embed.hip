// kernels_embed.hip -- pooled text vectors (csrc/fq_embed.h): the f64 column sums of the ln_f rows an eval leaves, carried from call to
// call in device memory, and the mean / unit vector made of them.
//
// The contract is the ORDER of a column's chain: row 0 of the first call first, one addition per row. It is kept by construction: ONE lane
// owns a column for the whole launch (never a second workgroup, never an atomic), and a launch starts from what the launch before it left.
// What a wave shares out is the columns: its 64 lanes read 64 neighbouring floats of a row (one 256-byte request), and a workgroup is one
// wave, so that n_embd / 64 workgroups spread over the chip (71 for Falcon-7B, 128 for Falcon-40B). Rows come in groups of FQ_EP_ROWS: the
// next group's loads are issued before this group's FQ_EP_ROWS dependent adds (two register buffers, as k_score_rows' chain lane reads LDS), so
// a group costs the longer of one round trip and its adds instead of their sum (measured: NOTEBOOK section 26).
#include "fq_device.h"
#include "hip_context.h"
#include "kernels.h"
#include "fq_embed.h"
#include "../../include/ggml-hip-ops.h"

#include <math.h>

#define FQ_EP_LANES 64
#define FQ_EP_ROWS 32               // rows in flight per lane

__global__ void __launch_bounds__(FQ_EP_LANES) k_embed_pool_accum(const float * __restrict__ rows, int n_rows, int n_embd,
                                                                   double * __restrict__ acc, long long * __restrict__ count) {
    const int col = blockIdx.x * FQ_EP_LANES + threadIdx.x;
    if (col == 0) *count = *count + (long long) n_rows;
    if (col >= n_embd) return;
    const float * x = rows + col;
    double a = acc[col];
    const int nb = n_rows / FQ_EP_ROWS;
    float cur[FQ_EP_ROWS], nxt[FQ_EP_ROWS];
    if (nb > 0) {
#pragma unroll
        for (int u = 0; u < FQ_EP_ROWS; ++u) cur[u] = x[(int64_t) u * n_embd];
    }
    for (int b = 0; b < nb; ++b) {
        const float * xn = x + (int64_t)(b + 1 < nb ? b + 1 : b) * FQ_EP_ROWS * n_embd;      // (the last group again: inside the rows, never used)
#pragma unroll
        for (int u = 0; u < FQ_EP_ROWS; ++u) nxt[u] = xn[(int64_t) u * n_embd];
#pragma unroll
        for (int u = 0; u < FQ_EP_ROWS; ++u) a = fq_embed_step(a, cur[u]);               // THE chain: row b * FQ_EP_ROWS + u after every row before it
#pragma unroll
        for (int u = 0; u < FQ_EP_ROWS; ++u) cur[u] = nxt[u];
    }
    for (int i = nb * FQ_EP_ROWS; i < n_rows; ++i) a = fq_embed_step(a, x[(int64_t) i * n_embd]);
    acc[col] = a;
}

// one workgroup: the means, then (normalize) s from per-thread strided partials combined in thread order by every thread alike, then the unit vector.
// s goes to *s_out; where it is 0 nothing is divided and out stays as it was (the host refuses)
__global__ void __launch_bounds__(FQ_EMBED_THREADS) k_embed_pool_finish(const double * __restrict__ acc, const long long * __restrict__ count, int n_embd,
                                                                         int normalize, float * __restrict__ out, double * __restrict__ s_out) {
    __shared__ double part[FQ_EMBED_THREADS];
    const int tid = threadIdx.x;
    const long long n = *count;
    if (n <= 0) return;
    if (!normalize) {
        for (int col = tid; col < n_embd; col += FQ_EMBED_THREADS) out[col] = fq_embed_mean(acc[col], n);
        return;
    }
    double p = 0.0;
    for (int col = tid; col < n_embd; col += FQ_EMBED_THREADS) p = fq_embed_sq_step(p, fq_embed_mean(acc[col], n));
    part[tid] = p;
    __syncthreads();
    double s = 0.0;
    for (int t = 0; t < FQ_EMBED_THREADS; ++t) s = s + part[t];
    if (tid == 0 && s_out) *s_out = s;
    if (s == 0.0) return;
    const double root = sqrt(s);
    for (int col = tid; col < n_embd; col += FQ_EMBED_THREADS) out[col] = fq_embed_unit(fq_embed_mean(acc[col], n), root);
}

void fq_launch_embed_pool_accum(const float * rows, int n_rows, int n_embd, double * acc, long long * count, hipStream_t st) {
    FQ_TL(st, "embed_pool_accum");
    if (n_rows < 1 || n_embd < 1) return;
    hipLaunchKernelGGL(k_embed_pool_accum, dim3((unsigned)((n_embd + FQ_EP_LANES - 1) / FQ_EP_LANES)), dim3(FQ_EP_LANES), 0, st, rows, n_rows, n_embd, acc, count);
}
void fq_launch_embed_pool_finish(const double * acc, const long long * count, int n_embd, int normalize, float * out, double * s_out, hipStream_t st) {
    FQ_TL(st, "embed_pool_finish");
    hipLaunchKernelGGL(k_embed_pool_finish, dim3(1), dim3(FQ_EMBED_THREADS), 0, st, acc, count, n_embd, normalize, out, s_out);
}

// count_dev's value and, with normalize, s are read back (the call synchronises): 1 for count 0 and 2 for s 0, after a message, with out_dev untouched
int fq_embed_pool_finish_checked(const double * acc, const long long * count, int n_embd, int normalize, float * out, double * s_dev, hipStream_t st) {
    long long n = 0;
    HIP_CHECK(hipMemcpyAsync(&n, count, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (n <= 0) { fprintf(stderr, "ggml-hip: embed_pool_finish: no rows were pooled (count %lld)\n", n); return 1; }
    fq_launch_embed_pool_finish(acc, count, n_embd, normalize, out, s_dev, st);
    if (!normalize) return 0;
    double s = 0.0;
    HIP_CHECK(hipMemcpyAsync(&s, s_dev, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (s == 0.0) { fprintf(stderr, "ggml-hip: embed_pool_finish: the mean is the zero vector, which has no direction\n"); return 2; }
    return 0;
}

// ------------------------------------------------------------------------------------------------ C ABI (include/ggml-hip-ops.h)
extern "C" int ggml_hip_embed_pool_accum(const float * rows_dev, int n_rows, int n_embd, double * acc_dev, int64_t * count_dev) {
    if (n_rows < 1 || n_embd < 1 || !rows_dev || !acc_dev || !count_dev) {
        fprintf(stderr, "ggml-hip: embed_pool_accum(%d rows, n_embd %d): needs n_rows >= 1, n_embd >= 1 and its pointers\n", n_rows, n_embd);
        return 1;
    }
    fq_launch_embed_pool_accum(rows_dev, n_rows, n_embd, acc_dev, (long long *) count_dev, fq_ctx().stream);
    return 0;
}
extern "C" int ggml_hip_embed_pool_finish(const double * acc_dev, const int64_t * count_dev, int n_embd, int normalize, float * out_dev) {
    if (n_embd < 1 || !acc_dev || !count_dev || !out_dev) { fprintf(stderr, "ggml-hip: embed_pool_finish(n_embd %d): needs n_embd >= 1 and its pointers\n", n_embd); return 3; }
    double * s_dev = nullptr;
    if (normalize) HIP_CHECK(hipMalloc((void **) &s_dev, 8));
    const int rc = fq_embed_pool_finish_checked(acc_dev, (const long long *) count_dev, n_embd, normalize, out_dev, s_dev, fq_ctx().stream);
    if (s_dev) HIP_CHECK(hipFree(s_dev));
    return rc;
}
