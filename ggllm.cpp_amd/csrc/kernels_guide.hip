// kernels_guide.hip -- classifier-free guidance: the mix of a leader row and a guide row of logits (the arithmetic is
// csrc/fq_guide.h), so that a guided decode step keeps both rows in HBM / L2 and stays one replay.
//
// One workgroup of FQ_GUIDE_LANES threads owns a pair. The contract is the ORDER of the rows' double sums, and it is kept by
// construction: lane j of the workgroup IS partial sum q_j -- it reads groups j, j + 256, ... of four consecutive elements in
// increasing order and adds their terms one after the other -- and the butterfly runs on the lanes: steps 1..32 inside the wave
// (__shfl_xor), steps 64 and 128 through LDS. Three passes over the two rows, which lie in L2 behind lm_head (2 x 260 KB at
// Falcon's vocabulary): the maxima, the terms and sums, the writes. The rows are read 16 bytes a lane where n % 4 == 0 and the
// three rows involved are 16-byte aligned, element by element with the same dealing otherwise; GD_UNROLL groups per row are in
// flight per lane (kernels_sample_row.h's `pass` records what one load per iteration costs). A pair's result depends on nothing
// but its two rows and its scale: not on n_pairs, not on its place in the launch, not on ggml_hip_reference_order. The logits
// are read, never written.
// Where the time goes (NOTEBOOK, the section on guidance): not into the passes' round trips -- 8 groups in flight instead of 4 took
// 5 % off -- but into pass 2's 2 x 254 fq_expf per lane, each with a dependent look-up of its 32-entry table behind a branch, one
// wave per SIMD to hide it. Only the ADDITIONS are ordered: the terms could come from any lane of a larger workgroup through LDS,
// as k_score_rows hands them to its chain lane, without touching the pinned order. Not done here.
#include "fq_device.h"
#include "hip_context.h"
#include "fq_guide.h"
#include "../../include/ggml-hip-ops.h"

#include <math.h>

#define GD_THREADS FQ_GUIDE_LANES
#define GD_UNROLL 8                 // groups of a row in flight per lane (two rows: 16 loads)
static_assert(GD_THREADS == 256 && FQ_GUIDE_GROUP == 4, "lane j is partial sum q_j; a group is one float4");

// group g of the row (elements 4g .. 4g + 3); elements at and beyond n read as element n - 1 (their use is masked by gd_count)
template <bool VEC>
__device__ __forceinline__ float4 gd_load(const float * __restrict__ x, int g, int n) {
    if constexpr (VEC) return *(const float4 *)(x + 4 * (int64_t) g);
    const int v = 4 * g, l = n - 1;
    return make_float4(x[v < l ? v : l], x[v + 1 < l ? v + 1 : l], x[v + 2 < l ? v + 2 : l], x[v + 3 < l ? v + 3 : l]);
}
template <bool VEC>
__device__ __forceinline__ int gd_count(int g, int n) { return VEC ? 4 : (n - 4 * g < 4 ? n - 4 * g : 4); }

// f(g, group g of the leader, group g of the guide) for this lane's groups in increasing order, the loads of GD_UNROLL groups issued first
template <bool VEC, class F>
__device__ __forceinline__ void gd_pass(const float * __restrict__ xb, const float * __restrict__ xg, int n, int tid, F f) {
    const int ng = (n + 3) / 4;
    for (int g0 = tid; g0 < ng; g0 += GD_UNROLL * GD_THREADS) {
        float4 b[GD_UNROLL], c[GD_UNROLL];
#pragma unroll
        for (int u = 0; u < GD_UNROLL; ++u) {
            const int g = g0 + u * GD_THREADS;
            b[u] = gd_load<VEC>(xb, g < ng ? g : g0, n);
            c[u] = gd_load<VEC>(xg, g < ng ? g : g0, n);
        }
#pragma unroll
        for (int u = 0; u < GD_UNROLL; ++u) {
            const int g = g0 + u * GD_THREADS;
            if (g < ng) f(g, b[u], c[u]);
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void gd_pair(const float * __restrict__ xb, const float * __restrict__ xg, int n, float scale, float * __restrict__ y,
                                        float * __restrict__ max_out, double * __restrict__ sum_out, float (* red)[GD_THREADS / 64], double (* qs)[GD_THREADS]) {
    const int tid = threadIdx.x;
    // pass 1: the maxima (a float max over finite values does not depend on the order)
    float mb = xb[0], mg = xg[0];
    gd_pass<VEC>(xb, xg, n, tid, [&](int g, float4 b, float4 c) {
        const int cnt = gd_count<VEC>(g, n);
        const float bv[4] = { b.x, b.y, b.z, b.w }, cv[4] = { c.x, c.y, c.z, c.w };
#pragma unroll
        for (int e = 0; e < 4; ++e) if (e < cnt) { mb = bv[e] > mb ? bv[e] : mb; mg = cv[e] > mg ? cv[e] : mg; }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float vb = __shfl_xor(mb, o), vg = __shfl_xor(mg, o);
        mb = vb > mb ? vb : mb; mg = vg > mg ? vg : mg;
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = mb; red[1][tid >> 6] = mg; }
    __syncthreads();
    mb = red[0][0]; mg = red[1][0];
#pragma unroll
    for (int w = 1; w < GD_THREADS / 64; ++w) { mb = red[0][w] > mb ? red[0][w] : mb; mg = red[1][w] > mg ? red[1][w] : mg; }

    // pass 2: this lane's partial sums, element after element in increasing order (two independent chains)
    double qb = 0.0, qg = 0.0;
    gd_pass<VEC>(xb, xg, n, tid, [&](int g, float4 b, float4 c) {
        const int cnt = gd_count<VEC>(g, n);
        const float bv[4] = { b.x, b.y, b.z, b.w }, cv[4] = { c.x, c.y, c.z, c.w };
#pragma unroll
        for (int e = 0; e < 4; ++e) if (e < cnt) { qb = fq_guide_step(qb, fq_score_term(bv[e], mb)); qg = fq_guide_step(qg, fq_score_term(cv[e], mg)); }
    });
    // the butterfly: q_j <- q_j + q_{j xor o}; o = 1 .. 32 between the wave's lanes, 64 and 128 between the waves
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) { const double ob = __shfl_xor(qb, o), og = __shfl_xor(qg, o); qb = qb + ob; qg = qg + og; }
#pragma unroll
    for (int o = 64; o < GD_THREADS; o <<= 1) {
        qs[0][tid] = qb; qs[1][tid] = qg;
        __syncthreads();
        const double ob = qs[0][tid ^ o], og = qs[1][tid ^ o];
        __syncthreads();                                    // (read before the next step's writes)
        qb = qb + ob; qg = qg + og;
    }
    // (every lane holds q_0's bits now: each step leaves both partners of an exchange with the same sum)
    const float Lb = fq_guide_log_sum(qb), Lg = fq_guide_log_sum(qg);

    // pass 3: the mix
    gd_pass<VEC>(xb, xg, n, tid, [&](int g, float4 b, float4 c) {
        float4 r;
        r.x = fq_guide_mix(fq_guide_lp(b.x, mb, Lb), fq_guide_lp(c.x, mg, Lg), scale);
        r.y = fq_guide_mix(fq_guide_lp(b.y, mb, Lb), fq_guide_lp(c.y, mg, Lg), scale);
        r.z = fq_guide_mix(fq_guide_lp(b.z, mb, Lb), fq_guide_lp(c.z, mg, Lg), scale);
        r.w = fq_guide_mix(fq_guide_lp(b.w, mb, Lb), fq_guide_lp(c.w, mg, Lg), scale);
        if constexpr (VEC) *(float4 *)(y + 4 * (int64_t) g) = r;
        else {
            const int cnt = gd_count<VEC>(g, n);
            const float rv[4] = { r.x, r.y, r.z, r.w };
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < cnt) y[4 * g + e] = rv[e];
        }
    });
    if (tid == 0) {
        if (max_out) { max_out[0] = mb; max_out[1] = mg; }
        if (sum_out) { sum_out[0] = qb; sum_out[1] = qg; }
    }
}

// pair p = blockIdx.x: leader row lead[p], guide row guide[p] of logits, scale[p] -> mixed + p * mixed_stride; max_out / sum_out
// (optional): [n_pairs][2], {leader, guide}. lead[p] < 0: no pair here, nothing is read or written for it.
__global__ void __launch_bounds__(GD_THREADS) k_guide_mix(const float * __restrict__ logits, int64_t stride, int n, const int32_t * __restrict__ lead,
        const int32_t * __restrict__ guide, const float * __restrict__ scale, float * __restrict__ mixed, int64_t mixed_stride,
        float * __restrict__ max_out, double * __restrict__ sum_out) {
    __shared__ float red[2][GD_THREADS / 64];
    __shared__ double qs[2][GD_THREADS];
    const int p = blockIdx.x;
    const int lb = lead[p];
    if (lb < 0) return;                                     // (the whole workgroup)
    const float * xb = logits + (int64_t) lb * stride, * xg = logits + (int64_t) guide[p] * stride;
    float * y = mixed + (int64_t) p * mixed_stride;
    float * mo = max_out ? max_out + 2 * p : nullptr;
    double * so = sum_out ? sum_out + 2 * p : nullptr;
    const bool vec = n % 4 == 0 && (((uintptr_t) xb | (uintptr_t) xg | (uintptr_t) y) & 15) == 0;      // (block-uniform)
    if (vec) gd_pair<true>(xb, xg, n, scale[p], y, mo, so, red, qs);
    else gd_pair<false>(xb, xg, n, scale[p], y, mo, so, red, qs);
}

void fq_launch_guide(const float * logits, int64_t row_stride, int n_vocab, int n_pairs, const int32_t * lead, const int32_t * guide,
                     const float * scale, float * mixed, int64_t mixed_stride, float * max_out, double * sum_out, hipStream_t st) {
    if (n_pairs < 1) return;
    hipLaunchKernelGGL(k_guide_mix, dim3((unsigned) n_pairs), dim3(GD_THREADS), 0, st, logits, row_stride, n_vocab, lead, guide, scale, mixed, mixed_stride, max_out, sum_out);
}

// ------------------------------------------------------------------------------------------------ C ABI (include/ggml-hip-ops.h)
extern "C" void ggml_hip_guide_rows(const float * logits_dev, int64_t row_stride, int n_vocab, int n_pairs, const int32_t * lead_dev,
                                    const int32_t * guide_dev, const float * scale_dev, float * mixed_dev, int64_t mixed_stride,
                                    float * max_dev, double * sum_dev) {
    if (n_vocab < 1 || n_pairs < 0 || !logits_dev || !lead_dev || !guide_dev || !scale_dev || !mixed_dev || mixed_stride < n_vocab) {
        fprintf(stderr, "ggml-hip: guide_rows(%d pairs, n_vocab %d, mixed_stride %lld): needs n_vocab >= 1, mixed_stride >= n_vocab and its pointers\n", n_pairs, n_vocab, (long long) mixed_stride);
        exit(1);
    }
    fq_launch_guide(logits_dev, row_stride, n_vocab, n_pairs, lead_dev, guide_dev, scale_dev, mixed_dev, mixed_stride, max_dev, sum_dev, fq_ctx().stream);
}
