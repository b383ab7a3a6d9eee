// kernels_f16.hip -- F16 weight matrices on the device: ggml_compute_forward_mul_mat_f16_f32 (ggml.c:11104-11316) over ggml_vec_dot_f16 (ggml.c:2306-2340, scalar
// branch), ggml_compute_forward_get_rows_f16 (ggml.c:11937-11973) and the fp16 image of the activations (the mat-mul's INIT phase, ggml.c:11176-11196).
//
// The contract (fq_f16.h): every output is ONE f64 chain over its row, element 0 first. It is kept by construction: a lane owns a weight row, and walks it with
// one dependent v_fma_f64 per element and column. What is shared is the memory traffic: a wave stages a tile of 64 rows x 128 weights through LDS, so that HBM sees
// 16-byte loads of 256 consecutive bytes per row, and the tile's activation values are widened to f64 once per wave and read back as LDS broadcasts.
//   weights      row-major fp16 as in the model file, 2 bytes per weight, no re-layout; a row is 2 K bytes (K % 32 == 0: 16-byte aligned)
//   LDS tile     rows 68 dwords apart (4 x 17: a lane's 16-byte reads of its own row spread over all banks)
//   columns      NC = 1 (decode), 2 / 4 (lock-step passes), 8 (token tiles of a prompt; column groups are the fast grid dimension, so the groups of one row tile run
//                together and re-read it out of the cache) -- all of them instances of ONE kernel body around fq_f16_chain_step: a token's bits do not depend on N
#include "fq_device.h"
#include "fq_f16.h"
#include "kernels.h"

#define F16_TM      64                      // rows per workgroup (one wave: lane = row)
#define F16_KC      128                     // weights per row and tile
#define F16_WSTRIDE (F16_KC / 2 + 4)        // dwords between LDS rows: 68 = 4 x 17
#define F16_NLOAD   (F16_TM * F16_KC * 2 / 16 / 64)      // 16-byte loads per lane and tile: 16

bool fq_f16_row_ok(int64_t K) { return K > 0 && K % FQ_F16_K_MULTIPLE == 0 && K < ((int64_t) 1 << 31); }

fq_weight fq_f16_weight_view(uint8_t * slab, int64_t K, int64_t M) {
    fq_weight w{};
    w.type = FQ_F16; w.K = K; w.M = M; w.nblk = K;
    w.bytes = (size_t) M * (size_t) K * 2;
    w.row_stride = (size_t) K * 2;
    for (int p = 0; p < FQ_MAX_PLANES; ++p) w.plane[p] = slab;
    return w;
}

// ------------------------------------------------------------------------------------------------ activation image: f32 -> fp16 (round to nearest even)
__global__ void __launch_bounds__(256) k_f16_image(const float * __restrict__ x, int64_t ldx, int64_t K, int64_t ncols, uint16_t * __restrict__ out, int64_t ldo) {
    const int64_t total = K * ncols;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        const int64_t c = i / K, k = i - c * K;
        out[c * ldo + k] = fq_f32_to_f16_bits(x[c * ldx + k]);
    }
}
void fq_launch_f16_image(const float * x, int64_t ldx, const fq_act & a, hipStream_t st) {
    FQ_TL(st, "f16_image");
    const int64_t total = a.K * a.ncols;
    if (total <= 0) return;
    const int blocks = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(k_f16_image, dim3(blocks), dim3(256), 0, st, x, ldx, a.K, a.ncols, (uint16_t *) a.base, (int64_t)(fq_f16_col_bytes(a.K) / 2));
}

// ------------------------------------------------------------------------------------------------ get_rows: an exact widening
__global__ void __launch_bounds__(256) k_f16_get_rows(const uint8_t * __restrict__ W, size_t row_stride, int64_t K, int64_t M, const int32_t * __restrict__ rows,
                                                      int64_t nrows, float * __restrict__ dst) {
    const int64_t total = nrows * K;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        const int64_t r = i / K, k = i - r * K;
        int64_t src = rows ? (int64_t) rows[r] : r;
        src = src < 0 ? 0 : (src >= M ? M - 1 : src);                       // (callers check their ids; a bad one must not leave the matrix)
        dst[i] = fq_f16_bits_to_f32(((const uint16_t *)(W + (size_t) src * row_stride))[k]);
    }
}
void fq_launch_f16_get_rows(const fq_weight & w, const int32_t * rows_dev, int64_t nrows, float * dst, hipStream_t st) {
    FQ_TL(st, "f16_get_rows");
    const int64_t total = nrows * w.K;
    if (total <= 0) return;
    const int blocks = (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
    hipLaunchKernelGGL(k_f16_get_rows, dim3(blocks), dim3(256), 0, st, (const uint8_t *) w.plane[0], w.row_stride, w.K, w.M, rows_dev, nrows, dst);
}

// ------------------------------------------------------------------------------------------------ mat-mul
// eight consecutive elements of one row against NC columns: the only place a sum advances
template <int NC>
__device__ __forceinline__ void f16_chain8(const uint4 q, const double * __restrict__ xt, double (&sum)[NC]) {
    const unsigned u[4] = { q.x, q.y, q.z, q.w };
    double w[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { w[2 * e] = fq_f16_bits_to_f64((uint16_t)(u[e] & 0xFFFFu)); w[2 * e + 1] = fq_f16_bits_to_f64((uint16_t)(u[e] >> 16)); }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int c = 0; c < NC; ++c) sum[c] = fq_f16_chain_step(sum[c], w[e], xt[c * F16_KC + e]);
    }
}

// grid (column groups of NC, row tiles of 64), one wave per workgroup. X: the fp16 image, column n at X + n * ldx (fp16 values).
template <int NC>
__global__ void __launch_bounds__(64) k_mul_mat_f16(const uint8_t * __restrict__ W, size_t row_stride, int K, int64_t M, const uint16_t * __restrict__ X, int64_t ldx,
                                                    int64_t N, float * __restrict__ dst, int64_t ldd, fq_gemv_epi ep) {
    __shared__ __attribute__((aligned(16))) unsigned wt[F16_TM * F16_WSTRIDE];
    __shared__ __attribute__((aligned(16))) double   xt[NC * F16_KC];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t) blockIdx.y * F16_TM, col0 = (int64_t) blockIdx.x * NC;
    const int seg = lane & 15, rsub = lane >> 4;                // staging: 16 lanes x 16 bytes = the 256 bytes of one row, 4 rows per load

    const uint8_t * wrow[F16_NLOAD];
#pragma unroll
    for (int i = 0; i < F16_NLOAD; ++i) {
        int64_t r = row0 + i * 4 + rsub;
        r = r < M ? r : M - 1;                                  // rows past the matrix re-read its last row (never stored)
        wrow[i] = W + (size_t) r * row_stride + (size_t) seg * 16;
    }
    const uint16_t * xcol[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { int64_t n = col0 + c; n = n < N ? n : N - 1; xcol[c] = X + n * ldx + 2 * lane; }

    uint4 wreg[F16_NLOAD]; unsigned xreg[NC];
    auto fetch = [&](int k0) {
        const bool wv = k0 + seg * 8 < K, xv = k0 + 2 * lane < K;      // (K % 32 == 0: a 16-byte piece / a pair is inside the row or wholly outside)
#pragma unroll
        for (int i = 0; i < F16_NLOAD; ++i) wreg[i] = wv ? *(const uint4 *)(wrow[i] + (size_t) k0 * 2) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int c = 0; c < NC; ++c) xreg[c] = xv ? *(const unsigned *)(xcol[c] + k0) : 0u;
    };

    double sum[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) sum[c] = 0.0;

    fetch(0);
    for (int k0 = 0; k0 < K; k0 += F16_KC) {
        __syncthreads();                                        // the previous tile has been read
#pragma unroll
        for (int i = 0; i < F16_NLOAD; ++i) *(uint4 *)(wt + (i * 4 + rsub) * F16_WSTRIDE + seg * 4) = wreg[i];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double2 d;
            d.x = fq_f16_bits_to_f64((uint16_t)(xreg[c] & 0xFFFFu)); d.y = fq_f16_bits_to_f64((uint16_t)(xreg[c] >> 16));
            *(double2 *)(xt + c * F16_KC + 2 * lane) = d;
        }
        __syncthreads();
        if (k0 + F16_KC < K) fetch(k0 + F16_KC);                 // the next tile's loads fly while this one is summed
        const int kn = K - k0 < F16_KC ? K - k0 : F16_KC;       // a multiple of 32
        const unsigned * mine = wt + lane * F16_WSTRIDE;
        for (int kk = 0; kk < kn; kk += 8) f16_chain8<NC>(*(const uint4 *)(mine + (kk >> 1)), xt + kk, sum);
    }

    const int64_t row = row0 + lane;
    if (row >= M) return;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int64_t col = col0 + c;
        if (col >= N) break;
        float v = (float) sum[c];
        if (ep.mode == FQ_EPI_GELU) {
            v = h2f_bits(ep.gelu_table[f2h_bits(v)]);                                          // ggml.c:3477-3484
        } else if (ep.mode == FQ_EPI_ADD2) {
            v = (v + ep.add1[col * ep.ld_add + row]) + ep.add2[col * ep.ld_add + row];         // libfalcon.cpp:2399-2400
        }
        dst[col * ldd + row] = v;
    }
}

template <int NC>
static void launch_f16(const fq_weight & w, const uint16_t * X, int64_t ldx, int64_t N, float * dst, int64_t ldd, const fq_gemv_epi & ep, hipStream_t st) {
    const dim3 grid((unsigned)((N + NC - 1) / NC), (unsigned)((w.M + F16_TM - 1) / F16_TM));
    hipLaunchKernelGGL((k_mul_mat_f16<NC>), grid, dim3(64), 0, st, (const uint8_t *) w.plane[0], w.row_stride, (int) w.K, w.M, X, ldx, N, dst, ldd, ep);
}

void fq_launch_mul_mat_f16(const fq_weight & w, const fq_act & act, int64_t N, float * dst, int64_t ldd, const fq_gemv_epi & ep0, hipStream_t st) {
    FQ_TL(st, "mul_mat_f16");
    if (w.type != FQ_F16 || act.type != FQ_F16 || act.K != w.K || !fq_f16_row_ok(w.K)) {
        fprintf(stderr, "ggml-hip: F16 mat-mul: weight type %d (K %lld) with an activation image of type %d (K %lld): needs F16 both, K a multiple of %d\n",
                w.type, (long long) w.K, act.type, (long long) act.K, FQ_F16_K_MULTIPLE);
        exit(1);
    }
    if (N <= 0 || w.M <= 0) return;
    if ((w.M + F16_TM - 1) / F16_TM > 65535) { fprintf(stderr, "ggml-hip: F16 mat-mul: %lld rows exceed the launch grid\n", (long long) w.M); exit(1); }
    const uint16_t * X = (const uint16_t *) act.base;
    const int64_t ldx = (int64_t)(fq_f16_col_bytes(w.K) / 2);
    // whole groups of 8 columns, then the rest in the narrowest form that holds it
    const int64_t n8 = N >= 8 ? (N / 8) * 8 : 0, rest = N - n8;
    if (n8) launch_f16<8>(w, X, ldx, n8, dst, ldd, ep0, st);
    if (rest) {
        fq_gemv_epi ep = ep0;
        if (ep.add1) ep.add1 += n8 * ep.ld_add;
        if (ep.add2) ep.add2 += n8 * ep.ld_add;
        const uint16_t * Xr = X + n8 * ldx; float * dr = dst + n8 * ldd;
        if (rest == 1)      launch_f16<1>(w, Xr, ldx, rest, dr, ldd, ep, st);
        else if (rest == 2) launch_f16<2>(w, Xr, ldx, rest, dr, ldd, ep, st);
        else if (rest <= 4) launch_f16<4>(w, Xr, ldx, rest, dr, ldd, ep, st);
        else                launch_f16<8>(w, Xr, ldx, rest, dr, ldd, ep, st);
    }
}
