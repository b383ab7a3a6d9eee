// micro-benchmark: what one element of the F16 mat-mul's strict chain costs (csrc/kernels_f16.hip: one dependent v_fma_f64 per element and column).
//   mode 0  a chain of dependent v_fma_f64 alone                              -> the latency of the instruction
//   mode 1  the chain fed as the kernel feeds it at N = 1: per element two conversions (fp16 -> f32 -> f64) of a weight and one fma
//   mode 2  the same with 4 columns (4 independent chains share a weight's conversions)
//   mode 3  the same with 8 columns
// for 1, 2 and 4 waves per SIMD, in wall-clock ns and shader-clock ticks per ELEMENT (s_memrealtime at 100 MHz / s_memtime).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off scripts/microbench/mb_f64_chain.hip -o scripts/microbench/mb_f64_chain
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <stdint.h>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

template <int NC>
__device__ __forceinline__ void step8(unsigned q0, unsigned q1, unsigned q2, unsigned q3, const double * xs, double (&sum)[NC]) {
    const unsigned u[4] = { q0, q1, q2, q3 };
    double w[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        w[2 * e]     = (double) __builtin_bit_cast(_Float16, (uint16_t)(u[e] & 0xFFFFu));
        w[2 * e + 1] = (double) __builtin_bit_cast(_Float16, (uint16_t)(u[e] >> 16));
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int c = 0; c < NC; ++c) sum[c] = __builtin_fma(w[e], xs[c * 8 + e], sum[c]);
}

template <int MODE>
__global__ void __launch_bounds__(1024) k(double * out, long long * t, int n, const unsigned * wsrc) {
    __shared__ double xs[64];
    __shared__ unsigned ws[1024 * 4];
    if (threadIdx.x < 64) xs[threadIdx.x] = 1.0 + threadIdx.x * 0.001;
    for (int i = 0; i < 4; ++i) ws[threadIdx.x * 4 + i] = wsrc[(threadIdx.x * 4 + i) & 255];
    __syncthreads();
    double x = threadIdx.x * 1e-3, y = 1.0000001;
    constexpr int NC = MODE == 1 ? 1 : (MODE == 2 ? 4 : 8);
    double sum[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) sum[c] = 0.0;
    const long long t0 = wall_clock64();
    const long long c0 = clock64();
    for (int i = 0; i < n; ++i) {
        if (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) x = __builtin_fma(x, y, 0.5);
        } else {
            const uint4 q = *(const uint4 *)(ws + ((threadIdx.x * 4 + 4 * i) & 4095 & ~3));      // the lane's own 16 bytes out of LDS, as in the kernel
            step8<NC>(q.x, q.y, q.z, q.w, xs, sum);
        }
    }
    const long long c1 = clock64();
    const long long t1 = wall_clock64();
    if (threadIdx.x == 0) { t[blockIdx.x * 2] = t1 - t0; t[blockIdx.x * 2 + 1] = c1 - c0; }
    double r = x;
#pragma unroll
    for (int c = 0; c < NC; ++c) r += sum[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

int main() {
    double * out; long long * t; unsigned * w;
    CK(hipMalloc(&out, 64 * 1024 * 8)); CK(hipMalloc(&t, 64 * 16)); CK(hipMalloc(&w, 1024));
    unsigned hw[256];
    for (int i = 0; i < 256; ++i) hw[i] = 0x2C002400u + (unsigned) i * 0x00010001u;      // small normal fp16 pairs
    CK(hipMemcpy(w, hw, sizeof hw, hipMemcpyHostToDevice));
    long long h[128];
    const int n = 4000;
    const char * names[4] = { "dependent v_fma_f64 alone", "N = 1: 2 cvt + 1 fma per element", "N = 4: 2 cvt + 4 fma per element", "N = 8: 2 cvt + 8 fma per element" };
    for (int waves = 1; waves <= 4; waves *= 2) {
        const int threads = 256 * waves;
        printf("--- %d wave(s) per SIMD (%d threads per workgroup, 32 workgroups)\n", waves, threads);
#define RUN(M) { hipLaunchKernelGGL((k<M>), dim3(32), dim3(threads), 0, 0, out, t, n, w); hipLaunchKernelGGL((k<M>), dim3(32), dim3(threads), 0, 0, out, t, n, w); CK(hipDeviceSynchronize()); \
        CK(hipMemcpy(h, t, 64 * 8, hipMemcpyDeviceToHost)); \
        printf("%-36s %7.3f ns / element / wave   %6.2f shader-clock ticks per element (ticks per us %.0f)\n", names[M], h[0] * 10.0 / (n * 8.0), (double) h[1] / (n * 8.0), h[1] / (h[0] * 0.01)); }
        RUN(0) RUN(1) RUN(2) RUN(3)
    }
    return 0;
}
