// The device build of csrc/pmath.h as a shared library for tests/test_gpu_pmath.py (ctypes, in a child interpreter).  Built twice with
// the product's flags (_buildid.FLAGS): as is (tables in the constant address space) and with -DPM_TABLES_IN_LDS, where every kernel
// first copies the tables to LDS and passes a workgroup barrier, as the product kernels do (kernels.hip).  Function ids are
// oracle_math's (oracle/oracle.cpp): 0 log, 1 exp, 2 sin, 3 cos, 4 cbrt, 5 pow, 6..11 the _cr routines, 12 sqrt, 13 rcp, 14 rsqrt,
// 15 div_by_invariant (y: the divisor, rd = pm_invariant_rcp(y)).  Plain C++ / HIP: no inline assembly.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../eradiate-kernel_amd/csrc/pmath.h"

namespace {

__device__ __forceinline__ void tables_ready() {
    pm_tables_to_lds(threadIdx.x);
    __syncthreads();
}

__device__ __forceinline__ float eval(int fn, float x, float y) {
    float s, c;
    switch (fn) {
        case 0: return pm_log(x);
        case 1: return pm_exp(x);
        case 2: pm_sincos(x, &s, &c); return s;
        case 3: pm_sincos(x, &s, &c); return c;
        case 4: return pm_cbrt(x);
        case 5: return pm_pow(x, y);
        case 6: return pm_log_cr(x);
        case 7: return pm_exp_cr(x);
        case 8: pm_sincos_cr(x, &s, &c); return s;
        case 9: pm_sincos_cr(x, &s, &c); return c;
        case 10: return pm_cbrt_cr(x);
        case 11: return pm_pow_cr(x, y);
        case 12: return pm_sqrt(x);
        case 13: return pm_rcp(x);
        case 14: return pm_rsqrt(x);
        case 15: return pm_div_by_invariant(x, y, pm_invariant_rcp(y));
    }
    return 0.f;
}

// out[i] = f(bits first + i, y), i < n
__global__ void k_sweep(int fn, uint32_t first, int64_t n, float y, float *out) {
    tables_ready();
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
        out[i] = eval(fn, pm_from_bits(first + (uint32_t) i), y);
}

__global__ void k_pairs(int fn, int64_t n, const float *x, const float *y, float *out) {
    tables_ready();
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
        out[i] = eval(fn, x[i], y[i]);
}

// pm_div_by_invariant(x, d, rd) against the device's own x / d for the dividends first .. first + n - 1 (both signs of each)
__global__ void k_div_sweep(uint32_t first, int64_t n, float d, float rd, unsigned long long *count) {
    unsigned long long bad = 0;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const float x = pm_from_bits(first + (uint32_t) i);
        const uint32_t a = pm_bits(pm_div_by_invariant(x, d, rd)), b = pm_bits(x / d);
        bad += a != b && !((a & 0x7fffffffu) > 0x7f800000u && (b & 0x7fffffffu) > 0x7f800000u);
    }
    if (bad) atomicAdd(count, bad);
}

__global__ void k_fp32_op(int op, int64_t n, const float *a, const float *b, const float *c, float *out) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const float x = a[i], y = b[i], z = c[i];
        float r = 0.f;
        switch (op) {
            case 0: r = x * y; break;
            case 1: r = x + y; break;
            case 2: r = __builtin_fmaf(x, y, z); break;
            case 3: r = x / y; break;
            case 4: r = __builtin_sqrtf(x); break;
            case 5: r = (float) ((double) x * (double) y); break;
            case 6: r = x < y ? 1.f : 0.f; break;
            case 7: r = x == y ? 1.f : 0.f; break;
        }
        out[i] = r;
    }
}

// Bitwise comparison of two device buffers (two NaNs are equal): the number of differing elements.
__global__ void k_compare(int64_t n, const float *a, const float *b, unsigned long long *count) {
    unsigned long long bad = 0;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const uint32_t u = pm_bits(a[i]), v = pm_bits(b[i]);
        bad += u != v && !((u & 0x7fffffffu) > 0x7f800000u && (v & 0x7fffffffu) > 0x7f800000u);
    }
    if (bad) atomicAdd(count, bad);
}

constexpr int BLOCK = 256;
int grid_for(int64_t n) { const int64_t g = (n + BLOCK - 1) / BLOCK; return (int) (g < 16384 ? (g < 1 ? 1 : g) : 16384); }
int done() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? 0 : 1; }

} // namespace

extern "C" {

int pmd_malloc(void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? 0 : 1; }
int pmd_host_malloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess ? 0 : 1; }
int pmd_free(void *p) { return hipFree(p) == hipSuccess ? 0 : 1; }
int pmd_host_free(void *p) { return hipHostFree(p) == hipSuccess ? 0 : 1; }
int pmd_to_device(void *d, const void *h, size_t bytes) { return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : 1; }
int pmd_to_host(void *h, const void *d, size_t bytes) { return hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1; }

int pmd_sweep(int fn, uint32_t first, int64_t n, float y, float *out) {
    hipLaunchKernelGGL(k_sweep, dim3(grid_for(n)), dim3(BLOCK), 0, 0, fn, first, n, y, out);
    return done();
}
int pmd_pairs(int fn, int64_t n, const float *x, const float *y, float *out) {
    hipLaunchKernelGGL(k_pairs, dim3(grid_for(n)), dim3(BLOCK), 0, 0, fn, n, x, y, out);
    return done();
}
int pmd_fp32_op(int op, int64_t n, const float *a, const float *b, const float *c, float *out) {
    hipLaunchKernelGGL(k_fp32_op, dim3(grid_for(n)), dim3(BLOCK), 0, 0, op, n, a, b, c, out);
    return done();
}
// *count: differing elements (device scratch word in `scratch`)
int pmd_compare(int64_t n, const float *a, const float *b, unsigned long long *scratch, unsigned long long *count) {
    if (hipMemset(scratch, 0, 8) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_compare, dim3(grid_for(n)), dim3(BLOCK), 0, 0, n, a, b, scratch);
    if (done()) return 1;
    return hipMemcpy(count, scratch, 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
int pmd_div_sweep(uint32_t first, int64_t n, float d, float rd, unsigned long long *scratch, unsigned long long *count) {
    if (hipMemset(scratch, 0, 8) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_div_sweep, dim3(grid_for(n)), dim3(BLOCK), 0, 0, first, n, d, rd, scratch);
    if (done()) return 1;
    return hipMemcpy(count, scratch, 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}

} // extern "C"
