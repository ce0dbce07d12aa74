// Test-only probes of the device RNG in common.hpp: they call the same
// inline functions the Monte-Carlo, GA and RL-env kernels use, so the
// tests can see the raw Philox words, the Box-Muller normals and the
// Box-Muller edges directly instead of through exp2 of sums of them.
// One thread per element, plain global loads and stores, nothing else.

#include <stdexcept>

#include "common.hpp"

namespace {

__global__ void __launch_bounds__(256) philox_probe_kernel(
    const uint64_t* __restrict__ ctr_lo,   // (n,)
    const uint64_t* __restrict__ ctr_hi,   // (n,)
    uint32_t* __restrict__ words,          // (n, 4) philox4x32
    float* __restrict__ normals,           // (n, 4) philox_normal4
    uint64_t seed, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t lo = ctr_lo[i], hi = ctr_hi[i];
    const Philox4 p = philox4x32(seed, lo, hi);
    const float4 z = philox_normal4(seed, lo, hi);
    words[i * 4 + 0] = p.x;
    words[i * 4 + 1] = p.y;
    words[i * 4 + 2] = p.z;
    words[i * 4 + 3] = p.w;
    normals[i * 4 + 0] = z.x;
    normals[i * 4 + 1] = z.y;
    normals[i * 4 + 2] = z.z;
    normals[i * 4 + 3] = z.w;
}

__global__ void __launch_bounds__(256) box_muller_probe_kernel(
    const uint32_t* __restrict__ a,        // (n,) u1 words
    const uint32_t* __restrict__ b,        // (n,) u2 words
    float* __restrict__ out,               // (n, 2) box_muller(a, b)
    long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 z = box_muller(a[i], b[i]);
    out[i * 2 + 0] = z.x;
    out[i * 2 + 1] = z.y;
}

}  // namespace

extern "C" void launch_philox_probe(const uint64_t* ctr_lo,
                                    const uint64_t* ctr_hi, uint32_t* words,
                                    float* normals, uint64_t seed, long n,
                                    hipStream_t stream) {
    if (n <= 0 || n > (1L << 30))
        throw std::runtime_error("philox_probe: n must be in [1, 2^30]");
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(philox_probe_kernel, dim3(blocks), dim3(256), 0,
                       stream, ctr_lo, ctr_hi, words, normals, seed, n);
}

extern "C" void launch_box_muller_probe(const uint32_t* a, const uint32_t* b,
                                        float* out, long n,
                                        hipStream_t stream) {
    if (n <= 0 || n > (1L << 30))
        throw std::runtime_error("box_muller_probe: n must be in [1, 2^30]");
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(box_muller_probe_kernel, dim3(blocks), dim3(256), 0,
                       stream, a, b, out, n);
}
