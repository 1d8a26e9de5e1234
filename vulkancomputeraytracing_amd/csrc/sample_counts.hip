// sample_counts.hip -- vcrt_sample_counts' kernel (include/vcrt.h, the definition;
// csrc/variance.cpp vcrt_sample_counts_host the same on the host), gfx950: the count plane of
// vcrt_draw_samples from a variance plane, element-wise. One statement serves both sides
// (variance_abi.h sample_count_of_variance), every fp32 operation rounded on its own, so the
// counts are the host function's. A code-generation unit of its own (Makefile, part 16).
// Bounds: an element index is below p.elements before either plane is touched.
#include <hip/hip_runtime.h>

#include "variance_abi.h"

#pragma clang fp contract(off)

using namespace vcrt;

// A grid-stride loop; a wave adds its counts to the block's tally slot. No lane returns early:
// the shuffles after the loop see the whole wave.
extern "C" __global__ void __launch_bounds__(vcrt::kSampleCountThreads)
vcrt_sample_counts_pass(SampleCountParams p) {
    const uint32_t stride = gridDim.x * kSampleCountThreads;
    unsigned long long sum = 0ull;
    for (uint32_t e = blockIdx.x * kSampleCountThreads + threadIdx.x; e < p.elements; e += stride) {
        const uint32_t c = sample_count_of_variance(p.variance[e], p.k, p.min_count, p.max_count);
        p.counts[e] = static_cast<uint16_t>(c);
        sum += c;  // (e + stride stays below 2^32: elements <= 2^31, stride <= 2^20)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63u) == 0u && sum)
        atomicAdd(&p.tallies[8u * (blockIdx.x % kSampleCountTallySlots)], sum);
}
