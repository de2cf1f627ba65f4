// What the two matrix-unit grouped 3x3 files share (grouped_mfma.hip: stride 1, grouped_mfma_s2.hip: stride 2): the staging pitch, the
// K-step count of a table, the transposing LDS read of the weight gradients, the dispatch over Cg, and the fixed-order reduce of the
// weight gradients' split partials with its launch.  Everything is file-local in the including file.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

constexpr int CH = 64;         // channels per block
constexpr int PITCH = 160;     // bytes per staged position (128 of data)
constexpr int LDS_MAX = 64 * 1024;

constexpr int steps_of(int cg) { return cg >= 32 ? 9 * (cg / 32) : 5; }

using lds_s16x4 = __attribute__((address_space(3))) s16x4;
using s16x8 = __attribute__((ext_vector_type(8))) short;

__device__ __forceinline__ bf16x8 tr_pair(const char* lo, const char* hi) {
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo);
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi);
    return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// The splits are many and the elements few at the wide maps (1682 splits of 4608 elements at C = 128, Cg = 4, 56^2): one thread per element
// walking all its splits is a chain of that many dependent-latency loads on a handful of blocks.  So 16 threads share an element: each adds
// a contiguous sixteenth of the splits in their order, and the sixteen sums are added in their order -- still one fixed order.
constexpr int RED_E = 16, RED_S = 16;      // elements per block x slices of the splits
__global__ __launch_bounds__(RED_E * RED_S) void gconv_mfma_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int n,
                                                                                int splits) {
    __shared__ double part[RED_S][RED_E];
    const int e = threadIdx.x % RED_E, sl = threadIdx.x / RED_E;
    const int i = blockIdx.x * RED_E + e;
    const int per = (splits + RED_S - 1) / RED_S;
    const int j0 = sl * per, j1 = min(splits, j0 + per);
    double s = 0.0;
    if (i < n)
        for (int j = j0; j < j1; ++j) s += (double)partial[(int64_t)j * n + i];
    part[sl][e] = s;
    __syncthreads();
    if (sl == 0 && i < n) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < RED_S; ++k) t += part[k][e];
        dw[i] = (float)t;
    }
}

// partial [splits][n] -> dw [n]
int launch_wgrad_reduce(const void* ws, float* dw, int n, int splits, void* stream) {
    hipLaunchKernelGGL(gconv_mfma_wgrad_reduce_kernel, dim3(cdiv(n, RED_E)), dim3(RED_E * RED_S), 0, (hipStream_t)stream, (const float*)ws, dw, n, splits);
    FVA_LAUNCH_CHECK("gconv_mfma_wgrad_reduce_kernel");
    return FVA_OK;
}

template <typename F>
void by_cg(int cg, F&& f) {
    switch (cg) {
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 32: f(std::integral_constant<int, 32>{}); break;
        default: f(std::integral_constant<int, 64>{}); break;
    }
}

// blocks of the split axis of a weight gradient over `nruns` staged runs: a few blocks per CU in flight, at most 64 MB of fp32 partials
struct WPlan {
    int nruns, splits, runs_per_split;
};
inline WPlan wgrad_plan_of(int nruns, int C, int cg) {
    WPlan p;
    p.nruns = nruns;
    const int64_t one = (int64_t)C * cg * 9 * 4;
    int64_t want = 4096 / (C / CH);
    const int64_t cap = (64ll << 20) / one > 0 ? (64ll << 20) / one : 1;
    if (want > cap) want = cap;
    if (want > p.nruns) want = p.nruns;
    if (want < 1) want = 1;
    p.runs_per_split = cdiv(p.nruns, want);
    p.splits = cdiv(p.nruns, p.runs_per_split);
    return p;
}

}  // namespace
