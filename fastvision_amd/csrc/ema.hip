// Exponential moving average of a model's weights (ModelEMA, fastvision_amd/ema.py): the third member beside multi-tensor Adam and
// SGD (optim.hip).  One tick kernel advances the update counter and the weight of this update in device memory, one chunked
// multi-tensor launch moves every tensor of the average towards the model:  e = fmaf(w, p - e, e),  w = 1 - d,
// d = decay * (1 - exp(-k / tau)) (the usual ramp: a young average follows the model).  Non-fp32 tensors (num_batches_tracked, integer
// or bool buffers) are copied byte for byte, so that a checkpoint of the average is consistent with the model it follows.
// HBM-bound: 12 B per fp32 element (read e, read p, write e).  No atomics, nothing read back: the counter lives on the device so that
// a captured training step (graphs.GraphedTrainStep) replays with the right weight.
#include <math.h>

#include "common.h"
#include "multi_tensor.h"

namespace {

constexpr int EMA_THREADS = 256;
constexpr int EMA_COPY = 1;             // kind 1: raw copy; kind 0: fp32 lerp

// state[0] = updates done (a double: exact to 2^53), state[1] = w = 1 - d of the update this launch applies
__global__ void ema_tick_kernel(double* state, double decay, double tau) {
    const double k = state[0] + 1.0;
    state[0] = k;
    const double d = tau > 0.0 ? decay * (1.0 - exp(-k / tau)) : decay;
    state[1] = 1.0 - d;
}

__device__ __forceinline__ f32x4 ema_lerp4(f32x4 e, f32x4 p, float w) {
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = fmaf(w, p[k] - e[k], e[k]);
    return e;
}

// tab: int64 [4][n] = EMA tensor | model tensor | count | kind.  chunks: one word per block (multi_tensor.h); a chunk is MT_CHUNK fp32
// elements of a kind-0 tensor (count in elements) or 4 * MT_CHUNK bytes of a kind-1 tensor (count in bytes).
__global__ __launch_bounds__(EMA_THREADS) void ema_kernel(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks,
                                                          const double* __restrict__ state) {
    const int64_t word = chunks[blockIdx.x];
    const int64_t t = mt_tensor(word), c = mt_number(word);
    const int64_t count = tab[2 * n + t];
    if (tab[3 * n + t] == EMA_COPY) {
        unsigned char* __restrict__ dst = (unsigned char*)tab[t];
        const unsigned char* __restrict__ src = (const unsigned char*)tab[n + t];
        const MtSpan s = mt_span(c, count, 4 * (int64_t)MT_CHUNK);
        const int64_t begin = s.begin, end = s.end;
        int64_t i = begin;
        if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0 && end > begin) {
            const int64_t vend = begin + ((end - begin) & ~(int64_t)15);
            for (int64_t j = begin + 16 * (int64_t)threadIdx.x; j < vend; j += 16 * EMA_THREADS) *(u32x4*)(dst + j) = *(const u32x4*)(src + j);
            i = vend;
        }
        for (int64_t j = i + threadIdx.x; j < end; j += EMA_THREADS) dst[j] = src[j];
        return;
    }
    const float w = (float)state[1];
    float* __restrict__ e = (float*)tab[t];
    const float* __restrict__ p = (const float*)tab[n + t];
    const MtSpan s = mt_span(c, count, MT_CHUNK);
    const int64_t begin = s.begin, end = s.end;
    int64_t i = begin;
    if ((((uintptr_t)e | (uintptr_t)p) & 15) == 0 && end > begin) {
        constexpr int64_t STEP = 4 * EMA_THREADS;
        const int64_t vend = begin + ((end - begin) & ~(int64_t)3);
        int64_t j = begin + 4 * (int64_t)threadIdx.x;
        for (; j + 3 * STEP < vend; j += 4 * STEP) {         // a full chunk: eight 16-byte loads in flight per thread before the first use
            const f32x4 e0 = *(const f32x4*)(e + j), e1 = *(const f32x4*)(e + j + STEP), e2 = *(const f32x4*)(e + j + 2 * STEP),
                        e3 = *(const f32x4*)(e + j + 3 * STEP);
            const f32x4 p0 = *(const f32x4*)(p + j), p1 = *(const f32x4*)(p + j + STEP), p2 = *(const f32x4*)(p + j + 2 * STEP),
                        p3 = *(const f32x4*)(p + j + 3 * STEP);
            *(f32x4*)(e + j) = ema_lerp4(e0, p0, w);
            *(f32x4*)(e + j + STEP) = ema_lerp4(e1, p1, w);
            *(f32x4*)(e + j + 2 * STEP) = ema_lerp4(e2, p2, w);
            *(f32x4*)(e + j + 3 * STEP) = ema_lerp4(e3, p3, w);
        }
        for (; j < vend; j += STEP) *(f32x4*)(e + j) = ema_lerp4(*(const f32x4*)(e + j), *(const f32x4*)(p + j), w);
        i = vend;
    }
    for (int64_t j = i + threadIdx.x; j < end; j += EMA_THREADS) {
        const float ev = e[j];
        e[j] = fmaf(w, p[j] - ev, ev);
    }
}

}  // namespace

extern "C" int fva_ema_chunk_elems(void) { return MT_CHUNK; }

extern "C" int fva_ema_update(const int64_t* tab_dev, int32_t n, const int64_t* chunks_dev, int32_t nchunks, double decay, double tau,
                              double* state_dev, void* stream) {
    if (!tab_dev || n < 1 || !chunks_dev || nchunks < 1 || !state_dev)
        return fva_fail(FVA_ERR_ARG, "fva_ema_update: bad argument (null table / chunk list / state, or nothing to update)");
    if (!(decay >= 0.0 && decay < 1.0)) return fva_fail(FVA_ERR_ARG, "fva_ema_update: decay must be in [0, 1) (got %g)", decay);
    if (!(tau >= 0.0)) return fva_fail(FVA_ERR_ARG, "fva_ema_update: tau must be >= 0 (got %g)", tau);
    hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state_dev, decay, tau);
    FVA_LAUNCH_CHECK("ema_tick_kernel");
    hipLaunchKernelGGL(ema_kernel, dim3(nchunks), dim3(EMA_THREADS), 0, (hipStream_t)stream, tab_dev, n, chunks_dev, (const double*)state_dev);
    FVA_LAUNCH_CHECK("ema_kernel");
    return FVA_OK;
}
