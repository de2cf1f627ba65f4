// Multi-tensor Adam for gfx950 with torch.optim.Adam's exact update order (single-tensor path of
// torch/optim/adam.py): L2 decay folded into the gradient, lerp for exp_avg, sqrt(v)/sqrt(bc2) + eps.
// HBM-bound: 16 B read + 12 B written per parameter; one launch for all tensors (blockIdx.y = tensor).
//
// Replaces torch.optim.Adam(..., betas=(0.937, 0.999), weight_decay=5e-4).step() as built by the reference
// (demos/yolov3_u/train.py:66-70).
//
// Multi-tensor SGD (torch.optim.SGD, single-tensor path of torch/optim/sgd.py) with the Faster R-CNN demo's global-norm clipping
// (demos/faster_rcnn/cfg/_fit.py:6-17) on the device: grad_sqnorm_partial -> clip_coef -> sgd_kernel.  The work is split into
// fixed-size chunks of MT_CHUNK elements (one block per chunk, host-built chunk table), not into tensors, so one 103 M-element
// tensor (VGG fc6) spreads over every CU instead of over blockIdx.x of one tensor.
#include <math.h>

#include "common.h"
#include "multi_tensor.h"

namespace {

// Device-resident step state (fva_adam_step_dev): the step count and the learning rate live in device memory, so that a
// captured HIP graph of the whole training step replays with the right bias corrections and follows an LR schedule.
// state[0] = step count (as a double: exact to 2^53), state[1] = lr / (1 - beta1^step), state[2] = sqrt(1 - beta2^step)
__global__ void adam_tick_kernel(double* state, const float* __restrict__ lr, double beta1, double beta2) {
    const double step = state[0] + 1.0;
    state[0] = step;
    state[1] = (double)*lr / (1.0 - pow(beta1, step));
    state[2] = sqrt(1.0 - pow(beta2, step));
}

__global__ __launch_bounds__(256) void adam_kernel(const void* const* __restrict__ ptrs, const int64_t* __restrict__ sizes, int n,
                                                   float step_size, float bc2_sqrt, float beta1, float beta2, float eps, float wd,
                                                   float gscale, const double* __restrict__ dev_state) {
    if (dev_state) {
        step_size = (float)dev_state[1];
        bc2_sqrt = (float)dev_state[2];
    }
    const int t = blockIdx.y;
    const int64_t size = sizes[t];
    float* p = (float*)ptrs[t];
    const float* g = (const float*)ptrs[n + t];
    float* m = (float*)ptrs[2 * n + t];
    float* v = (float*)ptrs[3 * n + t];
    if (g == nullptr) return;  // parameter without a gradient this step (torch skips it too)
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < size; i += (int64_t)gridDim.x * blockDim.x) {
        float gr = g[i] * gscale;
        const float pv = p[i];
        if (wd != 0.f) gr = gr + wd * pv;
        float mi = m[i], vi = v[i];
        mi = mi + (gr - mi) * (1.f - beta1);
        vi = vi * beta2 + (1.f - beta2) * gr * gr;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pv - step_size * (mi / denom);
        m[i] = mi;
        v[i] = vi;
    }
}

// dst[offs[t] + i] = (bf16 | f32) src_t[i] for the n tensors of a gradient bucket in ONE launch (blockIdx.y = tensor): the bucket
// copies of parallel.GradientReducer were 222 torch copy launches issued from per-parameter autograd hooks (~8 ms of host time per
// step); a null source pointer or a zero size skips the tensor.
__global__ __launch_bounds__(256) void gather_cast_kernel(const int64_t* __restrict__ table, int n, void* __restrict__ dst, int to_bf16) {
    const int t = blockIdx.y;
    const float* __restrict__ src = (const float*)table[t];
    const int64_t size = table[n + t], off = table[2 * n + t];
    if (src == nullptr || size <= 0) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (((size | off) & 3) == 0 && ((uintptr_t)src & 15) == 0) {
        const f32x4* s4 = (const f32x4*)src;
        if (to_bf16) {
            bf16x4* d4 = (bf16x4*)((bf16_t*)dst + off);
            for (int64_t i = i0; i < size / 4; i += stride) {
                const f32x4 v = s4[i];
                d4[i] = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
            }
        } else {
            f32x4* d4 = (f32x4*)((float*)dst + off);
            for (int64_t i = i0; i < size / 4; i += stride) d4[i] = s4[i];
        }
    } else if (to_bf16) {
        bf16_t* d = (bf16_t*)dst + off;
        for (int64_t i = i0; i < size; i += stride) d[i] = (bf16_t)src[i];
    } else {
        float* d = (float*)dst + off;
        for (int64_t i = i0; i < size; i += stride) d[i] = src[i];
    }
}


// ---- SGD --------------------------------------------------------------------------------------------------------------------
// tab: int64 [6][n] = param | grad | momentum buffer (0: none) | element count | group index | slot in the fresh-flag array.
// chunks: int64 [nchunks], one word per block (multi_tensor.h): chunks of MT_CHUNK elements.
// hyper: float [G][SGD_HYPER] = lr, weight decay, momentum, 1 - dampening, nesterov (0 / 1), one row per parameter group.
// fresh: int32 per slot; non-zero = the momentum buffer has no history yet (torch's `buf = clone(grad)`).
constexpr int SGD_THREADS = 256;
constexpr int SGD_HYPER = 5;

struct SgdChunk {
    int64_t t, begin, end;
};
__device__ __forceinline__ SgdChunk sgd_chunk(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks) {
    const int64_t word = chunks[blockIdx.x];
    SgdChunk c;
    c.t = mt_tensor(word);
    c.begin = mt_number(word) * MT_CHUNK;
    c.end = mt_end(c.begin, tab[3 * n + c.t], MT_CHUNK);
    return c;
}

// fixed-order block sum of one double per thread (wave64 butterfly, then the four waves in order): bit-identical from run to run
__device__ __forceinline__ double block_sum(double v, double* lds) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < SGD_THREADS / 64; ++w) s += lds[w];
    return s;        // valid in thread 0
}

// partial[chunk] = sum of grad^2 over the chunk, accumulated in fp64 (no atomics: one slot per chunk)
__global__ __launch_bounds__(SGD_THREADS) void grad_sqnorm_partial(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks,
                                                                  double* __restrict__ partial) {
    __shared__ double lds[SGD_THREADS / 64];
    const SgdChunk c = sgd_chunk(tab, n, chunks);
    const float* __restrict__ g = (const float*)tab[n + c.t];
    double acc = 0.0;
    int64_t i = c.begin;
    if (((uintptr_t)g & 15) == 0) {
        const int64_t vend = c.begin + ((c.end - c.begin) & ~(int64_t)3);
        for (int64_t j = c.begin + 4 * (int64_t)threadIdx.x; j < vend; j += 4 * SGD_THREADS) {
            const f32x4 v = *(const f32x4*)(g + j);
            acc += (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3];
        }
        i = vend;
    }
    for (int64_t j = i + threadIdx.x; j < c.end; j += SGD_THREADS) acc += (double)g[j] * g[j];
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[0] = norm = sqrt(sum of the partials, in chunk order) as fp32; out[1] = clip / max(norm, clip) as the reference's Python
// computes it (float norm -> double, Python's max keeps its first argument unless the second is larger: max(nan, c) = nan)
__global__ __launch_bounds__(SGD_THREADS) void clip_coef(const double* __restrict__ partial, int nchunks, double clip, float* __restrict__ out) {
    __shared__ double lds[SGD_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += SGD_THREADS) acc += partial[i];
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const double nd = (double)norm;
        const double m = clip > nd ? clip : nd;
        out[0] = norm;
        out[1] = (float)(clip / m);      // inf norm -> 0, nan norm -> nan
    }
}

struct SgdHyper {
    float lr, wd, momentum, keep, nesterov;      // keep = 1 - dampening
};

// torch's update order: g = coef * grad; g += wd * p; buf = g (first step) or momentum * buf + (1 - dampening) * g;
// g = g + momentum * buf (Nesterov) or buf; p -= lr * g
__device__ __forceinline__ void sgd_one(float& p, float gr, float& b, const SgdHyper& h, float coef, bool mom, bool first) {
    float g = coef * gr;
    if (h.wd != 0.f) g = g + h.wd * p;
    if (mom) {
        b = first ? g : h.momentum * b + h.keep * g;
        g = h.nesterov != 0.f ? g + h.momentum * b : b;
    }
    p = p - h.lr * g;
}

__global__ __launch_bounds__(SGD_THREADS) void sgd_kernel(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks,
                                                          const float* __restrict__ hyper, const int32_t* __restrict__ fresh,
                                                          const float* __restrict__ coef_dev) {
    const SgdChunk c = sgd_chunk(tab, n, chunks);
    float* __restrict__ p = (float*)tab[c.t];
    const float* __restrict__ g = (const float*)tab[n + c.t];
    float* __restrict__ b = (float*)tab[2 * n + c.t];
    const float* hp = hyper + tab[4 * n + c.t] * SGD_HYPER;
    const SgdHyper h{hp[0], hp[1], hp[2], hp[3], hp[4]};
    const float coef = coef_dev ? *coef_dev : 1.f;
    const bool mom = b != nullptr;
    const bool first = mom && fresh[tab[5 * n + c.t]] != 0;
    float dummy = 0.f;
    int64_t i = c.begin;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0) {
        const int64_t vend = c.begin + ((c.end - c.begin) & ~(int64_t)3);
        for (int64_t j = c.begin + 4 * (int64_t)threadIdx.x; j < vend; j += 4 * SGD_THREADS) {
            f32x4 pv = *(f32x4*)(p + j);
            const f32x4 gv = *(const f32x4*)(g + j);
            f32x4 bv = mom ? *(f32x4*)(b + j) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pv[k], bk = bv[k];
                sgd_one(pk, gv[k], bk, h, coef, mom, first);
                pv[k] = pk;
                bv[k] = bk;
            }
            *(f32x4*)(p + j) = pv;
            if (mom) *(f32x4*)(b + j) = bv;
        }
        i = vend;
    }
    for (int64_t j = i + threadIdx.x; j < c.end; j += SGD_THREADS) {
        float pk = p[j];
        float& bk = mom ? b[j] : dummy;
        sgd_one(pk, g[j], bk, h, coef, mom, first);
        p[j] = pk;
    }
}

// after an update that initialised buffers: their history starts now
__global__ void sgd_clear_fresh(const int64_t* __restrict__ tab, int n, int32_t* __restrict__ fresh) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) fresh[tab[5 * n + t]] = 0;
}

}  // namespace

extern "C" int fva_gather_cast(const int64_t* table_dev, int32_t n, int64_t max_size, void* dst, int dst_dtype, void* stream) {
    if (!table_dev || n < 1 || !dst || (dst_dtype != FVA_F32 && dst_dtype != FVA_BF16)) return fva_fail(FVA_ERR_ARG, "fva_gather_cast: bad argument");
    int64_t gx = (max_size / 4 + 255) / 256;
    if (gx > 256) gx = 256;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(gather_cast_kernel, dim3((int)gx, n), dim3(256), 0, (hipStream_t)stream, table_dev, n, dst, dst_dtype == FVA_BF16 ? 1 : 0);
    FVA_LAUNCH_CHECK("gather_cast_kernel");
    return FVA_OK;
}

extern "C" int fva_adam_step(const void* const* ptrs, const int64_t* sizes, int32_t n, int64_t max_size, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* stream) {
    if (!ptrs || !sizes || n < 1 || step < 1) return fva_fail(FVA_ERR_ARG, "fva_adam_step: bad argument");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    int64_t gx = (max_size + 1023) / 1024;
    if (gx > 128) gx = 128;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(adam_kernel, dim3((int)gx, n), dim3(256), 0, (hipStream_t)stream, ptrs, sizes, n, step_size, bc2_sqrt, beta1,
                       beta2, eps, weight_decay, grad_scale, (const double*)nullptr);
    FVA_LAUNCH_CHECK("adam_kernel");
    return FVA_OK;
}

extern "C" int fva_adam_step_dev(const void* const* ptrs, const int64_t* sizes, int32_t n, int64_t max_size, const float* lr_dev, float beta1,
                                 float beta2, float eps, float weight_decay, double* state_dev, float grad_scale, void* stream) {
    if (!ptrs || !sizes || n < 1 || !lr_dev || !state_dev) return fva_fail(FVA_ERR_ARG, "fva_adam_step_dev: bad argument");
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state_dev, lr_dev, (double)beta1, (double)beta2);
    FVA_LAUNCH_CHECK("adam_tick_kernel");
    int64_t gx = (max_size + 1023) / 1024;
    if (gx > 128) gx = 128;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(adam_kernel, dim3((int)gx, n), dim3(256), 0, (hipStream_t)stream, ptrs, sizes, n, 0.f, 1.f, beta1, beta2, eps,
                       weight_decay, grad_scale, (const double*)state_dev);
    FVA_LAUNCH_CHECK("adam_kernel");
    return FVA_OK;
}

extern "C" int fva_sgd_chunk_elems(void) { return MT_CHUNK; }

extern "C" int fva_sgd_clip_coef(const int64_t* tab_dev, int32_t n, const int64_t* chunks_dev, int32_t nchunks, double* partial_dev,
                                 double clip_norm, float* out_dev, void* stream) {
    if (!tab_dev || n < 1 || !chunks_dev || nchunks < 1 || !partial_dev || !out_dev)
        return fva_fail(FVA_ERR_ARG, "fva_sgd_clip_coef: bad argument (null table / buffer or empty chunk list)");
    if (!(clip_norm > 0.0) || isinf(clip_norm)) return fva_fail(FVA_ERR_ARG, "fva_sgd_clip_coef: clip_norm must be finite and > 0 (got %g)", clip_norm);
    hipLaunchKernelGGL(grad_sqnorm_partial, dim3(nchunks), dim3(SGD_THREADS), 0, (hipStream_t)stream, tab_dev, n, chunks_dev, partial_dev);
    FVA_LAUNCH_CHECK("grad_sqnorm_partial");
    hipLaunchKernelGGL(clip_coef, dim3(1), dim3(SGD_THREADS), 0, (hipStream_t)stream, (const double*)partial_dev, nchunks, clip_norm, out_dev);
    FVA_LAUNCH_CHECK("clip_coef");
    return FVA_OK;
}

extern "C" int fva_sgd_step(const int64_t* tab_dev, int32_t n, const int64_t* chunks_dev, int32_t nchunks, const float* hyper_dev,
                            int32_t* fresh_dev, int32_t clear_fresh, const float* coef_dev, void* stream) {
    if (!tab_dev || n < 1 || !chunks_dev || nchunks < 1 || !hyper_dev || !fresh_dev)
        return fva_fail(FVA_ERR_ARG, "fva_sgd_step: bad argument (null table / hyper-parameters / fresh flags or empty chunk list)");
    hipLaunchKernelGGL(sgd_kernel, dim3(nchunks), dim3(SGD_THREADS), 0, (hipStream_t)stream, tab_dev, n, chunks_dev, hyper_dev,
                       (const int32_t*)fresh_dev, coef_dev);
    FVA_LAUNCH_CHECK("sgd_kernel");
    if (clear_fresh) {
        hipLaunchKernelGGL(sgd_clear_fresh, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, tab_dev, n, fresh_dev);
        FVA_LAUNCH_CHECK("sgd_clear_fresh");
    }
    return FVA_OK;
}
