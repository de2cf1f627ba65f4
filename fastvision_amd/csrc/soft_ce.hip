// Softmax cross-entropy against SOFT targets (label smoothing, a MixUp / CutMix pair of labels, dense probability rows) and top-k
// accuracy for gfx950.  fva_softmax_ce_soft keeps the structure of fva_softmax_ce (classify.hip): one 256-thread block per row, an
// online (max, sum-exp) pass with fixed-order merges, a second pass over the row for the gradient, the row losses summed in double in a
// fixed order by a one-block finish -- latency-bound like it (R x C fp32 = 512 KB at 128 x 1000), no atomics, run-to-run bit-identical.
// What is new: the pass also carries the row's sum of logits (the smoothing term needs sum_k z_k), the target of a row is
//   q = (1 - eps) * t + eps / C,   t = onehot(y_r) | lam * onehot(y_r) + (1 - lam) * onehot(y_(r-1)) | dense[r][:]
// with lam read from the mix plan ON THE DEVICE, and
//   loss_r = w_r * (sum(q) * log(s) - sum_k q_k (z_k - m)),    grad = scale * w_r * (softmax * sum(q) - q)
// sum(q) is 1 for the two label forms (set, not summed).  With eps = 0 and plain labels every operation reduces to fva_softmax_ce's
// (1 * x, x + 0, fma(p, 1, -q)), so value and gradient have its bits; tests/test_gpu_soft_ce.py compares them.
#include <math.h>

#include "common.h"

namespace {

constexpr int SCE_THREADS = 256;
constexpr int SCE_WAVES = SCE_THREADS / 64;

// (m, s) = running max and sum of exp(z - m), merged as in classify.hip: an empty partial (s == 0, m == -inf) must not form exp(-inf - -inf)
struct MaxSum {
    float m, s;
};
__device__ __forceinline__ MaxSum ms_merge(MaxSum a, MaxSum b) {
    if (a.s == 0.f) return b;
    if (b.s == 0.f) return a;
    const float m = fmaxf(a.m, b.m);
    return MaxSum{m, a.s * expf(a.m - m) + b.s * expf(b.m - m)};
}

// Label of row r as an index in [0, C), or -1 when it is out of range or (float labels) not an integer.
__device__ __forceinline__ int row_label(const void* labels, int label_dtype, int r, int C) {
    if (label_dtype == FVA_LABEL_I64) {
        const int64_t v = ((const int64_t*)labels)[r];
        return (v >= 0 && v < C) ? (int)v : -1;
    }
    const float v = ((const float*)labels)[r];
    return (v >= 0.f && v < (float)C && floorf(v) == v) ? (int)v : -1;      // NaN fails every comparison
}

// sum over the block in a fixed order (wave butterflies, then the waves in order); every thread gets the total.  red: [SCE_WAVES]
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                  // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
    for (int w = 1; w < SCE_WAVES; ++w) t += red[w];
    return t;
}

__global__ __launch_bounds__(SCE_THREADS) void soft_ce_kernel(const float* __restrict__ logits, const void* __restrict__ labels, int label_dtype,
                                                              const float* __restrict__ dense, const float* __restrict__ weights, int R, int C,
                                                              float scale, float eps, const fva_mix_plan_t* __restrict__ plan,
                                                              float* __restrict__ row_loss, float* __restrict__ grad) {
    __shared__ MaxSum red[SCE_WAVES];
    __shared__ float fred[SCE_WAVES];
    const int r = blockIdx.x;
    const float* z = logits + (int64_t)r * C;
    MaxSum a{-INFINITY, 0.f};
    float sz = 0.f;
    for (int k = threadIdx.x; k < C; k += SCE_THREADS) {
        const float v = z[k];
        sz += v;
        if (a.s == 0.f) {
            a = MaxSum{v, 1.f};
        } else if (v > a.m) {
            a = MaxSum{v, a.s * expf(a.m - v) + 1.f};
        } else {
            a.s += expf(v - a.m);      // a NaN logit makes s NaN, as in torch
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        MaxSum b{__shfl_xor(a.m, o), __shfl_xor(a.s, o)};
        a = (threadIdx.x & o) ? ms_merge(b, a) : ms_merge(a, b);     // the same operand order on both lanes of a pair
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    a = red[0];
    for (int w = 1; w < SCE_WAVES; ++w) a = ms_merge(a, red[w]);
    const float w = weights ? weights[r] : 1.f;
    const float ls = logf(a.s);

    // T = sum_k t_k (z_k - m) and sum(t); the label forms index z with checked labels only
    float T, St = 1.f, lam = 1.f;
    int y0 = -1, y1 = -1;
    bool bad = false;
    if (dense != nullptr) {
        const float* d = dense + (int64_t)r * C;
        float pt = 0.f, ps = 0.f;
        for (int k = threadIdx.x; k < C; k += SCE_THREADS) {
            const float dk = d[k];
            pt = __builtin_fmaf(dk, z[k] - a.m, pt);
            ps += dk;
        }
        T = block_sum(pt, fred);
        St = block_sum(ps, fred);
    } else {
        y0 = row_label(labels, label_dtype, r, C);
        bad = y0 < 0;
        if (plan != nullptr) {
            lam = plan->lam;
            y1 = row_label(labels, label_dtype, r == 0 ? R - 1 : r - 1, C);
            bad = bad || y1 < 0;
            T = bad ? NAN : __builtin_fmaf(lam, z[y0] - a.m, (1.f - lam) * (z[y1] - a.m));
        } else {
            T = bad ? NAN : z[y0] - a.m;
        }
    }
    const float Sq = dense != nullptr ? __builtin_fmaf(1.f - eps, St, eps) : 1.f;
    const float ec = eps / (float)C;
    if (eps != 0.f) {
        sz = block_sum(sz, fred);
        T = __builtin_fmaf(ec, sz - (float)C * a.m, (1.f - eps) * T);              // sum_k (z_k - m) = sum z - C m
    }
    if (threadIdx.x == 0) row_loss[r] = bad ? NAN : __builtin_fmaf(Sq, ls, -T) * w;
    if (grad == nullptr) return;
    float* gr = grad + (int64_t)r * C;
    const float gs = bad ? NAN : scale * w, inv = 1.f / a.s;
    const float ome = 1.f - eps, oml = 1.f - lam;
    const float* d = dense != nullptr ? dense + (int64_t)r * C : nullptr;
    for (int k = threadIdx.x; k < C; k += SCE_THREADS) {
        const float p = expf(z[k] - a.m) * inv;
        float t;
        if (d != nullptr) t = d[k];
        else if (plan != nullptr) t = (k == y0 ? lam : 0.f) + (k == y1 ? oml : 0.f);
        else t = k == y0 ? 1.f : 0.f;
        const float q = __builtin_fmaf(ome, t, ec);
        gr[k] = gs * __builtin_fmaf(p, Sq, -q);
    }
}

// out[0] = (sum of part[0 .. n)) / denom, summed in double in a fixed order (one block)
__global__ __launch_bounds__(SCE_THREADS) void soft_ce_final_kernel(const float* __restrict__ part, int n, double denom, float* __restrict__ out) {
    __shared__ double red[SCE_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += SCE_THREADS) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0.0;
        for (int i = 0; i < SCE_THREADS; ++i) s += red[i];
        out[0] = (float)(s / denom);
    }
}

// ---- top-k accuracy -----------------------------------------------------------------------------------------------------------
// torch.argmax order (fva_top1_accuracy): a NaN beats every number, among equals (or NaNs) the smaller index wins.
__device__ __forceinline__ bool arg_better(float v, int i, float bv, int bi) {
    const bool vn = isnan(v), bn = isnan(bv);
    if (vn != bn) return vn;
    if (vn || v == bv) return i < bi;
    return v > bv;
}

// One wave per row (4 rows per block): hit[r] = 1 if fewer than k entries of the row beat the label's.
template <typename T>
__global__ __launch_bounds__(SCE_THREADS) void topk_kernel(const T* __restrict__ logits, const void* __restrict__ labels, int label_dtype, int R,
                                                           int C, int topk, int* __restrict__ hit) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * SCE_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;                       // whole waves leave together: the shuffles below stay within live waves
    const int y = row_label(labels, label_dtype, r, C);       // the same value in every lane
    if (y < 0) {
        if (lane == 0) hit[r] = 0;
        return;
    }
    const T* z = logits + (int64_t)r * C;
    const float zy = to_f(z[y]);
    int cnt = 0;
    for (int k = lane; k < C; k += 64) cnt += (k != y && arg_better(to_f(z[k]), k, zy, y)) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) hit[r] = cnt < topk;
}

// out[0] = (float)(sum of hit) / (float)R  (integer sum: exact and order-free)
__global__ __launch_bounds__(SCE_THREADS) void topk_final_kernel(const int* __restrict__ hit, int R, float* __restrict__ out) {
    __shared__ int red[SCE_THREADS];
    int s = 0;
    for (int i = threadIdx.x; i < R; i += SCE_THREADS) s += hit[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0;
        for (int i = 0; i < SCE_THREADS; ++i) s += red[i];
        out[0] = (float)s / (float)R;
    }
}

}  // namespace

extern "C" {

int fva_softmax_ce_soft(const float* logits, const void* labels, int label_dtype, const float* dense, const float* weights, int32_t R,
                        int32_t C, int32_t reduction, float smoothing, const fva_mix_plan_t* plan, float* loss_out, float* grad,
                        void* workspace, void* stream) {
    if (!logits || !loss_out || !workspace || (!labels && !dense)) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce_soft: null pointer");
    if (dense && plan) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce_soft: a mix plan goes with labels, not with dense targets");
    if (!dense && label_dtype != FVA_LABEL_I64 && label_dtype != FVA_LABEL_F32)
        return fva_fail(FVA_ERR_ARG, "fva_softmax_ce_soft: bad label dtype %d", label_dtype);
    if (reduction != FVA_REDUCE_MEAN && reduction != FVA_REDUCE_SUM) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce_soft: bad reduction %d", reduction);
    if (R < 1 || C < 1) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce_soft: bad shape R=%d C=%d", R, C);
    if (!(smoothing >= 0.f && smoothing <= 1.f)) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce_soft: smoothing = %g outside [0, 1]", (double)smoothing);
    const float scale = reduction == FVA_REDUCE_MEAN ? 1.f / (float)R : 1.f;
    hipLaunchKernelGGL(soft_ce_kernel, dim3(R), dim3(SCE_THREADS), 0, (hipStream_t)stream, logits, labels, label_dtype, dense, weights, R, C, scale,
                       smoothing, plan, (float*)workspace, grad);
    FVA_LAUNCH_CHECK("soft_ce_kernel");
    hipLaunchKernelGGL(soft_ce_final_kernel, dim3(1), dim3(SCE_THREADS), 0, (hipStream_t)stream, (const float*)workspace, R,
                       reduction == FVA_REDUCE_MEAN ? (double)R : 1.0, loss_out);
    FVA_LAUNCH_CHECK("soft_ce_final_kernel");
    return FVA_OK;
}

int fva_topk_accuracy(const void* logits, int logits_dtype, const void* labels, int label_dtype, int32_t R, int32_t C, int32_t k, float* out,
                      void* workspace, void* stream) {
    if (!logits || !labels || !out || !workspace) return fva_fail(FVA_ERR_ARG, "fva_topk_accuracy: null pointer");
    if (logits_dtype != FVA_F32 && logits_dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "fva_topk_accuracy: bad logits dtype %d", logits_dtype);
    if (label_dtype != FVA_LABEL_I64 && label_dtype != FVA_LABEL_F32) return fva_fail(FVA_ERR_ARG, "fva_topk_accuracy: bad label dtype %d", label_dtype);
    if (R < 1 || C < 1) return fva_fail(FVA_ERR_ARG, "fva_topk_accuracy: bad shape R=%d C=%d", R, C);
    if (k < 1) return fva_fail(FVA_ERR_ARG, "fva_topk_accuracy: k = %d must be at least 1", k);
    const int blocks = (R + SCE_WAVES - 1) / SCE_WAVES;
    if (logits_dtype == FVA_BF16)
        hipLaunchKernelGGL(topk_kernel<bf16_t>, dim3(blocks), dim3(SCE_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, labels, label_dtype, R,
                           C, k, (int*)workspace);
    else
        hipLaunchKernelGGL(topk_kernel<float>, dim3(blocks), dim3(SCE_THREADS), 0, (hipStream_t)stream, (const float*)logits, labels, label_dtype, R, C,
                           k, (int*)workspace);
    FVA_LAUNCH_CHECK("topk_kernel");
    hipLaunchKernelGGL(topk_final_kernel, dim3(1), dim3(SCE_THREADS), 0, (hipStream_t)stream, (const int*)workspace, R, out);
    FVA_LAUNCH_CHECK("topk_final_kernel");
    return FVA_OK;
}

}  // extern "C"
