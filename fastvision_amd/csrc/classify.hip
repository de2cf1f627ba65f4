// Classification top of Darknet-53 for gfx950: global average pooling (forward / backward), softmax cross-entropy (value and
// gradient in one pass over the logits) and top-1 accuracy.  None of these uses MFMA: the pooling kernels are HBM-bound (one
// coalesced pass, lanes along C), the loss and the metric are latency-bound (a few hundred KB of logits per step).
//
// Replaces the reference's classifier top nn.AdaptiveAvgPool2d((1, 1)) -> flatten (classfication/models/darknet53.py:65-137),
// CrossEntropyLoss (loss/classification_loss.py:8-33) and metrics/accuracy.py.
//
// Determinism: every sum runs in a fixed order (per-thread serial loops, wave64 butterflies, then the waves in order); there are no
// float atomics anywhere, so two runs on the same inputs give identical bits.
#include <math.h>

#include "common.h"

namespace {

constexpr int CLS_THREADS = 256;
constexpr int CLS_WAVES = CLS_THREADS / 64;

// ---- global average pooling ---------------------------------------------------------------------------------------------------
// Block = 64 channels x 4 waves: lane l of wave w sums channel c0 + l over the pixels p = w, w + 4, ... (fp32, serial), then the four
// partial sums are added in wave order.  A wave reads 64 consecutive channels of one pixel: 128 B (bf16) or 256 B (fp32), coalesced.
template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void gap_fwd_kernel(const T* __restrict__ x, int pad, int H, int W, int C, float* __restrict__ out) {
    __shared__ float red[CLS_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lane;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad, HW = H * W;
    float s = 0.f;
    if (c < C) {
        const T* xb = x + (int64_t)b * Hp * Wp * C + c;
        for (int p = wave; p < HW; p += CLS_WAVES) {
            const int y = p / W, xx = p - y * W;
            s += to_f(xb[((int64_t)(y + pad) * Wp + (xx + pad)) * C]);
        }
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < C) {
        float t = red[0][lane];
        for (int w = 1; w < CLS_WAVES; ++w) t += red[w][lane];
        out[(int64_t)b * C + c] = t / (float)HW;
    }
}

// dx[b][y][x][c] = g[b][c] / (H * W), dense NHWC in the compute dtype.  Block (blockIdx.x, blockIdx.y = b) covers GAP_BWD_PIX consecutive
// pixels of image b; a thread takes channels c = tid, tid + 256, ..., forms g / (H*W) once and stores it to each of those pixels:
// consecutive lanes write consecutive channels (coalesced), no integer division per element, one read of g per 8 stores.
constexpr int GAP_BWD_PIX = 8;
template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void gap_bwd_kernel(const float* __restrict__ g, int HW, int C, T* __restrict__ dx) {
    const int b = blockIdx.y, p0 = blockIdx.x * GAP_BWD_PIX;
    const int np = HW - p0 < GAP_BWD_PIX ? HW - p0 : GAP_BWD_PIX;
    const float hw = (float)HW;
    T* out = dx + ((int64_t)b * HW + p0) * C;
    for (int c = threadIdx.x; c < C; c += CLS_THREADS) {
        const T v = from_f<T>(g[(int64_t)b * C + c] / hw);
        for (int q = 0; q < np; ++q) out[(int64_t)q * C + c] = v;
    }
}

// ---- softmax cross-entropy ----------------------------------------------------------------------------------------------------
// (m, s) = running max and sum of exp(z - m).  Merging with an empty partial (s == 0, m == -inf) must not form exp(-inf - -inf).
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

// One block per row: pass 1 reads the row for its max / sum-exp (online, per thread, then fixed-order merges), pass 2 reads it again
// for the gradient.  row_loss[r] = w_r * (m + log s - z_y); grad[r][k] = scale * w_r * (softmax_k - [k == y]).
__global__ __launch_bounds__(CLS_THREADS) void softmax_ce_kernel(const float* __restrict__ logits, const void* __restrict__ labels, int label_dtype,
                                                                 const float* __restrict__ weights, int C, float scale,
                                                                 float* __restrict__ row_loss, float* __restrict__ grad) {
    __shared__ MaxSum red[CLS_WAVES];
    const int r = blockIdx.x;
    const float* z = logits + (int64_t)r * C;
    MaxSum a{-INFINITY, 0.f};
    for (int k = threadIdx.x; k < C; k += CLS_THREADS) {
        const float v = z[k];
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
    for (int w = 1; w < CLS_WAVES; ++w) a = ms_merge(a, red[w]);
    const int y = row_label(labels, label_dtype, r, C);
    const float w = weights ? weights[r] : 1.f;
    const float ls = logf(a.s);
    if (threadIdx.x == 0) row_loss[r] = y < 0 ? NAN : -((z[y] - a.m) - ls) * w;
    if (grad == nullptr) return;
    float* gr = grad + (int64_t)r * C;
    const float gs = y < 0 ? NAN : scale * w, inv = 1.f / a.s;
    for (int k = threadIdx.x; k < C; k += CLS_THREADS) {
        const float p = expf(z[k] - a.m) * inv;
        gr[k] = gs * (k == y ? p - 1.f : p);
    }
}

// out[0] = (sum of part[0 .. n)) / denom, summed in double in a fixed order (one block).
__global__ __launch_bounds__(CLS_THREADS) void ce_final_kernel(const float* __restrict__ part, int n, double denom, float* __restrict__ out) {
    __shared__ double red[CLS_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += CLS_THREADS) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0.0;
        for (int i = 0; i < CLS_THREADS; ++i) s += red[i];
        out[0] = (float)(s / denom);
    }
}

// ---- top-1 accuracy -----------------------------------------------------------------------------------------------------------
// torch.argmax order: a NaN beats every number, among equals (or NaNs) the smaller index wins.
__device__ __forceinline__ bool arg_better(float v, int i, float bv, int bi) {
    const bool vn = isnan(v), bn = isnan(bv);
    if (vn != bn) return vn;
    if (vn || v == bv) return i < bi;
    return v > bv;
}

// One wave per row (4 rows per block): hit[r] = 1 if the row's argmax equals its label.
template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void top1_kernel(const T* __restrict__ logits, const void* __restrict__ labels, int label_dtype, int R,
                                                           int C, int* __restrict__ hit) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * CLS_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;                       // whole waves leave together: the shuffles below stay within live waves
    const T* z = logits + (int64_t)r * C;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = lane; k < C; k += 64) {
        const float v = to_f(z[k]);
        if (arg_better(v, k, bv, bi)) bv = v, bi = k;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (arg_better(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    if (lane == 0) {
        int ok;
        if (label_dtype == FVA_LABEL_I64) ok = ((const int64_t*)labels)[r] == (int64_t)bi;
        else ok = ((const float*)labels)[r] == (float)bi;
        hit[r] = ok;
    }
}

// out[0] = (float)(sum of hit) / (float)R  (integer sum: exact and order-free)
__global__ __launch_bounds__(CLS_THREADS) void top1_final_kernel(const int* __restrict__ hit, int R, float* __restrict__ out) {
    __shared__ int red[CLS_THREADS];
    int s = 0;
    for (int i = threadIdx.x; i < R; i += CLS_THREADS) s += hit[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0;
        for (int i = 0; i < CLS_THREADS; ++i) s += red[i];
        out[0] = (float)s / (float)R;
    }
}

}  // namespace

extern "C" {

int fva_gap_fwd(int dtype, const void* x, int x_pad, int B, int H, int W, int C, float* out, void* stream) {
    if (!x || !out) return fva_fail(FVA_ERR_ARG, "fva_gap_fwd: null pointer");
    if (dtype != FVA_F32 && dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "fva_gap_fwd: bad dtype %d", dtype);
    if (x_pad < 0 || x_pad > 1 || B < 1 || H < 1 || W < 1 || C < 1 || B > 65535 || (int64_t)H * W >= (1ll << 31))
        return fva_fail(FVA_ERR_ARG, "fva_gap_fwd: bad shape B=%d H=%d W=%d C=%d pad=%d", B, H, W, C, x_pad);
    const dim3 grid((C + 63) / 64, B);
    if (dtype == FVA_BF16)
        hipLaunchKernelGGL(gap_fwd_kernel<bf16_t>, grid, dim3(CLS_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, x_pad, H, W, C, out);
    else
        hipLaunchKernelGGL(gap_fwd_kernel<float>, grid, dim3(CLS_THREADS), 0, (hipStream_t)stream, (const float*)x, x_pad, H, W, C, out);
    FVA_LAUNCH_CHECK("gap_fwd_kernel");
    return FVA_OK;
}

int fva_gap_bwd(int dtype, const float* g, int B, int H, int W, int C, void* dx, void* stream) {
    if (!g || !dx) return fva_fail(FVA_ERR_ARG, "fva_gap_bwd: null pointer");
    if (dtype != FVA_F32 && dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "fva_gap_bwd: bad dtype %d", dtype);
    if (B < 1 || H < 1 || W < 1 || C < 1 || (int64_t)H * W >= (1ll << 31))
        return fva_fail(FVA_ERR_ARG, "fva_gap_bwd: bad shape B=%d H=%d W=%d C=%d", B, H, W, C);
    if (B > 65535) return fva_fail(FVA_ERR_ARG, "fva_gap_bwd: B=%d exceeds 65535", B);
    const dim3 grid((H * W + GAP_BWD_PIX - 1) / GAP_BWD_PIX, B);
    if (dtype == FVA_BF16)
        hipLaunchKernelGGL(gap_bwd_kernel<bf16_t>, grid, dim3(CLS_THREADS), 0, (hipStream_t)stream, g, H * W, C, (bf16_t*)dx);
    else
        hipLaunchKernelGGL(gap_bwd_kernel<float>, grid, dim3(CLS_THREADS), 0, (hipStream_t)stream, g, H * W, C, (float*)dx);
    FVA_LAUNCH_CHECK("gap_bwd_kernel");
    return FVA_OK;
}

int64_t fva_softmax_ce_workspace(int32_t R) { return R < 1 ? 0 : (int64_t)R * (int64_t)sizeof(float); }

int fva_softmax_ce(const float* logits, const void* labels, int label_dtype, const float* weights, int32_t R, int32_t C, int32_t reduction,
                   float* loss_out, float* grad, void* workspace, void* stream) {
    if (!logits || !labels || !loss_out || !workspace) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce: null pointer");
    if (label_dtype != FVA_LABEL_I64 && label_dtype != FVA_LABEL_F32) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce: bad label dtype %d", label_dtype);
    if (reduction != FVA_REDUCE_MEAN && reduction != FVA_REDUCE_SUM) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce: bad reduction %d", reduction);
    if (R < 1 || C < 1) return fva_fail(FVA_ERR_ARG, "fva_softmax_ce: bad shape R=%d C=%d", R, C);
    const float scale = reduction == FVA_REDUCE_MEAN ? 1.f / (float)R : 1.f;
    hipLaunchKernelGGL(softmax_ce_kernel, dim3(R), dim3(CLS_THREADS), 0, (hipStream_t)stream, logits, labels, label_dtype, weights, C, scale,
                       (float*)workspace, grad);
    FVA_LAUNCH_CHECK("softmax_ce_kernel");
    hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(CLS_THREADS), 0, (hipStream_t)stream, (const float*)workspace, R,
                       reduction == FVA_REDUCE_MEAN ? (double)R : 1.0, loss_out);
    FVA_LAUNCH_CHECK("ce_final_kernel");
    return FVA_OK;
}

int fva_top1_accuracy(const void* logits, int logits_dtype, const void* labels, int label_dtype, int32_t R, int32_t C, float* out,
                      void* workspace, void* stream) {
    if (!logits || !labels || !out || !workspace) return fva_fail(FVA_ERR_ARG, "fva_top1_accuracy: null pointer");
    if (logits_dtype != FVA_F32 && logits_dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "fva_top1_accuracy: bad logits dtype %d", logits_dtype);
    if (label_dtype != FVA_LABEL_I64 && label_dtype != FVA_LABEL_F32) return fva_fail(FVA_ERR_ARG, "fva_top1_accuracy: bad label dtype %d", label_dtype);
    if (R < 1 || C < 1) return fva_fail(FVA_ERR_ARG, "fva_top1_accuracy: bad shape R=%d C=%d", R, C);
    const int blocks = (R + CLS_WAVES - 1) / CLS_WAVES;
    if (logits_dtype == FVA_BF16)
        hipLaunchKernelGGL(top1_kernel<bf16_t>, dim3(blocks), dim3(CLS_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, labels, label_dtype,
                           R, C, (int*)workspace);
    else
        hipLaunchKernelGGL(top1_kernel<float>, dim3(blocks), dim3(CLS_THREADS), 0, (hipStream_t)stream, (const float*)logits, labels, label_dtype,
                           R, C, (int*)workspace);
    FVA_LAUNCH_CHECK("top1_kernel");
    hipLaunchKernelGGL(top1_final_kernel, dim3(1), dim3(CLS_THREADS), 0, (hipStream_t)stream, (const int*)workspace, R, out);
    FVA_LAUNCH_CHECK("top1_final_kernel");
    return FVA_OK;
}

}  // extern "C"

// =========================================================================================================
// nn.AdaptiveAvgPool2d((7, 7)) + torch.flatten(x, 1) of the VGG classifiers (reference classfication/models/vgg.py:27,67-68).
// Input: halo / dense NHWC [B][H+2p][W+2p][C]; output [B][C*49] in the reference's flatten(NCHW) order (c * 49 + i * 7 + j), in the
// compute dtype: the operand of the first Linear as stored.  Windows as torch defines them: rows floor(i*H/7) .. ceil((i+1)*H/7), any H, W
// >= 1 (H < 7 repeats pixels, H % 7 != 0 overlaps).  One block per (image, 64 channels): 16-byte reads along the channel axis, window sums
// in scan order in fp32, the 64 x 49 tile turned through LDS (row stride 49 floats: odd, conflict-free), and written as ONE contiguous
// run of 64 * 49 elements with 16-byte stores.  At 7x7 this is a transpose.  Backward in gather form: the block loads its run of the
// gradient into LDS (divided by the window size), then every input pixel adds the windows that contain it in (i, j) order.  No atomics.
namespace {

constexpr int P7 = 7, P7_BINS = 49, P7_CB = 64;
__device__ __forceinline__ int p7_start(int i, int n) { return (i * n) / P7; }
__device__ __forceinline__ int p7_end(int i, int n) { return ((i + 1) * n + P7 - 1) / P7; }

template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void pool7_fwd_kernel(const T* __restrict__ x, int pad, int H, int W, int C, T* __restrict__ out) {
    constexpr int EPC = Vec16<T>::N, CPL = P7_CB / EPC, SLOTS = CLS_THREADS / CPL;
    __shared__ __attribute__((aligned(16))) float tile[P7_CB * P7_BINS];
    const int b = blockIdx.y, c0 = blockIdx.x * P7_CB;
    const int nch = C - c0 < P7_CB ? C - c0 : P7_CB;              // channels of this block (a multiple of EPC)
    const int chunk = threadIdx.x % CPL, slot = threadIdx.x / CPL;
    const int Wp = W + 2 * pad;
    const T* xb = x + ((int64_t)b * (H + 2 * pad) * Wp) * C + c0 + chunk * EPC;
    if (chunk * EPC < nch) {
        for (int bin = slot; bin < P7_BINS; bin += SLOTS) {
            const int i = bin / P7, j = bin - i * P7;
            const int h0 = p7_start(i, H), h1 = p7_end(i, H), w0 = p7_start(j, W), w1 = p7_end(j, W);
            float acc[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
            for (int hh = h0; hh < h1; ++hh)
                for (int ww = w0; ww < w1; ++ww) {
                    const Vec16<T> v = *(const Vec16<T>*)(xb + ((int64_t)(hh + pad) * Wp + (ww + pad)) * C);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) acc[e] += v.get(e);
                }
            const float cnt = (float)((h1 - h0) * (w1 - w0));
#pragma unroll
            for (int e = 0; e < EPC; ++e) tile[(chunk * EPC + e) * P7_BINS + bin] = acc[e] / cnt;
        }
    }
    __syncthreads();
    T* ob = out + ((int64_t)b * C + c0) * P7_BINS;                // 16-byte aligned: (b * C + c0) * 49 elements, C and c0 multiples of EPC
    const int nvec = nch * P7_BINS / EPC;
    for (int v = threadIdx.x; v < nvec; v += CLS_THREADS) {
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.set(e, tile[v * EPC + e]);
        *(Vec16<T>*)(ob + (int64_t)v * EPC) = o;
    }
}

template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void pool7_bwd_kernel(const T* __restrict__ g, int H, int W, int C, T* __restrict__ dx) {
    constexpr int EPC = Vec16<T>::N, CPL = P7_CB / EPC, SLOTS = CLS_THREADS / CPL;
    __shared__ __attribute__((aligned(16))) float tile[P7_CB * P7_BINS];
    const int b = blockIdx.y, c0 = blockIdx.x * P7_CB;
    const int nch = C - c0 < P7_CB ? C - c0 : P7_CB;
    const T* gb = g + ((int64_t)b * C + c0) * P7_BINS;
    const int nvec = nch * P7_BINS / EPC;
    for (int v = threadIdx.x; v < nvec; v += CLS_THREADS) {
        const Vec16<T> q = *(const Vec16<T>*)(gb + (int64_t)v * EPC);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int bin = (v * EPC + e) % P7_BINS, i = bin / P7, j = bin - i * P7;
            const float cnt = (float)((p7_end(i, H) - p7_start(i, H)) * (p7_end(j, W) - p7_start(j, W)));
            tile[v * EPC + e] = q.get(e) / cnt;
        }
    }
    __syncthreads();
    const int chunk = threadIdx.x % CPL, slot = threadIdx.x / CPL;
    if (chunk * EPC >= nch) return;
    for (int pix = slot; pix < H * W; pix += SLOTS) {
        const int hh = pix / W, ww = pix - hh * W;
        float acc[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
        for (int i = 0; i < P7; ++i) {
            if (hh < p7_start(i, H) || hh >= p7_end(i, H)) continue;
            for (int j = 0; j < P7; ++j) {
                if (ww < p7_start(j, W) || ww >= p7_end(j, W)) continue;
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] += tile[(chunk * EPC + e) * P7_BINS + i * P7 + j];
            }
        }
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.set(e, acc[e]);
        *(Vec16<T>*)(dx + (((int64_t)b * H + hh) * W + ww) * C + c0 + chunk * EPC) = o;
    }
}

int pool7_check(const char* who, int dtype, int B, int H, int W, int C) {
    if (dtype != FVA_F32 && dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "%s: bad dtype %d", who, dtype);
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    if (B < 1 || H < 1 || W < 1 || C < 1 || B > 65535 || H > 4096 || W > 4096 || C % epc)
        return fva_fail(FVA_ERR_ARG, "%s: bad shape B=%d H=%d W=%d C=%d (C must be a multiple of %d, B <= 65535, H, W <= 4096)", who, B, H, W, C, epc);
    return FVA_OK;
}

}  // namespace

extern "C" {

int fva_adaptive_avgpool7_fwd(int dtype, const void* x, int x_pad, int B, int H, int W, int C, void* out, void* stream) {
    if (!x || !out) return fva_fail(FVA_ERR_ARG, "fva_adaptive_avgpool7_fwd: null pointer");
    const int rc = pool7_check("fva_adaptive_avgpool7_fwd", dtype, B, H, W, C);
    if (rc) return rc;
    if (x_pad < 0 || x_pad > 1) return fva_fail(FVA_ERR_ARG, "fva_adaptive_avgpool7_fwd: bad pad %d", x_pad);
    const dim3 grid((C + P7_CB - 1) / P7_CB, B);
    if (dtype == FVA_BF16)
        hipLaunchKernelGGL(pool7_fwd_kernel<bf16_t>, grid, dim3(CLS_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, x_pad, H, W, C, (bf16_t*)out);
    else
        hipLaunchKernelGGL(pool7_fwd_kernel<float>, grid, dim3(CLS_THREADS), 0, (hipStream_t)stream, (const float*)x, x_pad, H, W, C, (float*)out);
    FVA_LAUNCH_CHECK("pool7_fwd_kernel");
    return FVA_OK;
}

int fva_adaptive_avgpool7_bwd(int dtype, const void* g, int B, int H, int W, int C, void* dx, void* stream) {
    if (!g || !dx) return fva_fail(FVA_ERR_ARG, "fva_adaptive_avgpool7_bwd: null pointer");
    const int rc = pool7_check("fva_adaptive_avgpool7_bwd", dtype, B, H, W, C);
    if (rc) return rc;
    const dim3 grid((C + P7_CB - 1) / P7_CB, B);
    if (dtype == FVA_BF16)
        hipLaunchKernelGGL(pool7_bwd_kernel<bf16_t>, grid, dim3(CLS_THREADS), 0, (hipStream_t)stream, (const bf16_t*)g, H, W, C, (bf16_t*)dx);
    else
        hipLaunchKernelGGL(pool7_bwd_kernel<float>, grid, dim3(CLS_THREADS), 0, (hipStream_t)stream, (const float*)g, H, W, C, (float*)dx);
    FVA_LAUNCH_CHECK("pool7_bwd_kernel");
    return FVA_OK;
}

}  // extern "C"
