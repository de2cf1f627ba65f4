// MixUp and CutMix on the device for gfx950 (not in the reference; the recipe its ResNet / ResNeXt / VGG classifiers are trained with):
//   fva_mix_plan    a one-thread tick kernel: draws mode, lambda and the CutMix box from Philox-4x32-10 keyed by (seed, call counter), both
//                   in device memory, and advances the counter -- a captured graph draws a new plan on every replay, no host read-back
//   fva_mix_apply   one streaming pass over planar [B][C][H][W]: out_b = mix of x_b and x_((b - 1 + B) % B) as the plan says
// The draw order, the uniform, Johnk's method and the box arithmetic are stated in include/fastvision_amd.h.  The apply pass is HBM-bound:
// MixUp reads two images per image written (3 bytes moved per byte of output), CutMix reads the partner only where a 16-byte chunk
// meets the box, mode 0 is a copy.  No atomics, no LDS: two runs on the same state give identical bits.
#include <math.h>

#include "common.h"

namespace {

struct Philox4 {
    uint32_t v[4];
};
// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): the ten rounds as published (the generator of fva_dropout_fwd)
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float uniform_of(uint32_t word) { return ((float)(word >> 8) + 0.5f) * 5.9604644775390625e-8f; }   // fp32: the sum rounds to even from 2^23 on

constexpr int JOHNK_MAX_PAIRS = 512;

// lam_raw ~ Beta(alpha, alpha), alpha <= 1: Johnk's method on the pairs (words 4 + 2 i, 5 + 2 i), in double, rounded once
__device__ float johnk_beta(double alpha, uint32_t n0, uint32_t n1, uint32_t k0, uint32_t k1) {
    const double inv = 1.0 / alpha;
    for (int i = 0; i < JOHNK_MAX_PAIRS; i += 2) {                 // one Philox block holds two pairs
        const Philox4 r = philox4x32_10((uint32_t)(1 + i / 2), 0u, n0, n1, k0, k1);
        for (int h = 0; h < 2; ++h) {
            const double U = (double)uniform_of(r.v[2 * h]), V = (double)uniform_of(r.v[2 * h + 1]);
            const double X = pow(U, inv), Y = pow(V, inv), XpY = X + Y;
            if (XpY <= 1.0) {
                if (XpY > 0.0) return (float)(X / XpY);
                double lx = log(U) * inv, ly = log(V) * inv;
                const double lm = lx > ly ? lx : ly;
                lx -= lm;
                ly -= lm;
                return (float)exp(lx - log(exp(lx) + exp(ly)));
            }
        }
    }
    return 0.5f;
}

__global__ __launch_bounds__(64) void mix_plan_kernel(long long* __restrict__ state, float mixup_alpha, float cutmix_alpha, float prob,
                                                      float switch_prob, int H, int W, fva_mix_plan_t* __restrict__ plan) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long seed = state[0], counter = state[1];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)((unsigned long long)seed >> 32);
    const uint32_t n0 = (uint32_t)counter, n1 = (uint32_t)((unsigned long long)counter >> 32);
    const Philox4 head = philox4x32_10(0u, 0u, n0, n1, k0, k1);
    fva_mix_plan_t p;
    p.mode = 0;
    p.lam_raw = p.lam = 1.f;
    p.rx = p.ry = p.x1 = p.y1 = p.x2 = p.y2 = 0;
    const bool both = mixup_alpha > 0.f && cutmix_alpha > 0.f;
    const bool cut = both ? uniform_of(head.v[1]) < switch_prob : cutmix_alpha > 0.f;
    const float alpha = cut ? cutmix_alpha : mixup_alpha;
    if (uniform_of(head.v[0]) < prob && alpha > 0.f) {
        p.lam_raw = johnk_beta((double)alpha, n0, n1, k0, k1);
        if (cut) {
            p.mode = 2;
            p.rx = (int)(((unsigned long long)head.v[2] * (unsigned long long)W) >> 32);
            p.ry = (int)(((unsigned long long)head.v[3] * (unsigned long long)H) >> 32);
            const float r = 0.5f * sqrtf(1.f - p.lam_raw);
            const int hw = (int)(r * (float)W), hh = (int)(r * (float)H);
            p.x1 = max(p.rx - hw, 0);
            p.x2 = min(p.rx + hw, W);
            p.y1 = max(p.ry - hh, 0);
            p.y2 = min(p.ry + hh, H);
            p.lam = 1.f - (float)((p.x2 - p.x1) * (p.y2 - p.y1)) / (float)(W * H);
        } else {
            p.mode = 1;
            p.lam = p.lam_raw;
        }
    }
    *plan = p;
    state[1] = counter + 1;
}

// 16-byte chunks: grid.y = image, grid.x strides over the CHW / EPC chunks of one image.  W % EPC == 0, so a chunk lies in one row.
template <typename T>
__global__ __launch_bounds__(256) void mix_apply_vec_kernel(const T* __restrict__ x, T* __restrict__ out, const fva_mix_plan_t* __restrict__ plan,
                                                            int B, FastDiv Hd, FastDiv wvd, int nvec) {
    constexpr int EPC = Vec16<T>::N;
    const int b = blockIdx.y, pb = b == 0 ? B - 1 : b - 1;
    const int mode = B == 1 ? 0 : plan->mode;
    const float lam = plan->lam, oml = 1.f - lam;
    const int x1 = plan->x1, x2 = plan->x2, y1 = plan->y1, y2 = plan->y2;
    const T* xb = x + (int64_t)b * nvec * EPC;                       // 64-bit element offsets; inside an image 32 bits are enough (host check)
    const T* xp = x + (int64_t)pb * nvec * EPC;
    T* ob = out + (int64_t)b * nvec * EPC;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < (uint32_t)nvec; v += gridDim.x * 256u) {
        Vec16<T> a = *(const Vec16<T>*)(xb + (int64_t)v * EPC);
        if (mode == 1) {
            const Vec16<T> q = *(const Vec16<T>*)(xp + (int64_t)v * EPC);
#pragma unroll
            for (int e = 0; e < EPC; ++e) a.set(e, __builtin_fmaf(lam, a.get(e), oml * q.get(e)));
        } else if (mode == 2) {
            const uint32_t row = fd_div(v, wvd);                     // row index over C * H; wvd.d = W / EPC chunks per row
            const int xs = (int)(v - row * wvd.d) * EPC, yy = (int)(row - fd_div(row, Hd) * Hd.d);
            if (yy >= y1 && yy < y2 && xs < x2 && xs + EPC > x1) {
                const Vec16<T> q = *(const Vec16<T>*)(xp + (int64_t)v * EPC);
#pragma unroll
                for (int e = 0; e < EPC; ++e)
                    if (xs + e >= x1 && xs + e < x2) a.v[e] = q.v[e];
            }
        }
        *(Vec16<T>*)(ob + (int64_t)v * EPC) = a;
    }
}

// any shape and alignment: one element per thread and step, plain stores
template <typename T>
__global__ __launch_bounds__(256) void mix_apply_elem_kernel(const T* __restrict__ x, T* __restrict__ out, const fva_mix_plan_t* __restrict__ plan,
                                                             int B, FastDiv Hd, FastDiv Wd, int n) {
    const int b = blockIdx.y, pb = b == 0 ? B - 1 : b - 1;
    const int mode = B == 1 ? 0 : plan->mode;
    const float lam = plan->lam, oml = 1.f - lam;
    const int x1 = plan->x1, x2 = plan->x2, y1 = plan->y1, y2 = plan->y2;
    const T* xb = x + (int64_t)b * n;
    const T* xp = x + (int64_t)pb * n;
    T* ob = out + (int64_t)b * n;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < (uint32_t)n; i += gridDim.x * 256u) {
        T a = xb[i];
        if (mode == 1) {
            a = from_f<T>(__builtin_fmaf(lam, to_f(a), oml * to_f(xp[i])));
        } else if (mode == 2) {
            const uint32_t row = fd_div(i, Wd);
            const int xx = (int)(i - row * Wd.d), yy = (int)(row - fd_div(row, Hd) * Hd.d);
            if (yy >= y1 && yy < y2 && xx >= x1 && xx < x2) a = xp[i];
        }
        ob[i] = a;
    }
}

inline int apply_grid_x(int64_t items, int B) {
    const int64_t want = (items + 255) / 256;
    const int64_t cap = 4096 / B > 1 ? 4096 / B : 1;                  // about 4096 blocks in all: the rest is the grid-stride loop
    return (int)(want < cap ? want : cap);
}

}  // namespace

extern "C" {

int fva_mix_plan(int64_t* state, float mixup_alpha, float cutmix_alpha, float prob, float switch_prob, int32_t H, int32_t W,
                 fva_mix_plan_t* plan, void* stream) {
    if (!state || !plan) return fva_fail(FVA_ERR_ARG, "fva_mix_plan: null pointer");
    if (!(mixup_alpha >= 0.f && mixup_alpha <= 1.f) || !(cutmix_alpha >= 0.f && cutmix_alpha <= 1.f))
        return fva_fail(FVA_ERR_ARG, "fva_mix_plan: mixup_alpha = %g, cutmix_alpha = %g: each must lie in [0, 1] (Johnk's method; alpha > 1 is not supported)",
                        (double)mixup_alpha, (double)cutmix_alpha);
    if (!(prob >= 0.f && prob <= 1.f) || !(switch_prob >= 0.f && switch_prob <= 1.f))
        return fva_fail(FVA_ERR_ARG, "fva_mix_plan: prob = %g, switch_prob = %g: each must lie in [0, 1]", (double)prob, (double)switch_prob);
    if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) return fva_fail(FVA_ERR_ARG, "fva_mix_plan: bad image size H=%d W=%d", H, W);
    hipLaunchKernelGGL(mix_plan_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)state, mixup_alpha, cutmix_alpha, prob, switch_prob,
                       H, W, plan);
    FVA_LAUNCH_CHECK("mix_plan_kernel");
    return FVA_OK;
}

int fva_mix_apply(int dtype, const void* x, void* out, const fva_mix_plan_t* plan, int32_t B, int32_t C, int32_t H, int32_t W, void* stream) {
    if (!x || !out || !plan) return fva_fail(FVA_ERR_ARG, "fva_mix_apply: null pointer");
    if (dtype != FVA_F32 && dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "fva_mix_apply: bad dtype %d", dtype);
    if (B < 1 || C < 1 || H < 1 || W < 1 || B > 65535 || (int64_t)C * H * W >= (1ll << 31))
        return fva_fail(FVA_ERR_ARG, "fva_mix_apply: bad shape B=%d C=%d H=%d W=%d (B <= 65535, C * H * W < 2^31)", B, C, H, W);
    if (x == out) return fva_fail(FVA_ERR_ARG, "fva_mix_apply: works out of place (image b reads image b - 1)");
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    const int64_t n = (int64_t)C * H * W;
    const bool vec = n % epc == 0 && W % epc == 0 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    const FastDiv Hd = make_fastdiv((uint32_t)H);
    if (vec) {
        const FastDiv wvd = make_fastdiv((uint32_t)(W / epc));
        const dim3 grid(apply_grid_x(n / epc, B), B);
        if (dtype == FVA_BF16)
            hipLaunchKernelGGL(mix_apply_vec_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)out, plan, B, Hd, wvd, (int)(n / epc));
        else
            hipLaunchKernelGGL(mix_apply_vec_kernel<float>, grid, dim3(256), 0, s, (const float*)x, (float*)out, plan, B, Hd, wvd, (int)(n / epc));
        FVA_LAUNCH_CHECK("mix_apply_vec_kernel");
    } else {
        const FastDiv Wd = make_fastdiv((uint32_t)W);
        const dim3 grid(apply_grid_x(n, B), B);
        if (dtype == FVA_BF16)
            hipLaunchKernelGGL(mix_apply_elem_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)out, plan, B, Hd, Wd, (int)n);
        else
            hipLaunchKernelGGL(mix_apply_elem_kernel<float>, grid, dim3(256), 0, s, (const float*)x, (float*)out, plan, B, Hd, Wd, (int)n);
        FVA_LAUNCH_CHECK("mix_apply_elem_kernel");
    }
    return FVA_OK;
}

}  // extern "C"
