// What the ResNet classifiers (reference classfication/models/resnet.py) need around the implicit-GEMM convolutions and the
// BatchNorm + ReLU passes of bn_act.hip, all HBM-bound streaming passes over NHWC tensors, 16 bytes per lane and access:
//   stem7_patches          the 7x7 / stride 2 / pad 3 stem (resnet.py:136-140) as a patch matrix P [B*OH*OW][Kp]: the stem convolution
//                          is then the 1x1 implicit GEMM over P (forward and weight gradient)
//   maxpool3s2_fwd / bwd   nn.MaxPool2d(3, 2, 1) (resnet.py:142-144); backward in gather form, the first maximum recomputed from x
//   subsample2_fwd / bwd   x[:, :, ::2, ::2]: the 1x1 stride-2 shortcut (resnet.py:49, :106) becomes the 1x1 stride-1 convolution over it
//   bn_add_relu_*          z = relu(bn(y) + r) (resnet.py:64-71, :117-124), r = the identity or a second normalised tensor bn_d(y_d):
//                          apply, backward reduce and backward apply, the table form of bn_act.hip's ReLU passes with the add INSIDE
//                          the ReLU.  u is recomputed in fp32 from the stored operands in all three passes (never read from the rounded z).
// Algorithmic bytes per element (bf16): apply 2 (y) + 2 (r) + 2 (z); reduce 2 (dz) + 2 (y) + 2 (r); backward apply 6 in, 4 out
// (dy and dr, or dy and dy_d).  Fixed summation order, no float atomics: run-to-run bit-identical.
//
// Channels: any multiple of the 16-byte chunk up to 2048.  A block of 256 threads is (ncol chunk columns) x (rpi pixels), ncol =
// min(cpp, 256), rpi = 256 / ncol; a lane keeps its channel chunk -- and the chunk's coefficients in registers -- for a whole row, and
// takes a second chunk column when cpp > 256 (fp32 with C > 1024).  Where cpp does not divide 256 the last 256 - ncol * rpi threads idle.
#include <type_traits>

#include "common.h"

namespace {

constexpr int MAX_C = 2048;

struct ColMap {
    int cpp, ncol, rpi;
};
__host__ __device__ inline ColMap col_map(int cpp) {
    ColMap m;
    m.cpp = cpp;
    m.ncol = cpp < 256 ? cpp : 256;
    m.rpi = 256 / m.ncol;
    return m;
}

template <typename T>
__device__ __forceinline__ Vec16<T> zero_vec() {
    Vec16<T> z;
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) z.set(e, 0.f);
    return z;
}

// ---- the stem's patch matrix --------------------------------------------------------------------------------------------------------
// one 16-byte chunk of P per thread and step: columns k = ci * 49 + kh * 7 + kw of one output pixel; taps outside the image and the
// columns from Cin * 49 up to Kp are zero.  The image reads are scalar and hit the caches (an image is read 49 / 4 times over).
template <typename T>
__global__ __launch_bounds__(256) void stem7_patches_kernel(const float* __restrict__ x, T* __restrict__ P, int Cin, int H, int W, int OH, int OW,
                                                            int Kp, int64_t total) {
    constexpr int EPC = Vec16<T>::N;
    const int cpr = Kp / EPC, K = Cin * 49;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / cpr;
        const int cc = (int)(i - row * cpr);
        const int64_t t = row / OW;
        const int ox = (int)(row - t * OW), b = (int)(t / OH), oy = (int)(t - (int64_t)b * OH);
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int k = cc * EPC + e;
            float v = 0.f;
            if (k < K) {
                const int ci = k / 49, rem = k - ci * 49, kh = rem / 7, kw = rem - kh * 7;
                const int iy = 2 * oy - 3 + kh, ix = 2 * ox - 3 + kw;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[(((int64_t)b * Cin + ci) * H + iy) * W + ix];
            }
            o.set(e, v);
        }
        *(Vec16<T>*)(P + row * Kp + cc * EPC) = o;
    }
}

// ---- MaxPool2d(3, 2, 1) -------------------------------------------------------------------------------------------------------------
// torch's scan: kh, then kw ascending, `if (v > m || isnan(v)) { m = v; arg = tap; }` from m = -inf: the first maximum wins a tie, a NaN
// wins over everything (and the last NaN over an earlier one).  Taps outside the image are skipped, never read.
// forward: one block per padded output row
template <typename T>
__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(const T* __restrict__ x, int x_pad, T* __restrict__ out, int pad, int H, int W, int C) {
    constexpr int EPC = Vec16<T>::N;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, cpp = C / EPC;
    const int Hp = OH + 2 * pad, Wp = OW + 2 * pad, xWp = W + 2 * x_pad;
    const int b = blockIdx.x / Hp, oy = blockIdx.x - b * Hp - pad;
    const bool row_in = oy >= 0 && oy < OH;
    T* orow = out + (int64_t)blockIdx.x * Wp * C;
    const T* ximg = x + (int64_t)b * (H + 2 * x_pad) * xWp * C;
    for (int i = threadIdx.x; i < Wp * cpp; i += 256) {
        const int xp = i / cpp, cc = i - xp * cpp, ox = xp - pad;
        Vec16<T> o = zero_vec<T>();
        if (row_in && ox >= 0 && ox < OW) {
            float m[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) m[e] = -__builtin_inff();
            for (int kh = 0; kh < 3; ++kh) {
                const int iy = 2 * oy - 1 + kh;
                if (iy < 0 || iy >= H) continue;
                for (int kw = 0; kw < 3; ++kw) {
                    const int ix = 2 * ox - 1 + kw;
                    if (ix < 0 || ix >= W) continue;
                    const Vec16<T> v = *(const Vec16<T>*)(ximg + ((int64_t)(iy + x_pad) * xWp + ix + x_pad) * C + cc * EPC);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        const float f = v.get(e);
                        if (f > m[e] || f != f) m[e] = f;
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, m[e]);
        }
        *(Vec16<T>*)(orow + (int64_t)xp * C + cc * EPC) = o;
    }
}

// backward, gather form: one block per input row.  Pixel (y, x) lies in the windows oy in [ceil((y - 1) / 2), floor((y + 1) / 2)] x the
// same in x (one for an even coordinate, two for an odd one), clipped to the output; for each of them the scan above is repeated over x
// and dz of that window is taken when the scan ends on this pixel.  Overlapping windows sum in the fixed order (oy, ox ascending).
template <typename T>
__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ x, int x_pad, T* __restrict__ dx, int H,
                                                             int W, int C) {
    constexpr int EPC = Vec16<T>::N;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, cpp = C / EPC, xWp = W + 2 * x_pad;
    const int b = blockIdx.x / H, y = blockIdx.x - b * H;
    T* orow = dx + (int64_t)blockIdx.x * W * C;
    const T* ximg = x + (int64_t)b * (H + 2 * x_pad) * xWp * C;
    const int oy0 = y >> 1, oy1 = min((y + 1) >> 1, OH - 1);
    for (int i = threadIdx.x; i < W * cpp; i += 256) {
        const int xx = i / cpp, cc = i - xx * cpp;
        const int ox0 = xx >> 1, ox1 = min((xx + 1) >> 1, OW - 1);
        float acc[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) {
                const int me = (y - (2 * oy - 1)) * 3 + (xx - (2 * ox - 1));
                const int first = (oy == 0 ? 3 : 0) + (ox == 0 ? 1 : 0);        // the window's first tap inside the image: where the scan starts
                float m[EPC];
                int arg[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) { m[e] = -__builtin_inff(); arg[e] = first; }
                for (int kh = 0; kh < 3; ++kh) {
                    const int iy = 2 * oy - 1 + kh;
                    if (iy < 0 || iy >= H) continue;
                    for (int kw = 0; kw < 3; ++kw) {
                        const int ix = 2 * ox - 1 + kw;
                        if (ix < 0 || ix >= W) continue;
                        const Vec16<T> v = *(const Vec16<T>*)(ximg + ((int64_t)(iy + x_pad) * xWp + ix + x_pad) * C + cc * EPC);
#pragma unroll
                        for (int e = 0; e < EPC; ++e) {
                            const float f = v.get(e);
                            if (f > m[e] || f != f) { m[e] = f; arg[e] = kh * 3 + kw; }
                        }
                    }
                }
                const Vec16<T> g = *(const Vec16<T>*)(dz + (((int64_t)b * OH + oy) * OW + ox) * C + cc * EPC);
#pragma unroll
                for (int e = 0; e < EPC; ++e)
                    if (arg[e] == me) acc[e] += g.get(e);
            }
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.set(e, acc[e]);
        *(Vec16<T>*)(orow + (int64_t)xx * C + cc * EPC) = o;
    }
}

// ---- even-pixel subsample -----------------------------------------------------------------------------------------------------------
// forward: one block per row of xs [B][H/2][W/2][C] (dense); x is a halo tensor
template <typename T>
__global__ __launch_bounds__(256) void subsample2_fwd_kernel(const T* __restrict__ x, int x_pad, T* __restrict__ xs, int H, int W, int C) {
    constexpr int EPC = Vec16<T>::N;
    const int OH = H / 2, OW = W / 2, cpp = C / EPC, xWp = W + 2 * x_pad;
    const int b = blockIdx.x / OH, i2 = blockIdx.x - b * OH;
    const T* xrow = x + (((int64_t)b * (H + 2 * x_pad) + 2 * i2 + x_pad) * xWp + x_pad) * C;
    T* orow = xs + (int64_t)blockIdx.x * OW * C;
    for (int i = threadIdx.x; i < OW * cpp; i += 256) {
        const int j = i / cpp, cc = i - j * cpp;
        *(Vec16<T>*)(orow + (int64_t)j * C + cc * EPC) = *(const Vec16<T>*)(xrow + (int64_t)(2 * j) * C + cc * EPC);
    }
}

// backward: one block per row of dx [B][H][W][C] (dense): dxs at the even positions, zeros (written) elsewhere
template <typename T>
__global__ __launch_bounds__(256) void subsample2_bwd_kernel(const T* __restrict__ dxs, T* __restrict__ dx, int H, int W, int C) {
    constexpr int EPC = Vec16<T>::N;
    const int OH = H / 2, OW = W / 2, cpp = C / EPC;
    const int b = blockIdx.x / H, y = blockIdx.x - b * H;
    const bool even_row = !(y & 1);
    const T* grow = dxs + ((int64_t)b * OH + (y >> 1)) * OW * C;
    T* orow = dx + (int64_t)blockIdx.x * W * C;
    for (int i = threadIdx.x; i < W * cpp; i += 256) {
        const int xx = i / cpp, cc = i - xx * cpp;
        Vec16<T> o = zero_vec<T>();
        if (even_row && !(xx & 1)) o = *(const Vec16<T>*)(grow + (int64_t)(xx >> 1) * C + cc * EPC);
        *(Vec16<T>*)(orow + (int64_t)xx * C + cc * EPC) = o;
    }
}

// ---- BatchNorm + add + ReLU ---------------------------------------------------------------------------------------------------------
// u of one element, the same expression in the three passes.  FORM2: q is y_d and the addend is its own normalisation.
template <bool FORM2>
__device__ __forceinline__ float add_relu_u(float y, float sc, float sh, float q, float scd, float shd) {
    const float main = __builtin_fmaf(y, sc, sh);
    return main + (FORM2 ? __builtin_fmaf(q, scd, shd) : q);
}

// the second operand's row: the identity is a halo tensor (border r_pad), y_d is dense
template <typename T, bool FORM2>
__device__ __forceinline__ const T* second_row(const T* r, int r_pad, int b, int yy, int H, int W, int C) {
    if (FORM2) return r + ((int64_t)b * H + yy) * W * C;
    return r + (((int64_t)b * (H + 2 * r_pad) + yy + r_pad) * (W + 2 * r_pad) + r_pad) * C;
}

// apply: one block per padded row of z
template <typename T, bool FORM2>
__global__ __launch_bounds__(256) void bn_add_relu_apply_kernel(const T* __restrict__ y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                                const T* __restrict__ r, int r_pad, const float* __restrict__ scale_d,
                                                                const float* __restrict__ shift_d, T* __restrict__ z, int z_pad, int H, int W, int C) {
    constexpr int EPC = Vec16<T>::N;
    const ColMap cm = col_map(C / EPC);
    const int Hp = H + 2 * z_pad, Wp = W + 2 * z_pad;
    const int b = blockIdx.x / Hp, yy = blockIdx.x - b * Hp - z_pad;
    const bool row_in = yy >= 0 && yy < H;
    const int py = threadIdx.x / cm.ncol, cx = threadIdx.x - py * cm.ncol;
    if (py >= cm.rpi) return;                     // (no barrier in this kernel)
    T* zrow = z + (int64_t)blockIdx.x * Wp * C;
    const T* yrow = row_in ? y + ((int64_t)b * H + yy) * W * C : y;
    const T* rrow = row_in ? second_row<T, FORM2>(r, r_pad, b, yy, H, W, C) : r;
    for (int cc = cx; cc < cm.cpp; cc += cm.ncol) {
        float sc[EPC], sh[EPC], scd[EPC], shd[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int c = cc * EPC + e;
            sc[e] = scale[c]; sh[e] = shift[c];
            scd[e] = FORM2 ? scale_d[c] : 0.f; shd[e] = FORM2 ? shift_d[c] : 0.f;
        }
        for (int xp = py; xp < Wp; xp += cm.rpi) {
            const int xx = xp - z_pad;
            Vec16<T> out = zero_vec<T>();
            if (row_in && xx >= 0 && xx < W) {
                const int64_t off = (int64_t)xx * C + cc * EPC;
                const Vec16<T> v = *(const Vec16<T>*)(yrow + off), q = *(const Vec16<T>*)(rrow + off);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float u = add_relu_u<FORM2>(v.get(e), sc[e], sh[e], q.get(e), scd[e], shd[e]);
                    out.set(e, u <= 0.f ? 0.f : u);          // a NaN stays a NaN, as in torch.relu
                }
            }
            *(Vec16<T>*)(zrow + (int64_t)xp * C + cc * EPC) = out;
        }
    }
}

// backward pass 1: block `blk` owns the pixels [blk * rows_per_block, ...) and writes row blk of partial [nblocks][2][C] = sums of dU and
// dU * xhat, dU = dz * (u > 0); FORM2 also row blk of partial_d = sums of dU (the same numbers: both BatchNorms share them) and
// dU * xhat_d.  A lane adds its pixels m0 + py, m0 + py + rpi, ... in that order; the rpi lanes of a channel are folded through LDS in
// the order of py.
template <typename T, bool FORM2>
__global__ __launch_bounds__(256) void bn_add_relu_bwd_reduce_kernel(const T* __restrict__ dz, const T* __restrict__ y, const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, const float* __restrict__ mean,
                                                                     const float* __restrict__ rstd, const T* __restrict__ r, int r_pad,
                                                                     const float* __restrict__ scale_d, const float* __restrict__ shift_d,
                                                                     const float* __restrict__ mean_d, const float* __restrict__ rstd_d,
                                                                     float* __restrict__ part, float* __restrict__ part_d, int64_t M, int H, int W, int C,
                                                                     int rows_per_block) {
    constexpr int EPC = Vec16<T>::N, NS = FORM2 ? 3 : 2;
    extern __shared__ float red[];                 // [NS][rpi][ncol * EPC]
    const ColMap cm = col_map(C / EPC);
    const int py = threadIdx.x / cm.ncol, cx = threadIdx.x - py * cm.ncol, ncolE = cm.ncol * EPC;
    const bool active = py < cm.rpi;
    const int64_t m0 = (int64_t)blockIdx.x * rows_per_block;
    int64_t m1 = m0 + rows_per_block;
    if (m1 > M) m1 = M;
    const int HW = H * W, rWp = W + 2 * r_pad;
    for (int pb = 0; pb < cm.cpp; pb += cm.ncol) {
        const int cc = pb + cx;
        float s1[EPC], s2[EPC], s3[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) s1[e] = s2[e] = s3[e] = 0.f;
        if (active && cc < cm.cpp) {
            float sc[EPC], sh[EPC], mu[EPC], rs[EPC], scd[EPC], shd[EPC], mud[EPC], rsd[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const int c = cc * EPC + e;
                sc[e] = scale[c]; sh[e] = shift[c]; mu[e] = mean[c]; rs[e] = rstd[c];
                scd[e] = FORM2 ? scale_d[c] : 0.f; shd[e] = FORM2 ? shift_d[c] : 0.f;
                mud[e] = FORM2 ? mean_d[c] : 0.f; rsd[e] = FORM2 ? rstd_d[c] : 0.f;
            }
            for (int64_t m = m0 + py; m < m1; m += cm.rpi) {
                const int64_t off = m * C + cc * EPC;
                int64_t roff = off;
                if (!FORM2) {
                    const int b = (int)(m / HW), rem = (int)(m - (int64_t)b * HW), yy = rem / W, xx = rem - yy * W;
                    roff = (((int64_t)b * (H + 2 * r_pad) + yy + r_pad) * rWp + xx + r_pad) * C + cc * EPC;
                }
                const Vec16<T> g = *(const Vec16<T>*)(dz + off), v = *(const Vec16<T>*)(y + off), q = *(const Vec16<T>*)(r + roff);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float yv = v.get(e), qv = q.get(e);
                    const float du = add_relu_u<FORM2>(yv, sc[e], sh[e], qv, scd[e], shd[e]) > 0.f ? g.get(e) : 0.f;
                    s1[e] += du;
                    s2[e] += du * (yv - mu[e]) * rs[e];
                    if (FORM2) s3[e] += du * (qv - mud[e]) * rsd[e];
                }
            }
        }
        if (active) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                red[(0 * cm.rpi + py) * ncolE + cx * EPC + e] = s1[e];
                red[(1 * cm.rpi + py) * ncolE + cx * EPC + e] = s2[e];
                if (FORM2) red[(2 * cm.rpi + py) * ncolE + cx * EPC + e] = s3[e];
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < NS * ncolE; i += 256) {
            const int which = i / ncolE, j = i - which * ncolE, c = pb * EPC + j;
            if (c >= C) continue;
            float s = 0.f;
            for (int k = 0; k < cm.rpi; ++k) s += red[(which * cm.rpi + k) * ncolE + j];
            if (which == 0) {
                part[((int64_t)blockIdx.x * 2 + 0) * C + c] = s;
                if (FORM2) part_d[((int64_t)blockIdx.x * 2 + 0) * C + c] = s;
            } else if (which == 1) {
                part[((int64_t)blockIdx.x * 2 + 1) * C + c] = s;
            } else {
                part_d[((int64_t)blockIdx.x * 2 + 1) * C + c] = s;
            }
        }
        __syncthreads();
    }
}

// coefficients of dY = a * dU + k1 * x + k2 of one channel (k1 = coefB * rstd, k2 = coefC - k1 * mean; coef = fva_bn_bwd_finalize's
// table).  fp32 tensors form the three-term sum in double and round once, as bn_act.hip's ReLU pass does; bf16 tensors in fp32.
struct KofF {
    float a, k1, k2;
};
struct KofD {
    double a, k1, k2;
};
template <typename T>
using Kof = typename std::conditional<std::is_same<T, float>::value, KofD, KofF>::type;
template <typename T>
__device__ __forceinline__ Kof<T> kof_pack(float a, float mean, float rstd, float coef_b, float coef_c) {
    Kof<T> k;
    if constexpr (std::is_same<T, float>::value) {
        k.a = (double)a;
        k.k1 = (double)coef_b * (double)rstd;
        k.k2 = (double)coef_c - k.k1 * (double)mean;
    } else {
        const BnBwdK p = bn_bwd_pack_coef(a, 0.f, mean, rstd, coef_b, coef_c);
        k.a = p.a; k.k1 = p.k1; k.k2 = p.k2;
    }
    return k;
}
template <typename K>
__device__ __forceinline__ float kof_dy(const K& k, float du, float x) {
    using F = decltype(k.a);
    return (float)(k.a * (F)du + (k.k1 * (F)x + k.k2));
}

// backward pass 2: one block per padded row of dy (and dy_d: the same geometry); the interior rows also write dr (dense) in form 1
template <typename T, bool FORM2>
__global__ __launch_bounds__(256) void bn_add_relu_bwd_apply_kernel(const T* __restrict__ dz, const T* __restrict__ y, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, const float* __restrict__ coef,
                                                                    const T* __restrict__ r, int r_pad, const float* __restrict__ scale_d,
                                                                    const float* __restrict__ shift_d, const float* __restrict__ mean_d,
                                                                    const float* __restrict__ rstd_d, const float* __restrict__ coef_d,
                                                                    T* __restrict__ dy, T* __restrict__ dy_d, int dy_pad, T* __restrict__ dr, int H, int W,
                                                                    int C) {
    constexpr int EPC = Vec16<T>::N;
    const ColMap cm = col_map(C / EPC);
    const int Hp = H + 2 * dy_pad, Wp = W + 2 * dy_pad;
    const int b = blockIdx.x / Hp, yy = blockIdx.x - b * Hp - dy_pad;
    const bool row_in = yy >= 0 && yy < H;
    const int py = threadIdx.x / cm.ncol, cx = threadIdx.x - py * cm.ncol;
    if (py >= cm.rpi) return;                     // (no barrier in this kernel)
    const int64_t orow = (int64_t)blockIdx.x * Wp * C;
    const int64_t m0 = row_in ? ((int64_t)b * H + yy) * W : 0;           // the dense operands' row
    const T* rrow = row_in ? second_row<T, FORM2>(r, r_pad, b, yy, H, W, C) : r;
    for (int cc = cx; cc < cm.cpp; cc += cm.ncol) {
        float sc[EPC], sh[EPC], scd[EPC], shd[EPC];
        Kof<T> k[EPC], kd[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int c = cc * EPC + e;
            sc[e] = scale[c]; sh[e] = shift[c];
            k[e] = kof_pack<T>(coef[c], mean[c], rstd[c], coef[C + c], coef[2 * C + c]);
            if (FORM2) {
                scd[e] = scale_d[c]; shd[e] = shift_d[c];
                kd[e] = kof_pack<T>(coef_d[c], mean_d[c], rstd_d[c], coef_d[C + c], coef_d[2 * C + c]);
            } else {
                scd[e] = shd[e] = 0.f;
                kd[e] = k[e];
            }
        }
        for (int xp = py; xp < Wp; xp += cm.rpi) {
            const int xx = xp - dy_pad;
            Vec16<T> o = zero_vec<T>(), od = zero_vec<T>();
            if (row_in && xx >= 0 && xx < W) {
                const int64_t off = (m0 + xx) * C + cc * EPC;
                const Vec16<T> g = *(const Vec16<T>*)(dz + off), v = *(const Vec16<T>*)(y + off), q = *(const Vec16<T>*)(rrow + (int64_t)xx * C + cc * EPC);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float yv = v.get(e), qv = q.get(e);
                    const float du = add_relu_u<FORM2>(yv, sc[e], sh[e], qv, scd[e], shd[e]) > 0.f ? g.get(e) : 0.f;
                    o.set(e, kof_dy(k[e], du, yv));
                    od.set(e, FORM2 ? kof_dy(kd[e], du, qv) : du);
                }
                if (!FORM2) *(Vec16<T>*)(dr + off) = od;
            }
            *(Vec16<T>*)(dy + orow + (int64_t)xp * C + cc * EPC) = o;
            if (FORM2) *(Vec16<T>*)(dy_d + orow + (int64_t)xp * C + cc * EPC) = od;
        }
    }
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------------
int chan_check(const char* who, int dtype, int C) {
    if (dtype != FVA_F32 && dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "%s: bad dtype %d", who, dtype);
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    if (C <= 0 || C % epc || C > MAX_C) return fva_fail(FVA_ERR_ARG, "%s: C = %d must be a multiple of %d up to %d", who, C, epc, MAX_C);
    return FVA_OK;
}
// B, H, W positive, the pads 0 or 1, and every padded tensor below 2^31 16-byte chunks' worth of rows times pixels (block indices are int)
int shape_check(const char* who, int B, int H, int W, int C, int pad_a, int pad_b) {
    if (B <= 0 || H <= 0 || W <= 0) return fva_fail(FVA_ERR_ARG, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    if (pad_a < 0 || pad_a > 1 || pad_b < 0 || pad_b > 1) return fva_fail(FVA_ERR_ARG, "%s: a border must be 0 or 1", who);
    if ((int64_t)B * (H + 2) * (W + 2) * C >= (1ll << 31)) return fva_fail(FVA_ERR_ARG, "%s: tensor too large", who);
    return FVA_OK;
}
template <typename F>
void by_type(int dtype, F&& f) {
    if (dtype == FVA_BF16) f(bf16_t());
    else f(float());
}
int reduce_rows_per_block(int64_t M, int cpp) {
    const int rpi = col_map(cpp).rpi;
    int64_t rows = (M + 2047) / 2048;           // at most 2048 blocks
    if (rows < (int64_t)rpi * 8) rows = (int64_t)rpi * 8;
    return (int)((rows + rpi - 1) / rpi * rpi);
}
// exactly one second operand: the identity r (form 1) or y_d with its coefficients (form 2)
int form_check(const char* who, const void* r, const void* y_d, bool& form2) {
    if ((r != nullptr) == (y_d != nullptr)) return fva_fail(FVA_ERR_ARG, "%s: exactly one of r (the identity) and y_d (the shortcut's output) must be given", who);
    form2 = y_d != nullptr;
    return FVA_OK;
}

}  // namespace

extern "C" {

// whole 128-byte k-tiles of the implicit GEMM that reduces over P: 32 columns in fp32, 64 in bf16
int32_t fva_stem7_kp(int dtype, int Cin) {
    if ((dtype != FVA_F32 && dtype != FVA_BF16) || Cin <= 0 || Cin > 1024) return 0;
    const int bk = dtype == FVA_BF16 ? 64 : 32;
    return (Cin * 49 + bk - 1) / bk * bk;
}

int fva_stem7_patches(int dtype, const float* x, void* P, int B, int Cin, int H, int W, void* stream) {
    if (dtype != FVA_F32 && dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "fva_stem7_patches: bad dtype %d", dtype);
    if (!x || !P || B <= 0 || H <= 0 || W <= 0 || fva_stem7_kp(dtype, Cin) == 0) return fva_fail(FVA_ERR_ARG, "fva_stem7_patches: bad argument");
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, Kp = fva_stem7_kp(dtype, Cin), epc = dtype == FVA_BF16 ? 8 : 4;
    if ((int64_t)B * Cin * H * W >= (1ll << 31) || (int64_t)B * OH * OW >= (1ll << 31)) return fva_fail(FVA_ERR_ARG, "fva_stem7_patches: tensor too large");
    const int64_t total = (int64_t)B * OH * OW * (Kp / epc);
    int64_t grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    by_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(stem7_patches_kernel<T>, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, x, (T*)P, Cin, H, W, OH, OW, Kp, total);
    });
    FVA_LAUNCH_CHECK("stem7_patches_kernel");
    return FVA_OK;
}

int fva_maxpool3s2_fwd(int dtype, const void* x, int x_pad, void* out, int out_pad, int B, int H, int W, int C, void* stream) {
    int rc = chan_check("fva_maxpool3s2_fwd", dtype, C);
    if (rc || (rc = shape_check("fva_maxpool3s2_fwd", B, H, W, C, x_pad, out_pad))) return rc;
    if (!x || !out) return fva_fail(FVA_ERR_ARG, "fva_maxpool3s2_fwd: null pointer");
    const int OH = (H - 1) / 2 + 1;
    by_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(maxpool3s2_fwd_kernel<T>, dim3(B * (OH + 2 * out_pad)), dim3(256), 0, (hipStream_t)stream, (const T*)x, x_pad, (T*)out, out_pad,
                           H, W, C);
    });
    FVA_LAUNCH_CHECK("maxpool3s2_fwd_kernel");
    return FVA_OK;
}

int fva_maxpool3s2_bwd(int dtype, const void* dz, const void* x, int x_pad, void* dx, int B, int H, int W, int C, void* stream) {
    int rc = chan_check("fva_maxpool3s2_bwd", dtype, C);
    if (rc || (rc = shape_check("fva_maxpool3s2_bwd", B, H, W, C, x_pad, 0))) return rc;
    if (!dz || !x || !dx) return fva_fail(FVA_ERR_ARG, "fva_maxpool3s2_bwd: null pointer");
    by_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(maxpool3s2_bwd_kernel<T>, dim3(B * H), dim3(256), 0, (hipStream_t)stream, (const T*)dz, (const T*)x, x_pad, (T*)dx, H, W, C);
    });
    FVA_LAUNCH_CHECK("maxpool3s2_bwd_kernel");
    return FVA_OK;
}

int fva_subsample2_fwd(int dtype, const void* x, int x_pad, void* xs, int B, int H, int W, int C, void* stream) {
    int rc = chan_check("fva_subsample2_fwd", dtype, C);
    if (rc || (rc = shape_check("fva_subsample2_fwd", B, H, W, C, x_pad, 0))) return rc;
    if (!x || !xs) return fva_fail(FVA_ERR_ARG, "fva_subsample2_fwd: null pointer");
    if ((H | W) & 1) return fva_fail(FVA_ERR_ARG, "fva_subsample2_fwd: H = %d and W = %d must be even", H, W);
    by_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(subsample2_fwd_kernel<T>, dim3(B * (H / 2)), dim3(256), 0, (hipStream_t)stream, (const T*)x, x_pad, (T*)xs, H, W, C);
    });
    FVA_LAUNCH_CHECK("subsample2_fwd_kernel");
    return FVA_OK;
}

int fva_subsample2_bwd(int dtype, const void* dxs, void* dx, int B, int H, int W, int C, void* stream) {
    int rc = chan_check("fva_subsample2_bwd", dtype, C);
    if (rc || (rc = shape_check("fva_subsample2_bwd", B, H, W, C, 0, 0))) return rc;
    if (!dxs || !dx) return fva_fail(FVA_ERR_ARG, "fva_subsample2_bwd: null pointer");
    if ((H | W) & 1) return fva_fail(FVA_ERR_ARG, "fva_subsample2_bwd: H = %d and W = %d must be even", H, W);
    by_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(subsample2_bwd_kernel<T>, dim3(B * H), dim3(256), 0, (hipStream_t)stream, (const T*)dxs, (T*)dx, H, W, C);
    });
    FVA_LAUNCH_CHECK("subsample2_bwd_kernel");
    return FVA_OK;
}

int fva_bn_add_relu_apply(int dtype, const void* y, const float* scale, const float* shift, const void* r, int r_pad, const void* y_d,
                          const float* scale_d, const float* shift_d, void* z, int z_pad, int B, int H, int W, int C, void* stream) {
    const char* who = "fva_bn_add_relu_apply";
    bool form2 = false;
    int rc = chan_check(who, dtype, C);
    if (rc || (rc = shape_check(who, B, H, W, C, r_pad, z_pad)) || (rc = form_check(who, r, y_d, form2))) return rc;
    if (!y || !scale || !shift || !z || (form2 && (!scale_d || !shift_d))) return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    const dim3 grid(B * (H + 2 * z_pad));
    by_type(dtype, [&](auto t) {
        using T = decltype(t);
        if (form2)
            hipLaunchKernelGGL((bn_add_relu_apply_kernel<T, true>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)y, scale, shift, (const T*)y_d, 0,
                               scale_d, shift_d, (T*)z, z_pad, H, W, C);
        else
            hipLaunchKernelGGL((bn_add_relu_apply_kernel<T, false>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)y, scale, shift, (const T*)r, r_pad,
                               scale_d, shift_d, (T*)z, z_pad, H, W, C);
    });
    FVA_LAUNCH_CHECK("bn_add_relu_apply_kernel");
    return FVA_OK;
}

int32_t fva_bn_add_relu_bwd_blocks(int dtype, int64_t M, int C) {
    if ((dtype != FVA_F32 && dtype != FVA_BF16) || M <= 0) return 0;
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    if (C <= 0 || C % epc || C > MAX_C) return 0;
    return cdiv(M, reduce_rows_per_block(M, C / epc));
}

int fva_bn_add_relu_bwd_reduce(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                               const float* save_rstd, const void* r, int r_pad, const void* y_d, const float* scale_d, const float* shift_d,
                               const float* save_mean_d, const float* save_rstd_d, float* partial, float* partial_d, int32_t nblocks, int B, int H,
                               int W, int C, void* stream) {
    const char* who = "fva_bn_add_relu_bwd_reduce";
    bool form2 = false;
    int rc = chan_check(who, dtype, C);
    if (rc || (rc = shape_check(who, B, H, W, C, r_pad, 0)) || (rc = form_check(who, r, y_d, form2))) return rc;
    if (!dz || !y || !scale || !shift || !save_mean || !save_rstd || !partial ||
        (form2 && (!scale_d || !shift_d || !save_mean_d || !save_rstd_d || !partial_d)))
        return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    const int64_t M = (int64_t)B * H * W;
    const int rows = reduce_rows_per_block(M, C / epc);
    if (nblocks != cdiv(M, rows)) return fva_fail(FVA_ERR_ARG, "%s: nblocks %d != fva_bn_add_relu_bwd_blocks() = %d", who, nblocks, cdiv(M, rows));
    const ColMap cm = col_map(C / epc);
    const int smem = (form2 ? 3 : 2) * cm.rpi * cm.ncol * epc * 4;
    by_type(dtype, [&](auto t) {
        using T = decltype(t);
        if (form2)
            hipLaunchKernelGGL((bn_add_relu_bwd_reduce_kernel<T, true>), dim3(nblocks), dim3(256), smem, (hipStream_t)stream, (const T*)dz, (const T*)y, scale,
                               shift, save_mean, save_rstd, (const T*)y_d, 0, scale_d, shift_d, save_mean_d, save_rstd_d, partial, partial_d, M, H, W, C,
                               rows);
        else
            hipLaunchKernelGGL((bn_add_relu_bwd_reduce_kernel<T, false>), dim3(nblocks), dim3(256), smem, (hipStream_t)stream, (const T*)dz, (const T*)y, scale,
                               shift, save_mean, save_rstd, (const T*)r, r_pad, scale_d, shift_d, save_mean_d, save_rstd_d, partial, partial_d, M, H, W, C,
                               rows);
    });
    FVA_LAUNCH_CHECK("bn_add_relu_bwd_reduce_kernel");
    return FVA_OK;
}

int fva_bn_add_relu_bwd_apply(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                              const float* save_rstd, const float* coef, const void* r, int r_pad, const void* y_d, const float* scale_d,
                              const float* shift_d, const float* save_mean_d, const float* save_rstd_d, const float* coef_d, void* dy, void* dy_d,
                              int dy_pad, void* dr, int B, int H, int W, int C, void* stream) {
    const char* who = "fva_bn_add_relu_bwd_apply";
    bool form2 = false;
    int rc = chan_check(who, dtype, C);
    if (rc || (rc = shape_check(who, B, H, W, C, r_pad, dy_pad)) || (rc = form_check(who, r, y_d, form2))) return rc;
    if (!dz || !y || !scale || !shift || !save_mean || !save_rstd || !coef || !dy || (!form2 && !dr) ||
        (form2 && (!scale_d || !shift_d || !save_mean_d || !save_rstd_d || !coef_d || !dy_d)))
        return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    const dim3 grid(B * (H + 2 * dy_pad));
    by_type(dtype, [&](auto t) {
        using T = decltype(t);
        if (form2)
            hipLaunchKernelGGL((bn_add_relu_bwd_apply_kernel<T, true>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)dz, (const T*)y, scale, shift,
                               save_mean, save_rstd, coef, (const T*)y_d, 0, scale_d, shift_d, save_mean_d, save_rstd_d, coef_d, (T*)dy, (T*)dy_d, dy_pad,
                               (T*)nullptr, H, W, C);
        else
            hipLaunchKernelGGL((bn_add_relu_bwd_apply_kernel<T, false>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)dz, (const T*)y, scale, shift,
                               save_mean, save_rstd, coef, (const T*)r, r_pad, scale_d, shift_d, save_mean_d, save_rstd_d, coef_d, (T*)dy, (T*)nullptr,
                               dy_pad, (T*)dr, H, W, C);
    });
    FVA_LAUNCH_CHECK("bn_add_relu_bwd_apply_kernel");
    return FVA_OK;
}

}  // extern "C"
