// BatchNorm2d (train/eval) + activation (SiLU with an optional residual add, or ReLU) forward and backward, and the FPN upsample/concat
// and layout helpers, for gfx950.  All of these are HBM-bound streaming kernels: 16 bytes per lane, channels
// contiguous (NHWC), no LDS except for the per-block channel reductions.
//
// Algorithmic bytes per element (bf16): apply = 2 (y) + 2 (z) [+2 residual]; backward pass 1 = 4 (dz, y);
// backward pass 2 = 4 + 2 (dy); frozen statistics: ONE backward pass = 4 + 2.
//
// Replaces nn.BatchNorm2d / nn.SiLU / `identity + conv2` (reference classfication/models/darknet53.py:11-17,
// 28-31, 58-62), Conv2d(bias) -> BatchNorm2d -> ReLU (classfication/models/vgg.py:39-48) and nn.Upsample + torch.cat
// (detection/neck/yolov3neck.py:71,105,110).
#include <type_traits>

#include "common.h"

namespace {


// ---------------------------------------------------------------------------------------------------------
// forward statistics -> coefficients.  Block = 16 channels x 64 partial-row groups (1024 threads): the partial
// table [nblocks][2][C] is summed with 4 independent loads in flight per thread, then in double across groups.
constexpr int FIN_G = 64;
__device__ __forceinline__ void reduce_partials(const float* __restrict__ part, int nblocks, int C, int c, int ry, double& s1,
                                                double& s2) {
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    int b = ry;
    for (; b + FIN_G < nblocks; b += 2 * FIN_G) {
        const float p0 = part[((int64_t)b * 2 + 0) * C + c], q0 = part[((int64_t)b * 2 + 1) * C + c];
        const float p1 = part[((int64_t)(b + FIN_G) * 2 + 0) * C + c], q1 = part[((int64_t)(b + FIN_G) * 2 + 1) * C + c];
        a0 += p0; b0 += q0; a1 += p1; b1 += q1;
    }
    if (b < nblocks) { a0 += part[((int64_t)b * 2 + 0) * C + c]; b0 += part[((int64_t)b * 2 + 1) * C + c]; }
    s1 = (double)a0 + (double)a1;
    s2 = (double)b0 + (double)b1;
}
// Layers with many row blocks (the 640^2 / 320^2 maps: up to 51200 partial rows for 2-4 channel groups) first fold
// chunks of PRE_ROWS rows in parallel into doubles kept in the tail of the same table (rows nblocks .. of
// fva_bn_partial_rows()): tail[(r * 2 + which) * C + c].  Fixed order everywhere: deterministic.
constexpr int PRE_ROWS = 256, PRE_MIN = 1024;
__global__ __launch_bounds__(1024) void bn_prereduce_kernel(const float* __restrict__ part, int nblocks, int C, double* __restrict__ tail) {
    __shared__ double red[2][FIN_G][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cx;
    const int r0 = blockIdx.y * PRE_ROWS;
    const int n = nblocks - r0 < PRE_ROWS ? nblocks - r0 : PRE_ROWS;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) reduce_partials(part + (int64_t)r0 * 2 * C, n, C, c, ry, s1, s2);
    red[0][ry][cx] = s1;
    red[1][ry][cx] = s2;
    __syncthreads();
    if (ry < 2 && c < C) {
        double s = 0.0;
        for (int k = 0; k < FIN_G; ++k) s += red[ry][k][cx];
        tail[((int64_t)blockIdx.y * 2 + ry) * C + c] = s;
    }
}

__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ part, int nblocks, double count, int C,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* running_mean, float* running_var, int64_t* nbt,
                                                           float momentum, float eps, float* save_mean, float* save_rstd,
                                                           float* scale, float* shift, const double* __restrict__ pre, int pre_rows) {
    __shared__ double red[2][FIN_G][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cx;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        if (pre_rows > 0) {  // pre-reduced doubles
            for (int r = ry; r < pre_rows; r += FIN_G) {
                s1 += pre[((int64_t)r * 2 + 0) * C + c];
                s2 += pre[((int64_t)r * 2 + 1) * C + c];
            }
        } else {
            reduce_partials(part, nblocks, C, c, ry, s1, s2);
        }
    }
    red[0][ry][cx] = s1;
    red[1][ry][cx] = s2;
    __syncthreads();
    if (ry == 0 && c < C) {
        s1 = s2 = 0.0;
        for (int k = 0; k < FIN_G; ++k) {
            s1 += red[0][k][cx];
            s2 += red[1][k][cx];
        }
        const BnN n = bn_n(count);
        const BnFwdCoef k = bn_fwd_coef(s1, s2, n, gamma[c], beta[c], eps);
        save_mean[c] = k.mean;
        save_rstd[c] = k.rstd;
        scale[c] = k.scale;
        shift[c] = k.shift;
        if (running_mean) bn_running_update(running_mean, running_var, c, k, n, momentum);
    }
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
}

__global__ void bn_eval_coeffs_kernel(int C, const float* gamma, const float* beta, const float* rm, const float* rv,
                                      float eps, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        const float sc = gamma[c] / sqrtf(rv[c] + eps);
        scale[c] = sc;
        shift[c] = beta[c] - rm[c] * sc;
    }
}

struct HaloIdx {
    int B, H, W, C, pad, Hp, Wp, cpp;  // cpp = 16-B chunks per pixel
    FastDiv div_cpp, div_wp, div_img;
    int64_t total;  // chunks over the padded buffer
};
HaloIdx make_halo(int B, int H, int W, int C, int pad, int epc) {
    HaloIdx h;
    h.B = B; h.H = H; h.W = W; h.C = C; h.pad = pad;
    h.Hp = H + 2 * pad; h.Wp = W + 2 * pad; h.cpp = C / epc;
    h.div_cpp = make_fastdiv(h.cpp);
    h.div_wp = make_fastdiv(h.Wp);
    h.div_img = make_fastdiv(h.Hp * h.Wp);
    h.total = (int64_t)B * h.Hp * h.Wp * h.cpp;
    return h;
}
// decode a chunk index of the padded buffer; returns false on the zero border
__device__ __forceinline__ bool halo_decode(const HaloIdx& h, uint32_t idx, int& b, int& y, int& x, int& cc) {
    const uint32_t pix = fd_div(idx, h.div_cpp);
    cc = idx - pix * h.cpp;
    b = fd_div(pix, h.div_img);
    const uint32_t rem = pix - (uint32_t)b * (h.Hp * h.Wp);
    const uint32_t yp = fd_div(rem, h.div_wp);
    const uint32_t xp = rem - yp * h.Wp;
    y = (int)yp - h.pad;
    x = (int)xp - h.pad;
    return y >= 0 && y < h.H && x >= 0 && x < h.W;
}

// The apply passes read their dense inputs (y; dz and y) for the last time before those tensors go cold; read non-temporal they leave
// the caches to what the pass WRITES, which the next convolution launches read.  Same-box A/B (bench.py, two runs each): 1053.6 / 1057.3
// against 1048.4 / 1046.4 img/s.  -DFVA_NT_BN=0 switches back; -DFVA_NT_RES=1 also reads the residual that way (measured neutral, as were
// non-temporal slab reads in the split-K reduce).
#ifndef FVA_NT_BN
#define FVA_NT_BN 1
#endif
#ifndef FVA_NT_RES
#define FVA_NT_RES 0
#endif
template <typename T>
__device__ __forceinline__ Vec16<T> ld_last(const T* p) {
#if FVA_NT_BN
    Vec16<T> r;
    const u32x4 raw = __builtin_nontemporal_load((const u32x4*)p);
    __builtin_memcpy(&r, &raw, 16);
    return r;
#else
    return *(const Vec16<T>*)p;
#endif
}

// One block per row of the padded output buffer (blockIdx.x = b * Hp + yp): no index division per chunk.  A thread keeps U chunks
// in flight per step (all loads of a step are issued before the first is used; masked chunks read a clamped address and store
// zeros -- no branch around a load): at one chunk per step the passes ran 4.3 (backward) - 5.6 TB/s, latency- not bandwidth-bound
// (PMC: 78 % of the wave cycles waiting, 10 % issuing).
#ifndef FVA_BN_UNROLL
#define FVA_BN_UNROLL 2      // measured 1 / 2 / 4 (tools/bench_bn.py, sum over the layer shapes): fwd 348 / 337 / 340 us, bwd 514 / 506 / 504 us
#endif
// FIN: the batch statistics arrive as fixed-point accumulators that the producing convolution's tiles added to (common.h fx_*); every
// block finalises ALL channels once in its prologue, through LDS (the arithmetic of bn_finalize_kernel, so all blocks agree to the bit),
// block 0 also writes mean / rstd / scale / shift for the backward pass, updates the running statistics and returns the layer's OTHER
// accumulator to zero (`zero`: the one this launch reads is still being read by its other blocks).  No finalize launch.
struct BnFwdAcc {
    long long* acc;          // [replicas][FX_WORDS][C]: the sums the producers added
    long long* zero;         // may be null: another accumulator of the same size that this launch returns to zero (the layer's other direction)
    int replicas;
    const float *gamma, *beta;
    float *running_mean, *running_var;
    long long* nbt;
    float momentum, eps;
    BnN n;
    float *save_mean, *save_rstd, *scale, *shift;
};
struct BnBwdAcc {
    long long* acc;          // sums of dU and dU * xhat
    long long* zero;
    int replicas;
    const float *gamma, *rstd, *mean, *shift;
    float *dgamma, *dbeta;
    int accumulate;
    BnN n;
};
// the accumulator finalised by a launch of its own: for consumers that cannot do it in their prologue (the thin fused 1x1 tile, foreign code)
__global__ __launch_bounds__(256) void bn_acc_finalize_kernel(const BnFwdAcc fin, int C) {     // ONE block; dynamic LDS: FX_WORDS * C int64
    extern __shared__ long long fx_words[];
    fx_gather_lds(fin.acc, C, fin.replicas, fx_words, threadIdx.x, 256);
    for (int c = threadIdx.x; c < C; c += 256) {
        double s1, s2;
        fx_value2(fx_from_lds(fx_words, C, c), s1, s2);
        const BnFwdCoef k = bn_fwd_coef(s1, s2, fin.n, fin.gamma[c], fin.beta[c], fin.eps);
        fin.save_mean[c] = k.mean; fin.save_rstd[c] = k.rstd; fin.scale[c] = k.scale; fin.shift[c] = k.shift;
        if (fin.running_mean) bn_running_update(fin.running_mean, fin.running_var, c, k, fin.n, fin.momentum);
    }
    fx_zero(fin.acc, C, fin.replicas, threadIdx.x, 256);          // nobody else reads it: this launch is the only consumer
    fx_zero(fin.zero, C, fin.replicas, threadIdx.x, 256);
    if (threadIdx.x == 0 && fin.nbt) *fin.nbt += 1;
}

// The activation behind the BatchNorm is a compile-time policy of the three streaming passes (apply, backward reduce, backward apply): one
// kernel per pass, instantiated for SiLU (Darknet-53 / YOLOv3; plain and accumulator forms, with a residual) and for ReLU (the VGG `_bn`
// classifiers, reference classfication/models/vgg.py:39-48; plain table form only).  A policy gives
//   fwd(y, sc, sh)       z from one element of the convolution output
//   du(dz, y, sc, sh)    dU = dz * act'(u) for the reduce pass; u = y * sc + sh is recomputed from y in both backward passes (the stored z
//                        is rounded: z == 0 and u > 0 can disagree)
//   Coef<T>, pack<T>, dy the per-channel coefficients of the backward apply pass and dY = a * dU + k1 * y + k2 formed from them
struct ActSiLU {
    template <typename T> using Coef = BnBwdK;
    static __device__ __forceinline__ float fwd(float y, float sc, float sh) { return bn_silu_fwd_elem(y, sc, sh); }
    static __device__ __forceinline__ float du(float dz, float y, float sc, float sh) { return dz * silu_grad(y * sc + sh); }
    template <typename T>
    static __device__ __forceinline__ BnBwdK pack(float a, float shift, float mean, float rstd, float coef_b, float coef_c) {
        return bn_bwd_pack_coef(a, shift, mean, rstd, coef_b, coef_c);
    }
    static __device__ __forceinline__ float dy(float dz, float y, float sc, const BnBwdK& k) { return bn_bwd_apply_elem(dz, y, sc, k.sh, k.a, k.k1, k.k2); }
};
// fp32 tensors: ReLU's three-term sum is formed in double and rounded ONCE (k1 = cb * rstd and k2 = cc - k1 * mean rounded to fp32 first
// would each leave 2^-24 of a term that may be larger than the result; v_fma_f64 runs at half the fp32 rate on this chip and the pass
// is HBM-bound).  bf16 tensors: fp32 arithmetic, the store's 2^-9 is the error.
struct BnBwdKd {
    float sh;
    double a, k1, k2;
};
struct ActReLU {
    template <typename T> using Coef = typename std::conditional<std::is_same<T, float>::value, BnBwdKd, BnBwdK>::type;
    static __device__ __forceinline__ float fwd(float y, float sc, float sh) {
        const float u = __builtin_fmaf(y, sc, sh);
        return u <= 0.f ? 0.f : u;       // a NaN stays a NaN, as in torch.relu
    }
    static __device__ __forceinline__ float du(float dz, float y, float sc, float sh) { return __builtin_fmaf(y, sc, sh) > 0.f ? dz : 0.f; }
    template <typename T>
    static __device__ __forceinline__ Coef<T> pack(float a, float shift, float mean, float rstd, float coef_b, float coef_c) {
        if constexpr (std::is_same<T, float>::value) {
            BnBwdKd k;
            k.sh = shift;
            k.a = (double)a;
            k.k1 = (double)coef_b * (double)rstd;
            k.k2 = (double)coef_c - k.k1 * (double)mean;
            return k;
        } else {
            return bn_bwd_pack_coef(a, shift, mean, rstd, coef_b, coef_c);
        }
    }
    template <typename K>
    static __device__ __forceinline__ float dy(float dz, float y, float sc, const K& k) {
        using F = decltype(k.a);
        return (float)(k.a * (F)du(dz, y, sc, k.sh) + (k.k1 * (F)y + k.k2));
    }
};

// One padded row of z per block and step (grid = rows for the plain form; the accumulator form runs at most 2048 blocks that walk the rows,
// so that its prologue is paid once per block).  FIN: scale / shift come from the layer's accumulator -- all C channels once per block,
// C / 256 per thread, through LDS (dynamic: 2 C floats), while the first row's loads are already in flight; block 0 also writes them out
// for the backward pass, updates the running statistics and returns the OTHER direction's accumulator to zero (its own one is still being
// read by the other blocks: the layer's backward pass zeroes that).
template <typename Act, typename T, bool FIN>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ y, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const T* __restrict__ res,
                                                       int res_pad, T* __restrict__ z, const HaloIdx h, const BnFwdAcc fin, int nrows) {
    constexpr int EPC = Vec16<T>::N, U = FVA_BN_UNROLL;
    extern __shared__ float fx_tab[];          // FIN: [2][C]
    const int row_chunks = h.Wp * h.cpp;
    const int cmask = h.cpp - 1, cshift = 31 - __builtin_clz(h.cpp);  // cpp is a power of two (BN channel counts)
    // cpp divides 256, so a lane keeps the same channel chunk for the whole row: its coefficients live in registers
    const int cc = threadIdx.x & cmask;
    const int rW = h.W + 2 * res_pad;
    const bool has_res = res != nullptr;
    Vec16<T> v[U], r[U];
    bool ok[U];
    const T *yrow = nullptr, *rrow = nullptr;
    auto set_row = [&](int row) -> bool {       // false: a border row
        const int b = row / h.Hp, yy = row - b * h.Hp - h.pad;
        if (yy < 0 || yy >= h.H) return false;
        yrow = y + ((int64_t)b * h.H + yy) * h.W * h.C;
        rrow = has_res ? res + (((int64_t)b * (h.H + 2 * res_pad) + yy + res_pad) * rW + res_pad) * h.C : nullptr;
        return true;
    };
    auto load = [&](int i0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            const int xx = (i >> cshift) - h.pad;
            ok[u] = i < row_chunks && xx >= 0 && xx < h.W;
            const int64_t off = (int64_t)(ok[u] ? xx : 0) * h.C + cc * EPC;
            v[u] = ld_last<T>(yrow + off);
            if (has_res) {
#if FVA_NT_RES
                r[u] = ld_last<T>(rrow + off);
#else
                r[u] = *(const Vec16<T>*)(rrow + off);
#endif
            }
        }
    };
    int row = blockIdx.x;
    bool row_in = row < nrows && set_row(row);
    if (FIN && row_in && (int)threadIdx.x < row_chunks) load(threadIdx.x);
    float sc[EPC], sh[EPC];
    if constexpr (FIN) {
        const bool writer = blockIdx.x == 0;
        long long* fx_words = (long long*)(fx_tab + 2 * h.C);      // replicas > 1: [FX_WORDS][C] behind the table
        if (fin.replicas > 1) fx_gather_lds(fin.acc, h.C, fin.replicas, fx_words, threadIdx.x, 256);
        for (int c = threadIdx.x; c < h.C; c += 256) {
            double s1, s2;
            if (fin.replicas > 1) fx_value2(fx_from_lds(fx_words, h.C, c), s1, s2);
            else fx_load2(fin.acc, h.C, 1, c, s1, s2);
            const BnFwdCoef k = bn_fwd_coef(s1, s2, fin.n, fin.gamma[c], fin.beta[c], fin.eps);
            fx_tab[c] = k.scale;
            fx_tab[h.C + c] = k.shift;
            if (writer) {
                fin.save_mean[c] = k.mean; fin.save_rstd[c] = k.rstd; fin.scale[c] = k.scale; fin.shift[c] = k.shift;
                if (fin.running_mean) bn_running_update(fin.running_mean, fin.running_var, c, k, fin.n, fin.momentum);
            }
        }
        if (writer) {
            if (threadIdx.x == 0 && fin.nbt) *fin.nbt += 1;
            fx_zero(fin.zero, h.C, fin.replicas, threadIdx.x, 256);
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            sc[e] = fx_tab[cc * EPC + e];
            sh[e] = fx_tab[h.C + cc * EPC + e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            sc[e] = scale[cc * EPC + e];
            sh[e] = shift[cc * EPC + e];
        }
    }
    bool first = FIN;
    for (; row < nrows; row += gridDim.x, row_in = row < nrows && set_row(row)) {
        T* zrow = z + (int64_t)row * row_chunks * EPC;
        if (!row_in) {   // a border row: zeros (block-uniform branch)
            Vec16<T> zero;
#pragma unroll
            for (int e = 0; e < EPC; ++e) zero.set(e, 0.f);
            for (int i = threadIdx.x; i < row_chunks; i += 256) *(Vec16<T>*)(zrow + (int64_t)i * EPC) = zero;
            first = false;
            continue;
        }
        for (int i0 = threadIdx.x; i0 < row_chunks; i0 += 256 * U) {
            if (!first) load(i0);
            first = false;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * 256;
                Vec16<T> out;
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    float o = Act::fwd(v[u].get(e), sc[e], sh[e]);
                    if (has_res) o += r[u].get(e);
                    out.set(e, ok[u] ? o : 0.f);
                }
                if (i < row_chunks) *(Vec16<T>*)(zrow + (int64_t)i * EPC) = out;
            }
        }
    }
}

// backward pass 1: per-channel partial sums of dU and dU*xhat.  threads = (channel chunk, pixel row group)
template <typename Act, typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dz, const T* __restrict__ y,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            float* __restrict__ part, long long* acc, int replicas, int64_t M, int C, int rows_per_block) {
    constexpr int EPC = Vec16<T>::N;
    extern __shared__ float red[];  // [2][rpi][C]
    const int cpp = C / EPC, rpi = 256 / cpp;
    const int cx = threadIdx.x % cpp, py = threadIdx.x / cpp;
    float sc[EPC], sh[EPC], mu[EPC], rs[EPC], s1[EPC], s2[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const int c = cx * EPC + e;
        sc[e] = scale[c]; sh[e] = shift[c]; mu[e] = mean[c]; rs[e] = rstd[c];
        s1[e] = s2[e] = 0.f;
    }
    const int64_t m0 = (int64_t)blockIdx.x * rows_per_block;
    int64_t m1 = m0 + rows_per_block;
    if (m1 > M) m1 = M;
    for (int64_t m = m0 + py; m < m1; m += rpi) {
        const Vec16<T> g = *(const Vec16<T>*)(dz + m * C + cx * EPC);
        const Vec16<T> v = *(const Vec16<T>*)(y + m * C + cx * EPC);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const float yv = v.get(e);
            const float du = Act::du(g.get(e), yv, sc[e], sh[e]);
            s1[e] += du;
            s2[e] += du * (yv - mu[e]) * rs[e];
        }
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        red[(0 * rpi + py) * C + cx * EPC + e] = s1[e];
        red[(1 * rpi + py) * C + cx * EPC + e] = s2[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        const int which = i / C, c = i - which * C;
        float s = 0.f;
        for (int k = 0; k < rpi; ++k) s += red[(which * rpi + k) * C + c];
        if (acc != nullptr) fx_atomic_add(fx_replica(acc, C, replicas), C, which, c, s);
        else part[((int64_t)blockIdx.x * 2 + which) * C + c] = s;
    }
}

__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float* __restrict__ part, int nblocks, double count, int C,
                                                               const float* __restrict__ gamma, const float* __restrict__ rstd,
                                                               float* dgamma, float* dbeta, int accumulate, float* coef,
                                                               const double* __restrict__ pre, int pre_rows) {
    __shared__ double red[2][FIN_G][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cx;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        if (pre_rows > 0) {
            for (int r = ry; r < pre_rows; r += FIN_G) {
                s1 += pre[((int64_t)r * 2 + 0) * C + c];
                s2 += pre[((int64_t)r * 2 + 1) * C + c];
            }
        } else {
            reduce_partials(part, nblocks, C, c, ry, s1, s2);
        }
    }
    red[0][ry][cx] = s1;
    red[1][ry][cx] = s2;
    __syncthreads();
    if (ry == 0 && c < C) {
        s1 = s2 = 0.0;
        for (int k = 0; k < FIN_G; ++k) {
            s1 += red[0][k][cx];
            s2 += red[1][k][cx];
        }
        const BnBwdCoef k = bn_bwd_coef(s1, s2, bn_n(count), gamma[c], rstd[c]);
        dbeta[c] = accumulate ? dbeta[c] + k.dbeta : k.dbeta;
        dgamma[c] = accumulate ? dgamma[c] + k.dgamma : k.dgamma;
        coef[c] = k.a;
        coef[C + c] = k.cb;
        coef[2 * C + c] = k.cc;
    }
}

// FIN: dgamma, dbeta and the three coefficients come from the layer's backward accumulator (the sums the dgrad epilogues / the reduce
// pass added), all C channels once per block through LDS (dynamic: 5 C floats); block 0 writes dgamma / dbeta and returns the layer's
// FORWARD accumulator to zero (fin.zero) -- nobody reads that one any more; its own is zeroed by the layer's next forward pass.
template <typename Act, typename T, bool FIN>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dz, const T* __restrict__ y,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ coef, T* __restrict__ dy, const HaloIdx h, int nrows,
                                                           const BnBwdAcc fin) {
    constexpr int EPC = Vec16<T>::N, U = FVA_BN_UNROLL;
    extern __shared__ float fx_tab[];          // FIN: [5][C]
    const int row_chunks = h.Wp * h.cpp;
    const int cmask = h.cpp - 1, cshift = 31 - __builtin_clz(h.cpp);
    // lane-constant channel chunk (cpp divides 256): dY = a*dU + k1*y + k2 with k1 = coefB*rstd, k2 = coefC - k1*mean
    const int cc = threadIdx.x & cmask;
    using K = typename Act::template Coef<T>;
    static_assert(!FIN || std::is_same<K, BnBwdK>::value, "the accumulator form keeps its coefficients as floats in LDS");
    float sc[EPC];
    K k[EPC];
    Vec16<T> g[U], v[U];
    bool ok[U];
    int64_t m0 = 0;
    auto set_row = [&](int row) -> bool {       // false: a border row
        const int b = row / h.Hp, yy = row - b * h.Hp - h.pad;
        m0 = ((int64_t)b * h.H + yy) * h.W;
        return yy >= 0 && yy < h.H;
    };
    auto load = [&](int i0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            const int xx = (i >> cshift) - h.pad;
            ok[u] = i < row_chunks && xx >= 0 && xx < h.W;
            const int64_t off = (m0 + (ok[u] ? xx : 0)) * h.C + cc * EPC;
            g[u] = ld_last<T>(dz + off);
            v[u] = ld_last<T>(y + off);
        }
    };
    // FIN: the first row's operands are requested before the prologue and stay in flight across its (cold) accumulator reads
    bool first = FIN && (int)blockIdx.x < nrows && set_row(blockIdx.x) && (int)threadIdx.x < row_chunks;
    if (first) load(threadIdx.x);
    if constexpr (FIN) {
        const bool writer = blockIdx.x == 0;
        long long* fx_words = (long long*)(fx_tab + 5 * h.C + (h.C & 1));     // replicas > 1: [FX_WORDS][C] behind the table, 8-byte aligned
        if (fin.replicas > 1) fx_gather_lds(fin.acc, h.C, fin.replicas, fx_words, threadIdx.x, 256);
        for (int c = threadIdx.x; c < h.C; c += 256) {
            double s1, s2;
            if (fin.replicas > 1) fx_value2(fx_from_lds(fx_words, h.C, c), s1, s2);
            else fx_load2(fin.acc, h.C, 1, c, s1, s2);
            const BnBwdCoef q = bn_bwd_coef(s1, s2, fin.n, fin.gamma[c], rstd[c]);
            const BnBwdK p = bn_bwd_pack_coef(q.a, shift[c], mean[c], rstd[c], q.cb, q.cc);
            fx_tab[c] = scale[c];
            fx_tab[h.C + c] = p.sh;
            fx_tab[2 * h.C + c] = p.a;
            fx_tab[3 * h.C + c] = p.k1;
            fx_tab[4 * h.C + c] = p.k2;
            if (writer) {
                fin.dbeta[c] = fin.accumulate ? fin.dbeta[c] + q.dbeta : q.dbeta;
                fin.dgamma[c] = fin.accumulate ? fin.dgamma[c] + q.dgamma : q.dgamma;
            }
        }
        if (writer) fx_zero(fin.zero, h.C, fin.replicas, threadIdx.x, 256);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int c = cc * EPC + e;
            sc[e] = fx_tab[c]; k[e].sh = fx_tab[h.C + c]; k[e].a = fx_tab[2 * h.C + c]; k[e].k1 = fx_tab[3 * h.C + c]; k[e].k2 = fx_tab[4 * h.C + c];
        }
    } else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int c = cc * EPC + e;
            k[e] = Act::template pack<T>(coef[c], shift[c], mean[c], rstd[c], coef[h.C + c], coef[2 * h.C + c]);
            sc[e] = scale[c];
        }
    }
    // one padded row per block and step
    for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
        const bool row_in = set_row(row);
        T* orow = dy + (int64_t)row * row_chunks * EPC;
        if (!row_in) {
            Vec16<T> zero;
#pragma unroll
            for (int e = 0; e < EPC; ++e) zero.set(e, 0.f);
            for (int i = threadIdx.x; i < row_chunks; i += 256) *(Vec16<T>*)(orow + (int64_t)i * EPC) = zero;
            continue;
        }
        for (int i0 = threadIdx.x; i0 < row_chunks; i0 += 256 * U) {
            if (!first) load(i0);
            first = false;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * 256;
                Vec16<T> out;
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    out.set(e, ok[u] ? Act::dy(g[u].get(e), v[u].get(e), sc[e], k[e]) : 0.f);
                }
                if (i < row_chunks) *(Vec16<T>*)(orow + (int64_t)i * EPC) = out;
            }
        }
    }
}

// Frozen statistics (the BatchNorm in eval mode, its convolution and affine parameters still training): scale and shift do not depend
// on the batch, so dY = scale * dU needs no batch sum and the two backward passes above collapse into this one -- 4 (dz, y) + 2 (dY)
// bytes per element in bf16 where reduce + apply move 10.  The row walk, the lane-constant channel chunk, the U loads in flight and the
// zero border rows are those of bn_bwd_apply_kernel.  SUMS: the lane also keeps s1 = sum dU and s2 = sum dU * (y - m) * r of its channel
// chunk in registers (m = the running mean, minus the convolution bias in the VGG block; r = 1 / sqrt(running_var + eps)); the block folds
// them through LDS ([2][256 / cpp][C] floats, as bn_bwd_reduce_kernel) into ONE row of the [gridDim.x][2][C] table: fixed order, no
// atomics.  Without SUMS (neither gamma nor beta asks for a gradient) nothing but dY is written.
//
// One element: dU and dY = scale * dU.  dY has no second term, so whatever dU loses shows in full.  ReLU: dU is dz or 0 and the product is
// rounded once.  SiLU'(u) = s (1 + u (1 - s)) has a zero at u = -1.278 where the two terms cancel: there the 2^-24 of an fp32 sigmoid is
// many ulps of the result (a CPU model of this arithmetic missed 32 x (e32 + 2^-24 |dY|) on 1 of 122 880 and 17 of 1.1 M elements).  fp32
// tensors therefore evaluate it in double and round once, as ReLU's fp32 three-term sum above (the fp32 pass moves 12 B per element and
// stays HBM-bound); bf16 tensors keep fp32 arithmetic -- half a bf16 ulp, 2^-9 of the result, is the error of the store.
template <typename Act, typename T>
__device__ __forceinline__ void frozen_elem(float dz, float y, float sc, float sh, float& du, float& dy) {
    if constexpr (std::is_same<Act, ActSiLU>::value && std::is_same<T, float>::value) {
        const double u = __builtin_fma((double)y, (double)sc, (double)sh);
        const double s = 1.0 / (1.0 + exp(-u));
        const double d = (double)dz * (s * (1.0 + u * (1.0 - s)));
        du = (float)d;
        dy = (float)((double)sc * d);
    } else {
        du = Act::du(dz, y, sc, sh);
        dy = sc * du;
    }
}

template <typename Act, typename T, bool SUMS>
__global__ __launch_bounds__(256) void bn_frozen_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ y,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ m, const float* __restrict__ r,
                                                            float* __restrict__ part, T* __restrict__ dy, const HaloIdx h, int nrows) {
    constexpr int EPC = Vec16<T>::N, U = FVA_BN_UNROLL;
    extern __shared__ float red[];             // SUMS: [2][rpi][C]
    const int row_chunks = h.Wp * h.cpp;
    const int cmask = h.cpp - 1, cshift = 31 - __builtin_clz(h.cpp);
    const int cc = threadIdx.x & cmask;
    float sc[EPC], sh[EPC], mu[EPC], rs[EPC], s1[EPC], s2[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const int c = cc * EPC + e;
        sc[e] = scale[c]; sh[e] = shift[c];
        if constexpr (SUMS) { mu[e] = m[c]; rs[e] = r[c]; s1[e] = s2[e] = 0.f; }
    }
    Vec16<T> g[U], v[U];
    bool ok[U];
    int64_t m0 = 0;
    auto set_row = [&](int row) -> bool {       // false: a border row
        const int b = row / h.Hp, yy = row - b * h.Hp - h.pad;
        m0 = ((int64_t)b * h.H + yy) * h.W;
        return yy >= 0 && yy < h.H;
    };
    auto load = [&](int i0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            const int xx = (i >> cshift) - h.pad;
            ok[u] = i < row_chunks && xx >= 0 && xx < h.W;
            const int64_t off = (m0 + (ok[u] ? xx : 0)) * h.C + cc * EPC;
            g[u] = ld_last<T>(dz + off);
            v[u] = ld_last<T>(y + off);
        }
    };
    for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
        const bool row_in = set_row(row);
        T* orow = dy + (int64_t)row * row_chunks * EPC;
        if (!row_in) {
            Vec16<T> zero;
#pragma unroll
            for (int e = 0; e < EPC; ++e) zero.set(e, 0.f);
            for (int i = threadIdx.x; i < row_chunks; i += 256) *(Vec16<T>*)(orow + (int64_t)i * EPC) = zero;
            continue;
        }
        for (int i0 = threadIdx.x; i0 < row_chunks; i0 += 256 * U) {
            load(i0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * 256;
                Vec16<T> out;
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float yv = v[u].get(e);
                    float du, dyv;
                    frozen_elem<Act, T>(g[u].get(e), yv, sc[e], sh[e], du, dyv);
                    if (!ok[u]) du = dyv = 0.f;                                                 // a masked chunk adds nothing to the sums
                    out.set(e, dyv);
                    if constexpr (SUMS) {
                        s1[e] += du;
                        s2[e] += du * (yv - mu[e]) * rs[e];
                    }
                }
                if (i < row_chunks) *(Vec16<T>*)(orow + (int64_t)i * EPC) = out;
            }
        }
    }
    if constexpr (SUMS) {
        const int rpi = 256 >> cshift, py = threadIdx.x >> cshift;
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            red[(0 * rpi + py) * h.C + cc * EPC + e] = s1[e];
            red[(1 * rpi + py) * h.C + cc * EPC + e] = s2[e];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * h.C; i += 256) {
            const int which = i >= h.C, c = i - which * h.C;
            float s = 0.f;
            for (int k = 0; k < rpi; ++k) s += red[(which * rpi + k) * h.C + c];
            part[((int64_t)blockIdx.x * 2 + which) * h.C + c] = s;
        }
    }
}

// the table of bn_frozen_bwd_kernel -> dbeta = s1, dgamma = s2 and, for a convolution bias in front of the BatchNorm (which no longer
// cancels with fixed statistics), dbias = scale * s1.  The two-level fold of the other finalize kernels; no coefficient table.
__global__ __launch_bounds__(1024) void bn_frozen_bwd_finalize_kernel(const float* __restrict__ part, int nblocks, int C,
                                                                      const float* __restrict__ scale, float* dgamma, float* dbeta, float* dbias,
                                                                      const double* __restrict__ pre, int pre_rows) {
    __shared__ double red[2][FIN_G][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cx;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        if (pre_rows > 0) {
            for (int r = ry; r < pre_rows; r += FIN_G) {
                s1 += pre[((int64_t)r * 2 + 0) * C + c];
                s2 += pre[((int64_t)r * 2 + 1) * C + c];
            }
        } else {
            reduce_partials(part, nblocks, C, c, ry, s1, s2);
        }
    }
    red[0][ry][cx] = s1;
    red[1][ry][cx] = s2;
    __syncthreads();
    if (ry == 0 && c < C) {
        s1 = s2 = 0.0;
#pragma unroll 8                                 // (fully unrolled, the 128 LDS doubles in flight spill at 1024 threads per block)
        for (int k = 0; k < FIN_G; ++k) {
            s1 += red[0][k][cx];
            s2 += red[1][k][cx];
        }
        if (dbeta) dbeta[c] = (float)s1;
        if (dgamma) dgamma[c] = (float)s2;
        if (dbias) dbias[c] = (float)((double)scale[c] * s1);
    }
}

// m = running_mean (- bias), r = 1 / sqrt(running_var + eps): the divisor of bn_eval_coeffs_kernel, so that scale == gamma * r up to one rounding
__global__ void bn_frozen_stats_kernel(int C, const float* __restrict__ rm, const float* __restrict__ rv, const float* __restrict__ bias, float eps,
                                       float* m, float* r) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        m[c] = bias ? rm[c] - bias[c] : rm[c];
        r[c] = 1.0f / sqrtf(rv[c] + eps);
    }
}

// ---------------------------------------------------------------------------------------------------------
// nearest x2 upsample + channel concat into a halo buffer (pad 1)
template <typename T>
__global__ __launch_bounds__(256) void upcat_fwd_kernel(const T* __restrict__ up, int up_pad, const T* __restrict__ skip,
                                                        int skip_pad, T* __restrict__ out, const HaloIdx h, int hh, int ww,
                                                        int Cup, int Cskip, int up_first) {
    constexpr int EPC = Vec16<T>::N;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < h.total; i += (int64_t)gridDim.x * blockDim.x) {
        int b, yy, xx, cc;
        Vec16<T> v;
        if (halo_decode(h, (uint32_t)i, b, yy, xx, cc)) {
            int c = cc * EPC;
            const bool from_up = up_first ? (c < Cup) : (c >= Cskip);
            if (from_up) {
                if (!up_first) c -= Cskip;
                const int64_t pix = ((int64_t)b * (hh + 2 * up_pad) + (yy >> 1) + up_pad) * (ww + 2 * up_pad) + (xx >> 1) + up_pad;
                v = *(const Vec16<T>*)(up + pix * Cup + c);
            } else {
                if (up_first) c -= Cup;
                const int64_t pix = ((int64_t)b * (2 * hh + 2 * skip_pad) + yy + skip_pad) * (2 * ww + 2 * skip_pad) + xx + skip_pad;
                v = *(const Vec16<T>*)(skip + pix * Cskip + c);
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPC; ++e) v.set(e, 0.f);
        }
        *(Vec16<T>*)(out + i * EPC) = v;
    }
}

// dcat dense [B][2h][2w][Ct] -> dup dense [B][h][w][Cup] (sum of the 2x2 block) and dskip dense [B][2h][2w][Cskip]
template <typename T>
__global__ __launch_bounds__(256) void upcat_bwd_kernel(const T* __restrict__ dcat, T* __restrict__ dup, T* __restrict__ dskip,
                                                        int B, int hh, int ww, int Cup, int Cskip, int up_first) {
    constexpr int EPC = Vec16<T>::N;
    const int Ct = Cup + Cskip, cu = Cup / EPC, cs = Cskip / EPC;
    const int64_t n_up = (int64_t)B * hh * ww * cu, n_sk = (int64_t)B * 4 * hh * ww * cs;
    const int uoff = up_first ? 0 : Cskip, soff = up_first ? Cup : 0;
    // 32-bit item arithmetic (the host checks the item count): 64-bit divisions cost more than the 16-byte copy they address
    const uint32_t total = (uint32_t)(n_up + n_sk), nu = (uint32_t)n_up;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        if (i < nu) {
            const uint32_t pix = i / (uint32_t)cu, cc = i - pix * (uint32_t)cu;
            const uint32_t row = pix / (uint32_t)ww, x = pix - row * (uint32_t)ww;        // row = b * hh + y
            const uint32_t b = row / (uint32_t)hh, y = row - b * (uint32_t)hh;
            float acc[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
            Vec16<T> v[4];
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int64_t sp = ((int64_t)b * 2 * hh + 2 * y + dy) * (2 * ww) + 2 * x + dx;
                    v[dy * 2 + dx] = *(const Vec16<T>*)(dcat + sp * Ct + uoff + cc * EPC);
                }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[e] += v[q].get(e);
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, acc[e]);
            *(Vec16<T>*)(dup + (int64_t)pix * Cup + cc * EPC) = o;
        } else {
            const uint32_t j = i - nu;
            const uint32_t pix = j / (uint32_t)cs, cc = j - pix * (uint32_t)cs;
            *(Vec16<T>*)(dskip + (int64_t)pix * Cskip + cc * EPC) = *(const Vec16<T>*)(dcat + (int64_t)pix * Ct + soff + cc * EPC);
        }
    }
}

// arbitrary-stride [B,C,H,W] (fp32 or bf16) -> halo NHWC of T.  One thread per output element (small tensors only).
template <typename T, typename S>
__global__ void pack_nchw_kernel(const S* __restrict__ src, int64_t sb, int64_t sc, int64_t sh, int64_t sw, T* __restrict__ dst,
                                 int pad, int B, int C, int H, int W) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int64_t total = (int64_t)B * Hp * Wp * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t pix = i / C;
        const int xp = (int)(pix % Wp), yp = (int)((pix / Wp) % Hp), b = (int)(pix / ((int64_t)Wp * Hp));
        const int y = yp - pad, x = xp - pad;
        float v = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) v = to_f(src[b * sb + c * sc + y * sh + x * sw]);
        dst[i] = from_f<T>(v);
    }
}

template <typename TD, typename TS>
__global__ void cast_nhwc_kernel(const TS* __restrict__ src, int spad, TD* __restrict__ dst, int dpad, int B, int H, int W, int C) {
    const int Hd = H + 2 * dpad, Wd = W + 2 * dpad, Hs = H + 2 * spad, Ws = W + 2 * spad;
    const int64_t total = (int64_t)B * Hd * Wd * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t pix = i / C;
        const int xp = (int)(pix % Wd), yp = (int)((pix / Wd) % Hd), b = (int)(pix / ((int64_t)Wd * Hd));
        const int y = yp - dpad, x = xp - dpad;
        float v = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) v = to_f(src[(((int64_t)b * Hs + y + spad) * Ws + x + spad) * C + c]);
        dst[i] = from_f<TD>(v);
    }
}

constexpr int ACC_GRID = 2048;    // blocks of the accumulator forms of the apply kernels: each walks rows, its prologue paid once (1280 ... one block per row measured alike)

inline int stream_grid(int64_t items) {
    int64_t g = (items + 255) / 256;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

// ---- argument checks and launches shared by the entry points below
int check_chan(int dtype, int C, const char* who) {
    if (dtype != FVA_F32 && dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "%s: bad dtype", who);
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    if (C <= 0 || C % epc) return fva_fail(FVA_ERR_ARG, "%s: C=%d not a multiple of %d", who, C, epc);
    return FVA_OK;
}

int fill_fwd_acc(const fva_bn_fwd_acc* a, int64_t M, BnFwdAcc& f, const char* who) {
    if (!a || !a->acc || !a->gamma || !a->beta || !a->save_mean || !a->save_rstd || !a->scale || !a->shift)
        return fva_fail(FVA_ERR_ARG, "%s: null pointer in the accumulator descriptor", who);
    if (a->zero == a->acc) return fva_fail(FVA_ERR_ARG, "%s: `zero` must be another accumulator (this one is still being read)", who);
    if (!fva_replicas_ok(a->replicas)) return fva_fail(FVA_ERR_ARG, "%s: replicas = %d is not a power of two in 1..%d", who, a->replicas, FVA_BN_ACC_MAX_REPLICAS);
    f.acc = (long long*)a->acc; f.zero = (long long*)a->zero; f.replicas = a->replicas; f.gamma = a->gamma; f.beta = a->beta;
    f.running_mean = a->running_mean; f.running_var = a->running_var; f.nbt = (long long*)a->num_batches_tracked;
    f.momentum = a->momentum; f.eps = a->eps; f.n = bn_n((double)M);
    f.save_mean = a->save_mean; f.save_rstd = a->save_rstd; f.scale = a->scale; f.shift = a->shift;
    return FVA_OK;
}

// f(T()) with T = bf16_t or float, as `dtype` says (check_chan has refused every other code)
template <typename F>
void by_dtype(int dtype, F&& f) {
    if (dtype == FVA_BF16) f(bf16_t());
    else f(float());
}

// the HaloIdx of an apply pass, checked; `strict` (the ReLU entries) also refuses an empty shape and a pad other than 0 / 1
int checked_halo(const char* who, int dtype, int B, int H, int W, int C, int pad, bool strict, HaloIdx& h) {
    if (strict && (B <= 0 || H <= 0 || W <= 0 || pad < 0 || pad > 1)) return fva_fail(FVA_ERR_ARG, "%s: bad shape B=%d H=%d W=%d pad=%d", who, B, H, W, pad);
    h = make_halo(B, H, W, C, pad, dtype == FVA_BF16 ? 8 : 4);
    if (h.total >= (1ll << 31)) return fva_fail(FVA_ERR_ARG, "%s: tensor too large", who);
    if ((h.cpp & (h.cpp - 1)) || h.cpp > 256) return fva_fail(FVA_ERR_ARG, "%s: C=%d must be a power of two (<= 256 chunks)", who, C);
    return FVA_OK;
}

// FIN: the accumulator form (scale / shift come out of `acc`); otherwise the plain form, one block per padded row
template <typename Act, bool FIN>
int apply_impl(const char* who, int dtype, const void* y, const float* scale, const float* shift, const fva_bn_fwd_acc* acc, const void* residual,
               int res_pad, void* z, int z_pad, int B, int H, int W, int C, void* stream) {
    int rc = check_chan(dtype, C, who);
    if (rc) return rc;
    if (!y || !z || (!FIN && (!scale || !shift))) return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    BnFwdAcc f = BnFwdAcc();
    if (FIN && (rc = fill_fwd_acc(acc, (int64_t)B * H * W, f, who))) return rc;
    HaloIdx h;
    if ((rc = checked_halo(who, dtype, B, H, W, C, z_pad, std::is_same<Act, ActReLU>::value, h))) return rc;
    const int nrows = B * h.Hp, grid = FIN && nrows > ACC_GRID ? ACC_GRID : nrows;
    const int smem = FIN ? 2 * C * 4 + (f.replicas > 1 ? FX_WORDS * C * 8 : 0) : 0;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bn_apply_kernel<Act, T, FIN>), dim3(grid), dim3(256), smem, (hipStream_t)stream, (const T*)y, scale, shift,
                           (const T*)residual, res_pad, (T*)z, h, f, nrows);
    });
    FVA_LAUNCH_CHECK(FIN ? "bn_apply_kernel<acc>" : "bn_apply_kernel");
    return FVA_OK;
}

int bwd_rows_per_block(int64_t M, int C, int epc) {
    const int rpi = 256 / (C / epc) > 0 ? 256 / (C / epc) : 1;
    int64_t rows = (M + 2047) / 2048;           // at most 2048 blocks
    if (rows < (int64_t)rpi * 8) rows = (int64_t)rpi * 8;
    rows = (rows + rpi - 1) / rpi * rpi;
    return (int)rows;
}

template <typename Act>
int bwd_reduce_impl(const char* who, int dtype, const void* dz, const void* y, const float* scale, const float* shift,
                    const float* save_mean, const float* save_rstd, float* partial, int64_t* acc, int replicas, int32_t nblocks, int64_t M, int C,
                    void* stream) {
    constexpr bool relu = std::is_same<Act, ActReLU>::value;      // its entry also refuses M <= 0 and words two refusals in its own way
    int rc = check_chan(dtype, C, who);
    if (acc && !fva_replicas_ok(replicas)) return fva_fail(FVA_ERR_ARG, "%s: replicas = %d is not a power of two in 1..%d", who, replicas, FVA_BN_ACC_MAX_REPLICAS);
    if (rc) return rc;
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    const int cpp = C / epc;
    if (cpp > 256 || 256 % cpp) return fva_fail(FVA_ERR_ARG, "%s: C=%d unsupported", who, C);
    if (!dz || !y || !scale || !shift || !save_mean || !save_rstd || (!partial && !acc) || (relu && M <= 0))
        return fva_fail(FVA_ERR_ARG, relu ? "%s: bad argument" : "%s: null pointer", who);
    const int rows = bwd_rows_per_block(M, C, epc);
    if (acc) nblocks = cdiv(M, rows);
    if (nblocks != cdiv(M, rows))
        return fva_fail(FVA_ERR_ARG, relu ? "%s: nblocks %d != fva_bn_bwd_blocks() = %d" : "%s: nblocks %d != %d", who, nblocks, cdiv(M, rows));
    const int smem = 2 * (256 / cpp) * C * 4;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<Act, T>), dim3(nblocks), dim3(256), smem, (hipStream_t)stream, (const T*)dz, (const T*)y, scale,
                           shift, save_mean, save_rstd, partial, (long long*)acc, replicas, M, C, rows);
    });
    FVA_LAUNCH_CHECK("bn_bwd_reduce_kernel");
    return FVA_OK;
}

// FIN: the accumulator form (`a`, at most ACC_GRID blocks that walk the rows); otherwise `coef`, one block per padded row
template <typename Act, bool FIN>
int bwd_apply_impl(const char* who, int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                   const float* save_rstd, const float* coef, const fva_bn_bwd_acc* a, void* dy, int dy_pad, int B, int H, int W, int C,
                   void* stream) {
    int rc = check_chan(dtype, C, who);
    if (rc) return rc;
    if (!dz || !y || !scale || !shift || !save_mean || !save_rstd || (!coef && !a) || !dy) return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    HaloIdx h;
    if ((rc = checked_halo(who, dtype, B, H, W, C, dy_pad, std::is_same<Act, ActReLU>::value, h))) return rc;
    BnBwdAcc f = BnBwdAcc();
    if (FIN) {
        if (!a->acc || !a->gamma || !a->dgamma || !a->dbeta) return fva_fail(FVA_ERR_ARG, "%s: null pointer in the accumulator descriptor", who);
        if (a->zero == a->acc) return fva_fail(FVA_ERR_ARG, "%s: `zero` must be another accumulator (this one is still being read)", who);
        if (!fva_replicas_ok(a->replicas)) return fva_fail(FVA_ERR_ARG, "%s: replicas = %d is not a power of two in 1..%d", who, a->replicas, FVA_BN_ACC_MAX_REPLICAS);
        f.acc = (long long*)a->acc; f.zero = (long long*)a->zero; f.replicas = a->replicas; f.gamma = a->gamma; f.dgamma = a->dgamma; f.dbeta = a->dbeta;
        f.accumulate = a->accumulate; f.n = bn_n((double)B * H * W);
    }
    const int nrows = B * h.Hp, grid = FIN && nrows > ACC_GRID ? ACC_GRID : nrows;
    const int smem = FIN ? (5 * C + (C & 1)) * 4 + (f.replicas > 1 ? FX_WORDS * C * 8 : 0) : 0;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bn_bwd_apply_kernel<Act, T, FIN>), dim3(grid), dim3(256), smem, (hipStream_t)stream, (const T*)dz, (const T*)y, scale, shift,
                           save_mean, save_rstd, coef, (T*)dy, h, nrows, f);
    });
    FVA_LAUNCH_CHECK(FIN ? "bn_bwd_apply_kernel<acc>" : "bn_bwd_apply_kernel");
    return FVA_OK;
}

// The grid of the frozen pass: blocks walk the padded rows, at most FROZEN_GRID of them (256 CUs x 4 resident blocks of 4 waves at the
// register count of the bf16 form) -- and at most one per 64 pixels, so that the partial table (2 C floats per block, written once and read
// once: 16 C bytes) stays under 16 / (64 * 6) = 4.2 % of the pass's own 6 M C bytes (bf16).
constexpr int FROZEN_GRID = 1024;
int frozen_grid(const HaloIdx& h) {
    const int64_t nrows = (int64_t)h.B * h.Hp, by_pixels = (int64_t)h.B * h.H * h.W / 64;
    int64_t g = nrows < FROZEN_GRID ? nrows : FROZEN_GRID;
    if (g > by_pixels) g = by_pixels;
    return g < 1 ? 1 : (int)g;
}

template <typename Act>
int frozen_bwd_impl(const char* who, int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* m,
                    const float* r, float* partial, void* dy, int dy_pad, int B, int H, int W, int C, void* stream) {
    int rc = check_chan(dtype, C, who);
    if (rc) return rc;
    if (!dz || !y || !scale || !shift || !dy || (partial && (!m || !r))) return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    HaloIdx h;
    if ((rc = checked_halo(who, dtype, B, H, W, C, dy_pad, true, h))) return rc;
    // without sums there is no table to keep small: one block per padded row up to ACC_GRID, as the apply passes (at frozen_grid()'s 200
    // blocks the 32 x 20 x 20 x 1024 map took 48 us where the pass with sums and its fold took 37; one block per row: 20 us)
    const int nrows = B * h.Hp, grid = partial ? frozen_grid(h) : (nrows < ACC_GRID ? nrows : ACC_GRID);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (partial)
            hipLaunchKernelGGL((bn_frozen_bwd_kernel<Act, T, true>), dim3(grid), dim3(256), 2 * 256 * Vec16<T>::N * 4, (hipStream_t)stream, (const T*)dz,
                               (const T*)y, scale, shift, m, r, partial, (T*)dy, h, nrows);
        else
            hipLaunchKernelGGL((bn_frozen_bwd_kernel<Act, T, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)dz, (const T*)y, scale,
                               shift, m, r, partial, (T*)dy, h, nrows);
    });
    FVA_LAUNCH_CHECK("bn_frozen_bwd_kernel");
    return FVA_OK;
}

}  // namespace

extern "C" {

int32_t fva_bn_frozen_bwd_blocks(int dtype, int B, int H, int W, int C, int dy_pad) {
    HaloIdx h;
    if (check_chan(dtype, C, "fva_bn_frozen_bwd_blocks") || checked_halo("fva_bn_frozen_bwd_blocks", dtype, B, H, W, C, dy_pad, true, h)) return 0;
    return frozen_grid(h);
}

int fva_bn_silu_frozen_bwd(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* m, const float* r,
                           float* partial, void* dy, int dy_pad, int B, int H, int W, int C, void* stream) {
    return frozen_bwd_impl<ActSiLU>("fva_bn_silu_frozen_bwd", dtype, dz, y, scale, shift, m, r, partial, dy, dy_pad, B, H, W, C, stream);
}

int fva_bn_relu_frozen_bwd(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* m, const float* r,
                           float* partial, void* dy, int dy_pad, int B, int H, int W, int C, void* stream) {
    return frozen_bwd_impl<ActReLU>("fva_bn_relu_frozen_bwd", dtype, dz, y, scale, shift, m, r, partial, dy, dy_pad, B, H, W, C, stream);
}

int fva_bn_frozen_bwd_finalize(float* partial, int32_t nblocks, int32_t partial_rows, int C, const float* scale, float* dgamma, float* dbeta,
                               float* dbias, void* stream) {
    if (!partial || (!dgamma && !dbeta && !dbias) || (dbias && !scale) || nblocks <= 0 || C <= 0)
        return fva_fail(FVA_ERR_ARG, "fva_bn_frozen_bwd_finalize: bad argument");
    if (partial_rows < fva_bn_partial_rows(nblocks))
        return fva_fail(FVA_ERR_WORKSPACE, "fva_bn_frozen_bwd_finalize: the table holds %d rows, %d rows of producers need fva_bn_partial_rows() = %d",
                        partial_rows, nblocks, fva_bn_partial_rows(nblocks));
    const double* pre = nullptr;
    int pre_rows = 0;
    if (nblocks >= PRE_MIN) {
        pre_rows = cdiv(nblocks, PRE_ROWS);
        double* tail = (double*)(partial + ((int64_t)nblocks * 2 * C + 1) / 2 * 2);
        pre = tail;
        hipLaunchKernelGGL(bn_prereduce_kernel, dim3(cdiv(C, 16), pre_rows), dim3(1024), 0, (hipStream_t)stream, partial, nblocks, C, tail);
        FVA_LAUNCH_CHECK("bn_prereduce_kernel");
    }
    hipLaunchKernelGGL(bn_frozen_bwd_finalize_kernel, dim3(cdiv(C, 16)), dim3(1024), 0, (hipStream_t)stream, partial, nblocks, C, scale, dgamma,
                       dbeta, dbias, pre, pre_rows);
    FVA_LAUNCH_CHECK("bn_frozen_bwd_finalize_kernel");
    return FVA_OK;
}

int fva_bn_frozen_stats(int32_t C, const float* rm, const float* rv, const float* bias, float eps, float* m, float* r, void* stream) {
    if (!rm || !rv || !m || !r || C <= 0) return fva_fail(FVA_ERR_ARG, "fva_bn_frozen_stats: bad argument");
    hipLaunchKernelGGL(bn_frozen_stats_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, C, rm, rv, bias, eps, m, r);
    FVA_LAUNCH_CHECK("bn_frozen_stats_kernel");
    return FVA_OK;
}

int fva_bn_finalize(float* part, int32_t nblocks, int32_t partial_rows, int64_t count, int32_t C, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                    float* save_mean, float* save_rstd, float* scale, float* shift, void* stream) {
    if (!part || !gamma || !beta || !save_mean || !save_rstd || !scale || !shift || nblocks <= 0 || count <= 0 || C <= 0)
        return fva_fail(FVA_ERR_ARG, "fva_bn_finalize: bad argument");
    if (partial_rows < fva_bn_partial_rows(nblocks))
        return fva_fail(FVA_ERR_WORKSPACE, "fva_bn_finalize: the table holds %d rows, %d rows of producers need fva_bn_partial_rows() = %d", partial_rows, nblocks,
                        fva_bn_partial_rows(nblocks));
    const double* pre = nullptr;
    int pre_rows = 0;
    if (nblocks >= PRE_MIN) {
        pre_rows = cdiv(nblocks, PRE_ROWS);
        // the table was allocated with fva_bn_partial_rows(nblocks) rows: doubles live behind the nblocks float rows
        double* tail = (double*)(part + ((int64_t)nblocks * 2 * C + 1) / 2 * 2);
        pre = tail;
        hipLaunchKernelGGL(bn_prereduce_kernel, dim3(cdiv(C, 16), pre_rows), dim3(1024), 0, (hipStream_t)stream, (const float*)part, nblocks,
                           C, tail);
        FVA_LAUNCH_CHECK("bn_prereduce_kernel");
    }
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 16)), dim3(1024), 0, (hipStream_t)stream, (const float*)part, nblocks, (double)count,
                       C, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, save_mean, save_rstd,
                       scale, shift, pre, pre_rows);
    FVA_LAUNCH_CHECK("bn_finalize_kernel");
    return FVA_OK;
}

int32_t fva_bn_partial_rows(int32_t nblocks) {
    if (nblocks < PRE_MIN) return nblocks;
    return nblocks + 2 * cdiv(nblocks, PRE_ROWS) + 1;   // pre-reduced doubles (2 floats each) + alignment slack
}

int fva_bn_eval_coeffs(int32_t C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                       float* scale, float* shift, void* stream) {
    if (!gamma || !beta || !rm || !rv || !scale || !shift || C <= 0) return fva_fail(FVA_ERR_ARG, "fva_bn_eval_coeffs: bad argument");
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, C, gamma, beta, rm, rv, eps,
                       scale, shift);
    FVA_LAUNCH_CHECK("bn_eval_coeffs_kernel");
    return FVA_OK;
}

int fva_bn_acc_finalize(const fva_bn_fwd_acc* acc, int64_t M, int C, void* stream) {
    BnFwdAcc f = BnFwdAcc();
    const int rc = fill_fwd_acc(acc, M, f, "fva_bn_acc_finalize");
    if (rc) return rc;
    if (C < 1 || M < 1) return fva_fail(FVA_ERR_ARG, "fva_bn_acc_finalize: bad size");
    if (C > 2048) return fva_fail(FVA_ERR_ARG, "fva_bn_acc_finalize: C = %d > 2048", C);
    hipLaunchKernelGGL(bn_acc_finalize_kernel, dim3(1), dim3(256), FX_WORDS * C * 8, (hipStream_t)stream, f, C);
    FVA_LAUNCH_CHECK("bn_acc_finalize_kernel");
    return FVA_OK;
}

int fva_bn_silu_apply(int dtype, const void* y, const float* scale, const float* shift, const void* residual, int res_pad,
                      void* z, int z_pad, int B, int H, int W, int C, void* stream) {
    return apply_impl<ActSiLU, false>("fva_bn_silu_apply", dtype, y, scale, shift, nullptr, residual, res_pad, z, z_pad, B, H, W, C, stream);
}

int fva_bn_silu_apply_acc(int dtype, const void* y, const fva_bn_fwd_acc* acc, const void* residual, int res_pad, void* z, int z_pad, int B,
                          int H, int W, int C, void* stream) {
    return apply_impl<ActSiLU, true>("fva_bn_silu_apply_acc", dtype, y, nullptr, nullptr, acc, residual, res_pad, z, z_pad, B, H, W, C, stream);
}

int fva_bn_relu_apply(int dtype, const void* y, const float* scale, const float* shift, void* z, int z_pad, int B, int H, int W, int C,
                      void* stream) {
    return apply_impl<ActReLU, false>("fva_bn_relu_apply", dtype, y, scale, shift, nullptr, nullptr, 0, z, z_pad, B, H, W, C, stream);
}

int32_t fva_bn_bwd_blocks(int dtype, int64_t M, int C) {
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    if (C % epc || C / epc > 256 || 256 % (C / epc)) return 0;
    return cdiv(M, bwd_rows_per_block(M, C, epc));
}

int fva_bn_silu_bwd_reduce(int dtype, const void* dz, const void* y, const float* scale, const float* shift,
                           const float* save_mean, const float* save_rstd, float* partial, int32_t nblocks, int64_t M, int C,
                           void* stream) {
    if (!partial) return fva_fail(FVA_ERR_ARG, "fva_bn_silu_bwd_reduce: null pointer");
    return bwd_reduce_impl<ActSiLU>("fva_bn_silu_bwd_reduce", dtype, dz, y, scale, shift, save_mean, save_rstd, partial, nullptr, 1, nblocks, M, C, stream);
}

int fva_bn_silu_bwd_reduce_acc(int dtype, const void* dz, const void* y, const float* scale, const float* shift,
                               const float* save_mean, const float* save_rstd, int64_t* acc, int32_t replicas, int64_t M, int C, void* stream) {
    if (!acc) return fva_fail(FVA_ERR_ARG, "fva_bn_silu_bwd_reduce_acc: null pointer");
    return bwd_reduce_impl<ActSiLU>("fva_bn_silu_bwd_reduce_acc", dtype, dz, y, scale, shift, save_mean, save_rstd, nullptr, acc, replicas, 0, M, C, stream);
}

int fva_bn_relu_bwd_reduce(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                           const float* save_rstd, float* partial, int32_t nblocks, int64_t M, int C, void* stream) {
    return bwd_reduce_impl<ActReLU>("fva_bn_relu_bwd_reduce", dtype, dz, y, scale, shift, save_mean, save_rstd, partial, nullptr, 1, nblocks, M, C, stream);
}

int fva_bn_bwd_finalize(float* partial, int32_t nblocks, int32_t partial_rows, int64_t M, int C, const float* gamma, const float* save_rstd,
                        float* dgamma, float* dbeta, int accumulate, float* coef, void* stream) {
    if (!partial || !gamma || !save_rstd || !dgamma || !dbeta || !coef || nblocks <= 0 || M <= 0 || C <= 0)
        return fva_fail(FVA_ERR_ARG, "fva_bn_bwd_finalize: bad argument");
    if (partial_rows < fva_bn_partial_rows(nblocks))
        return fva_fail(FVA_ERR_WORKSPACE, "fva_bn_bwd_finalize: the table holds %d rows, %d rows of producers need fva_bn_partial_rows() = %d", partial_rows,
                        nblocks, fva_bn_partial_rows(nblocks));
    // long tables (the fused dgrad epilogues write one row per 128- or 256-pixel block) are first folded in parallel, as in the
    // forward pass: C / 16 blocks walking 1600 rows of a C = 128 layer took 72 us, the two-level form takes 5 + 5 (the caller
    // allocated fva_bn_partial_rows(nblocks) rows: the doubles live behind the table)
    const double* pre = nullptr;
    int pre_rows = 0;
    if (nblocks >= PRE_MIN) {
        pre_rows = cdiv(nblocks, PRE_ROWS);
        double* tail = (double*)(partial + ((int64_t)nblocks * 2 * C + 1) / 2 * 2);
        pre = tail;
        hipLaunchKernelGGL(bn_prereduce_kernel, dim3(cdiv(C, 16), pre_rows), dim3(1024), 0, (hipStream_t)stream, partial, nblocks, C, tail);
        FVA_LAUNCH_CHECK("bn_prereduce_kernel");
    }
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, 16)), dim3(1024), 0, (hipStream_t)stream, partial, nblocks, (double)M, C,
                       gamma, save_rstd, dgamma, dbeta, accumulate, coef, pre, pre_rows);
    FVA_LAUNCH_CHECK("bn_bwd_finalize_kernel");
    return FVA_OK;
}

int fva_bn_silu_bwd_apply(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                          const float* save_rstd, const float* coef, void* dy, int dy_pad, int B, int H, int W, int C, void* stream) {
    if (!coef) return fva_fail(FVA_ERR_ARG, "fva_bn_silu_bwd_apply: null pointer");
    return bwd_apply_impl<ActSiLU, false>("fva_bn_silu_bwd_apply", dtype, dz, y, scale, shift, save_mean, save_rstd, coef, nullptr, dy, dy_pad, B, H, W, C, stream);
}

int fva_bn_silu_bwd_apply_acc(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                              const float* save_rstd, const fva_bn_bwd_acc* acc, void* dy, int dy_pad, int B, int H, int W, int C, void* stream) {
    if (!acc) return fva_fail(FVA_ERR_ARG, "fva_bn_silu_bwd_apply_acc: null pointer");
    return bwd_apply_impl<ActSiLU, true>("fva_bn_silu_bwd_apply_acc", dtype, dz, y, scale, shift, save_mean, save_rstd, nullptr, acc, dy, dy_pad, B, H, W, C, stream);
}

int fva_bn_relu_bwd_apply(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                          const float* save_rstd, const float* coef, void* dy, int dy_pad, int B, int H, int W, int C, void* stream) {
    return bwd_apply_impl<ActReLU, false>("fva_bn_relu_bwd_apply", dtype, dz, y, scale, shift, save_mean, save_rstd, coef, nullptr, dy, dy_pad, B, H, W, C, stream);
}

int fva_upsample2_concat_fwd(int dtype, const void* up, int up_pad, const void* skip, int skip_pad, void* out, int B, int h, int w,
                             int Cup, int Cskip, int up_first, void* stream) {
    int rc = check_chan(dtype, Cup, "fva_upsample2_concat_fwd");
    if (!rc) rc = check_chan(dtype, Cskip, "fva_upsample2_concat_fwd");
    if (rc) return rc;
    if (!up || !skip || !out) return fva_fail(FVA_ERR_ARG, "fva_upsample2_concat_fwd: null pointer");
    const HaloIdx hi = make_halo(B, 2 * h, 2 * w, Cup + Cskip, 1, dtype == FVA_BF16 ? 8 : 4);
    if (hi.total >= (1ll << 31)) return fva_fail(FVA_ERR_ARG, "fva_upsample2_concat_fwd: tensor too large");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FVA_BF16)
        hipLaunchKernelGGL(upcat_fwd_kernel<bf16_t>, dim3(stream_grid(hi.total)), dim3(256), 0, s, (const bf16_t*)up, up_pad,
                           (const bf16_t*)skip, skip_pad, (bf16_t*)out, hi, h, w, Cup, Cskip, up_first);
    else
        hipLaunchKernelGGL(upcat_fwd_kernel<float>, dim3(stream_grid(hi.total)), dim3(256), 0, s, (const float*)up, up_pad,
                           (const float*)skip, skip_pad, (float*)out, hi, h, w, Cup, Cskip, up_first);
    FVA_LAUNCH_CHECK("upcat_fwd_kernel");
    return FVA_OK;
}

int fva_upsample2_concat_bwd(int dtype, const void* dcat, void* dup, void* dskip, int B, int h, int w, int Cup, int Cskip,
                             int up_first, void* stream) {
    int rc = check_chan(dtype, Cup, "fva_upsample2_concat_bwd");
    if (!rc) rc = check_chan(dtype, Cskip, "fva_upsample2_concat_bwd");
    if (rc) return rc;
    if (!dcat || !dup || !dskip) return fva_fail(FVA_ERR_ARG, "fva_upsample2_concat_bwd: null pointer");
    const int epc = dtype == FVA_BF16 ? 8 : 4;
    const int64_t items = (int64_t)B * h * w * (Cup / epc) + (int64_t)B * 4 * h * w * (Cskip / epc);
    if (items >= (1ll << 31)) return fva_fail(FVA_ERR_ARG, "fva_upsample2_concat_bwd: tensor too large");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FVA_BF16)
        hipLaunchKernelGGL(upcat_bwd_kernel<bf16_t>, dim3(stream_grid(items)), dim3(256), 0, s, (const bf16_t*)dcat, (bf16_t*)dup,
                           (bf16_t*)dskip, B, h, w, Cup, Cskip, up_first);
    else
        hipLaunchKernelGGL(upcat_bwd_kernel<float>, dim3(stream_grid(items)), dim3(256), 0, s, (const float*)dcat, (float*)dup,
                           (float*)dskip, B, h, w, Cup, Cskip, up_first);
    FVA_LAUNCH_CHECK("upcat_bwd_kernel");
    return FVA_OK;
}

int fva_pack_nchw(int dtype, const void* src, int src_is_bf16, int64_t sb, int64_t sc, int64_t sh, int64_t sw, void* dst,
                  int dst_pad, int B, int C, int H, int W, void* stream) {
    if (!src || !dst || (dtype != FVA_F32 && dtype != FVA_BF16)) return fva_fail(FVA_ERR_ARG, "fva_pack_nchw: bad argument");
    const int64_t total = (int64_t)B * (H + 2 * dst_pad) * (W + 2 * dst_pad) * C;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g(stream_grid(total)), b(256);
    if (dtype == FVA_BF16 && src_is_bf16)
        hipLaunchKernelGGL((pack_nchw_kernel<bf16_t, bf16_t>), g, b, 0, s, (const bf16_t*)src, sb, sc, sh, sw, (bf16_t*)dst, dst_pad, B, C, H, W);
    else if (dtype == FVA_BF16)
        hipLaunchKernelGGL((pack_nchw_kernel<bf16_t, float>), g, b, 0, s, (const float*)src, sb, sc, sh, sw, (bf16_t*)dst, dst_pad, B, C, H, W);
    else if (src_is_bf16)
        hipLaunchKernelGGL((pack_nchw_kernel<float, bf16_t>), g, b, 0, s, (const bf16_t*)src, sb, sc, sh, sw, (float*)dst, dst_pad, B, C, H, W);
    else
        hipLaunchKernelGGL((pack_nchw_kernel<float, float>), g, b, 0, s, (const float*)src, sb, sc, sh, sw, (float*)dst, dst_pad, B, C, H, W);
    FVA_LAUNCH_CHECK("pack_nchw_kernel");
    return FVA_OK;
}

int fva_cast_nhwc(const void* src, int src_dtype, int src_pad, void* dst, int dst_dtype, int dst_pad, int B, int H, int W, int C,
                  void* stream) {
    if (!src || !dst) return fva_fail(FVA_ERR_ARG, "fva_cast_nhwc: null pointer");
    const int64_t total = (int64_t)B * (H + 2 * dst_pad) * (W + 2 * dst_pad) * C;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g(stream_grid(total)), b(256);
    if (dst_dtype == FVA_BF16 && src_dtype == FVA_BF16)
        hipLaunchKernelGGL((cast_nhwc_kernel<bf16_t, bf16_t>), g, b, 0, s, (const bf16_t*)src, src_pad, (bf16_t*)dst, dst_pad, B, H, W, C);
    else if (dst_dtype == FVA_BF16)
        hipLaunchKernelGGL((cast_nhwc_kernel<bf16_t, float>), g, b, 0, s, (const float*)src, src_pad, (bf16_t*)dst, dst_pad, B, H, W, C);
    else if (src_dtype == FVA_BF16)
        hipLaunchKernelGGL((cast_nhwc_kernel<float, bf16_t>), g, b, 0, s, (const bf16_t*)src, src_pad, (float*)dst, dst_pad, B, H, W, C);
    else
        hipLaunchKernelGGL((cast_nhwc_kernel<float, float>), g, b, 0, s, (const float*)src, src_pad, (float*)dst, dst_pad, B, H, W, C);
    FVA_LAUNCH_CHECK("cast_nhwc_kernel");
    return FVA_OK;
}

}  // extern "C"

namespace {

// The convolution bias in front of BatchNorm (vgg.py:43 builds Conv2d(bias=True)): training subtracts it again with the batch mean, so
// the convolution runs without it; what it leaves is the running mean (it tracks mean(y) + b: running_mean += momentum * b after
// fva_bn_finalize) and the eval-mode shift, beta + (b - running_mean) * scale.
__global__ void bn_bias_running_mean_kernel(int C, float* running_mean, const float* __restrict__ bias, float momentum) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) running_mean[c] = __builtin_fmaf(momentum, bias[c], running_mean[c]);
}
__global__ void bn_eval_coeffs_bias_kernel(int C, const float* gamma, const float* beta, const float* rm, const float* rv, const float* bias,
                                           float eps, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        const float sc = gamma[c] / sqrtf(rv[c] + eps);
        scale[c] = sc;
        shift[c] = beta[c] + (bias[c] - rm[c]) * sc;
    }
}

}  // namespace

extern "C" {

int fva_bn_bias_running_mean(int32_t C, float* running_mean, const float* bias, float momentum, void* stream) {
    if (!running_mean || !bias || C <= 0) return fva_fail(FVA_ERR_ARG, "fva_bn_bias_running_mean: bad argument");
    hipLaunchKernelGGL(bn_bias_running_mean_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, C, running_mean, bias, momentum);
    FVA_LAUNCH_CHECK("bn_bias_running_mean_kernel");
    return FVA_OK;
}

int fva_bn_eval_coeffs_bias(int32_t C, const float* gamma, const float* beta, const float* rm, const float* rv, const float* bias, float eps,
                            float* scale, float* shift, void* stream) {
    if (!gamma || !beta || !rm || !rv || !bias || !scale || !shift || C <= 0) return fva_fail(FVA_ERR_ARG, "fva_bn_eval_coeffs_bias: bad argument");
    hipLaunchKernelGGL(bn_eval_coeffs_bias_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, C, gamma, beta, rm, rv, bias, eps,
                       scale, shift);
    FVA_LAUNCH_CHECK("bn_eval_coeffs_bias_kernel");
    return FVA_OK;
}

}  // extern "C"
