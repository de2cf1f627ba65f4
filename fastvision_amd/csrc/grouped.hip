// Grouped 3x3 convolution (padding 1, stride 1 or 2, Cin == Cout == C, groups = C / Cg): conv2 of the ResNeXt bottleneck (reference
// classfication/models/resnext.py:40).  Forward with BatchNorm statistics, data gradient, weight gradient; fp32 and bf16 tensors, the fp32
// OIHW master weight [C][Cg][3][3] as it stands (no packed copy, nothing cached: a captured step replays the same launches).
//
// THE PLAIN PATH.  All three are straight FMA kernels; no MFMA kernel is built yet (DESIGN 3.12 says what that costs).
//   gather kernel (forward and data gradient, both strides): a block owns 256 output pixels x one slab of 16 consecutive channels, a
//       thread one pixel x the 16 channels.  The slab's filter taps sit in LDS as [tap][k][16] floats (bf16 tensors: rounded to bf16
//       first, the value an MFMA kernel would multiply), read as broadcast float4s; the source pixels come straight from global memory,
//       16 bytes per load.  Cg < 16: the slab is 16 / Cg whole groups and only the diagonal blocks are multiplied.  Cg >= 16: the slab lies
//       inside one group.  The data gradient is the same kernel with the transposed tap table; at stride 2 a pixel's parity selects its
//       1, 2, 2 or 4 taps.  fp32 tensors accumulate in double (products of floats are exact there: one rounding per output), bf16 in fp32,
//       a tap's Cg terms first and then the taps.
//       Statistics: the unrounded accumulators of the block, summed per channel in double in pixel order -> one row of the table per
//       pixel block.
//   weight gradient: a block owns a slab of 16 output channels x a run of output rows; a thread owns (source channel, tap) items and
//       their 16 (Cg < 16: Cg) output channels, accumulates in double over 16-pixel row pieces staged in LDS, and leaves a double partial
//       [split][C][Cg][9] in the workspace; a second launch adds the splits in their order and rounds once.
// No atomics, fixed order everywhere: the same bits on every run.
#include <type_traits>

#include "common.h"

namespace {

constexpr int PIX = 256;       // output pixels per block of the gather kernel = rows of one statistics block
constexpr int SLAB = 16;       // channels per block
constexpr int OWT = 16;        // output pixels of one staged row piece of the weight gradient
constexpr int XWMAX = (OWT - 1) * 2 + 3;

template <typename T>
struct AccOf { using type = float; };
template <>
struct AccOf<float> { using type = double; };

template <typename T>
__device__ __forceinline__ float stage_w(float w) { return w; }
template <>
__device__ __forceinline__ float stage_w<bf16_t>(float w) { return (float)(bf16_t)w; }

struct GGeom {
    int OH, OW;            // the pixel grid this launch writes (forward: the output map; data gradient: the input map)
    int SH, SW, spad;      // the source halo tensor's logical map and border
    int C, stride;
    int64_t M;             // B * OH * OW
};

// out [M][C] dense; src halo [B][SH + 2 spad][SW + 2 spad][C]; w fp32 OIHW; stats [blocks][2][C] or null
template <typename T, int CG, bool DGRAD>
__global__ __launch_bounds__(PIX) void gconv_gather_kernel(const T* __restrict__ src, const float* __restrict__ w, T* __restrict__ out,
                                                           float* __restrict__ stats, GGeom g) {
    using Acc = typename AccOf<T>::type;
    constexpr int EPC = Vec16<T>::N;
    constexpr int WL = 9 * CG * SLAB;
    constexpr int LDS_N = WL > PIX * SLAB ? WL : PIX * SLAB;
    __shared__ __attribute__((aligned(16))) float lds[LDS_N];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * SLAB;
    const int gbase = (c0 / CG) * CG;                     // Cg >= 16: the slab's group
    for (int i = tid; i < WL; i += PIX) {
        const int o = i & (SLAB - 1), k = (i / SLAB) % CG, tap = i / (SLAB * CG);
        const int c = c0 + o;
        const int co = DGRAD ? (c / CG) * CG + k : c;
        const int ci = DGRAD ? c % CG : k;
        lds[i] = stage_w<T>(w[((int64_t)co * CG + ci) * 9 + tap]);
    }
    __syncthreads();
    const int64_t pix = (int64_t)blockIdx.x * PIX + tid;
    const bool live = pix < g.M;
    Acc acc[SLAB];
#pragma unroll
    for (int o = 0; o < SLAB; ++o) acc[o] = 0;
    if (live) {
        const int64_t t = pix / g.OW;
        const int ox = (int)(pix - t * g.OW), b = (int)(t / g.OH), oy = (int)(t - (int64_t)b * g.OH);
        const int sWp = g.SW + 2 * g.spad;
        const T* simg = src + (int64_t)b * (g.SH + 2 * g.spad) * sWp * g.C;
        for (int kh = 0; kh < 3; ++kh) {
            int sy;
            if (DGRAD) {
                const int ty = oy + 1 - kh;
                if (g.stride == 2 && (ty & 1)) continue;
                sy = g.stride == 2 ? ty >> 1 : ty;
            } else {
                sy = oy * g.stride - 1 + kh;
            }
            for (int kw = 0; kw < 3; ++kw) {
                int sx;
                if (DGRAD) {
                    const int tx = ox + 1 - kw;
                    if (g.stride == 2 && (tx & 1)) continue;
                    sx = g.stride == 2 ? tx >> 1 : tx;
                } else {
                    sx = ox * g.stride - 1 + kw;
                }
                const T* sp = simg + ((int64_t)(sy + g.spad) * sWp + sx + g.spad) * g.C;
                const float* wl = lds + (kh * 3 + kw) * CG * SLAB;
                Acc tap[SLAB];                            // one tap's terms first, then the nine taps: two short chains of additions, not one of 9 Cg
#pragma unroll
                for (int o = 0; o < SLAB; ++o) tap[o] = 0;
                if (CG < SLAB) {
                    float xs[SLAB];
#pragma unroll
                    for (int v = 0; v < SLAB / EPC; ++v) {
                        const Vec16<T> x = *(const Vec16<T>*)(sp + c0 + v * EPC);
#pragma unroll
                        for (int e = 0; e < EPC; ++e) xs[v * EPC + e] = x.get(e);
                    }
#pragma unroll
                    for (int k = 0; k < CG; ++k) {
                        float wv[SLAB];
#pragma unroll
                        for (int q = 0; q < SLAB / 4; ++q) {
                            const f32x4 w4 = *(const f32x4*)(wl + k * SLAB + q * 4);
                            wv[q * 4] = w4[0]; wv[q * 4 + 1] = w4[1]; wv[q * 4 + 2] = w4[2]; wv[q * 4 + 3] = w4[3];
                        }
#pragma unroll
                        for (int o = 0; o < SLAB; ++o) tap[o] += (Acc)xs[(o / CG) * CG + k] * (Acc)wv[o];
                    }
                } else {
#pragma unroll 1
                    for (int k0 = 0; k0 < CG; k0 += EPC) {
                        const Vec16<T> x = *(const Vec16<T>*)(sp + gbase + k0);
#pragma unroll
                        for (int e = 0; e < EPC; ++e) {
                            const Acc xv = (Acc)x.get(e);
#pragma unroll
                            for (int q = 0; q < SLAB / 4; ++q) {
                                const f32x4 w4 = *(const f32x4*)(wl + (k0 + e) * SLAB + q * 4);
                                tap[q * 4] += xv * (Acc)w4[0];
                                tap[q * 4 + 1] += xv * (Acc)w4[1];
                                tap[q * 4 + 2] += xv * (Acc)w4[2];
                                tap[q * 4 + 3] += xv * (Acc)w4[3];
                            }
                        }
                    }
                }
#pragma unroll
                for (int o = 0; o < SLAB; ++o) acc[o] += tap[o];
            }
        }
        T* op = out + pix * g.C + c0;
#pragma unroll
        for (int v = 0; v < SLAB / EPC; ++v) {
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, (float)acc[v * EPC + e]);
            *(Vec16<T>*)(op + v * EPC) = o;
        }
    }
    if (!DGRAD && stats != nullptr) {
        __syncthreads();                                  // the tap table is dead: the block's accumulators take its place, dead pixels as zeros
#pragma unroll
        for (int o = 0; o < SLAB; ++o) lds[tid * SLAB + o] = (float)acc[o];
        __syncthreads();
        if (tid < 2 * SLAB) {
            const int ch = tid & (SLAB - 1), which = tid / SLAB;
            double s = 0.0;
            for (int r = 0; r < PIX; ++r) {
                const double v = (double)lds[r * SLAB + ch];
                s += which ? v * v : v;
            }
            stats[((int64_t)blockIdx.x * 2 + which) * g.C + c0 + ch] = (float)s;
        }
    }
}

struct WGeom {
    int B, H, W, OH, OW, C, stride, in_pad, dy_pad;
    int rows_per_split;    // output rows (b, oy) per block
};

// partial [split][C][CG][9] doubles
template <typename T, int CG>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, double* __restrict__ partial, WGeom g) {
    constexpr int EPC = Vec16<T>::N;
    constexpr int KS = CG < SLAB ? SLAB : CG;             // source channels the slab's outputs read
    constexpr int NCO = CG < SLAB ? CG : SLAB;            // output channels one source channel meets
    constexpr int NITEM = 9 * KS;
    constexpr int NI = (NITEM + 255) / 256;
    __shared__ __attribute__((aligned(16))) float xs[3 * XWMAX * KS];
    __shared__ __attribute__((aligned(16))) float ds[OWT * SLAB];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * SLAB;
    const int sb = CG < SLAB ? c0 : (c0 / CG) * CG;
    const int rows = g.B * g.OH;
    const int r0 = blockIdx.y * g.rows_per_split, r1 = min(rows, r0 + g.rows_per_split);
    const int xWp = g.W + 2 * g.in_pad, dWp = g.OW + 2 * g.dy_pad;
    double acc[NI][NCO];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NCO; ++j) acc[i][j] = 0.0;
    for (int r = r0; r < r1; ++r) {
        const int b = r / g.OH, oy = r - b * g.OH;
        const T* ximg = x + (int64_t)b * (g.H + 2 * g.in_pad) * xWp * g.C;
        const T* drow = dy + (((int64_t)b * (g.OH + 2 * g.dy_pad) + oy + g.dy_pad) * dWp + g.dy_pad) * g.C;
        for (int ox0 = 0; ox0 < g.OW; ox0 += OWT) {
            const int n = min(OWT, g.OW - ox0);
            const int xw = (n - 1) * g.stride + 3;        // source columns ox0 * stride - 1 ... needed by the n pixels
            __syncthreads();
            for (int i = tid; i < OWT * (SLAB / EPC); i += 256) {
                const int p = i / (SLAB / EPC), v = i - p * (SLAB / EPC);
                Vec16<T> d = {};
                if (p < n) d = *(const Vec16<T>*)(drow + (int64_t)(ox0 + p) * g.C + c0 + v * EPC);
#pragma unroll
                for (int e = 0; e < EPC; ++e) ds[p * SLAB + v * EPC + e] = p < n ? d.get(e) : 0.f;
            }
            for (int i = tid; i < 3 * XWMAX * (KS / EPC); i += 256) {
                const int v = i % (KS / EPC), col = (i / (KS / EPC)) % XWMAX, kh = i / ((KS / EPC) * XWMAX);
                const bool in = col < xw;
                Vec16<T> q = {};
                if (in) {
                    const int iy = oy * g.stride - 1 + kh, ix = ox0 * g.stride - 1 + col;
                    q = *(const Vec16<T>*)(ximg + ((int64_t)(iy + g.in_pad) * xWp + ix + g.in_pad) * g.C + sb + v * EPC);
                }
#pragma unroll
                for (int e = 0; e < EPC; ++e) xs[(kh * XWMAX + col) * KS + v * EPC + e] = in ? q.get(e) : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int it = tid + 256 * i;
                if (it < NITEM) {
                    const int k = it % KS, tap = it / KS, kh = tap / 3, kw = tap - kh * 3;
                    const int ob = CG < SLAB ? (k / CG) * CG : 0;
                    for (int p = 0; p < n; ++p) {
                        const double xv = (double)xs[(kh * XWMAX + p * g.stride + kw) * KS + k];
#pragma unroll
                        for (int j = 0; j < NCO; ++j) acc[i][j] += xv * (double)ds[p * SLAB + ob + j];
                    }
                }
            }
        }
    }
    double* pout = partial + (int64_t)blockIdx.y * g.C * CG * 9;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int it = tid + 256 * i;
        if (it < NITEM) {
            const int k = it % KS, tap = it / KS;
            const int ob = CG < SLAB ? (k / CG) * CG : 0;
            const int ci = CG < SLAB ? k % CG : k;
#pragma unroll
            for (int j = 0; j < NCO; ++j) pout[((int64_t)(c0 + ob + j) * CG + ci) * 9 + tap] = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(256) void gconv_wgrad_reduce_kernel(const double* __restrict__ partial, float* __restrict__ dw, int n, int splits) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < splits; ++j) s += partial[(int64_t)j * n + i];
    dw[i] = (float)s;
}

int check(const char* who, const fva_gconv_desc* d) {
    if (!d) return fva_fail(FVA_ERR_ARG, "%s: null descriptor", who);
    if (d->dtype != FVA_F32 && d->dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "%s: dtype %d is neither FVA_F32 nor FVA_BF16", who, d->dtype);
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fva_fail(FVA_ERR_ARG, "%s: B = %d, H = %d, W = %d must be positive", who, d->B, d->H, d->W);
    if (d->C <= 0 || d->C % 64 || d->C > 2048)
        return fva_fail(FVA_ERR_ARG, "%s: C = %d is outside the contract (C %% 64 == 0, C <= 2048, C = groups * Cg, Cg in {4, 8, 16, 32, 64})", who, d->C);
    const int cg = d->groups > 0 && d->C % d->groups == 0 ? d->C / d->groups : 0;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64)
        return fva_fail(FVA_ERR_ARG, "%s: C = %d with groups = %d is outside the contract (C = groups * Cg, Cg in {4, 8, 16, 32, 64})", who, d->C, d->groups);
    if (d->stride != 1 && d->stride != 2) return fva_fail(FVA_ERR_ARG, "%s: stride %d (1 or 2)", who, d->stride);
    if (d->stride == 2 && ((d->H | d->W) & 1)) return fva_fail(FVA_ERR_ARG, "%s: stride 2 needs an even map, got %d x %d", who, d->H, d->W);
    if (d->in_pad < 1 || d->dy_pad < 1 || d->in_pad > 8 || d->dy_pad > 8)
        return fva_fail(FVA_ERR_ARG, "%s: in_pad = %d and dy_pad = %d must be 1 ... 8", who, d->in_pad, d->dy_pad);
    if ((int64_t)d->B * (d->H + 16) * (d->W + 16) >= (1ll << 31)) return fva_fail(FVA_ERR_ARG, "%s: B * H * W does not fit 31 bits", who);
    return FVA_OK;
}

template <typename F>
void by_type_cg(int dtype, int cg, F&& f) {
    auto with_t = [&](auto t) {
        using T = decltype(t);
        switch (cg) {
            case 4: f(T{}, std::integral_constant<int, 4>{}); break;
            case 8: f(T{}, std::integral_constant<int, 8>{}); break;
            case 16: f(T{}, std::integral_constant<int, 16>{}); break;
            case 32: f(T{}, std::integral_constant<int, 32>{}); break;
            default: f(T{}, std::integral_constant<int, 64>{}); break;
        }
    };
    if (dtype == FVA_BF16) with_t(bf16_t{}); else with_t(float{});
}

struct WPlan {
    int splits, rows_per_split;
};
WPlan wgrad_plan(const fva_gconv_desc* d) {
    const int OH = (d->H - 1) / d->stride + 1;
    const int rows = d->B * OH, slabs = d->C / SLAB, cg = d->C / d->groups;
    int64_t want = 2048 / slabs > 0 ? 2048 / slabs : 1;
    const int64_t one = (int64_t)d->C * cg * 9 * 8;
    const int64_t cap = (64ll << 20) / one > 0 ? (64ll << 20) / one : 1;          // at most 64 MB of partials
    if (want > cap) want = cap;
    if (want > rows) want = rows;
    WPlan p;
    p.rows_per_split = cdiv(rows, want);
    p.splits = cdiv(rows, p.rows_per_split);
    return p;
}

}  // namespace

extern "C" {

int32_t fva_gconv_stat_blocks(const fva_gconv_desc* d) {
    if (check("fva_gconv_stat_blocks", d)) return 0;
    const int OH = (d->H - 1) / d->stride + 1, OW = (d->W - 1) / d->stride + 1;
    return cdiv((int64_t)d->B * OH * OW, PIX);
}

int fva_gconv_fwd(const fva_gconv_desc* d, const void* x, const float* w_oihw, void* y, float* stats_partial, void* stream) {
    int rc = check("fva_gconv_fwd", d);
    if (rc) return rc;
    if (!x || !w_oihw || !y) return fva_fail(FVA_ERR_ARG, "fva_gconv_fwd: null pointer");
    GGeom g;
    g.OH = (d->H - 1) / d->stride + 1; g.OW = (d->W - 1) / d->stride + 1;
    g.SH = d->H; g.SW = d->W; g.spad = d->in_pad; g.C = d->C; g.stride = d->stride;
    g.M = (int64_t)d->B * g.OH * g.OW;
    const dim3 grid(cdiv(g.M, PIX), d->C / SLAB);
    by_type_cg(d->dtype, d->C / d->groups, [&](auto t, auto cg) {
        using T = decltype(t);
        hipLaunchKernelGGL((gconv_gather_kernel<T, decltype(cg)::value, false>), grid, dim3(PIX), 0, (hipStream_t)stream, (const T*)x, w_oihw, (T*)y,
                           stats_partial, g);
    });
    FVA_LAUNCH_CHECK("gconv_gather_kernel (forward)");
    return FVA_OK;
}

int fva_gconv_dgrad(const fva_gconv_desc* d, const void* dy, const float* w_oihw, void* dx, void* stream) {
    int rc = check("fva_gconv_dgrad", d);
    if (rc) return rc;
    if (!dy || !w_oihw || !dx) return fva_fail(FVA_ERR_ARG, "fva_gconv_dgrad: null pointer");
    GGeom g;
    g.OH = d->H; g.OW = d->W;
    g.SH = (d->H - 1) / d->stride + 1; g.SW = (d->W - 1) / d->stride + 1; g.spad = d->dy_pad; g.C = d->C; g.stride = d->stride;
    g.M = (int64_t)d->B * d->H * d->W;
    const dim3 grid(cdiv(g.M, PIX), d->C / SLAB);
    by_type_cg(d->dtype, d->C / d->groups, [&](auto t, auto cg) {
        using T = decltype(t);
        hipLaunchKernelGGL((gconv_gather_kernel<T, decltype(cg)::value, true>), grid, dim3(PIX), 0, (hipStream_t)stream, (const T*)dy, w_oihw, (T*)dx,
                           (float*)nullptr, g);
    });
    FVA_LAUNCH_CHECK("gconv_gather_kernel (data gradient)");
    return FVA_OK;
}

int64_t fva_gconv_wgrad_workspace(const fva_gconv_desc* d) {
    if (check("fva_gconv_wgrad_workspace", d)) return 0;
    return (int64_t)wgrad_plan(d).splits * d->C * (d->C / d->groups) * 9 * 8;
}

int fva_gconv_wgrad(const fva_gconv_desc* d, const void* x, const void* dy, float* dw_oihw, void* workspace, int64_t workspace_bytes, void* stream) {
    int rc = check("fva_gconv_wgrad", d);
    if (rc) return rc;
    if (!x || !dy || !dw_oihw || !workspace) return fva_fail(FVA_ERR_ARG, "fva_gconv_wgrad: null pointer");
    const WPlan p = wgrad_plan(d);
    const int cg = d->C / d->groups;
    const int n = d->C * cg * 9;
    if (workspace_bytes < (int64_t)p.splits * n * 8)
        return fva_fail(FVA_ERR_WORKSPACE, "fva_gconv_wgrad: workspace of %lld bytes, fva_gconv_wgrad_workspace() = %lld", (long long)workspace_bytes,
                        (long long)p.splits * n * 8);
    WGeom g;
    g.B = d->B; g.H = d->H; g.W = d->W; g.OH = (d->H - 1) / d->stride + 1; g.OW = (d->W - 1) / d->stride + 1;
    g.C = d->C; g.stride = d->stride; g.in_pad = d->in_pad; g.dy_pad = d->dy_pad; g.rows_per_split = p.rows_per_split;
    const dim3 grid(d->C / SLAB, p.splits);
    by_type_cg(d->dtype, cg, [&](auto t, auto cgc) {
        using T = decltype(t);
        hipLaunchKernelGGL((gconv_wgrad_kernel<T, decltype(cgc)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)dy,
                           (double*)workspace, g);
    });
    FVA_LAUNCH_CHECK("gconv_wgrad_kernel");
    hipLaunchKernelGGL(gconv_wgrad_reduce_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, dw_oihw, n, p.splits);
    FVA_LAUNCH_CHECK("gconv_wgrad_reduce_kernel");
    return FVA_OK;
}

}  // extern "C"
