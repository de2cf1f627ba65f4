// Grouped 3x3 convolution on the matrix units: bf16 tensors, stride 1, border 1 (conv2 of the ResNeXt bottleneck at its 13 of 16 / 30 of 33
// stride-1 layers).  Forward with BatchNorm statistics, data gradient, weight gradient, and the pack pass of the master weight.  It stands
// beside the plain path of grouped.hip behind entry points of its own (fva_gconv_mfma_*); stride 2 and fp32 stay there.
//
// LAYOUT.  With border 1 the halo tensor is [B][H + 2][W + 2][C] and a stride-1 3x3 tap is a CONSTANT shift of the padded-linear position
// Q = (b (H + 2) + yy) (W + 2) + xx over the whole batch: out[Q] = sum over taps of src[Q + (kh - 1)(W + 2) + (kw - 1)].  The border
// positions of Q are computed like the others (they cost (H + 2)(W + 2) / (H W) of the MFMAs) and masked in the store and the statistics.
//
//   forward / data gradient (one kernel): a block owns RUN = 256 consecutive positions x 64 consecutive channels (whole groups at every
//       Cg).  It stages src[Q0 - (W + 3) .. Q0 + RUN + (W + 3)) x 64 channels into LDS ONCE, 16 bytes per load, at a pitch of 160 bytes per
//       position; all nine taps read LDS.  One wave per slab of 16 output channels: the slab's packed taps live in registers (read once per
//       block), the positions are the N side of v_mfma_f32_16x16x32_bf16 in 16 tiles of 16, the accumulators of all 16 tiles stay in
//       registers.  Cg >= 32: a K-step is 32 input channels of one tap (9 or 18 steps, no padded FLOPs).  Cg <= 16: the slab is 16 / Cg
//       whole groups, a K-step is two taps x the slab's 16 channels against a block-diagonal fragment (zeros off the diagonal), 5 steps,
//       the tenth half-step zero on both sides.  Epilogue: statistics from the unrounded accumulators of the real pixels (double, fixed
//       order: a lane's 16 tiles, then the 16 lanes of its row), one row [2][C] per block; the bf16 results go through LDS (over the dead
//       staging area) and leave as 16-byte pieces, 128 contiguous bytes per pixel.  The data gradient is this kernel on dy with the
//       flipped, transposed table.
//   weight gradient: dw[co][ci][tap] = sum over Q of dy[Q][co] x[Q + shift(tap)][ci] over the padded positions (dy's border is zero by
//       contract, so a border position adds exact zeros).  A block owns 64 channels and a range of runs of 128 positions; per run it stages
//       dy[run] and x[run -+ (W + 3)] in LDS, both position-major, and reads both MFMA operands with the transposing LDS read
//       (ds_read_b64_tr_b16): M = the wave's 16 output channels, N = 16 input channels, K = 32 positions per step.  fp32 partials
//       [split][C][Cg][9] in the workspace; a second launch adds the splits in their order.  Cg < 16: only the diagonal blocks are written.
//   pack: fp32 OIHW -> two bf16 tables in fragment order, [C / 16 slabs][steps][64 lanes][8]: lane l, element j of a step is
//       A[row m = l & 15][k = 8 (l >> 4) + j] (the table layout is spelled out in include/fastvision_amd.h).
//
// LDS.  Pitch 160 bytes: the 16-byte fragment reads of 16 neighbouring positions fall on 16 different 16-byte slots of the 256-byte bank row
// (at a pitch of 128 they would share two), and the transposed reads of a 32-lane half take 8 consecutive rows = 8 different 32-byte
// slots; the K index of the weight gradient is permuted for that (the same permutation on both operands).  Everything fits the default
// 64 KB; a map too wide for that is not served (fva_gconv_mfma_serves).
// No atomics, fixed order everywhere: the same bits on every run.
#include <type_traits>

#include "common.h"

namespace {

constexpr int RUN = 256;       // positions per block, forward and data gradient = rows of one statistics block
constexpr int WRUN = 128;      // positions per staged run of the weight gradient
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

// ------------------------------------------------------------------------------------------------ pack
template <int CG>
__global__ __launch_bounds__(256) void gconv_mfma_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ fwd, bf16_t* __restrict__ dgrad, int n) {
    constexpr int NS = steps_of(CG);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = i & 7, lane = (i >> 3) & 63, step = (i >> 9) % NS, slab = (i >> 9) / NS;
    const int m = lane & 15, k = 8 * (lane >> 4) + j;
    const int c = slab * 16 + m;                           // the row's output channel (data gradient: the input channel dx is taken for)
    float f = 0.f, b = 0.f;
    if (CG >= 32) {
        const int tap = step / (CG / 32), kc = (step % (CG / 32)) * 32 + k, gb = (c / CG) * CG;
        f = w[((int64_t)c * CG + kc) * 9 + tap];
        b = w[((int64_t)(gb + kc) * CG + (c - gb)) * 9 + (8 - tap)];
    } else {
        const int tap = 2 * step + (k >> 4), kc = k & 15;
        if (tap < 9 && kc / CG == m / CG) {                // the diagonal blocks; everything else, and the tenth half-step, stays zero
            f = w[((int64_t)c * CG + kc % CG) * 9 + tap];
            b = w[((int64_t)(slab * 16 + kc) * CG + m % CG) * 9 + (8 - tap)];
        }
    }
    fwd[i] = (bf16_t)f;
    dgrad[i] = (bf16_t)b;
}

// ------------------------------------------------------------------------------------------------ forward / data gradient
struct MGeom {
    int H, W, C, Wp, HpWp;
    int64_t total;         // B (H + 2)(W + 2)
};

// src halo [total][C] bf16 (border 1); wpack [C / 16][steps][64][8]; out dense [B H W][C]; stats [blocks][2][C] or null
template <int CG>
__global__ __launch_bounds__(256) void gconv_mfma_kernel(const bf16_t* __restrict__ src, const bf16_t* __restrict__ wpack, bf16_t* __restrict__ out,
                                                         float* __restrict__ stats, MGeom g) {
    constexpr int NS = steps_of(CG);
    constexpr int NT = RUN / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g4 = lane >> 4, n = lane & 15;
    const int halo = g.W + 3;
    const int S = RUN + 2 * halo;
    int* dense = (int*)(smem + S * PITCH);
    const int64_t Q0 = (int64_t)blockIdx.x * RUN;
    const int c0 = blockIdx.y * CH;

    bf16x8 wf[NS];                                          // the slab's packed taps: read once per block, 16 bytes per lane
    {
        const bf16x8* wp = (const bf16x8*)wpack + (int64_t)(c0 / 16 + wv) * NS * 64 + lane;
#pragma unroll
        for (int s = 0; s < NS; ++s) wf[s] = wp[s * 64];
    }
    // STAGING BOUNDS: the staged range [Q0 - halo, Q0 + RUN + halo) is clipped to the tensor [0, total) HERE; a position outside it is
    // filled with zeros and never loaded, whatever happens to its results later.
#pragma unroll 4
    for (int i = tid; i < S * 8; i += 256) {
        const int s = i >> 3, piece = i & 7;
        const int64_t Q = Q0 - halo + s;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (Q >= 0 && Q < g.total) v = *(const u32x4*)(src + Q * g.C + c0 + piece * 8);
        *(u32x4*)(smem + s * PITCH + piece * 16) = v;
    }
    {   // position -> dense pixel index, -1 for the border and beyond the tensor
        const int64_t Q = Q0 + tid;
        int dn = -1;
        if (Q < g.total) {
            const int q = (int)Q, b = q / g.HpWp, rem = q - b * g.HpWp, yy = rem / g.Wp, xx = rem - yy * g.Wp;
            if (yy >= 1 && yy <= g.H && xx >= 1 && xx <= g.W) dn = (b * g.H + yy - 1) * g.W + xx - 1;
        }
        dense[tid] = dn;
    }
    __syncthreads();

    // per-lane byte offset of the B fragment of tile 0 for every K-step: position n + shift(tap), 8 channels of the step
    int off[NS];
    bool dead_last = false;                                 // Cg <= 16: the tenth half-step (tap 9) of lanes 32 ... 63
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        int tap, ch;
        if (CG >= 32) {
            tap = s / (CG / 32);
            ch = ((wv * 16) / CG) * CG + (s % (CG / 32)) * 32 + 8 * g4;
        } else {
            tap = 2 * s + (g4 >> 1);
            ch = wv * 16 + 8 * (g4 & 1);
            if (tap > 8) { tap = 8; dead_last = true; }
        }
        const int shift = (tap / 3 - 1) * g.Wp + (tap % 3 - 1);
        off[s] = (n + halo + shift) * PITCH + ch * 2;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            bf16x8 b = *(const bf16x8*)(smem + off[s] + t * 16 * PITCH);
            if (CG < 32 && s == NS - 1 && dead_last) b = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], b, acc[t], 0, 0, 0);
        }
    }
    // lane (g4, n) holds channels c0 + 16 wv + 4 g4 + r (r = 0 ... 3) of the positions 16 t + n
    if (stats != nullptr) {
        double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool live = dense[t * 16 + n] >= 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = live ? (double)acc[t][r] : 0.0;
                s1[r] += v;
                s2[r] += v * v;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                s1[r] += __shfl_xor(s1[r], o);
                s2[r] += __shfl_xor(s2[r], o);
            }
        }
        if (n == 0) {
            float* row = stats + (int64_t)blockIdx.x * 2 * g.C + c0 + wv * 16 + 4 * g4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                row[r] = (float)s1[r];
                row[g.C + r] = (float)s2[r];
            }
        }
    }
    __syncthreads();                                        // the staged source is dead: the block's bf16 results take its place
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        u32x2 o;
        o[0] = cvt_pk_bf16(acc[t][0], acc[t][1]);
        o[1] = cvt_pk_bf16(acc[t][2], acc[t][3]);
        *(u32x2*)(smem + (t * 16 + n) * PITCH + (wv * 16 + 4 * g4) * 2) = o;
    }
    __syncthreads();
#pragma unroll
    for (int i = tid; i < RUN * 8; i += 256) {
        const int p = i >> 3, piece = i & 7;
        const int dn = dense[p];
        if (dn >= 0) *(u32x4*)(out + (int64_t)dn * g.C + c0 + piece * 8) = *(const u32x4*)(smem + p * PITCH + piece * 16);
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct WGeom {
    int W, C, Wp;
    int64_t total;
    int nruns, runs_per_split;
};

// partial [split][C][CG][9] floats
template <int CG>
__global__ __launch_bounds__(256) void gconv_mfma_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ partial,
                                                               WGeom g) {
    constexpr int NT = CG >= 16 ? CG / 16 : 1;              // tiles of 16 input channels the slab's outputs meet
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g4 = lane >> 4, n = lane & 15, q = n >> 2, p = n & 3;
    const int halo = g.W + 3;
    const int SX = WRUN + 2 * halo;
    char* xs = smem;
    char* ds = smem + SX * PITCH;
    const int c0 = blockIdx.y * CH;
    const int cib = CG >= 16 ? ((wv * 16) / CG) * CG : wv * 16;      // first input channel (of the block's 64) the slab meets
    // K order inside a 32-position step: element j of lane group g4 is position 16 (j >> 2) + 4 g4 + (j & 3) -- the same on both
    // operands -- so that one transposed read of a 32-lane half takes 8 consecutive rows.
    const int rowoff = (4 * g4 + q) * PITCH + 8 * p;
    const int aoff = rowoff + wv * 16 * 2;
    int boff[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) boff[tap] = rowoff + (halo + (tap / 3 - 1) * g.Wp + (tap % 3 - 1)) * PITCH + cib * 2;
    f32x4 acc[9][NT];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[tap][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int r0 = blockIdx.x * g.runs_per_split, r1 = min(g.nruns, r0 + g.runs_per_split);
    for (int run = r0; run < r1; ++run) {
        const int64_t Q0 = (int64_t)run * WRUN;
        __syncthreads();
        // STAGING BOUNDS: both ranges are clipped to the tensor [0, total) here; positions outside it are zeros and are never loaded.
#pragma unroll 4
        for (int i = tid; i < SX * 8; i += 256) {
            const int s = i >> 3, piece = i & 7;
            const int64_t Q = Q0 - halo + s;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (Q >= 0 && Q < g.total) v = *(const u32x4*)(x + Q * g.C + c0 + piece * 8);
            *(u32x4*)(xs + s * PITCH + piece * 16) = v;
        }
#pragma unroll
        for (int i = tid; i < WRUN * 8; i += 256) {
            const int s = i >> 3, piece = i & 7;
            const int64_t Q = Q0 + s;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (Q < g.total) v = *(const u32x4*)(dy + Q * g.C + c0 + piece * 8);
            *(u32x4*)(ds + s * PITCH + piece * 16) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int k0 = 0; k0 < WRUN; k0 += 32) {
            const char* da = ds + k0 * PITCH + aoff;
            const bf16x8 a = tr_pair(da, da + 16 * PITCH);
            const char* xb = xs + k0 * PITCH;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const char* bp = xb + boff[tap] + t * 32;
                    const bf16x8 b = tr_pair(bp, bp + 16 * PITCH);
                    acc[tap][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[tap][t], 0, 0, 0);
                }
            }
        }
    }
    // lane (g4, n): rows co = 16 wv + 4 g4 + r, column ci = cib + 16 t + n
    float* pout = partial + (int64_t)blockIdx.x * g.C * CG * 9;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int col = 4 * g4 + r, co = c0 + wv * 16 + col;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int ci = t * 16 + n;
            bool live = true;
            if (CG < 16) {
                live = n / CG == col / CG;
                ci = n % CG;
            }
            if (live) {
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) pout[((int64_t)co * CG + ci) * 9 + tap] = acc[tap][t][r];
            }
        }
    }
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

// ------------------------------------------------------------------------------------------------ host
const char* const CONTRACT =
    "the MFMA path serves FVA_BF16 at stride 1 with in_pad == dy_pad == 1, C % 64 == 0, C <= 2048, C = groups * Cg, Cg in {4, 8, 16, 32, 64}, "
    "B (H + 2)(W + 2) < 2^31 and a map narrow enough to stage in 64 KB of LDS (W <= 70); ask fva_gconv_mfma_serves";

int fwd_lds(int W) { return (RUN + 2 * (W + 3)) * PITCH + RUN * 4; }
int wgrad_lds(int W) { return (2 * WRUN + 2 * (W + 3)) * PITCH; }

bool serves(const fva_gconv_desc* d) {
    if (!d || d->dtype != FVA_BF16 || d->stride != 1 || d->in_pad != 1 || d->dy_pad != 1) return false;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->C % 64 || d->C > 2048) return false;
    const int cg = d->groups > 0 && d->C % d->groups == 0 ? d->C / d->groups : 0;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64) return false;
    if (d->W > 4096 || d->H > (1 << 24) || (int64_t)d->B * (d->H + 2) * (d->W + 2) >= (1ll << 31)) return false;
    return fwd_lds(d->W) <= LDS_MAX && wgrad_lds(d->W) <= LDS_MAX;
}

int refuse(const char* who, const fva_gconv_desc* d) {
    if (!d) return fva_fail(FVA_ERR_ARG, "%s: null descriptor", who);
    return fva_fail(FVA_ERR_ARG, "%s: %s; got dtype %d, B %d, H %d, W %d, C %d, groups %d, stride %d, in_pad %d, dy_pad %d", who, CONTRACT, d->dtype, d->B,
                    d->H, d->W, d->C, d->groups, d->stride, d->in_pad, d->dy_pad);
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

int64_t total_of(const fva_gconv_desc* d) { return (int64_t)d->B * (d->H + 2) * (d->W + 2); }

int64_t pack_elems(const fva_gconv_desc* d) { return (int64_t)(d->C / 16) * steps_of(d->C / d->groups) * 512; }

int launch_gather(const char* who, const fva_gconv_desc* d, const void* src, const void* wpack, void* out, float* stats, void* stream) {
    MGeom g;
    g.H = d->H; g.W = d->W; g.C = d->C; g.Wp = d->W + 2; g.HpWp = (d->H + 2) * (d->W + 2); g.total = total_of(d);
    const dim3 grid(cdiv(g.total, RUN), d->C / CH);
    const int lds = fwd_lds(d->W);
    by_cg(d->C / d->groups, [&](auto cg) {
        hipLaunchKernelGGL((gconv_mfma_kernel<decltype(cg)::value>), grid, dim3(256), lds, (hipStream_t)stream, (const bf16_t*)src, (const bf16_t*)wpack,
                           (bf16_t*)out, stats, g);
    });
    FVA_LAUNCH_CHECK(who);
    return FVA_OK;
}

struct WPlan {
    int nruns, splits, runs_per_split;
};
WPlan wgrad_plan(const fva_gconv_desc* d) {
    WPlan p;
    p.nruns = cdiv(total_of(d), WRUN);
    const int64_t one = (int64_t)d->C * (d->C / d->groups) * 9 * 4;
    int64_t want = 4096 / (d->C / CH);                                             // blocks in flight: a few per CU
    const int64_t cap = (64ll << 20) / one > 0 ? (64ll << 20) / one : 1;           // at most 64 MB of partials
    if (want > cap) want = cap;
    if (want > p.nruns) want = p.nruns;
    if (want < 1) want = 1;
    p.runs_per_split = cdiv(p.nruns, want);
    p.splits = cdiv(p.nruns, p.runs_per_split);
    return p;
}

}  // namespace

extern "C" {

int fva_gconv_mfma_serves(const fva_gconv_desc* d) { return serves(d) ? 1 : 0; }

int64_t fva_gconv_mfma_pack_bytes(const fva_gconv_desc* d) { return serves(d) ? pack_elems(d) * 2 : 0; }

int fva_gconv_mfma_pack(const fva_gconv_desc* d, const float* w_oihw, void* wpack_fwd, void* wpack_dgrad, void* stream) {
    if (!serves(d)) return refuse("fva_gconv_mfma_pack", d);
    if (!w_oihw || !wpack_fwd || !wpack_dgrad) return fva_fail(FVA_ERR_ARG, "fva_gconv_mfma_pack: null pointer");
    const int n = (int)pack_elems(d);
    by_cg(d->C / d->groups, [&](auto cg) {
        hipLaunchKernelGGL((gconv_mfma_pack_kernel<decltype(cg)::value>), dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w_oihw,
                           (bf16_t*)wpack_fwd, (bf16_t*)wpack_dgrad, n);
    });
    FVA_LAUNCH_CHECK("gconv_mfma_pack_kernel");
    return FVA_OK;
}

int32_t fva_gconv_mfma_stat_blocks(const fva_gconv_desc* d) { return serves(d) ? cdiv(total_of(d), RUN) : 0; }

int fva_gconv_mfma_fwd(const fva_gconv_desc* d, const void* x, const void* wpack_fwd, void* y, float* stats_partial, void* stream) {
    if (!serves(d)) return refuse("fva_gconv_mfma_fwd", d);
    if (!x || !wpack_fwd || !y) return fva_fail(FVA_ERR_ARG, "fva_gconv_mfma_fwd: null pointer");
    return launch_gather("gconv_mfma_kernel (forward)", d, x, wpack_fwd, y, stats_partial, stream);
}

int fva_gconv_mfma_dgrad(const fva_gconv_desc* d, const void* dy, const void* wpack_dgrad, void* dx, void* stream) {
    if (!serves(d)) return refuse("fva_gconv_mfma_dgrad", d);
    if (!dy || !wpack_dgrad || !dx) return fva_fail(FVA_ERR_ARG, "fva_gconv_mfma_dgrad: null pointer");
    return launch_gather("gconv_mfma_kernel (data gradient)", d, dy, wpack_dgrad, dx, nullptr, stream);
}

int64_t fva_gconv_mfma_wgrad_workspace(const fva_gconv_desc* d) {
    if (!serves(d)) return 0;
    return (int64_t)wgrad_plan(d).splits * d->C * (d->C / d->groups) * 9 * 4;
}

int fva_gconv_mfma_wgrad(const fva_gconv_desc* d, const void* x, const void* dy, float* dw_oihw, void* ws, int64_t ws_bytes, void* stream) {
    if (!serves(d)) return refuse("fva_gconv_mfma_wgrad", d);
    if (!x || !dy || !dw_oihw || !ws) return fva_fail(FVA_ERR_ARG, "fva_gconv_mfma_wgrad: null pointer");
    const WPlan p = wgrad_plan(d);
    const int cg = d->C / d->groups;
    const int n = d->C * cg * 9;
    if (ws_bytes < (int64_t)p.splits * n * 4)
        return fva_fail(FVA_ERR_WORKSPACE, "fva_gconv_mfma_wgrad: workspace of %lld bytes, fva_gconv_mfma_wgrad_workspace() = %lld", (long long)ws_bytes,
                        (long long)p.splits * n * 4);
    WGeom g;
    g.W = d->W; g.C = d->C; g.Wp = d->W + 2; g.total = total_of(d); g.nruns = p.nruns; g.runs_per_split = p.runs_per_split;
    const dim3 grid(p.splits, d->C / CH);
    const int lds = wgrad_lds(d->W);
    by_cg(cg, [&](auto cgc) {
        hipLaunchKernelGGL((gconv_mfma_wgrad_kernel<decltype(cgc)::value>), grid, dim3(256), lds, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)dy,
                           (float*)ws, g);
    });
    FVA_LAUNCH_CHECK("gconv_mfma_wgrad_kernel");
    hipLaunchKernelGGL(gconv_mfma_wgrad_reduce_kernel, dim3(cdiv(n, RED_E)), dim3(RED_E * RED_S), 0, (hipStream_t)stream, (const float*)ws, dw_oihw, n, p.splits);
    FVA_LAUNCH_CHECK("gconv_mfma_wgrad_reduce_kernel");
    return FVA_OK;
}

}  // extern "C"
