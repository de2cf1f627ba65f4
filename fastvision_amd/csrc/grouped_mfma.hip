// Grouped 3x3 convolution on the matrix units: bf16 tensors, border 1, stride 1 and stride 2 (conv2 of every ResNeXt bottleneck).  Forward
// with BatchNorm statistics, data gradient, weight gradient, and the pack pass of the master weight, behind entry points of their own
// (fva_gconv_mfma_* at stride 1, fva_gconv_mfma_s2_* at stride 2) beside the plain path of grouped.hip, where fp32 stays.
//
// ONE SKELETON, TWO GEOMETRIES.  In both strides a tap is a CONSTANT shift of a linear position over the whole batch, so a block stages a
// run of positions once and all nine taps read LDS.  The forward, the weight gradient and the pack kernel are written once; what a stride
// decides sits in a policy struct (S1, S2): the run lengths, the kernel's geometry arguments, how a run is staged (stage, stage_dy), which
// dense pixel a position is (dense_of) and where a tap reads (tap_offset).  The stride-2 data gradient loops four parity classes over one
// staging and has no stride-1 twin: it is a kernel of its own on the same helpers (load_taps, step_half, step_channel, tiles_to_lds).
// Its class-masked store and the forward's dense store stay apart: one loop for both would have to branch on its caller.
//
// LAYOUT, stride 1.  With border 1 the halo tensor is [B][H + 2][W + 2][C] and a 3x3 tap is a constant shift of the padded-linear position
// Q = (b (H + 2) + yy) (W + 2) + xx: out[Q] = sum over taps of src[Q + (kh - 1)(W + 2) + (kw - 1)].  The border positions of Q are computed
// like the others (they cost (H + 2)(W + 2) / (H W) of the MFMAs) and masked in the store and the statistics.  A block stages
// src[Q0 - (W + 3) .. Q0 + RUN + (W + 3)).
//
// PARITY PLANES, stride 2.  There a tap is no constant shift of Q any more.  Split the padded input xp [B][H + 2][W + 2] into four planes
// P[pr][pc][b][i][j] = xp[b][2 i + pr][2 j + pc], i < Hh = OH + 1, j < Wh = OW + 1 (zero where 2 i + pr > H + 1 or 2 j + pc > W + 1), and
// with the plane-linear position T = (b Hh + i) Wh + j
//       y[T] = sum over (kh, kw) of P[kh & 1][kw & 1][T + (kh >> 1) Wh + (kw >> 1)] w[kh][kw],        real where i < OH and j < OW:
// every tap is a constant shift again, inside one of four planes.  The planes never exist in HBM: they are formed while staging (a position
// of a plane is 128 contiguous bytes of the halo tensor), and de-interleaving there is what keeps the LDS reads free of conflicts -- the 16
// neighbouring outputs of a tile read 16 consecutive positions of ONE plane, 16 different 16-byte slots; read from an interleaved row they
// would sit 320 bytes apart, 4 to a slot.  A block stages plane (0,0) over [T0, T0 + RUN + Wh + 1), (0,1) over + Wh, (1,0) over + 1,
// (1,1) over + 0: (4 RUN + 2 Wh + 2) positions, 51 KB at Wh = 29.  The non-real positions cost (OH + 1)(OW + 1) / (OH OW) of the MFMAs.
//
//   forward (stride 1: also the data gradient, on dy with the flipped, transposed table): a block owns RUN (256 / 64) consecutive positions
//       x 64 consecutive channels (whole groups at every Cg) and stages its source ONCE, 16 bytes per load.  One wave per slab of 16 output
//       channels: the slab's packed taps live in registers (read once per block), the positions are the N side of v_mfma_f32_16x16x32_bf16
//       in tiles of 16, the accumulators of all tiles stay in registers.  Cg >= 32: a K-step is 32 input channels of one tap (9 or 18 steps,
//       no padded FLOPs).  Cg <= 16: the slab is 16 / Cg whole groups, a K-step is two taps x the slab's 16 channels against a
//       block-diagonal fragment (zeros off the diagonal), 5 steps, the tenth half-step zero on both sides.  Epilogue: statistics from the
//       unrounded accumulators of the real pixels (double, fixed order: a lane's tiles, then the 16 lanes of its row), one row [2][C] per
//       block; the bf16 results go through LDS (over the dead staging area) and leave as 16-byte pieces, 128 contiguous bytes per pixel.
//   data gradient, stride 2: by the parity (py, px) of (iy, ix) a dx pixel meets 1, 2, 2 or 4 taps, each a constant shift (0, 1, OW + 2,
//       OW + 3) of the dy-halo position anchored at R = (b, i + 1, j + 1), iy = 2 i + py, ix = 2 j + px.  A block owns DRUN = 128
//       consecutive R x 64 channels, stages dy[R0, R0 + DRUN + OW + 3) once, and LOOPS the four classes over that one staging: per class its
//       own packed fragments (the table is in class order), one set of tile accumulators, the class's pixels out through a second LDS area.
//       9 taps per anchor in all: no padded FLOPs beyond the Cg <= 16 diagonal (2 taps per K-step inside a class: 1 + 1 + 1 + 2 = 5 steps,
//       the first half-step zero).  Every dx element is written exactly once.
//   weight gradient: dw[co][ci][tap] = sum over positions of dy[position][co] x[position + shift(tap)][ci].  Stride 1: over the padded
//       positions Q (dy's border is zero by contract, so a border position adds exact zeros).  Stride 2: over T with
//       dy_T = dy_halo[b][i + 1][j + 1] (always inside the tensor; zero by contract at i = OH and j = OW, so a non-real T adds exact zeros).
//       A block owns 64 channels and a range of runs of WRUN (128 / 64) positions; per run it stages dy[run] and the x ranges of the
//       forward in LDS, all position-major, and reads both MFMA operands with the transposing LDS read (ds_read_b64_tr_b16): M = the wave's
//       16 output channels, N = 16 input channels, K = 32 positions per step.  fp32 partials [split][C][Cg][9] in the workspace; a second
//       launch adds the splits in their order.  Cg < 16: only the diagonal blocks are written.
//   pack: fp32 OIHW -> two bf16 tables in fragment order, [C / 16 slabs][steps][64 lanes][8]: lane l, element j of a step is
//       A[row m = l & 15][k = 8 (l >> 4) + j].  The forward table is the same in both strides; the data-gradient table holds the flipped
//       taps at stride 1 and the taps in class order at stride 2 (the table layouts are spelled out in include/fastvision_amd.h).
//
// LDS.  Pitch 160 bytes: the 16-byte fragment reads of 16 neighbouring positions fall on 16 different 16-byte slots of the 256-byte bank row
// (at a pitch of 128 they would share two), and the transposed reads of a 32-lane half take 8 consecutive rows = 8 different 32-byte
// slots; the K index of the weight gradient is permuted for that (the same permutation on both operands).  Everything fits the default
// 64 KB; a map too wide for that is not served (fva_gconv_mfma_serves, fva_gconv_mfma_s2_serves).
// No atomics, fixed order everywhere: the same bits on every run.
#include <type_traits>

#include "common.h"

namespace {

constexpr int CH = 64;         // channels per block
constexpr int PITCH = 160;     // bytes per staged position (128 of data)
constexpr int LDS_MAX = 64 * 1024;
constexpr int DRUN = 128;      // dy-halo positions per block of the stride-2 data gradient

constexpr int steps_of(int cg) { return cg >= 32 ? 9 * (cg / 32) : 5; }
__host__ __device__ constexpr int out_of(int n) { return (n - 1) / 2 + 1; }

using lds_s16x4 = __attribute__((address_space(3))) s16x4;
using s16x8 = __attribute__((ext_vector_type(8))) short;

__device__ __forceinline__ bf16x8 tr_pair(const char* lo, const char* hi) {
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo);
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi);
    return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ------------------------------------------------------------------------------------------------ the two geometries
// A geometry names its positions (pos_t), carries the kernels' arguments (Args; total = the positions of the whole batch) and lays a
// staged run out in LDS: staged(run, g) positions from smem on, read by tap 3 kh + kw at tap_offset(tap, run, g) bytes for the run's
// first output.
struct S1 {
    static constexpr int STRIDE = 1;
    static constexpr int RUN = 256;        // positions per block, forward and data gradient = rows of one statistics block
    static constexpr int WRUN = 128;       // positions per staged run of the weight gradient
    using pos_t = int64_t;
    struct Args {
        int H, W, C, Wp, HpWp;
        int64_t total;                     // B (H + 2)(W + 2) padded positions
        int nruns, runs_per_split;         // weight gradient only
    };
    static Args geom(const fva_gconv_desc* d) {
        Args g;
        g.H = d->H; g.W = d->W; g.C = d->C; g.Wp = d->W + 2; g.HpWp = (d->H + 2) * (d->W + 2);
        g.total = (int64_t)d->B * (d->H + 2) * (d->W + 2);
        g.nruns = g.runs_per_split = 0;
        return g;
    }
    __host__ __device__ static int staged(int run, const Args& g) { return run + 2 * (g.W + 3); }

    // STAGING BOUNDS: the staged range [Q0 - halo, Q0 + run + halo) is clipped to the tensor [0, total) HERE; a position outside it is
    // filled with zeros and never loaded, whatever happens to its results later.
    __device__ __forceinline__ static void stage(char* smem, const bf16_t* __restrict__ src, const Args& g, pos_t Q0, int run, int c0, int tid) {
        const int halo = g.W + 3;
        const int S = run + 2 * halo;
#pragma unroll 4
        for (int i = tid; i < S * 8; i += 256) {
            const int s = i >> 3, piece = i & 7;
            const int64_t Q = Q0 - halo + s;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (Q >= 0 && Q < g.total) v = *(const u32x4*)(src + Q * g.C + c0 + piece * 8);
            *(u32x4*)(smem + s * PITCH + piece * 16) = v;
        }
    }
    // STAGING BOUNDS: clipped to the tensor [0, total) here as well; positions outside it are zeros and are never loaded.
    __device__ __forceinline__ static void stage_dy(char* ds, const bf16_t* __restrict__ dy, const Args& g, pos_t Q0, int c0, int tid) {
#pragma unroll
        for (int i = tid; i < WRUN * 8; i += 256) {
            const int s = i >> 3, piece = i & 7;
            const int64_t Q = Q0 + s;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (Q < g.total) v = *(const u32x4*)(dy + Q * g.C + c0 + piece * 8);
            *(u32x4*)(ds + s * PITCH + piece * 16) = v;
        }
    }
    // position -> dense pixel index, -1 for the border and beyond the tensor
    __device__ __forceinline__ static int dense_of(const Args& g, pos_t Q) {
        int dn = -1;
        if (Q < g.total) {
            const int q = (int)Q, b = q / g.HpWp, rem = q - b * g.HpWp, yy = rem / g.Wp, xx = rem - yy * g.Wp;
            if (yy >= 1 && yy <= g.H && xx >= 1 && xx <= g.W) dn = (b * g.H + yy - 1) * g.W + xx - 1;
        }
        return dn;
    }
    __device__ __forceinline__ static int tap_offset(int tap, int run, const Args& g) {
        return (g.W + 3 + (tap / 3 - 1) * g.Wp + (tap % 3 - 1)) * PITCH;
    }
};

struct S2 {
    static constexpr int STRIDE = 2;
    static constexpr int RUN = 64;         // plane positions per block of the forward = rows of one statistics block
    static constexpr int WRUN = 64;        // plane positions per staged run of the weight gradient
    using pos_t = int;
    struct Args {
        int H, W, C, OH, OW, Hh, Wh;       // Hh = OH + 1, Wh = OW + 1
        int total;                         // B Hh Wh plane positions
        int nruns, runs_per_split;         // weight gradient only
    };
    static Args geom(const fva_gconv_desc* d) {
        Args g;
        g.H = d->H; g.W = d->W; g.C = d->C; g.OH = out_of(d->H); g.OW = out_of(d->W); g.Hh = g.OH + 1; g.Wh = g.OW + 1;
        g.total = d->B * g.Hh * g.Wh;
        g.nruns = g.runs_per_split = 0;
        return g;
    }
    // positions staged in front of plane pl = 2 pr + pc of a run of `run` positions; pl = 4: all of them
    __host__ __device__ static constexpr int plane_base(int pl, int run, int Wh) {
        return pl == 0 ? 0 : pl == 1 ? run + Wh + 1 : pl == 2 ? 2 * run + 2 * Wh + 1 : pl == 3 ? 3 * run + 2 * Wh + 2 : 4 * run + 2 * Wh + 2;
    }
    __host__ __device__ static int staged(int run, const Args& g) { return plane_base(4, run, g.Wh); }

    // STAGING BOUNDS of the four plane ranges of the run [T0, T0 + run): whether an element exists is decided HERE, where its load is
    // issued -- T inside [0, total), row 2 i + pr <= H + 1 and column 2 j + pc <= W + 1 of image b < B: inside the halo tensor.  Everything
    // else is filled with zeros and never loaded.
    __device__ __forceinline__ static void stage(char* smem, const bf16_t* __restrict__ x, const Args& g, pos_t T0, int run, int c0, int tid) {
        const int n = (run + g.Wh + 1) * 8;
        for (int idx = tid; idx < n; idx += 256) {
            const int s = idx >> 3, piece = idx & 7;
            const int T = T0 + s;
            const bool in = T < g.total;
            const int bi = T / g.Wh, j = T - bi * g.Wh, b = bi / g.Hh, i = bi - b * g.Hh;
            const bf16_t* src = x + ((int64_t)(b * (g.H + 2) + 2 * i) * (g.W + 2) + 2 * j) * g.C + c0 + piece * 8;
#pragma unroll
            for (int pl = 0; pl < 4; ++pl) {
                const int pr = pl >> 1, pc = pl & 1;
                if (s < run + (pr ? 0 : g.Wh) + (pc ? 0 : 1)) {
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (in && 2 * i + pr <= g.H + 1 && 2 * j + pc <= g.W + 1) v = *(const u32x4*)(src + (int64_t)(pr * (g.W + 2) + pc) * g.C);
                    *(u32x4*)(smem + (plane_base(pl, run, g.Wh) + s) * PITCH + piece * 16) = v;
                }
            }
        }
    }
    // dy_T = dy_halo[b][i + 1][j + 1], i <= OH, j <= OW: inside the tensor for every T < total; zeros beyond the batch
    __device__ __forceinline__ static void stage_dy(char* ds, const bf16_t* __restrict__ dy, const Args& g, pos_t T0, int c0, int tid) {
#pragma unroll
        for (int idx = tid; idx < WRUN * 8; idx += 256) {
            const int s = idx >> 3, piece = idx & 7;
            const int T = T0 + s;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (T < g.total) {
                const int bi = T / g.Wh, j = T - bi * g.Wh, b = bi / g.Hh, i = bi - b * g.Hh;
                v = *(const u32x4*)(dy + ((int64_t)(b * (g.OH + 2) + i + 1) * (g.OW + 2) + j + 1) * g.C + c0 + piece * 8);
            }
            *(u32x4*)(ds + s * PITCH + piece * 16) = v;
        }
    }
    // position -> dense pixel index, -1 for i = OH, j = OW and beyond the batch
    __device__ __forceinline__ static int dense_of(const Args& g, pos_t T) {
        int dn = -1;
        if (T < g.total) {
            const int bi = T / g.Wh, j = T - bi * g.Wh, b = bi / g.Hh, i = bi - b * g.Hh;
            if (i < g.OH && j < g.OW) dn = (b * g.OH + i) * g.OW + j;
        }
        return dn;
    }
    __device__ __forceinline__ static int tap_offset(int tap, int run, const Args& g) {
        const int kh = tap / 3, kw = tap % 3;
        return (plane_base(2 * (kh & 1) + (kw & 1), run, g.Wh) + (kh >> 1) * g.Wh + (kw >> 1)) * PITCH;
    }
};

// The stride-2 data gradient runs over the dy-halo positions, not over the planes: a geometry of its own.
struct DGeom {
    int H, W, C, OH, OW;
    int total;                             // B (OH + 2)(OW + 2) dy-halo positions
};

// The stride-2 data gradient's taps in class order: class (py, px) = (0,0) {4}, (0,1) {3, 5}, (1,0) {1, 7}, (1,1) {0, 2, 6, 8}; tap = 3 kh + kw.
__host__ __device__ constexpr int dtap(int slot) { return (int)((0x862071534ll >> (4 * slot)) & 15); }
// first K-step of a class (class 4 = the end).  Cg >= 32: slot * (Cg / 32) + half.  Cg <= 16: step s holds slots 2 s - 1 and 2 s.
constexpr int class_step(int cg, int cls) {
    return cg >= 32 ? (cls == 0 ? 0 : cls == 1 ? 1 : cls == 2 ? 3 : cls == 3 ? 5 : 9) * (cg / 32) : (cls < 4 ? cls : 5);
}
// The tap of half-step h of the data-gradient table, -1 for the dead one.  Stride 1: the flipped taps, the dead half-step last.
// Stride 2: class order; at Cg <= 16 the dead half-step comes first, so that every class begins on a whole K-step.
template <int CG, int STRIDE>
__device__ __forceinline__ int dgrad_tap(int h) {
    if (STRIDE == 1) return h < 9 ? 8 - h : -1;
    const int slot = CG >= 32 ? h : h - 1;
    return slot >= 0 ? dtap(slot) : -1;
}

// ------------------------------------------------------------------------------------------------ what the kernels share
// the slab's packed taps: read once per block, 16 bytes per lane
template <int NS>
__device__ __forceinline__ void load_taps(bf16x8 (&wf)[NS], const bf16_t* __restrict__ wpack, int c0, int wv, int lane) {
    const bf16x8* wp = (const bf16x8*)wpack + (int64_t)(c0 / 16 + wv) * NS * 64 + lane;
#pragma unroll
    for (int s = 0; s < NS; ++s) wf[s] = wp[s * 64];
}

// K-step s as lane group g4 of wave wv reads it: the half-step (Cg >= 32: the tap; Cg <= 16: 0 ... 9, two to a step) and the first of its
// 8 channels among the block's 64
template <int CG>
__device__ __forceinline__ int step_half(int s, int g4) {
    if constexpr (CG >= 32) return s / (CG / 32);
    else return 2 * s + (g4 >> 1);
}
template <int CG>
__device__ __forceinline__ int step_channel(int s, int wv, int g4) {
    if constexpr (CG >= 32) return ((wv * 16) / CG) * CG + (s % (CG / 32)) * 32 + 8 * g4;
    else return wv * 16 + 8 * (g4 & 1);
}

// lane (g4, n) holds channels 16 wv + 4 g4 + r (r = 0 ... 3) of the positions 16 t + n: rounded to bf16 into dst, position-major
template <int NT>
__device__ __forceinline__ void tiles_to_lds(const f32x4 (&acc)[NT], char* dst, int n, int wv, int g4) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        u32x2 o;
        o[0] = cvt_pk_bf16(acc[t][0], acc[t][1]);
        o[1] = cvt_pk_bf16(acc[t][2], acc[t][3]);
        *(u32x2*)(dst + (t * 16 + n) * PITCH + (wv * 16 + 4 * g4) * 2) = o;
    }
}

// ------------------------------------------------------------------------------------------------ pack
template <int CG, int STRIDE>
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
        b = w[((int64_t)(gb + kc) * CG + (c - gb)) * 9 + dgrad_tap<CG, STRIDE>(tap)];
    } else {
        const int tap = 2 * step + (k >> 4), back = dgrad_tap<CG, STRIDE>(tap), kc = k & 15;
        if (kc / CG == m / CG) {                           // the diagonal blocks; everything else, and the dead half-steps, stay zero
            if (tap < 9) f = w[((int64_t)c * CG + kc % CG) * 9 + tap];
            if (back >= 0) b = w[((int64_t)(slab * 16 + kc) * CG + m % CG) * 9 + back];
        }
    }
    fwd[i] = (bf16_t)f;
    dgrad[i] = (bf16_t)b;
}

// ------------------------------------------------------------------------------------------------ forward (stride 1: and data gradient)
// src halo [B][H + 2][W + 2][C] bf16 (border 1); wpack [C / 16][steps][64][8]; out dense [pixels][C]; stats [blocks][2][C] or null
template <int CG, typename G>
__global__ __launch_bounds__(256) void gconv_mfma_fwd_kernel(const bf16_t* __restrict__ src, const bf16_t* __restrict__ wpack, bf16_t* __restrict__ out,
                                                             float* __restrict__ stats, typename G::Args g) {
    constexpr int NS = steps_of(CG);
    constexpr int RUN = G::RUN;
    constexpr int NT = RUN / 16;
    static_assert(RUN <= 256 && RUN % 16 == 0, "one thread per position of the run, whole tiles");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g4 = lane >> 4, n = lane & 15;
    int* dense = (int*)(smem + G::staged(RUN, g) * PITCH);
    const typename G::pos_t P0 = (typename G::pos_t)blockIdx.x * RUN;
    const int c0 = blockIdx.y * CH;

    bf16x8 wf[NS];
    load_taps(wf, wpack, c0, wv, lane);
    G::stage(smem, src, g, P0, RUN, c0, tid);
    if (RUN == 256 || tid < RUN) dense[tid] = G::dense_of(g, P0 + tid);      // 256 threads: at RUN = 256 no branch at all
    __syncthreads();

    // per-lane byte offset of the B fragment of tile 0 for every K-step: position n + shift(tap), 8 channels of the step
    int off[NS];
    bool dead_last = false;                                 // Cg <= 16: the tenth half-step (tap 9) of lanes 32 ... 63
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        int tap = step_half<CG>(s, g4);
        if (tap > 8) { tap = 8; dead_last = true; }
        off[s] = G::tap_offset(tap, RUN, g) + n * PITCH + step_channel<CG>(s, wv, g4) * 2;
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
    tiles_to_lds(acc, smem, n, wv, g4);
    __syncthreads();
#pragma unroll
    for (int i = tid; i < RUN * 8; i += 256) {
        const int p = i >> 3, piece = i & 7;
        const int dn = dense[p];
        if (dn >= 0) *(u32x4*)(out + (int64_t)dn * g.C + c0 + piece * 8) = *(const u32x4*)(smem + p * PITCH + piece * 16);
    }
}

// ------------------------------------------------------------------------------------------------ data gradient, stride 2
// dy halo [B][OH + 2][OW + 2][C] bf16 (zero border); wpack in class order; dx dense [B][H][W][C]
template <int CG>
__global__ __launch_bounds__(256) void gconv_mfma_s2_dgrad_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ wpack,
                                                                  bf16_t* __restrict__ dx, DGeom g) {
    constexpr int NS = steps_of(CG);
    constexpr int NT = DRUN / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g4 = lane >> 4, n = lane & 15;
    const int OWp = g.OW + 2, img = (g.OH + 2) * OWp;
    const int S = DRUN + OWp + 1;
    char* outb = smem + S * PITCH;
    int* pix = (int*)(outb + DRUN * PITCH);                 // pixel (2 i, 2 j) of the anchor, -1 if it anchors nothing
    int* odd = pix + DRUN;                                  // bit 0: row 2 i + 1 < H, bit 1: column 2 j + 1 < W
    const int64_t total = (int64_t)g.total;
    const int64_t R0 = (int64_t)blockIdx.x * DRUN;
    const int c0 = blockIdx.y * CH;

    bf16x8 wf[NS];
    load_taps(wf, wpack, c0, wv, lane);
    // STAGING BOUNDS: the staged range [R0, R0 + S) is clipped to the tensor [0, total) HERE; a position outside it is zeros, never loaded.
#pragma unroll 4
    for (int i = tid; i < S * 8; i += 256) {
        const int s = i >> 3, piece = i & 7;
        const int64_t R = R0 + s;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (R < total) v = *(const u32x4*)(dy + R * g.C + c0 + piece * 8);
        *(u32x4*)(smem + s * PITCH + piece * 16) = v;
    }
    if (tid < DRUN) {
        const int64_t R = R0 + tid;
        int px0 = -1, fl = 0;
        if (R < total) {
            const int q = (int)R, b = q / img, rem = q - b * img, r = rem / OWp, c = rem - r * OWp;
            if (r >= 1 && r <= g.OH && c >= 1 && c <= g.OW) {
                px0 = (b * g.H + 2 * (r - 1)) * g.W + 2 * (c - 1);
                fl = (2 * r - 1 < g.H ? 1 : 0) | (2 * c - 1 < g.W ? 2 : 0);
            }
        }
        pix[tid] = px0;
        odd[tid] = fl;
    }
    __syncthreads();

    // per-lane byte offset of the B fragment of tile 0 for every K-step: tap (kh, kw) reads dy-halo row + (kh == 0), column + (kw == 0)
    int off[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        int slot = step_half<CG>(s, g4) - (CG >= 32 ? 0 : 1);
        if (slot < 0) slot = 0;                             // the dead first half-step: its fragment is replaced by zeros below
        const int tap = dtap(slot);
        off[s] = (n + (tap / 3 == 0 ? OWp : 0) + (tap % 3 == 0 ? 1 : 0)) * PITCH + step_channel<CG>(s, wv, g4) * 2;
    }
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) {
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = class_step(CG, cls); s < class_step(CG, cls + 1); ++s) {
                bf16x8 b = *(const bf16x8*)(smem + off[s] + t * 16 * PITCH);
                if (CG < 32 && s == 0 && g4 < 2) b = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], b, acc[t], 0, 0, 0);
            }
        }
        if (cls > 0) __syncthreads();                       // the previous class has left the output area
        tiles_to_lds(acc, outb, n, wv, g4);
        __syncthreads();
        const int py = cls >> 1, pxl = cls & 1;
#pragma unroll
        for (int i = tid; i < DRUN * 8; i += 256) {
            const int p = i >> 3, piece = i & 7;
            const int px0 = pix[p], fl = odd[p];
            if (px0 >= 0 && (!py || (fl & 1)) && (!pxl || (fl & 2)))
                *(u32x4*)(dx + (int64_t)(px0 + py * g.W + pxl) * g.C + c0 + piece * 8) = *(const u32x4*)(outb + p * PITCH + piece * 16);
        }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// partial [split][C][CG][9] floats
template <int CG, typename G>
__global__ __launch_bounds__(256) void gconv_mfma_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ partial,
                                                               typename G::Args g) {
    constexpr int WRUN = G::WRUN;
    constexpr int NT = CG >= 16 ? CG / 16 : 1;              // tiles of 16 input channels the slab's outputs meet
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g4 = lane >> 4, n = lane & 15, q = n >> 2, p = n & 3;
    char* ds = smem + G::staged(WRUN, g) * PITCH;
    const int c0 = blockIdx.y * CH;
    const int cib = CG >= 16 ? ((wv * 16) / CG) * CG : wv * 16;      // first input channel (of the block's 64) the slab meets
    // K order inside a 32-position step: element j of lane group g4 is position 16 (j >> 2) + 4 g4 + (j & 3) -- the same on both
    // operands -- so that one transposed read of a 32-lane half takes 8 consecutive rows.
    const int rowoff = (4 * g4 + q) * PITCH + 8 * p;
    const int aoff = rowoff + wv * 16 * 2;
    int boff[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) boff[tap] = rowoff + G::tap_offset(tap, WRUN, g) + cib * 2;
    f32x4 acc[9][NT];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[tap][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int r0 = blockIdx.x * g.runs_per_split, r1 = min(g.nruns, r0 + g.runs_per_split);
    for (int run = r0; run < r1; ++run) {
        const typename G::pos_t P0 = (typename G::pos_t)run * WRUN;
        __syncthreads();
        G::stage(smem, x, g, P0, WRUN, c0, tid);
        G::stage_dy(ds, dy, g, P0, c0, tid);
        __syncthreads();
#pragma unroll 1
        for (int k0 = 0; k0 < WRUN; k0 += 32) {
            const char* da = ds + k0 * PITCH + aoff;
            const bf16x8 a = tr_pair(da, da + 16 * PITCH);
            const char* xb = smem + k0 * PITCH;
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
const char* const CONTRACT_S1 =
    "the MFMA path serves FVA_BF16 at stride 1 with in_pad == dy_pad == 1, C % 64 == 0, C <= 2048, C = groups * Cg, Cg in {4, 8, 16, 32, 64}, "
    "B (H + 2)(W + 2) < 2^31 and a map narrow enough to stage in 64 KB of LDS (W <= 70); ask fva_gconv_mfma_serves";
const char* const CONTRACT_S2 =
    "the stride-2 MFMA path serves FVA_BF16 at stride 2 with in_pad == dy_pad == 1, C % 64 == 0, C <= 2048, C = groups * Cg, Cg in {4, 8, 16, 32, 64}, "
    "B (H + 2)(W + 2) < 2^31 and a map narrow enough to stage in 64 KB of LDS (W <= 84); ask fva_gconv_mfma_s2_serves";

template <typename G>
int fwd_lds(const typename G::Args& g) { return G::staged(G::RUN, g) * PITCH + G::RUN * 4; }
template <typename G>
int wgrad_lds(const typename G::Args& g) { return (G::staged(G::WRUN, g) + G::WRUN) * PITCH; }
int dgrad_s2_lds(int OW) { return (2 * DRUN + OW + 3) * PITCH + 2 * DRUN * 4; }

template <typename G>
bool lds_fits(const fva_gconv_desc* d) {
    const typename G::Args g = G::geom(d);
    return fwd_lds<G>(g) <= LDS_MAX && wgrad_lds<G>(g) <= LDS_MAX;
}

bool serves(const fva_gconv_desc* d, int stride) {
    if (!d || d->dtype != FVA_BF16 || d->stride != stride || d->in_pad != 1 || d->dy_pad != 1) return false;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->C % 64 || d->C > 2048) return false;
    const int cg = d->groups > 0 && d->C % d->groups == 0 ? d->C / d->groups : 0;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64) return false;
    if (d->W > 4096 || d->H > (1 << 24) || (int64_t)d->B * (d->H + 2) * (d->W + 2) >= (1ll << 31)) return false;
    return stride == 1 ? lds_fits<S1>(d) : lds_fits<S2>(d) && dgrad_s2_lds(out_of(d->W)) <= LDS_MAX;
}

int refuse(const char* who, const fva_gconv_desc* d, int stride) {
    if (!d) return fva_fail(FVA_ERR_ARG, "%s: null descriptor", who);
    return fva_fail(FVA_ERR_ARG, "%s: %s; got dtype %d, B %d, H %d, W %d, C %d, groups %d, stride %d, in_pad %d, dy_pad %d", who,
                    stride == 1 ? CONTRACT_S1 : CONTRACT_S2, d->dtype, d->B, d->H, d->W, d->C, d->groups, d->stride, d->in_pad, d->dy_pad);
}

int64_t pack_elems(const fva_gconv_desc* d) { return (int64_t)(d->C / 16) * steps_of(d->C / d->groups) * 512; }

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

template <typename G>
WPlan wgrad_plan(const fva_gconv_desc* d) { return wgrad_plan_of(cdiv(G::geom(d).total, G::WRUN), d->C, d->C / d->groups); }

template <typename G>
int64_t pack_bytes(const fva_gconv_desc* d) { return serves(d, G::STRIDE) ? pack_elems(d) * 2 : 0; }

template <typename G>
int pack(const char* who, const fva_gconv_desc* d, const float* w_oihw, void* wpack_fwd, void* wpack_dgrad, void* stream) {
    if (!serves(d, G::STRIDE)) return refuse(who, d, G::STRIDE);
    if (!w_oihw || !wpack_fwd || !wpack_dgrad) return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    const int n = (int)pack_elems(d);
    by_cg(d->C / d->groups, [&](auto cg) {
        hipLaunchKernelGGL((gconv_mfma_pack_kernel<decltype(cg)::value, G::STRIDE>), dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w_oihw,
                           (bf16_t*)wpack_fwd, (bf16_t*)wpack_dgrad, n);
    });
    FVA_LAUNCH_CHECK("gconv_mfma_pack_kernel");
    return FVA_OK;
}

template <typename G>
int32_t stat_blocks(const fva_gconv_desc* d) { return serves(d, G::STRIDE) ? cdiv(G::geom(d).total, G::RUN) : 0; }

// `what`: the kernel in the role it is launched in, for the launch check
template <typename G>
int fwd(const char* who, const char* what, const fva_gconv_desc* d, const void* src, const void* wpack, void* out, float* stats, void* stream) {
    if (!serves(d, G::STRIDE)) return refuse(who, d, G::STRIDE);
    if (!src || !wpack || !out) return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    const typename G::Args g = G::geom(d);
    const dim3 grid(cdiv(g.total, G::RUN), d->C / CH);
    by_cg(d->C / d->groups, [&](auto cg) {
        hipLaunchKernelGGL((gconv_mfma_fwd_kernel<decltype(cg)::value, G>), grid, dim3(256), fwd_lds<G>(g), (hipStream_t)stream, (const bf16_t*)src,
                           (const bf16_t*)wpack, (bf16_t*)out, stats, g);
    });
    FVA_LAUNCH_CHECK(what);
    return FVA_OK;
}

template <typename G>
int64_t wgrad_workspace(const fva_gconv_desc* d) {
    if (!serves(d, G::STRIDE)) return 0;
    return (int64_t)wgrad_plan<G>(d).splits * d->C * (d->C / d->groups) * 9 * 4;
}

template <typename G>
int wgrad(const char* who, const fva_gconv_desc* d, const void* x, const void* dy, float* dw_oihw, void* ws, int64_t ws_bytes, void* stream) {
    if (!serves(d, G::STRIDE)) return refuse(who, d, G::STRIDE);
    if (!x || !dy || !dw_oihw || !ws) return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    const WPlan p = wgrad_plan<G>(d);
    const int cg = d->C / d->groups;
    const int n = d->C * cg * 9;
    if (ws_bytes < (int64_t)p.splits * n * 4)
        return fva_fail(FVA_ERR_WORKSPACE, "%s: workspace of %lld bytes, %s_workspace() = %lld", who, (long long)ws_bytes, who,
                        (long long)p.splits * n * 4);
    typename G::Args g = G::geom(d);
    g.nruns = p.nruns; g.runs_per_split = p.runs_per_split;
    const dim3 grid(p.splits, d->C / CH);
    by_cg(cg, [&](auto cgc) {
        hipLaunchKernelGGL((gconv_mfma_wgrad_kernel<decltype(cgc)::value, G>), grid, dim3(256), wgrad_lds<G>(g), (hipStream_t)stream, (const bf16_t*)x,
                           (const bf16_t*)dy, (float*)ws, g);
    });
    FVA_LAUNCH_CHECK("gconv_mfma_wgrad_kernel");
    // partial [splits][n] -> dw [n]
    hipLaunchKernelGGL(gconv_mfma_wgrad_reduce_kernel, dim3(cdiv(n, RED_E)), dim3(RED_E * RED_S), 0, (hipStream_t)stream, (const float*)ws, dw_oihw, n,
                       p.splits);
    FVA_LAUNCH_CHECK("gconv_mfma_wgrad_reduce_kernel");
    return FVA_OK;
}

int dgrad_s2(const char* who, const fva_gconv_desc* d, const void* dy, const void* wpack_dgrad, void* dx, void* stream) {
    if (!serves(d, 2)) return refuse(who, d, 2);
    if (!dy || !wpack_dgrad || !dx) return fva_fail(FVA_ERR_ARG, "%s: null pointer", who);
    DGeom g;
    g.H = d->H; g.W = d->W; g.C = d->C; g.OH = out_of(d->H); g.OW = out_of(d->W);
    g.total = d->B * (g.OH + 2) * (g.OW + 2);
    const dim3 grid(cdiv(g.total, DRUN), d->C / CH);
    by_cg(d->C / d->groups, [&](auto cg) {
        hipLaunchKernelGGL((gconv_mfma_s2_dgrad_kernel<decltype(cg)::value>), grid, dim3(256), dgrad_s2_lds(g.OW), (hipStream_t)stream, (const bf16_t*)dy,
                           (const bf16_t*)wpack_dgrad, (bf16_t*)dx, g);
    });
    FVA_LAUNCH_CHECK("gconv_mfma_s2_dgrad_kernel");
    return FVA_OK;
}

}  // namespace

extern "C" {

int fva_gconv_mfma_serves(const fva_gconv_desc* d) { return serves(d, 1) ? 1 : 0; }
int64_t fva_gconv_mfma_pack_bytes(const fva_gconv_desc* d) { return pack_bytes<S1>(d); }
int fva_gconv_mfma_pack(const fva_gconv_desc* d, const float* w_oihw, void* wpack_fwd, void* wpack_dgrad, void* stream) {
    return pack<S1>("fva_gconv_mfma_pack", d, w_oihw, wpack_fwd, wpack_dgrad, stream);
}
int32_t fva_gconv_mfma_stat_blocks(const fva_gconv_desc* d) { return stat_blocks<S1>(d); }
int fva_gconv_mfma_fwd(const fva_gconv_desc* d, const void* x, const void* wpack_fwd, void* y, float* stats_partial, void* stream) {
    return fwd<S1>("fva_gconv_mfma_fwd", "gconv_mfma_fwd_kernel (stride 1, forward)", d, x, wpack_fwd, y, stats_partial, stream);
}
int fva_gconv_mfma_dgrad(const fva_gconv_desc* d, const void* dy, const void* wpack_dgrad, void* dx, void* stream) {
    return fwd<S1>("fva_gconv_mfma_dgrad", "gconv_mfma_fwd_kernel (stride 1, data gradient)", d, dy, wpack_dgrad, dx, nullptr, stream);
}
int64_t fva_gconv_mfma_wgrad_workspace(const fva_gconv_desc* d) { return wgrad_workspace<S1>(d); }
int fva_gconv_mfma_wgrad(const fva_gconv_desc* d, const void* x, const void* dy, float* dw_oihw, void* ws, int64_t ws_bytes, void* stream) {
    return wgrad<S1>("fva_gconv_mfma_wgrad", d, x, dy, dw_oihw, ws, ws_bytes, stream);
}

int fva_gconv_mfma_s2_serves(const fva_gconv_desc* d) { return serves(d, 2) ? 1 : 0; }
int64_t fva_gconv_mfma_s2_pack_bytes(const fva_gconv_desc* d) { return pack_bytes<S2>(d); }
int fva_gconv_mfma_s2_pack(const fva_gconv_desc* d, const float* w_oihw, void* wpack_fwd, void* wpack_dgrad, void* stream) {
    return pack<S2>("fva_gconv_mfma_s2_pack", d, w_oihw, wpack_fwd, wpack_dgrad, stream);
}
int32_t fva_gconv_mfma_s2_stat_blocks(const fva_gconv_desc* d) { return stat_blocks<S2>(d); }
int fva_gconv_mfma_s2_fwd(const fva_gconv_desc* d, const void* x, const void* wpack_fwd, void* y, float* stats_partial, void* stream) {
    return fwd<S2>("fva_gconv_mfma_s2_fwd", "gconv_mfma_fwd_kernel (stride 2)", d, x, wpack_fwd, y, stats_partial, stream);
}
int fva_gconv_mfma_s2_dgrad(const fva_gconv_desc* d, const void* dy, const void* wpack_dgrad, void* dx, void* stream) {
    return dgrad_s2("fva_gconv_mfma_s2_dgrad", d, dy, wpack_dgrad, dx, stream);
}
int64_t fva_gconv_mfma_s2_wgrad_workspace(const fva_gconv_desc* d) { return wgrad_workspace<S2>(d); }
int fva_gconv_mfma_s2_wgrad(const fva_gconv_desc* d, const void* x, const void* dy, float* dw_oihw, void* ws, int64_t ws_bytes, void* stream) {
    return wgrad<S2>("fva_gconv_mfma_s2_wgrad", d, x, dy, dw_oihw, ws, ws_bytes, stream);
}

}  // extern "C"
