// Grouped 3x3 convolution of STRIDE 2 on the matrix units: bf16 tensors, border 1 (the first conv2 of res3, res4 and res5 of a ResNeXt).
// Forward with BatchNorm statistics, data gradient, weight gradient and the pack pass, behind entry points of their own
// (fva_gconv_mfma_s2_*) beside grouped_mfma.hip, whose stride-1 kernels refuse these layers.
//
// PARITY PLANES.  At stride 2 a tap is no constant shift of the padded-linear position any more.  Split the padded input xp [B][H + 2][W + 2]
// into four planes P[pr][pc][b][i][j] = xp[b][2 i + pr][2 j + pc], i < Hh = OH + 1, j < Wh = OW + 1 (zero where 2 i + pr > H + 1 or
// 2 j + pc > W + 1), and with the plane-linear position T = (b Hh + i) Wh + j
//       y[T] = sum over (kh, kw) of P[kh & 1][kw & 1][T + (kh >> 1) Wh + (kw >> 1)] w[kh][kw],        real where i < OH and j < OW:
// every tap is a constant shift again, inside one of four planes.  The planes never exist in HBM: they are formed while staging (a position
// of a plane is 128 contiguous bytes of the halo tensor), and de-interleaving there is what keeps the LDS reads free of conflicts -- the 16
// neighbouring outputs of a tile read 16 consecutive positions of ONE plane at the 160-byte pitch of grouped_mfma.hip, 16 different 16-byte
// slots; read from an interleaved row they would sit 320 bytes apart, 4 to a slot.
//
//   forward: a block owns RUN = 64 consecutive T x 64 channels and stages plane (0,0) over [T0, T0 + RUN + Wh + 1), (0,1) over + Wh,
//       (1,0) over + 1, (1,1) over + 0: (4 RUN + 2 Wh + 2) positions, 51 KB at Wh = 29.  One wave per 16-channel slab, the packed taps in
//       registers, the K-steps and the table exactly those of the stride-1 forward; epilogue as there (statistics of the real outputs from
//       the unrounded accumulators in double, one row [2][C] per block; bf16 results through LDS, 16-byte pieces).  The non-real positions
//       cost (OH + 1)(OW + 1) / (OH OW) of the MFMAs.
//   data gradient: by the parity (py, px) of (iy, ix) a dx pixel meets 1, 2, 2 or 4 taps, each a constant shift (0, 1, OW + 2, OW + 3) of
//       the dy-halo position anchored at R = (b, i + 1, j + 1), iy = 2 i + py, ix = 2 j + px.  A block owns DRUN = 128 consecutive R x 64
//       channels, stages dy[R0, R0 + DRUN + OW + 3) once, and LOOPS the four classes over that one staging: per class its own packed
//       fragments (the table is in class order), one set of tile accumulators, the class's pixels out through a second LDS area.  9 taps per
//       anchor in all: no padded FLOPs beyond the Cg <= 16 diagonal (2 taps per K-step inside a class: 1 + 1 + 1 + 2 = 5 steps, the first
//       half-step zero).  Every dx element is written exactly once.
//   weight gradient: dw[co][ci][tap] = sum over T of dy_T[co] P[kh & 1][kw & 1][T + shift][ci], dy_T = dy_halo[b][i + 1][j + 1] (always
//       inside the tensor; zero by contract at i = OH and j = OW, so a non-real T adds exact zeros).  Per run of WRUN = 64 T the block
//       stages dy_T and the four plane ranges position-major and reads both operands with ds_read_b64_tr_b16 as the stride-1 kernel does
//       (M = 16 co, N = 16 ci, K = 32 positions, one K permutation on both sides); fp32 partials [split][C][Cg][9], then the shared reduce.
//   pack: fp32 OIHW -> the forward table in the stride-1 layout and the data-gradient table in class order (include/fastvision_amd.h).
//
// No atomics, fixed order everywhere: the same bits on every run.  Everything fits the default 64 KB of LDS; a map too wide for the weight
// gradient's five staged ranges is not served (fva_gconv_mfma_s2_serves).
#include "grouped_mfma_common.h"

namespace {

constexpr int RUN = 64;        // plane positions per block of the forward = rows of one statistics block
constexpr int DRUN = 128;      // dy-halo positions per block of the data gradient
constexpr int WRUN = 64;       // plane positions per staged run of the weight gradient

// The data gradient's taps in class order: class (py, px) = (0,0) {4}, (0,1) {3, 5}, (1,0) {1, 7}, (1,1) {0, 2, 6, 8}; tap = 3 kh + kw.
constexpr int dtap(int slot) { return (int)((0x862071534ll >> (4 * slot)) & 15); }
// first K-step of a class (class 4 = the end).  Cg >= 32: slot * (Cg / 32) + half.  Cg <= 16: step s holds slots 2 s - 1 and 2 s.
constexpr int class_step(int cg, int cls) {
    return cg >= 32 ? (cls == 0 ? 0 : cls == 1 ? 1 : cls == 2 ? 3 : cls == 3 ? 5 : 9) * (cg / 32) : (cls < 4 ? cls : 5);
}

struct SGeom {
    int H, W, C, OH, OW, Hh, Wh;      // Hh = OH + 1, Wh = OW + 1
    int total;                        // B Hh Wh plane positions
    int nruns, runs_per_split;        // weight gradient only
};

// positions staged in front of plane pl = 2 pr + pc of a run of `run` positions; pl = 4: all of them
__device__ __host__ constexpr int plane_base(int pl, int run, int Wh) {
    return pl == 0 ? 0 : pl == 1 ? run + Wh + 1 : pl == 2 ? 2 * run + 2 * Wh + 1 : pl == 3 ? 3 * run + 2 * Wh + 2 : 4 * run + 2 * Wh + 2;
}

// STAGING BOUNDS of the four plane ranges of the run [T0, T0 + run): whether an element exists is decided HERE, where its load is issued --
// T inside [0, total), row 2 i + pr <= H + 1 and column 2 j + pc <= W + 1 of image b < B: inside the halo tensor.  Everything else is
// filled with zeros and never loaded.
__device__ __forceinline__ void stage_planes(char* smem, const bf16_t* __restrict__ x, const SGeom& g, int T0, int run, int c0, int tid) {
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

// byte offset, from the first staged position of a run, of what tap 3 kh + kw reads for the run's first output
__device__ __forceinline__ int tap_offset(int tap, int run, int Wh) {
    const int kh = tap / 3, kw = tap % 3;
    return (plane_base(2 * (kh & 1) + (kw & 1), run, Wh) + (kh >> 1) * Wh + (kw >> 1)) * PITCH;
}

// ------------------------------------------------------------------------------------------------ pack
template <int CG>
__global__ __launch_bounds__(256) void gconv_s2_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ fwd, bf16_t* __restrict__ dgrad, int n) {
    constexpr int NS = steps_of(CG);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = i & 7, lane = (i >> 3) & 63, step = (i >> 9) % NS, slab = (i >> 9) / NS;
    const int m = lane & 15, k = 8 * (lane >> 4) + j;
    const int c = slab * 16 + m;                           // the row's output channel (data gradient: the input channel dx is taken for)
    float f = 0.f, b = 0.f;
    if (CG >= 32) {
        const int slot = step / (CG / 32), kc = (step % (CG / 32)) * 32 + k, gb = (c / CG) * CG;      // forward: the slot is the tap
        f = w[((int64_t)c * CG + kc) * 9 + slot];
        b = w[((int64_t)(gb + kc) * CG + (c - gb)) * 9 + dtap(slot)];
    } else {
        const int tap = 2 * step + (k >> 4), slot = tap - 1, kc = k & 15;
        if (kc / CG == m / CG) {                           // the diagonal blocks; everything else, and the two dead half-steps, stay zero
            if (tap < 9) f = w[((int64_t)c * CG + kc % CG) * 9 + tap];
            if (slot >= 0) b = w[((int64_t)(slab * 16 + kc) * CG + m % CG) * 9 + dtap(slot)];
        }
    }
    fwd[i] = (bf16_t)f;
    dgrad[i] = (bf16_t)b;
}

// ------------------------------------------------------------------------------------------------ forward
// x halo [B][H + 2][W + 2][C] bf16; wpack [C / 16][steps][64][8]; y dense [B OH OW][C]; stats [blocks][2][C] or null
template <int CG>
__global__ __launch_bounds__(256) void gconv_s2_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wpack, bf16_t* __restrict__ y,
                                                           float* __restrict__ stats, SGeom g) {
    constexpr int NS = steps_of(CG);
    constexpr int NT = RUN / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g4 = lane >> 4, n = lane & 15;
    int* dense = (int*)(smem + plane_base(4, RUN, g.Wh) * PITCH);
    const int T0 = blockIdx.x * RUN;
    const int c0 = blockIdx.y * CH;

    bf16x8 wf[NS];                                          // the slab's packed taps: read once per block, 16 bytes per lane
    {
        const bf16x8* wp = (const bf16x8*)wpack + (int64_t)(c0 / 16 + wv) * NS * 64 + lane;
#pragma unroll
        for (int s = 0; s < NS; ++s) wf[s] = wp[s * 64];
    }
    stage_planes(smem, x, g, T0, RUN, c0, tid);
    if (tid < RUN) {                                        // position -> dense pixel index, -1 for i = OH, j = OW and beyond the batch
        const int T = T0 + tid;
        int dn = -1;
        if (T < g.total) {
            const int bi = T / g.Wh, j = T - bi * g.Wh, b = bi / g.Hh, i = bi - b * g.Hh;
            if (i < g.OH && j < g.OW) dn = (b * g.OH + i) * g.OW + j;
        }
        dense[tid] = dn;
    }
    __syncthreads();

    // per-lane byte offset of the B fragment of tile 0 for every K-step: position n + shift(tap) of the tap's plane, 8 channels of the step
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
        off[s] = tap_offset(tap, RUN, g.Wh) + n * PITCH + ch * 2;
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
    __syncthreads();                                        // the staged planes are dead: the block's bf16 results take their place
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
        if (dn >= 0) *(u32x4*)(y + (int64_t)dn * g.C + c0 + piece * 8) = *(const u32x4*)(smem + p * PITCH + piece * 16);
    }
}

// ------------------------------------------------------------------------------------------------ data gradient
// dy halo [B][OH + 2][OW + 2][C] bf16 (zero border); wpack in class order; dx dense [B][H][W][C]
template <int CG>
__global__ __launch_bounds__(256) void gconv_s2_dgrad_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ wpack, bf16_t* __restrict__ dx,
                                                             SGeom g) {
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
    const int64_t total = (int64_t)g.total;                 // here: B (OH + 2)(OW + 2) dy-halo positions
    const int64_t R0 = (int64_t)blockIdx.x * DRUN;
    const int c0 = blockIdx.y * CH;

    bf16x8 wf[NS];
    {
        const bf16x8* wp = (const bf16x8*)wpack + (int64_t)(c0 / 16 + wv) * NS * 64 + lane;
#pragma unroll
        for (int s = 0; s < NS; ++s) wf[s] = wp[s * 64];
    }
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
        int slot, ch;
        if (CG >= 32) {
            slot = s / (CG / 32);
            ch = ((wv * 16) / CG) * CG + (s % (CG / 32)) * 32 + 8 * g4;
        } else {
            slot = 2 * s + (g4 >> 1) - 1;
            ch = wv * 16 + 8 * (g4 & 1);
            if (slot < 0) slot = 0;                         // the dead first half-step: its fragment is replaced by zeros below
        }
        const int tap = dtap(slot);
        off[s] = (n + (tap / 3 == 0 ? OWp : 0) + (tap % 3 == 0 ? 1 : 0)) * PITCH + ch * 2;
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
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            u32x2 o;
            o[0] = cvt_pk_bf16(acc[t][0], acc[t][1]);
            o[1] = cvt_pk_bf16(acc[t][2], acc[t][3]);
            *(u32x2*)(outb + (t * 16 + n) * PITCH + (wv * 16 + 4 * g4) * 2) = o;
        }
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
template <int CG>
__global__ __launch_bounds__(256) void gconv_s2_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ partial,
                                                             SGeom g) {
    constexpr int NT = CG >= 16 ? CG / 16 : 1;              // tiles of 16 input channels the slab's outputs meet
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g4 = lane >> 4, n = lane & 15, q = n >> 2, p = n & 3;
    char* ds = smem + plane_base(4, WRUN, g.Wh) * PITCH;
    const int c0 = blockIdx.y * CH;
    const int cib = CG >= 16 ? ((wv * 16) / CG) * CG : wv * 16;      // first input channel (of the block's 64) the slab meets
    // K order inside a 32-position step as in the stride-1 kernel: element j of lane group g4 is position 16 (j >> 2) + 4 g4 + (j & 3)
    // on both operands, so that one transposed read of a 32-lane half takes 8 consecutive rows.
    const int rowoff = (4 * g4 + q) * PITCH + 8 * p;
    const int aoff = rowoff + wv * 16 * 2;
    int boff[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) boff[tap] = rowoff + tap_offset(tap, WRUN, g.Wh) + cib * 2;
    f32x4 acc[9][NT];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[tap][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int r0 = blockIdx.x * g.runs_per_split, r1 = min(g.nruns, r0 + g.runs_per_split);
    for (int run = r0; run < r1; ++run) {
        const int T0 = run * WRUN;
        __syncthreads();
        stage_planes(smem, x, g, T0, WRUN, c0, tid);
        // dy_T = dy_halo[b][i + 1][j + 1], i <= OH, j <= OW: inside the tensor for every T < total; zeros beyond the batch
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

// ------------------------------------------------------------------------------------------------ host
const char* const CONTRACT =
    "the stride-2 MFMA path serves FVA_BF16 at stride 2 with in_pad == dy_pad == 1, C % 64 == 0, C <= 2048, C = groups * Cg, Cg in {4, 8, 16, 32, 64}, "
    "B (H + 2)(W + 2) < 2^31 and a map narrow enough to stage in 64 KB of LDS (W <= 84); ask fva_gconv_mfma_s2_serves";

int out_of(int n) { return (n - 1) / 2 + 1; }
int fwd_lds(int Wh) { return plane_base(4, RUN, Wh) * PITCH + RUN * 4; }
int dgrad_lds(int OW) { return (2 * DRUN + OW + 3) * PITCH + 2 * DRUN * 4; }
int wgrad_lds(int Wh) { return (plane_base(4, WRUN, Wh) + WRUN) * PITCH; }

bool serves(const fva_gconv_desc* d) {
    if (!d || d->dtype != FVA_BF16 || d->stride != 2 || d->in_pad != 1 || d->dy_pad != 1) return false;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->C % 64 || d->C > 2048) return false;
    const int cg = d->groups > 0 && d->C % d->groups == 0 ? d->C / d->groups : 0;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64) return false;
    if (d->W > 4096 || d->H > (1 << 24) || (int64_t)d->B * (d->H + 2) * (d->W + 2) >= (1ll << 31)) return false;
    const int OW = out_of(d->W);
    return fwd_lds(OW + 1) <= LDS_MAX && dgrad_lds(OW) <= LDS_MAX && wgrad_lds(OW + 1) <= LDS_MAX;
}

int refuse(const char* who, const fva_gconv_desc* d) {
    if (!d) return fva_fail(FVA_ERR_ARG, "%s: null descriptor", who);
    return fva_fail(FVA_ERR_ARG, "%s: %s; got dtype %d, B %d, H %d, W %d, C %d, groups %d, stride %d, in_pad %d, dy_pad %d", who, CONTRACT, d->dtype, d->B,
                    d->H, d->W, d->C, d->groups, d->stride, d->in_pad, d->dy_pad);
}

SGeom geom_of(const fva_gconv_desc* d) {
    SGeom g;
    g.H = d->H; g.W = d->W; g.C = d->C; g.OH = out_of(d->H); g.OW = out_of(d->W); g.Hh = g.OH + 1; g.Wh = g.OW + 1;
    g.total = d->B * g.Hh * g.Wh;
    g.nruns = g.runs_per_split = 0;
    return g;
}

int64_t pack_elems(const fva_gconv_desc* d) { return (int64_t)(d->C / 16) * steps_of(d->C / d->groups) * 512; }

WPlan wgrad_plan(const fva_gconv_desc* d) { return wgrad_plan_of(cdiv(geom_of(d).total, WRUN), d->C, d->C / d->groups); }

}  // namespace

extern "C" {

int fva_gconv_mfma_s2_serves(const fva_gconv_desc* d) { return serves(d) ? 1 : 0; }

int64_t fva_gconv_mfma_s2_pack_bytes(const fva_gconv_desc* d) { return serves(d) ? pack_elems(d) * 2 : 0; }

int fva_gconv_mfma_s2_pack(const fva_gconv_desc* d, const float* w_oihw, void* wpack_fwd, void* wpack_dgrad, void* stream) {
    if (!serves(d)) return refuse("fva_gconv_mfma_s2_pack", d);
    if (!w_oihw || !wpack_fwd || !wpack_dgrad) return fva_fail(FVA_ERR_ARG, "fva_gconv_mfma_s2_pack: null pointer");
    const int n = (int)pack_elems(d);
    by_cg(d->C / d->groups, [&](auto cg) {
        hipLaunchKernelGGL((gconv_s2_pack_kernel<decltype(cg)::value>), dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w_oihw, (bf16_t*)wpack_fwd,
                           (bf16_t*)wpack_dgrad, n);
    });
    FVA_LAUNCH_CHECK("gconv_s2_pack_kernel");
    return FVA_OK;
}

int32_t fva_gconv_mfma_s2_stat_blocks(const fva_gconv_desc* d) { return serves(d) ? cdiv(geom_of(d).total, RUN) : 0; }

int fva_gconv_mfma_s2_fwd(const fva_gconv_desc* d, const void* x, const void* wpack_fwd, void* y, float* stats_partial, void* stream) {
    if (!serves(d)) return refuse("fva_gconv_mfma_s2_fwd", d);
    if (!x || !wpack_fwd || !y) return fva_fail(FVA_ERR_ARG, "fva_gconv_mfma_s2_fwd: null pointer");
    const SGeom g = geom_of(d);
    const dim3 grid(cdiv(g.total, RUN), d->C / CH);
    by_cg(d->C / d->groups, [&](auto cg) {
        hipLaunchKernelGGL((gconv_s2_fwd_kernel<decltype(cg)::value>), grid, dim3(256), fwd_lds(g.Wh), (hipStream_t)stream, (const bf16_t*)x,
                           (const bf16_t*)wpack_fwd, (bf16_t*)y, stats_partial, g);
    });
    FVA_LAUNCH_CHECK("gconv_s2_fwd_kernel");
    return FVA_OK;
}

int fva_gconv_mfma_s2_dgrad(const fva_gconv_desc* d, const void* dy, const void* wpack_dgrad, void* dx, void* stream) {
    if (!serves(d)) return refuse("fva_gconv_mfma_s2_dgrad", d);
    if (!dy || !wpack_dgrad || !dx) return fva_fail(FVA_ERR_ARG, "fva_gconv_mfma_s2_dgrad: null pointer");
    SGeom g = geom_of(d);
    g.total = d->B * (g.OH + 2) * (g.OW + 2);               // the data gradient runs over the dy-halo positions
    const dim3 grid(cdiv(g.total, DRUN), d->C / CH);
    by_cg(d->C / d->groups, [&](auto cg) {
        hipLaunchKernelGGL((gconv_s2_dgrad_kernel<decltype(cg)::value>), grid, dim3(256), dgrad_lds(g.OW), (hipStream_t)stream, (const bf16_t*)dy,
                           (const bf16_t*)wpack_dgrad, (bf16_t*)dx, g);
    });
    FVA_LAUNCH_CHECK("gconv_s2_dgrad_kernel");
    return FVA_OK;
}

int64_t fva_gconv_mfma_s2_wgrad_workspace(const fva_gconv_desc* d) {
    if (!serves(d)) return 0;
    return (int64_t)wgrad_plan(d).splits * d->C * (d->C / d->groups) * 9 * 4;
}

int fva_gconv_mfma_s2_wgrad(const fva_gconv_desc* d, const void* x, const void* dy, float* dw_oihw, void* ws, int64_t ws_bytes, void* stream) {
    if (!serves(d)) return refuse("fva_gconv_mfma_s2_wgrad", d);
    if (!x || !dy || !dw_oihw || !ws) return fva_fail(FVA_ERR_ARG, "fva_gconv_mfma_s2_wgrad: null pointer");
    const WPlan p = wgrad_plan(d);
    const int cg = d->C / d->groups;
    const int n = d->C * cg * 9;
    if (ws_bytes < (int64_t)p.splits * n * 4)
        return fva_fail(FVA_ERR_WORKSPACE, "fva_gconv_mfma_s2_wgrad: workspace of %lld bytes, fva_gconv_mfma_s2_wgrad_workspace() = %lld",
                        (long long)ws_bytes, (long long)p.splits * n * 4);
    SGeom g = geom_of(d);
    g.nruns = p.nruns; g.runs_per_split = p.runs_per_split;
    const dim3 grid(p.splits, d->C / CH);
    by_cg(cg, [&](auto cgc) {
        hipLaunchKernelGGL((gconv_s2_wgrad_kernel<decltype(cgc)::value>), grid, dim3(256), wgrad_lds(g.Wh), (hipStream_t)stream, (const bf16_t*)x,
                           (const bf16_t*)dy, (float*)ws, g);
    });
    FVA_LAUNCH_CHECK("gconv_s2_wgrad_kernel");
    return launch_wgrad_reduce(ws, dw_oihw, n, p.splits, stream);
}

}  // extern "C"
