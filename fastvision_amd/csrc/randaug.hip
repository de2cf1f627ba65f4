// RandAugment and RandomErasing on the device for gfx950 (not in the reference: the per-image augmentation of the large-batch ImageNet
// recipe, which no DataLoader worker pool feeds at the rates of the classifiers here).  uint8 canvases [B][H][W][3] in, the same out.
//   fva_randaug_plan        a one-block tick kernel: for every (image, round) an op, uniform over the enabled ones, and its signed value,
//                           from Philox-4x32-10 keyed by (seed, call counter) in device memory; advances the counter (the protocol of
//                           fva_mix_plan: a captured graph draws a new plan on every replay)
//   fva_randaug_plan_fixed  copies a caller-given [B][N] op / value table into the plan
//   fva_randaug_stats       round r: a block owns a strip of one image and builds the R, G, B and grey histograms of the strip per wave in
//                           LDS, then adds them into the image's int32 [4][256] with integer atomics (order-independent: deterministic).
//                           Blocks of an image whose op needs no statistics leave after reading the plan.
//   fva_randaug_apply       round r: a block owns a 32 x 64 output tile of one image and reads the image's op ONCE -- one switch per block,
//                           no per-pixel divergence.  Byte maps (Identity, Brightness, Contrast, Solarize, Posterize, AutoContrast,
//                           Equalize) become a 3 x 256 table in LDS, built from the plan value and the image's histograms, and the tile
//                           streams through it 48 bytes (16 pixels, three 16-byte accesses) per thread.  Color blends every pixel with
//                           its own grey in the same units.  Sharpness and the five geometric ops stage their source window in LDS.
//   fva_random_erase        torchvision's RandomErasing on the normalised planar batch: box per image drawn on the device, constant or
//                           N(0, 1) Philox noise, one pass, in place (only the boxes are touched) or into `out`.
// Who clears the histograms: the workspace holds TWO sets and two words {a, b}.  A stats launch reads g = a, adds into set g & 1, returns
// set (g + 1) & 1 -- read by the apply launch before it -- to zero, and writes b = g + 1; the apply launch reads g = b - 1 and writes
// a = b.  Each word is written by one kind of launch and read by the other, so no launch reads a word that a block of its own writes, and
// the rule holds across calls and graph replays with no host state.  A stats launch and an apply launch alternate on one stream.
// Compiled with -ffp-contract=off: the op arithmetic is the fp32 sequence stated in include/fastvision_amd.h, product by product.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

enum { OP_IDENTITY = 0, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y, OP_ROTATE, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST, OP_SHARPNESS,
       OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST, OP_EQUALIZE, NUM_OPS };
static_assert(NUM_OPS == FVA_RANDAUG_NUM_OPS, "the header's op count");
constexpr uint32_t SIGNED_OPS = (1u << OP_SHEAR_X) | (1u << OP_SHEAR_Y) | (1u << OP_TRANSLATE_X) | (1u << OP_TRANSLATE_Y) | (1u << OP_ROTATE) |
                                (1u << OP_BRIGHTNESS) | (1u << OP_COLOR) | (1u << OP_CONTRAST) | (1u << OP_SHARPNESS);
constexpr uint32_t STAT_OPS = (1u << OP_CONTRAST) | (1u << OP_AUTOCONTRAST) | (1u << OP_EQUALIZE);

constexpr int NT = 256;                    // threads per block: four waves
constexpr int TW = 64, TH = 32;            // the apply tile: a wave spans a tile row, 16-pixel units tile it exactly
constexpr int STRIP_PX = 4096;             // pixels per stats block
constexpr int WS_HEAD = 4;                 // int32 words in front of the histograms: {a, b, 0, 0}
constexpr int HIST_WORDS = 4 * 256;
// the LDS window of Sharpness and the geometric ops: holds the tile with its ring (34 x 66 x 3) and the source of a tile rotated by up to
// 35 degrees (73 x 65 x 3 with the margins; the standard space ends at 30) or sheared by 0.3; a larger window -- a rotation near 45
// degrees, a shear beyond the space -- is gathered from global memory
constexpr int STAGE_BYTES = 14336;

struct Philox4 {
    uint32_t v[4];
};
// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), the generator of fva_mix_plan and fva_dropout_fwd
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
__device__ __forceinline__ float uniform_of(uint32_t word) { return ((float)(word >> 8) + 0.5f) * 5.9604644775390625e-8f; }   // (0, 1]

struct Key {
    uint32_t k0, k1, n0, n1;               // the seed's halves and the call counter's
};
__device__ __forceinline__ Key key_of(long long seed, long long counter) {
    return Key{(uint32_t)seed, (uint32_t)((unsigned long long)seed >> 32), (uint32_t)counter, (uint32_t)((unsigned long long)counter >> 32)};
}

// ---------------------------------------------------------------------------------------------------------------- the plan
struct MagTable {
    float v[NUM_OPS];                      // the unsigned value of every op at the chosen bin (computed on the host, in double)
};

__global__ __launch_bounds__(NT) void randaug_plan_kernel(long long* __restrict__ state, int total, uint32_t mask, MagTable mag,
                                                          fva_randaug_op_t* __restrict__ plan) {
    const long long counter = state[1];
    const Key k = key_of(state[0], counter);
    __syncthreads();                       // every thread has read the counter before thread 0 advances it
    const uint32_t enabled = (uint32_t)__popc(mask);
    for (int e = threadIdx.x; e < total; e += NT) {
        const Philox4 w = philox4x32_10((uint32_t)e, 0u, k.n0, k.n1, k.k0, k.k1);
        uint32_t m = mask;
        for (uint32_t skip = (uint32_t)(((unsigned long long)w.v[0] * enabled) >> 32); skip > 0; --skip) m &= m - 1;
        const int op = __ffs((int)m) - 1;
        float v = mag.v[op];
        if (((SIGNED_OPS >> op) & 1u) && (w.v[1] >> 31)) v = -v;
        plan[e] = fva_randaug_op_t{op, v};
    }
    if (threadIdx.x == 0) state[1] = counter + 1;
}

__global__ __launch_bounds__(NT) void randaug_plan_fixed_kernel(const int32_t* __restrict__ ops, const float* __restrict__ values, int total,
                                                                fva_randaug_op_t* __restrict__ plan) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const int op = ops[e];
    plan[e] = fva_randaug_op_t{(unsigned)op < (unsigned)NUM_OPS ? op : OP_IDENTITY, values[e]};
}

// ---------------------------------------------------------------------------------------------------------------- shared pieces
__device__ __forceinline__ int grey_of(int r, int g, int b) { return (int)(0.2989f * (float)r + 0.587f * (float)g + 0.114f * (float)b); }
__device__ __forceinline__ int blend(float x, float d, float f) {
    const float t = d + f * (x - d);                                  // = f x + (1 - f) d; in this form x == d gives x whatever f is
    return (int)fminf(fmaxf(t, 0.f), 255.f);
}
// 16 pixels = 48 bytes = three 16-byte accesses; byte j of the unit is channel j % 3 of pixel j / 3
struct Unit {
    uint32_t w[12];
    __device__ __forceinline__ int get(int j) const { return (w[j >> 2] >> ((j & 3) * 8)) & 255; }
    __device__ __forceinline__ void put(int j, int v) { w[j >> 2] |= (uint32_t)v << ((j & 3) * 8); }
};
__device__ __forceinline__ Unit load_unit(const uint8_t* p) {
    Unit u;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const u32x4 v = *(const u32x4*)(p + 16 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) u.w[4 * q + i] = v[i];
    }
    return u;
}
__device__ __forceinline__ void store_unit(uint8_t* p, const Unit& u) {
#pragma unroll
    for (int q = 0; q < 3; ++q) *(u32x4*)(p + 16 * q) = u32x4{u.w[4 * q], u.w[4 * q + 1], u.w[4 * q + 2], u.w[4 * q + 3]};
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// grid (strips, B).  vec: W % 16 == 0 and the canvases 16-byte aligned -- then every image and every 16-pixel unit starts on 16 bytes.
__global__ __launch_bounds__(NT) void randaug_stats_kernel(const uint8_t* __restrict__ img, const fva_randaug_op_t* __restrict__ plan, int round,
                                                           int N, int32_t* __restrict__ ws, int B, int HW, int vec) {
    __shared__ int h[4][HIST_WORDS];       // one set per wave: a quarter of the LDS atomic collisions
    const int b = blockIdx.y, t = threadIdx.x;
    const int g = ws[0];
    if (blockIdx.x == 0 && b == 0 && t == 0) ws[1] = g + 1;
    int32_t* cur = ws + WS_HEAD + ((int64_t)(g & 1) * B + b) * HIST_WORDS;
    int32_t* other = ws + WS_HEAD + ((int64_t)((g + 1) & 1) * B + b) * HIST_WORDS;
    for (int i = blockIdx.x * NT + t; i < HIST_WORDS; i += gridDim.x * NT) other[i] = 0;
    const int op = plan[b * N + round].op;
    if (!((STAT_OPS >> op) & 1u)) return;
    for (int i = t; i < 4 * HIST_WORDS; i += NT) (&h[0][0])[i] = 0;
    __syncthreads();
    int* mine = h[t >> 6];
    const uint8_t* base = img + (int64_t)b * HW * 3;
    const int p0 = blockIdx.x * STRIP_PX, p1 = min(p0 + STRIP_PX, HW);
    if (vec) {
        for (int p = p0 + t * 16; p < p1; p += NT * 16) {              // HW % 16 == 0: whole units
            const Unit u = load_unit(base + (int64_t)p * 3);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = u.get(3 * q), gg = u.get(3 * q + 1), bl = u.get(3 * q + 2);
                atomicAdd(&mine[r], 1);
                atomicAdd(&mine[256 + gg], 1);
                atomicAdd(&mine[512 + bl], 1);
                atomicAdd(&mine[768 + grey_of(r, gg, bl)], 1);
            }
        }
    } else {
        for (int p = p0 + t; p < p1; p += NT) {
            const uint8_t* q = base + (int64_t)p * 3;
            const int r = q[0], gg = q[1], bl = q[2];
            atomicAdd(&mine[r], 1);
            atomicAdd(&mine[256 + gg], 1);
            atomicAdd(&mine[512 + bl], 1);
            atomicAdd(&mine[768 + grey_of(r, gg, bl)], 1);
        }
    }
    __syncthreads();
    for (int i = t; i < HIST_WORDS; i += NT) {
        const int s = h[0][i] + h[1][i] + h[2][i] + h[3][i];
        if (s) atomicAdd(&cur[i], s);
    }
}

// ---------------------------------------------------------------------------------------------------------------- apply
struct Tile {
    int x0, y0, cols, rows;                // the part of the 32 x 64 tile that lies in the image
};

// the 3 x 256 byte table of a byte-map op.  hist: the image's [4][256] (read by the three ops that need it only).  Ends with a barrier.
__device__ void build_table(int op, float v, const int32_t* __restrict__ hist, int HW, uint8_t* lut, int* scan, int* lohi, long long* red) {
    const int t = threadIdx.x;
    if (t < 3) { lohi[t] = 256; lohi[3 + t] = -1; }
    __syncthreads();
    if (op == OP_AUTOCONTRAST || op == OP_EQUALIZE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int n = hist[c * 256 + t];
            scan[c * 256 + t] = n;
            if (n != 0) { atomicMin(&lohi[c], t); atomicMax(&lohi[3 + c], t); }
        }
    } else if (op == OP_CONTRAST) {
        long long s = (long long)t * hist[768 + t];                  // sum of the grey bytes: exact
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((t & 63) == 0) red[t >> 6] = s;
    }
    __syncthreads();
    if (op == OP_EQUALIZE) {
        for (int o = 1; o < 256; o <<= 1) {                           // inclusive prefix sums, the three channels side by side
            int add[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) add[c] = t >= o ? scan[c * 256 + t - o] : 0;
            __syncthreads();
#pragma unroll
            for (int c = 0; c < 3; ++c) scan[c * 256 + t] += add[c];
            __syncthreads();
        }
    }
    const float f = 1.f + v;
    float mean = 0.f;
    if (op == OP_CONTRAST) mean = (float)((double)(red[0] + red[1] + red[2] + red[3]) / (double)HW);
    const int bits = (int)fminf(fmaxf(v, 0.f), 8.f);
    const int keep = 0xFF & ~((1 << (8 - bits)) - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int out = t;
        switch (op) {
            case OP_BRIGHTNESS: out = blend((float)t, 0.f, f); break;
            case OP_CONTRAST: out = blend((float)t, mean, f); break;
            case OP_SOLARIZE: out = (float)t >= v ? 255 - t : t; break;
            case OP_POSTERIZE: out = t & keep; break;
            case OP_AUTOCONTRAST: {
                const int lo = lohi[c], hi = lohi[3 + c];
                if (hi > lo) out = min(max((t - lo) * 255 / (hi - lo), 0), 255);      // integers: the truncated quotient, exactly
                break;
            }
            case OP_EQUALIZE: {
                const int hi = lohi[3 + c];
                const int last = hi >= 0 ? scan[c * 256 + hi] - (hi > 0 ? scan[c * 256 + hi - 1] : 0) : 0;
                const int step = (HW - last) / 255;
                if (step > 0) out = t == 0 ? 0 : min(255, (scan[c * 256 + t - 1] + step / 2) / step);
                break;
            }
            default: break;                                           // Identity
        }
        lut[c * 256 + t] = (uint8_t)out;
    }
    __syncthreads();
}

// rows [wy0, wy0 + wh) x columns [wx0, wx0 + ww) of the image into LDS, row by row: a wave per row, consecutive lanes consecutive bytes
__device__ __forceinline__ void stage_window(const uint8_t* __restrict__ base, int W, int wx0, int wy0, int ww, int wh, uint8_t* stage) {
    const int lane = threadIdx.x & 63, rowb = ww * 3;
    for (int ry = threadIdx.x >> 6; ry < wh; ry += NT / 64) {
        const uint8_t* src = base + ((int64_t)(wy0 + ry) * W + wx0) * 3;
        for (int o = lane; o < rowb; o += 64) stage[ry * rowb + o] = src[o];
    }
}

struct Affine {
    float a, b, c, d;                      // source = (a dx + b dy + cx, c dx + d dy + cy), (dx, dy) = (x - cx, y - cy)
    int tx, ty;                            // TranslateX / TranslateY: source = (x - tx, y - ty) in integers
    bool integer;
};
__device__ __forceinline__ void source_of(const Affine& m, int x, int y, float cx, float cy, int& ix, int& iy) {
    if (m.integer) {
        ix = (int)((unsigned)x - (unsigned)m.tx);
        iy = (int)((unsigned)y - (unsigned)m.ty);
        return;
    }
    const float dx = (float)x - cx, dy = (float)y - cy;
    ix = __float2int_rd(m.a * dx + m.b * dy + cx + 0.5f);
    iy = __float2int_rd(m.c * dx + m.d * dy + cy + 0.5f);
}

// grid (tiles, B): tile = ty * tiles_x + tx.  in != out.
__global__ __launch_bounds__(NT) void randaug_apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                           const fva_randaug_op_t* __restrict__ plan, int round, int N, int32_t* __restrict__ ws,
                                                           int B, int H, int W, int tiles_x, uint32_t fill, int vec) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
    __shared__ uint8_t lut[768];
    __shared__ int scan[768];
    __shared__ int lohi[6];
    __shared__ long long red[4];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int g = ws[1] - 1;
    if (blockIdx.x == 0 && b == 0 && t == 0) ws[0] = g + 1;
    const int32_t* hist = ws + WS_HEAD + ((int64_t)(g & 1) * B + b) * HIST_WORDS;
    const fva_randaug_op_t job = plan[b * N + round];
    const int op = job.op;
    const float v = job.value;
    const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
    Tile tl;
    tl.x0 = txi * TW; tl.y0 = tyi * TH;
    tl.cols = min(TW, W - tl.x0); tl.rows = min(TH, H - tl.y0);
    const uint8_t* src = in + (int64_t)b * H * W * 3;
    uint8_t* dst = out + (int64_t)b * H * W * 3;
    const float f = 1.f + v;

    switch (op) {
        case OP_COLOR: {
            if (vec) {
                const int upr = tl.cols >> 4;
                for (int u = t; u < tl.rows * upr; u += NT) {
                    const int ry = u / upr, k = u - ry * upr;
                    const int64_t off = ((int64_t)(tl.y0 + ry) * W + tl.x0 + k * 16) * 3;
                    const Unit a = load_unit(src + off);
                    Unit o = {};
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int r = a.get(3 * q), gg = a.get(3 * q + 1), bl = a.get(3 * q + 2);
                        const float grey = (float)grey_of(r, gg, bl);
                        o.put(3 * q, blend((float)r, grey, f));
                        o.put(3 * q + 1, blend((float)gg, grey, f));
                        o.put(3 * q + 2, blend((float)bl, grey, f));
                    }
                    store_unit(dst + off, o);
                }
            } else if (lane < tl.cols) {
                for (int ry = wave; ry < tl.rows; ry += NT / 64) {
                    const int64_t off = ((int64_t)(tl.y0 + ry) * W + tl.x0 + lane) * 3;
                    const int r = src[off], gg = src[off + 1], bl = src[off + 2];
                    const float grey = (float)grey_of(r, gg, bl);
                    dst[off] = (uint8_t)blend((float)r, grey, f);
                    dst[off + 1] = (uint8_t)blend((float)gg, grey, f);
                    dst[off + 2] = (uint8_t)blend((float)bl, grey, f);
                }
            }
            break;
        }
        case OP_SHARPNESS: {
            // the tile and a one-pixel ring where the image has one; border pixels of the IMAGE are copied
            const int wx0 = max(tl.x0 - 1, 0), wy0 = max(tl.y0 - 1, 0);
            const int ww = min(tl.x0 + tl.cols + 1, W) - wx0, wh = min(tl.y0 + tl.rows + 1, H) - wy0;
            stage_window(src, W, wx0, wy0, ww, wh, stage);
            __syncthreads();
            if (lane < tl.cols) {
                const int x = tl.x0 + lane, rowb = ww * 3;
                for (int ry = wave; ry < tl.rows; ry += NT / 64) {
                    const int y = tl.y0 + ry;
                    const uint8_t* c0 = stage + (y - wy0) * rowb + (x - wx0) * 3;
                    const bool inner = x > 0 && x < W - 1 && y > 0 && y < H - 1;
                    const int64_t off = ((int64_t)y * W + x) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        int val = c0[c];
                        if (inner) {
                            const int s = c0[c - rowb - 3] + c0[c - rowb] + c0[c - rowb + 3] + c0[c - 3] + 5 * val + c0[c + 3] + c0[c + rowb - 3] +
                                          c0[c + rowb] + c0[c + rowb + 3];
                            val = blend((float)val, (float)((2 * s + 13) / 26), f);      // s / 13 to nearest: no ties, 13 is odd
                        }
                        dst[off + c] = (uint8_t)val;
                    }
                }
            }
            break;
        }
        case OP_SHEAR_X: case OP_SHEAR_Y: case OP_TRANSLATE_X: case OP_TRANSLATE_Y: case OP_ROTATE: {
            const float cx = (float)(W - 1) * 0.5f, cy = (float)(H - 1) * 0.5f;
            Affine m = {1.f, 0.f, 0.f, 1.f, 0, 0, false};
            if (op == OP_SHEAR_X) m.b = v;
            else if (op == OP_SHEAR_Y) m.c = v;
            else if (op == OP_ROTATE) {
                const float rad = v * 0.017453292519943295f;
                const float cs = cosf(rad), sn = sinf(rad);
                m.a = cs; m.b = -sn; m.c = sn; m.d = cs;
            } else {
                m.integer = true;
                const int shift = __float2int_rz(v);
                if (op == OP_TRANSLATE_X) m.tx = shift; else m.ty = shift;
            }
            // the bounding box of the tile's sources: an affine map takes its extremes at the corners; one pixel of margin, clamped to
            // the image.  A sample that falls outside the staged window all the same is read from global memory.
            int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int ix, iy;
                source_of(m, tl.x0 + (k & 1) * (tl.cols - 1), tl.y0 + (k >> 1) * (tl.rows - 1), cx, cy, ix, iy);
                bx0 = min(bx0, ix); bx1 = max(bx1, ix); by0 = min(by0, iy); by1 = max(by1, iy);
            }
            const int wx0 = min(max(bx0, 1) - 1, W), wy0 = min(max(by0, 1) - 1, H);
            const int wx1 = min(max(min(bx1, W), -2) + 2, W), wy1 = min(max(min(by1, H), -2) + 2, H);
            const int ww = max(wx1 - wx0, 0), wh = max(wy1 - wy0, 0);
            const bool staged = ww > 0 && wh > 0 && (int64_t)ww * wh * 3 <= STAGE_BYTES;
            if (staged) stage_window(src, W, wx0, wy0, ww, wh, stage);
            __syncthreads();
            if (lane < tl.cols) {
                const int x = tl.x0 + lane;
                for (int ry = wave; ry < tl.rows; ry += NT / 64) {
                    const int y = tl.y0 + ry;
                    int ix, iy;
                    source_of(m, x, y, cx, cy, ix, iy);
                    int r = fill & 255, gg = (fill >> 8) & 255, bl = (fill >> 16) & 255;
                    if ((unsigned)ix < (unsigned)W && (unsigned)iy < (unsigned)H) {
                        const uint8_t* p = staged && ix >= wx0 && ix < wx1 && iy >= wy0 && iy < wy1
                                               ? stage + ((iy - wy0) * ww + (ix - wx0)) * 3
                                               : src + ((int64_t)iy * W + ix) * 3;
                        r = p[0]; gg = p[1]; bl = p[2];
                    }
                    const int64_t off = ((int64_t)y * W + x) * 3;
                    dst[off] = (uint8_t)r; dst[off + 1] = (uint8_t)gg; dst[off + 2] = (uint8_t)bl;
                }
            }
            break;
        }
        default: {                                                    // the byte maps, Identity among them
            build_table(op, v, hist, H * W, lut, scan, lohi, red);
            if (vec) {
                const int upr = tl.cols >> 4;
                for (int u = t; u < tl.rows * upr; u += NT) {
                    const int ry = u / upr, k = u - ry * upr;
                    const int64_t off = ((int64_t)(tl.y0 + ry) * W + tl.x0 + k * 16) * 3;
                    const Unit a = load_unit(src + off);
                    Unit o = {};
#pragma unroll
                    for (int j = 0; j < 48; ++j) o.put(j, lut[(j % 3) * 256 + a.get(j)]);
                    store_unit(dst + off, o);
                }
            } else {
                const int rowb = tl.cols * 3;
                for (int ry = wave; ry < tl.rows; ry += NT / 64) {
                    const int64_t off = ((int64_t)(tl.y0 + ry) * W + tl.x0) * 3;
                    for (int o = lane; o < rowb; o += 64) dst[off + o] = lut[(o % 3) * 256 + src[off + o]];
                }
            }
            break;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- RandomErasing
struct EraseParams {
    float p, scale_lo, scale_hi, log_ratio_lo, log_ratio_hi;
};

// boxes[b] = {top, left, height, width}; all zero: no erase
__global__ __launch_bounds__(NT) void erase_plan_kernel(long long* __restrict__ state, int B, int H, int W, EraseParams q, int32_t* __restrict__ boxes) {
    const long long counter = state[1];
    const Key k = key_of(state[0], counter);
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += NT) {
        int top = 0, left = 0, bh = 0, bw = 0;
        const Philox4 head = philox4x32_10((uint32_t)b, 0u, k.n0, k.n1, k.k0, k.k1);
        if (q.p >= 1.f || uniform_of(head.v[0]) < q.p) {
            for (int a = 0; a < 10; ++a) {
                const Philox4 w = philox4x32_10((uint32_t)b, (uint32_t)(1 + a), k.n0, k.n1, k.k0, k.k1);
                const float area = (float)(H * W) * (q.scale_lo + (q.scale_hi - q.scale_lo) * uniform_of(w.v[0]));
                const float aspect = expf(q.log_ratio_lo + (q.log_ratio_hi - q.log_ratio_lo) * uniform_of(w.v[1]));
                const int eh = __float2int_rn(sqrtf(area * aspect)), ew = __float2int_rn(sqrtf(area / aspect));
                if (!(eh < H && ew < W)) continue;
                top = (int)(((unsigned long long)w.v[2] * (unsigned long long)(H - eh + 1)) >> 32);
                left = (int)(((unsigned long long)w.v[3] * (unsigned long long)(W - ew + 1)) >> 32);
                bh = eh; bw = ew;
                break;
            }
        }
        boxes[4 * b] = top; boxes[4 * b + 1] = left; boxes[4 * b + 2] = bh; boxes[4 * b + 3] = bw;
    }
    if (threadIdx.x == 0) state[1] = counter + 1;
}

// N(0, 1) for element e of image b: Box-Muller on the pair (e & 3) >> 1 of Philox block (e >> 2, 2^16 + b) -- the box draws use (b, 0 .. 10)
__device__ __forceinline__ float normal_at(uint32_t e, int b, const Key& k) {
    const Philox4 w = philox4x32_10(e >> 2, 0x10000u + (uint32_t)b, k.n0, k.n1, k.k0, k.k1);
    const int pair = (e >> 1) & 1;
    const float rad = sqrtf(-2.f * logf(uniform_of(w.v[2 * pair]))), th = 6.283185307179586f * uniform_of(w.v[2 * pair + 1]);
    return (e & 1) ? rad * sinf(th) : rad * cosf(th);
}

// in place: the elements of the boxes and nothing else; grid (x, B)
template <typename T>
__global__ __launch_bounds__(NT) void erase_box_kernel(T* __restrict__ x, const int32_t* __restrict__ boxes, const long long* __restrict__ state, int C,
                                                       int H, int W, int noise, float value) {
    const int b = blockIdx.y;
    const int top = boxes[4 * b], left = boxes[4 * b + 1], bh = boxes[4 * b + 2], bw = boxes[4 * b + 3];
    if (bh <= 0 || bw <= 0) return;
    const Key k = key_of(state[0], state[1] - 1);                      // the call that drew the boxes
    T* xb = x + (int64_t)b * C * H * W;
    const int per = bh * bw, n = C * per;
    for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
        const int c = i / per, rem = i - c * per, ry = rem / bw, rx = rem - ry * bw;
        const uint32_t e = (uint32_t)((c * H + top + ry) * W + left + rx);
        xb[e] = from_f<T>(noise ? normal_at(e, b, k) : value);
    }
}

// into out: one pass over the batch, EPC elements per thread and step (a 16-byte chunk, or 1); W % EPC == 0, so a chunk lies in one row
template <typename T, int EPC>
__global__ __launch_bounds__(NT) void erase_stream_kernel(const T* __restrict__ x, T* __restrict__ out, const int32_t* __restrict__ boxes,
                                                          const long long* __restrict__ state, FastDiv Hd, FastDiv wcd, int nchunk, int noise, float value) {
    const int b = blockIdx.y;
    const int top = boxes[4 * b], left = boxes[4 * b + 1], bh = boxes[4 * b + 2], bw = boxes[4 * b + 3];
    const Key k = key_of(state[0], state[1] - 1);
    const T* xb = x + (int64_t)b * nchunk * EPC;
    T* ob = out + (int64_t)b * nchunk * EPC;
    for (uint32_t v = blockIdx.x * NT + threadIdx.x; v < (uint32_t)nchunk; v += gridDim.x * NT) {
        const uint32_t row = fd_div(v, wcd);                             // over C * H; wcd.d = W / EPC chunks per row
        const int xs = (int)(v - row * wcd.d) * EPC, yy = (int)(row - fd_div(row, Hd) * Hd.d);
        const bool hit = yy >= top && yy < top + bh && xs < left + bw && xs + EPC > left;
        if constexpr (EPC == 1) {
            ob[v] = hit ? from_f<T>(noise ? normal_at(v, b, k) : value) : xb[v];
        } else {
            Vec16<T> a = *(const Vec16<T>*)(xb + (int64_t)v * EPC);
            if (hit) {
#pragma unroll
                for (int e = 0; e < EPC; ++e)
                    if (xs + e >= left && xs + e < left + bw) a.set(e, noise ? normal_at(v * EPC + e, b, k) : value);
            }
            *(Vec16<T>*)(ob + (int64_t)v * EPC) = a;
        }
    }
}

inline int grid_x(int64_t items, int B) {
    const int64_t want = (items + NT - 1) / NT;
    const int64_t cap = 4096 / B > 1 ? 4096 / B : 1;                  // about 4096 blocks in all: the rest is the grid-stride loop
    return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

template <typename T>
void launch_erase(const T* x, T* out, const int32_t* boxes, const long long* state, int B, int C, int H, int W, int noise, float value, hipStream_t s) {
    const int64_t n = (int64_t)C * H * W;
    if ((const void*)x == (void*)out) {
        hipLaunchKernelGGL(erase_box_kernel<T>, dim3(grid_x(n, B), B), dim3(NT), 0, s, out, boxes, state, C, H, W, noise, value);
        return;
    }
    constexpr int E = Vec16<T>::N;
    const FastDiv Hd = make_fastdiv((uint32_t)H);
    if (W % E == 0 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0)
        hipLaunchKernelGGL((erase_stream_kernel<T, E>), dim3(grid_x(n / E, B), B), dim3(NT), 0, s, x, out, boxes, state, Hd, make_fastdiv((uint32_t)(W / E)),
                           (int)(n / E), noise, value);
    else
        hipLaunchKernelGGL((erase_stream_kernel<T, 1>), dim3(grid_x(n, B), B), dim3(NT), 0, s, x, out, boxes, state, Hd, make_fastdiv((uint32_t)W), (int)n,
                           noise, value);
}

bool shape_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && (int64_t)H * W * 3 < (1ll << 31); }

}  // namespace

extern "C" {

int fva_randaug_plan(int64_t* state, int32_t B, int32_t num_ops, int32_t magnitude, int32_t num_bins, int32_t H, int32_t W, uint32_t op_mask,
                     fva_randaug_op_t* plan, void* stream) {
    if (!state || !plan) return fva_fail(FVA_ERR_ARG, "fva_randaug_plan: null pointer");
    if (!shape_ok(B, H, W) || num_ops < 1 || num_ops > FVA_RANDAUG_MAX_OPS)
        return fva_fail(FVA_ERR_ARG, "fva_randaug_plan: bad shape B=%d num_ops=%d H=%d W=%d (1 <= num_ops <= %d)", B, num_ops, H, W, FVA_RANDAUG_MAX_OPS);
    if (num_bins < 2 || magnitude < 0 || magnitude >= num_bins)
        return fva_fail(FVA_ERR_ARG, "fva_randaug_plan: magnitude %d is no bin of %d (num_bins >= 2)", magnitude, num_bins);
    if (op_mask == 0 || op_mask >> NUM_OPS) return fva_fail(FVA_ERR_ARG, "fva_randaug_plan: op_mask 0x%x must enable at least one of the %d ops and nothing else", op_mask, NUM_OPS);
    const double frac = (double)magnitude / (double)(num_bins - 1);
    MagTable mag = {};
    mag.v[OP_SHEAR_X] = mag.v[OP_SHEAR_Y] = (float)(0.3 * frac);
    mag.v[OP_TRANSLATE_X] = (float)trunc(150.0 / 331.0 * (double)W * frac);
    mag.v[OP_TRANSLATE_Y] = (float)trunc(150.0 / 331.0 * (double)H * frac);
    mag.v[OP_ROTATE] = (float)(30.0 * frac);
    mag.v[OP_BRIGHTNESS] = mag.v[OP_COLOR] = mag.v[OP_CONTRAST] = mag.v[OP_SHARPNESS] = (float)(0.9 * frac);
    mag.v[OP_POSTERIZE] = (float)(8.0 - nearbyint((double)magnitude / ((double)(num_bins - 1) / 4.0)));
    mag.v[OP_SOLARIZE] = (float)(255.0 - 255.0 * frac);
    hipLaunchKernelGGL(randaug_plan_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (long long*)state, B * num_ops, op_mask, mag, plan);
    FVA_LAUNCH_CHECK("randaug_plan_kernel");
    return FVA_OK;
}

int fva_randaug_plan_fixed(const int32_t* ops, const float* values, int32_t B, int32_t num_ops, fva_randaug_op_t* plan, void* stream) {
    if (!ops || !values || !plan) return fva_fail(FVA_ERR_ARG, "fva_randaug_plan_fixed: null pointer");
    if (B < 1 || B > 65535 || num_ops < 1 || num_ops > FVA_RANDAUG_MAX_OPS)
        return fva_fail(FVA_ERR_ARG, "fva_randaug_plan_fixed: bad shape B=%d num_ops=%d (1 <= num_ops <= %d)", B, num_ops, FVA_RANDAUG_MAX_OPS);
    hipLaunchKernelGGL(randaug_plan_fixed_kernel, dim3(cdiv(B * num_ops, NT)), dim3(NT), 0, (hipStream_t)stream, ops, values, B * num_ops, plan);
    FVA_LAUNCH_CHECK("randaug_plan_fixed_kernel");
    return FVA_OK;
}

int64_t fva_randaug_workspace(int32_t B) { return B < 1 ? 0 : (int64_t)sizeof(int32_t) * (WS_HEAD + 2ll * B * HIST_WORDS); }

int fva_randaug_stats(const uint8_t* canvases, const fva_randaug_op_t* plan, int32_t round, int32_t num_ops, int32_t B, int32_t H, int32_t W,
                      int32_t* workspace, void* stream) {
    if (!canvases || !plan || !workspace) return fva_fail(FVA_ERR_ARG, "fva_randaug_stats: null pointer");
    if (!shape_ok(B, H, W) || num_ops < 1 || num_ops > FVA_RANDAUG_MAX_OPS || round < 0 || round >= num_ops)
        return fva_fail(FVA_ERR_ARG, "fva_randaug_stats: bad shape B=%d H=%d W=%d, round %d of %d", B, H, W, round, num_ops);
    const int vec = W % 16 == 0 && (uintptr_t)canvases % 16 == 0;
    hipLaunchKernelGGL(randaug_stats_kernel, dim3(cdiv((int64_t)H * W, STRIP_PX), B), dim3(NT), 0, (hipStream_t)stream, canvases, plan, round, num_ops,
                       workspace, B, H * W, vec);
    FVA_LAUNCH_CHECK("randaug_stats_kernel");
    return FVA_OK;
}

int fva_randaug_apply(const uint8_t* in, uint8_t* out, const fva_randaug_op_t* plan, int32_t round, int32_t num_ops, int32_t B, int32_t H, int32_t W,
                      uint32_t fill_rgb, int32_t* workspace, void* stream) {
    if (!in || !out || !plan || !workspace) return fva_fail(FVA_ERR_ARG, "fva_randaug_apply: null pointer");
    if (!shape_ok(B, H, W) || num_ops < 1 || num_ops > FVA_RANDAUG_MAX_OPS || round < 0 || round >= num_ops)
        return fva_fail(FVA_ERR_ARG, "fva_randaug_apply: bad shape B=%d H=%d W=%d, round %d of %d", B, H, W, round, num_ops);
    const int64_t bytes = (int64_t)B * H * W * 3;
    if (in < out + bytes && out < in + bytes) return fva_fail(FVA_ERR_ARG, "fva_randaug_apply: works out of place (a tile reads its neighbours' pixels)");
    const int vec = W % 16 == 0 && ((uintptr_t)in | (uintptr_t)out) % 16 == 0;
    const int tiles_x = cdiv(W, TW);
    hipLaunchKernelGGL(randaug_apply_kernel, dim3(tiles_x * cdiv(H, TH), B), dim3(NT), 0, (hipStream_t)stream, in, out, plan, round, num_ops, workspace, B,
                       H, W, tiles_x, fill_rgb & 0xFFFFFFu, vec);
    FVA_LAUNCH_CHECK("randaug_apply_kernel");
    return FVA_OK;
}

int fva_random_erase(int dtype, const void* x, void* out, int64_t* state, int32_t B, int32_t C, int32_t H, int32_t W, float p, float scale_lo,
                     float scale_hi, float ratio_lo, float ratio_hi, int32_t noise, float value, int32_t* boxes, void* stream) {
    if (!x || !out || !state || !boxes) return fva_fail(FVA_ERR_ARG, "fva_random_erase: null pointer");
    if (dtype != FVA_F32 && dtype != FVA_BF16) return fva_fail(FVA_ERR_ARG, "fva_random_erase: bad dtype %d", dtype);
    if (B < 1 || C < 1 || H < 1 || W < 1 || B > 65535 || (int64_t)C * H * W >= (1ll << 31))
        return fva_fail(FVA_ERR_ARG, "fva_random_erase: bad shape B=%d C=%d H=%d W=%d (B <= 65535, C * H * W < 2^31)", B, C, H, W);
    if (!(p >= 0.f && p <= 1.f) || !(scale_lo >= 0.f && scale_lo <= scale_hi && scale_hi <= 1.f) || !(ratio_lo > 0.f && ratio_lo <= ratio_hi))
        return fva_fail(FVA_ERR_ARG, "fva_random_erase: p = %g in [0, 1], 0 <= scale (%g, %g) <= 1 and 0 < ratio (%g, %g), each in order", (double)p,
                        (double)scale_lo, (double)scale_hi, (double)ratio_lo, (double)ratio_hi);
    if (x != out) {
        const int64_t bytes = (int64_t)B * C * H * W * (dtype == FVA_BF16 ? 2 : 4);
        const char *a = (const char*)x, *o = (const char*)out;
        if (a < o + bytes && o < a + bytes) return fva_fail(FVA_ERR_ARG, "fva_random_erase: x and out overlap (pass the same pointer to work in place)");
    }
    hipStream_t s = (hipStream_t)stream;
    const EraseParams q = {p, scale_lo, scale_hi, (float)log((double)ratio_lo), (float)log((double)ratio_hi)};
    hipLaunchKernelGGL(erase_plan_kernel, dim3(1), dim3(NT), 0, s, (long long*)state, B, H, W, q, boxes);
    FVA_LAUNCH_CHECK("erase_plan_kernel");
    if (dtype == FVA_BF16)
        launch_erase<bf16_t>((const bf16_t*)x, (bf16_t*)out, boxes, (const long long*)state, B, C, H, W, noise != 0, value, s);
    else
        launch_erase<float>((const float*)x, (float*)out, boxes, (const long long*)state, B, C, H, W, noise != 0, value, s);
    FVA_LAUNCH_CHECK("erase kernel");
    return FVA_OK;
}

}  // extern "C"
