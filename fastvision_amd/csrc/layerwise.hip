// Layer-wise adaptive optimizers for gfx950: LARS (on torch.optim.SGD's update) and LAMB (on Adam's moments), multi-tensor, every
// parameter group in the same launches.  Both need two per-tensor L2 norms before any weight of that tensor may be written, so a step
// is three passes over the chunk table of multi_tensor.h (one block per MT_CHUNK elements; a tensor's chunks are consecutive):
//
//   norm pass   one block per chunk: two fp64 partial sums into partial[2][nchunks], no atomics
//                 LARS  reads p, g (8 B / element)                  row 0 = sum g^2, row 1 = sum p^2
//                 LAMB  reads g, m, v, p, writes m, v (24 B)        row 0 = sum u^2, row 1 = sum p^2   (u formed in registers only)
//   trust pass  one block per tensor: adds that tensor's partials in chunk order, writes ratio[t] (fp64 arithmetic, stored as fp32);
//               for LARS with clipping every block also adds all of row 0 (the global gradient norm: no extra pass over the gradients)
//   apply pass  one block per chunk, 16-byte accesses, scalar tail
//                 LARS  reads p, g, buf, writes p, buf (20 B)       LAMB  reads m, v, p, writes p (16 B), u recomputed by lamb_u
//
// 28 B per parameter for LARS with momentum (SGD: 20), 40 B for LAMB (Adam: 28).  Every sum has a fixed order: bit-identical runs.
//
// tab: int64 [6][n] = param | grad | momentum buffer (0: none) or exp_avg | element count | group index | fresh-flag slot (LARS) or
//      exp_avg_sq (LAMB): rows 0..4 are the SGD table's, so LAMB's global clipping norm comes from fva_sgd_clip_coef unchanged.
// first: int64 [n + 1], first[t] = index of tensor t's first chunk in the chunk table, first[n] = nchunks.
// hyper: double [G][LARS_HYPER | LAMB_HYPER], one row per parameter group, read at run time (captured steps follow an LR schedule).
#include <math.h>

#include "common.h"
#include "multi_tensor.h"

namespace {

constexpr int LW_THREADS = 256;
constexpr int LARS_HYPER = 7;      // lr, weight decay, momentum, 1 - dampening, nesterov (0 / 1), trust coefficient, eps
constexpr int LAMB_HYPER = 6;      // lr, beta1, beta2, eps, weight decay, trust (0 / 1)

struct LwChunk {
    int64_t t, begin, end, vend;   // elements [begin, end) of tensor t; [begin, vend) in whole float4
};
__device__ __forceinline__ LwChunk lw_chunk(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks) {
    const int64_t word = chunks[blockIdx.x];
    LwChunk c;
    c.t = mt_tensor(word);
    c.begin = mt_number(word) * MT_CHUNK;
    c.end = mt_end(c.begin, tab[3 * n + c.t], MT_CHUNK);
    c.vend = c.begin + ((c.end - c.begin) & ~(int64_t)3);
    return c;
}

// the fixed-order block sum of optim.hip (wave64 butterfly, then the four waves in order), for two sums at once; valid in thread 0
struct Sum2 {
    double a, b;
};
__device__ __forceinline__ Sum2 block_sum2(double a, double b, double (*lds)[LW_THREADS / 64]) {
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    if ((threadIdx.x & 63) == 0) {
        lds[0][threadIdx.x >> 6] = a;
        lds[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    Sum2 s{0.0, 0.0};
    if (threadIdx.x == 0)
        for (int w = 0; w < LW_THREADS / 64; ++w) {
            s.a += lds[0][w];
            s.b += lds[1][w];
        }
    return s;
}

__device__ __forceinline__ double sq4(f32x4 v) { return (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3]; }

// ---- LARS ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LW_THREADS) void lars_norm_kernel(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks,
                                                               int nchunks, double* __restrict__ partial) {
    __shared__ double lds[2][LW_THREADS / 64];
    const LwChunk c = lw_chunk(tab, n, chunks);
    const float* __restrict__ p = (const float*)tab[c.t];
    const float* __restrict__ g = (const float*)tab[n + c.t];
    double sg = 0.0, sp = 0.0;
    int64_t i = c.begin;
    if ((((uintptr_t)p | (uintptr_t)g) & 15) == 0) {
#pragma unroll 4
        for (int64_t j = c.begin + 4 * (int64_t)threadIdx.x; j < c.vend; j += 4 * LW_THREADS) {
            sg += sq4(*(const f32x4*)(g + j));
            sp += sq4(*(const f32x4*)(p + j));
        }
        i = c.vend;
    }
    for (int64_t j = i + threadIdx.x; j < c.end; j += LW_THREADS) {
        sg += (double)g[j] * g[j];
        sp += (double)p[j] * p[j];
    }
    const Sum2 s = block_sum2(sg, sp, lds);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s.a;
        partial[nchunks + blockIdx.x] = s.b;
    }
}

struct LarsHyper {
    float lr, wd, momentum, keep, nesterov;
};

// g = q * (coef * grad + wd * p); buf = g (first step) or momentum * buf + (1 - dampening) * g; p -= lr * (g + momentum * buf | buf)
__device__ __forceinline__ void lars_one(float& p, float gr, float& b, const LarsHyper& h, float coef, float q, bool mom, bool first) {
    float g = q * (coef * gr + h.wd * p);
    if (mom) {
        b = first ? g : h.momentum * b + h.keep * g;
        g = h.nesterov != 0.f ? g + h.momentum * b : b;
    }
    p = p - h.lr * g;
}

__global__ __launch_bounds__(LW_THREADS) void lars_apply_kernel(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks,
                                                                const double* __restrict__ hyper, const int32_t* __restrict__ fresh,
                                                                const float* __restrict__ ratio, const float* __restrict__ coef_dev) {
    const LwChunk c = lw_chunk(tab, n, chunks);
    float* __restrict__ p = (float*)tab[c.t];
    const float* __restrict__ g = (const float*)tab[n + c.t];
    float* __restrict__ b = (float*)tab[2 * n + c.t];
    const double* hp = hyper + tab[4 * n + c.t] * LARS_HYPER;
    const LarsHyper h{(float)hp[0], (float)hp[1], (float)hp[2], (float)hp[3], (float)hp[4]};
    const float coef = coef_dev ? *coef_dev : 1.f;
    const float q = ratio[c.t];
    const bool mom = b != nullptr;
    const bool first = mom && fresh[tab[5 * n + c.t]] != 0;
    float dummy = 0.f;
    int64_t i = c.begin;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0) {
#pragma unroll 2
        for (int64_t j = c.begin + 4 * (int64_t)threadIdx.x; j < c.vend; j += 4 * LW_THREADS) {
            f32x4 pv = *(f32x4*)(p + j);
            const f32x4 gv = *(const f32x4*)(g + j);
            f32x4 bv = mom ? *(f32x4*)(b + j) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pv[k], bk = bv[k];
                lars_one(pk, gv[k], bk, h, coef, q, mom, first);
                pv[k] = pk;
                bv[k] = bk;
            }
            *(f32x4*)(p + j) = pv;
            if (mom) *(f32x4*)(b + j) = bv;
        }
        i = c.vend;
    }
    for (int64_t j = i + threadIdx.x; j < c.end; j += LW_THREADS) {
        float pk = p[j];
        float& bk = mom ? b[j] : dummy;
        lars_one(pk, g[j], bk, h, coef, q, mom, first);
        p[j] = pk;
    }
}

// after an update that initialised buffers: their history starts now (as sgd_clear_fresh)
__global__ void lars_clear_fresh(const int64_t* __restrict__ tab, int n, int32_t* __restrict__ fresh) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) fresh[tab[5 * n + t]] = 0;
}

// ---- LAMB ---------------------------------------------------------------------------------------------------------------------
// state: double [1 + 2 G] = step count (exact to 2^53) | 1 - beta1^step, 1 - beta2^step per group; ticked on the device so that a
// captured step replays with the right bias corrections (as adam_tick_kernel)
__global__ __launch_bounds__(64) void lamb_tick_kernel(double* state, const double* __restrict__ hyper, int groups) {
    const double step = state[0] + 1.0;
    __syncthreads();
    if (threadIdx.x == 0) state[0] = step;
    for (int g = threadIdx.x; g < groups; g += 64) {
        state[1 + 2 * g] = 1.0 - pow(hyper[g * LAMB_HYPER + 1], step);
        state[2 + 2 * g] = 1.0 - pow(hyper[g * LAMB_HYPER + 2], step);
    }
}

struct LambHyper {
    float beta1, keep1, beta2, keep2, eps, wd, bc1, bc2;      // keep = 1 - beta, bc = 1 - beta^step
};
__device__ __forceinline__ LambHyper lamb_hyper(const double* __restrict__ hyper, const double* __restrict__ state, int64_t group) {
    const double* hp = hyper + group * LAMB_HYPER;
    return LambHyper{(float)hp[1], (float)(1.0 - hp[1]), (float)hp[2], (float)(1.0 - hp[2]), (float)hp[3], (float)hp[4],
                     (float)state[1 + 2 * group], (float)state[2 + 2 * group]};
}

// The update direction from the moments AS STORED: the norm pass measures it and the apply pass applies it, so both call this one
// function on the same fp32 m, v, p and get the same bits.
__device__ __forceinline__ float lamb_u(float m, float v, float p, const LambHyper& h) {
    return fmaf(h.wd, p, (m / h.bc1) / (sqrtf(v / h.bc2) + h.eps));      // an explicit fma: nothing left for contraction to decide
}

__device__ __forceinline__ void lamb_moments(float& m, float& v, float gr, float coef, const LambHyper& h) {
    const float g = coef * gr;
    m = h.beta1 * m + h.keep1 * g;
    v = h.beta2 * v + h.keep2 * g * g;
}

__global__ __launch_bounds__(LW_THREADS) void lamb_norm_kernel(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks,
                                                               int nchunks, const double* __restrict__ hyper, const double* __restrict__ state,
                                                               const float* __restrict__ coef_dev, double* __restrict__ partial) {
    __shared__ double lds[2][LW_THREADS / 64];
    const LwChunk c = lw_chunk(tab, n, chunks);
    const float* __restrict__ p = (const float*)tab[c.t];
    const float* __restrict__ g = (const float*)tab[n + c.t];
    float* __restrict__ m = (float*)tab[2 * n + c.t];
    float* __restrict__ v = (float*)tab[5 * n + c.t];
    const LambHyper h = lamb_hyper(hyper, state, tab[4 * n + c.t]);
    const float coef = coef_dev ? *coef_dev : 1.f;
    double su = 0.0, sp = 0.0;
    int64_t i = c.begin;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
#pragma unroll 2
        for (int64_t j = c.begin + 4 * (int64_t)threadIdx.x; j < c.vend; j += 4 * LW_THREADS) {
            const f32x4 pv = *(const f32x4*)(p + j), gv = *(const f32x4*)(g + j);
            f32x4 mv = *(f32x4*)(m + j), vv = *(f32x4*)(v + j), uv;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float mk = mv[k], vk = vv[k];
                lamb_moments(mk, vk, gv[k], coef, h);
                mv[k] = mk;
                vv[k] = vk;
                uv[k] = lamb_u(mk, vk, pv[k], h);
            }
            *(f32x4*)(m + j) = mv;
            *(f32x4*)(v + j) = vv;
            su += sq4(uv);
            sp += sq4(pv);
        }
        i = c.vend;
    }
    for (int64_t j = i + threadIdx.x; j < c.end; j += LW_THREADS) {
        float mk = m[j], vk = v[j];
        const float pk = p[j];
        lamb_moments(mk, vk, g[j], coef, h);
        m[j] = mk;
        v[j] = vk;
        const float u = lamb_u(mk, vk, pk, h);
        su += (double)u * u;
        sp += (double)pk * pk;
    }
    const Sum2 s = block_sum2(su, sp, lds);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s.a;
        partial[nchunks + blockIdx.x] = s.b;
    }
}

__global__ __launch_bounds__(LW_THREADS) void lamb_apply_kernel(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ chunks,
                                                                const double* __restrict__ hyper, const double* __restrict__ state,
                                                                const float* __restrict__ ratio) {
    const LwChunk c = lw_chunk(tab, n, chunks);
    float* __restrict__ p = (float*)tab[c.t];
    const float* __restrict__ m = (const float*)tab[2 * n + c.t];
    const float* __restrict__ v = (const float*)tab[5 * n + c.t];
    const int64_t group = tab[4 * n + c.t];
    const LambHyper h = lamb_hyper(hyper, state, group);
    const float step = (float)hyper[group * LAMB_HYPER] * ratio[c.t];       // lr * r
    int64_t i = c.begin;
    if ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
#pragma unroll 4
        for (int64_t j = c.begin + 4 * (int64_t)threadIdx.x; j < c.vend; j += 4 * LW_THREADS) {
            f32x4 pv = *(f32x4*)(p + j);
            const f32x4 mv = *(const f32x4*)(m + j), vv = *(const f32x4*)(v + j);
#pragma unroll
            for (int k = 0; k < 4; ++k) pv[k] = pv[k] - step * lamb_u(mv[k], vv[k], pv[k], h);
            *(f32x4*)(p + j) = pv;
        }
        i = c.vend;
    }
    for (int64_t j = i + threadIdx.x; j < c.end; j += LW_THREADS) {
        const float pk = p[j];
        p[j] = pk - step * lamb_u(m[j], v[j], pk, h);
    }
}

// ---- trust pass -----------------------------------------------------------------------------------------------------------------
// sum of row[lo, hi) in a fixed order: thread i adds the i-th contiguous stretch front to back, then the block sum.  Right for fewer
// entries than threads (one chunk: thread 0 alone) and for more.  Valid in thread 0 (row 1's sum rides along in .b).
__device__ __forceinline__ Sum2 stretch_sum2(const double* __restrict__ row0, const double* __restrict__ row1, int64_t lo, int64_t hi,
                                             double (*lds)[LW_THREADS / 64]) {
    const int64_t per = (hi - lo + LW_THREADS - 1) / LW_THREADS;
    const int64_t b = lo + threadIdx.x * per;
    const int64_t e = b + per < hi ? b + per : hi;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = b; i < e; ++i) {
        a0 += row0[i];
        a1 += row1[i];
    }
    __syncthreads();          // lds may still be read by thread 0 from an earlier sum
    return block_sum2(a0, a1, lds);
}

// ratio[t] for every tensor.  LARS: q = eta * wn / (gn + wd * wn + eps) if eta, wn, gn > 0, else 1, with gn = coef * |grad|; clip > 0:
// coef = clip / max(norm, clip) of the global norm (all of row 0), computed as clip_coef of optim.hip computes it and stored by block
// 0 into clip_out = {norm, coef} for the apply pass.  LAMB: r = wn / un if trust and wn, un > 0, else 1.
template <bool LAMB>
__global__ __launch_bounds__(LW_THREADS) void trust_kernel(const int64_t* __restrict__ tab, int n, const int64_t* __restrict__ first,
                                                           const double* __restrict__ partial, int nchunks, const double* __restrict__ hyper,
                                                           double clip, float* __restrict__ clip_out, float* __restrict__ ratio) {
    __shared__ double lds[2][LW_THREADS / 64];
    const int t = blockIdx.x;
    const double* hp = hyper + tab[4 * n + t] * (LAMB ? LAMB_HYPER : LARS_HYPER);
    double coef = 1.0;
    if (!LAMB && clip > 0.0) {
        const Sum2 all = stretch_sum2(partial, partial, 0, nchunks, lds);
        if (threadIdx.x == 0) {
            const float norm = (float)sqrt(all.a);
            const double nd = (double)norm;
            const float cf = (float)(clip / (clip > nd ? clip : nd));        // inf norm -> 0, nan norm -> nan
            coef = (double)cf;
            if (t == 0) {
                clip_out[0] = norm;
                clip_out[1] = cf;
            }
        }
    }
    const Sum2 s = stretch_sum2(partial, partial + nchunks, first[t], first[t + 1], lds);
    if (threadIdx.x != 0) return;
    const double wn = sqrt(s.b);
    double r = 1.0;
    if (LAMB) {
        const double un = sqrt(s.a);
        if (hp[5] != 0.0 && wn > 0.0 && un > 0.0) r = wn / un;
    } else {
        const double gn = coef * sqrt(s.a), eta = hp[5];
        if (eta > 0.0 && wn > 0.0 && gn > 0.0) r = eta * wn / (gn + hp[1] * wn + hp[6]);
    }
    ratio[t] = (float)r;
}

bool bad_common(const void* tab, int32_t n, const void* chunks, int32_t nchunks, const void* first, const void* hyper, double clip,
                const void* partial, const void* ratio, const void* clip_out) {
    return !tab || n < 1 || !chunks || nchunks < 1 || !first || !hyper || !partial || !ratio || !(clip >= 0.0) || isinf(clip) ||
           (clip > 0.0 && !clip_out);
}

}  // namespace

extern "C" int fva_lars_step(const int64_t* tab_dev, int32_t n, const int64_t* chunks_dev, int32_t nchunks, const int64_t* first_dev,
                             const double* hyper_dev, int32_t* fresh_dev, int32_t clear_fresh, double clip_norm, double* partial_dev,
                             float* ratio_dev, float* clip_out_dev, void* stream) {
    if (bad_common(tab_dev, n, chunks_dev, nchunks, first_dev, hyper_dev, clip_norm, partial_dev, ratio_dev, clip_out_dev) || !fresh_dev)
        return fva_fail(FVA_ERR_ARG, "fva_lars_step: bad argument (null table / chunk list / hyper-parameters / fresh flags / workspace, empty "
                                     "chunk list, or clip_norm not finite and >= 0 or without clip_out)");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lars_norm_kernel, dim3(nchunks), dim3(LW_THREADS), 0, s, tab_dev, n, chunks_dev, nchunks, partial_dev);
    FVA_LAUNCH_CHECK("lars_norm_kernel");
    hipLaunchKernelGGL(trust_kernel<false>, dim3(n), dim3(LW_THREADS), 0, s, tab_dev, n, first_dev, (const double*)partial_dev, nchunks,
                       hyper_dev, clip_norm, clip_out_dev, ratio_dev);
    FVA_LAUNCH_CHECK("trust_kernel<lars>");
    hipLaunchKernelGGL(lars_apply_kernel, dim3(nchunks), dim3(LW_THREADS), 0, s, tab_dev, n, chunks_dev, hyper_dev, (const int32_t*)fresh_dev,
                       (const float*)ratio_dev, clip_norm > 0.0 ? (const float*)(clip_out_dev + 1) : (const float*)nullptr);
    FVA_LAUNCH_CHECK("lars_apply_kernel");
    if (clear_fresh) {
        hipLaunchKernelGGL(lars_clear_fresh, dim3((n + 255) / 256), dim3(256), 0, s, tab_dev, n, fresh_dev);
        FVA_LAUNCH_CHECK("lars_clear_fresh");
    }
    return FVA_OK;
}

extern "C" int fva_lamb_step(const int64_t* tab_dev, int32_t n, const int64_t* chunks_dev, int32_t nchunks, const int64_t* first_dev,
                             const double* hyper_dev, int32_t groups, double* state_dev, double clip_norm, double* partial_dev,
                             float* ratio_dev, float* clip_out_dev, void* stream) {
    if (bad_common(tab_dev, n, chunks_dev, nchunks, first_dev, hyper_dev, clip_norm, partial_dev, ratio_dev, clip_out_dev) || groups < 1 ||
        !state_dev)
        return fva_fail(FVA_ERR_ARG, "fva_lamb_step: bad argument (null table / chunk list / hyper-parameters / step state / workspace, empty "
                                     "chunk list, no group, or clip_norm not finite and >= 0 or without clip_out)");
    const hipStream_t s = (hipStream_t)stream;
    // the global norm has to exist before the moments: the SGD launches read rows 1 (grad) and 3 (count), which this table shares
    if (clip_norm > 0.0 && fva_sgd_clip_coef(tab_dev, n, chunks_dev, nchunks, partial_dev, clip_norm, clip_out_dev, stream) != FVA_OK) return -1;
    const float* coef = clip_norm > 0.0 ? clip_out_dev + 1 : nullptr;
    hipLaunchKernelGGL(lamb_tick_kernel, dim3(1), dim3(64), 0, s, state_dev, hyper_dev, groups);
    FVA_LAUNCH_CHECK("lamb_tick_kernel");
    hipLaunchKernelGGL(lamb_norm_kernel, dim3(nchunks), dim3(LW_THREADS), 0, s, tab_dev, n, chunks_dev, nchunks, hyper_dev,
                       (const double*)state_dev, coef, partial_dev);
    FVA_LAUNCH_CHECK("lamb_norm_kernel");
    hipLaunchKernelGGL(trust_kernel<true>, dim3(n), dim3(LW_THREADS), 0, s, tab_dev, n, first_dev, (const double*)partial_dev, nchunks,
                       hyper_dev, 0.0, (float*)nullptr, ratio_dev);
    FVA_LAUNCH_CHECK("trust_kernel<lamb>");
    hipLaunchKernelGGL(lamb_apply_kernel, dim3(nchunks), dim3(LW_THREADS), 0, s, tab_dev, n, chunks_dev, hyper_dev, (const double*)state_dev,
                       (const float*)ratio_dev);
    FVA_LAUNCH_CHECK("lamb_apply_kernel");
    return FVA_OK;
}
