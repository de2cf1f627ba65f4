// The chunk list of the launches that split their work into fixed-size chunks, not tensors (SGD in optim.hip, ema.hip): one int64
// word (tensor << 32) | chunk number per block, built by fastvision_amd/multi_tensor.py.  A block works on units [begin, end) of its
// tensor, begin = number * per: elements with per = MT_CHUNK, or bytes with per = 4 * MT_CHUNK.
#pragma once
#include <stdint.h>

constexpr int MT_CHUNK = 16384;         // fp32 elements per block (64 KiB of each tensor): 16 float4 iterations of 256 threads

__device__ __forceinline__ int64_t mt_tensor(int64_t word) { return word >> 32; }           // row of the pointer table
__device__ __forceinline__ int64_t mt_number(int64_t word) { return word & 0xffffffffll; }  // chunk of that tensor
__device__ __forceinline__ int64_t mt_end(int64_t begin, int64_t count, int64_t per) {      // in a tensor of `count` units
    return begin + per < count ? begin + per : count;
}

// begin and end at once for a caller that already holds `count` (ema.hip).  sgd_chunk (optim.hip) reads its count from the table
// between the two and calls mt_end itself: either way the kernels compile to the instructions they had with the decode written out.
struct MtSpan {
    int64_t begin, end;
};
__device__ __forceinline__ MtSpan mt_span(int64_t number, int64_t count, int64_t per) {
    MtSpan s;
    s.begin = number * per;
    s.end = mt_end(s.begin, count, per);
    return s;
}
