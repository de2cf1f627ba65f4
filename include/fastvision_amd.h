/*
 * fastvision_amd.h -- C ABI of libfastvision_amd.so: the MI355X (gfx950) kernels behind the
 * YOLOv3 training hot path of ielym/fastvision.
 *
 * The reference is pure Python on PyTorch and has NO FFI of its own: the boundary a
 * maintainer would bind is the set of ATen ops its modules issue.  Each entry point below names the
 * reference call site it replaces (paths relative to the reference root).  INTEGRATION.md shows the
 * ctypes binding the reference side would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller for the
 *     duration of the call (borrowed from torch.Tensor.data_ptr()); outputs are preallocated;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); nothing here
 *     synchronises the host, allocates, or copies to the host;
 *   - every function returns 0 on success, a negative fva_status otherwise; fva_last_error()
 *     returns a static message for the calling thread;
 *   - dtype: FVA_F32 (exact fp32, f32-input MFMA) or FVA_BF16 (bf16 storage, fp32 accumulate).
 *
 * Activation layout ("halo NHWC"): a feature map of logical shape [B,C,H,W] is stored as
 * [B][H+2*pad][W+2*pad][C] with a zero border of `pad` pixels (pad is 1 for every map a 3x3 conv or
 * its dgrad reads, 0 otherwise).  Channels are contiguous.  Raw conv outputs (pre-BN) are dense
 * [B*OH*OW][Cout] (pad 0).
 */
#ifndef FASTVISION_AMD_H
#define FASTVISION_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { FVA_F32 = 0, FVA_BF16 = 1 } fva_dtype;

typedef enum {
    FVA_OK = 0,
    FVA_ERR_ARG = -1,      /* unsupported shape / null pointer / bad enum */
    FVA_ERR_LAUNCH = -2,   /* hipLaunchKernel or hipGetLastError failed */
    FVA_ERR_WORKSPACE = -3 /* workspace too small: call the matching *_workspace() */
} fva_status;

const char* fva_last_error(void);
int fva_version(void);

/* Live timing of the MFMA convolution entry points with HIP events on their launch stream, taken inside the library (no
 * per-call host work in the caller).  fva_profile_start(max_spans) creates the events -- call it OUTSIDE the region being
 * timed -- and arms the spans; fva_profile_stop() synchronises the device, disarms and returns the number of spans with
 * cls (low byte: 0 forward incl. head, 1 dgrad, 2 wgrad incl. its reduce, 3 a forward launch that also carries the apply pass of the
 * block before it (fva_conv1x1_fwd_apply[_acc]; FLOPs = the convolution's); bits 8..: the layer's kernel size), algorithmic
 * FLOPs and elapsed milliseconds of each.
 * fva_profile_classes(mask, stride) restricts the spans to the classes whose bit is set and, of those calls, to every
 * stride-th one (default: all classes, stride 1).  A span costs two event packets on the stream and the kernels on either
 * side of them no longer overlap their launch with the neighbour's tail (measured: ~7 us of GPU time per span, 3 % of the
 * train step when every forward convolution is bracketed), so a throughput measurement brackets a sample of the kernel
 * class it reports. */
int fva_profile_start(int32_t max_spans);
int fva_profile_classes(uint32_t mask, int32_t stride);

/* A low-priority side stream for work that nothing waits for until the end of the backward pass (the weight gradients).
 * fork: the side stream (returned) waits for everything enqueued on main_stream so far.  join: main_stream waits for
 * everything enqueued on the side stream so far.  Buffers the side stream reads or writes must stay alive until a join.
 * renew: drain and drop the side stream; the next fork creates a fresh one (how a stream maps onto the hardware queues is decided at its
 * creation, and a stream that landed badly no longer yields to the launch stream -- ops.autotune_wgrad_side_stream() asks for another). */
int fva_side_stream_fork(void* main_stream, void** side_stream);
int fva_side_stream_join(void* main_stream);
int fva_side_stream_renew(void);
int32_t fva_profile_stop(int32_t* cls, double* flop, float* ms, int32_t cap);

/* ------------------------------------------------------------------------------------------------
 * Convolution (no bias), implicit GEMM on MFMA.  Replaces nn.Conv2d as used by ConvBlock3x3 /
 * ConvBlock1x1 (classfication/models/darknet53.py:5-9,22-44; detection/neck/yolov3neck.py:5-9,22-44;
 * demos/yolov3_u/models/{darknet,yolov3}.py:6-40) and its autograd backward.
 * ksize in {1,3}, padding = ksize/2, stride in {1,2}, groups 1, dilation 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t dtype;   /* fva_dtype of activations and packed weights */
    int32_t B, H, W; /* logical input size */
    int32_t Cin, Cout;
    int32_t ksize, stride;
    int32_t in_pad;  /* zero border of the input buffer  (>= ksize/2) */
    int32_t dy_pad;  /* zero border of the dY buffer used by dgrad/wgrad (>= 1 when ksize==3) */
} fva_conv_desc;

/* fp32 OIHW master weights [Cout][Cin][k][k] -> the two packed operand layouts (dtype of desc):
 *   w_fwd [k*k (+1 pad tap if Cin==32 && bf16)][Cout][Cin]   and   w_dgrad [k*k (+pad)][Cin][Cout].
 * Either output may be NULL.  Sizes in elements: fva_conv_packed_elems(). */
int fva_conv_pack_weights(const fva_conv_desc* d, const float* w_oihw, void* w_fwd, void* w_dgrad, void* stream);
int64_t fva_conv_packed_elems(const fva_conv_desc* d, int for_dgrad);
/* The same for every conv layer of a model in ONE launch (after each optimizer step): `table` is a DEVICE array of n
 * entries; taps_fwd / taps_dgrad = fva_conv_packed_elems(...) / (Cout*Cin); max_elems = largest taps*Cout*Cin. */
typedef struct {
    const float* w;       /* fp32 OIHW master weight */
    void* w_fwd;          /* [taps_fwd][Cout][Cin]   (may be NULL) */
    void* w_dgrad;        /* [taps_dgrad][Cin][Cout] (may be NULL) */
    int32_t Cout, Cin, ksize, taps_fwd, taps_dgrad, dtype;
    int32_t dgrad_paired; /* 1 when taps_dgrad == 12: the paired stride-2 layout [6][2*Cin][Cout] thin layers use
                           * (fva_conv_packed_elems() of a stride-2 descriptor tells; see conv_igemm.hip dgrad_paired) */
    int32_t tile_start;   /* fva_conv_pack_weights_tiled: 32 x 32 (Cout x Cin) tiles of the entries BEFORE this one, i.e. the running sum of
                           * ceil(Cout / 32) * ceil(Cin / 32); ignored by fva_conv_pack_weights_multi */
} fva_pack_entry;
int fva_conv_pack_weights_multi(const fva_pack_entry* table, int32_t n, int64_t max_elems, void* stream);
/* The same result from a launch of ONE block per 32 x 32 weight tile of any layer (total_tiles = the running sum after the last
 * entry): no idle blocks for small layers, 16-byte loads and 8-byte stores on aligned bf16 tiles. */
int fva_conv_pack_weights_tiled(const fva_pack_entry* table, int32_t n, int32_t total_tiles, void* stream);

/* Which MFMA kernel the calling thread's last convolution entry point launched: "igemm8" (256x256 8-phase), "igemm128", "igemm256x64",
 * "pconv", "pdgrad2" (patch kernels); "wgrad8", "wgrad128", "wgrad128thin", "wgrad64f32", "pwgrad".  For tests that must know what they compared. */
const char* fva_conv_last_kernel(void);

/* Diagnostic: while set (non-NULL), every block of an 8-phase convolution launch writes eight values to stamps[block * 8 ..]:
 * wall_clock64 (100 MHz) at block entry, first k-tile ready, k-loop done and exit, then the shader-clock cycle counter at the
 * same four points (cycles / wall time = the shader clock under load).  `rows` = capacity of the buffer in blocks (8 values
 * each): blocks beyond it do not stamp.  NULL switches the stamps off.  With FVA_STAMP_IGEMM=1 in the environment the 128x128 /
 * 256x64 kernels stamp too, eight wall-clock values per block: entry, first DMA issued, first k-tile landed, k loop done, tile staged
 * in LDS, exit, source rows ready, epilogue operands requested (tools/tile_timing.py pw). */
int fva_conv_debug_stamps(void* stamps, int32_t rows);
/* The thin 3x3 stride-1 bf16 layers (reduction channels <= 128, outputs <= 128, maps of 64 x 64 and more) run on the patch kernel
 * (conv_igemm.hip pconv_kernel: the input patch of an 8 x 32 output tile is staged once for the nine taps).  This switches it off /
 * on for the process (default on; env FVA_PCONV=0) and returns the previous setting: fva_conv_stat_blocks / fva_conv_dgrad_stat_rows
 * follow the setting, so do not change it between sizing a table and the launch that fills it. */
int fva_conv_patch_kernel(int on);

/* y[B*OH*OW][Cout] = conv(x) (dense, dtype).  If stats_partial != NULL also writes per-row-block
 * partial sums for BatchNorm: stats_partial[blk][0][c] = sum_y, [blk][1][c] = sum_y^2 over the rows of
 * that block (blk < fva_conv_stat_blocks()); they are reduced by fva_bn_finalize(). */
int fva_conv_fwd(const fva_conv_desc* d, const void* x, const void* w_fwd, void* y, float* stats_partial, void* stream);
/* Training forward of a 1x1 layer whose input z has not been produced yet: z = SiLU(y_prev * scale + shift) (+ residual) -- the
 * apply pass of the block before it (fva_bn_silu_apply: same arithmetic, same bits) -- is computed in this launch's operand path,
 * written ONCE to the halo buffer z (border d->in_pad <= 1 included, for every other reader of z: the residual identity, the weight
 * gradient, the next block) and fed to the MFMAs from LDS without being read back: the separate apply launch and one read of z go
 * (classfication/models/darknet53.py:46-63: a residual block's conv1 always follows the previous block's SiLU + add).  y / statistics
 * as fva_conv_fwd (same tiles, same rows, same bits).  bf16; Cin % 64 == 0, Cin <= 512; Cout <= 128 (one column block, so that every element
 * is transformed once); y_prev dense [B*H*W][Cin]; residual (optional) a halo buffer of z's shape with border res_pad. */
int fva_conv1x1_fwd_apply(const fva_conv_desc* d, const void* y_prev, const float* scale, const float* shift, const void* residual,
                          int32_t res_pad, void* z, const void* w_fwd, void* y, float* stats_partial, void* stream);
/* Inference form: eval-mode BatchNorm folded into a per-channel affine and SiLU applied in the convolution's epilogue,
 * z = SiLU(conv(x) * scale[c] + shift[c]) (+ residual), written straight into the halo buffer z [B][OH+2p][OW+2p][Cout]
 * (interior by the MFMA kernel, zero border by a small second launch).  residual (optional) has z's geometry.
 * Replaces conv + bn (running statistics) + SiLU (+ add) of ConvBlock / ResidualBlock in eval mode
 * (classfication/models/darknet53.py:28-31,58-62) with one pass over the output instead of three. */
int fva_conv_fwd_bnact(const fva_conv_desc* d, const void* x, const void* w_fwd, const float* scale, const float* shift,
                       const void* residual, void* z, int32_t z_pad, void* stream);
int32_t fva_conv_stat_blocks(const fva_conv_desc* d);

/* dx[B][H][W][Cin] (dense, dtype) = conv_transpose(dy, w) (+ addend).  dy is halo NHWC with border d->dy_pad.
 * addend (optional, dense like dx, may alias dx) is added in the epilogue: the residual-branch gradient sum. */
int fva_conv_dgrad(const fva_conv_desc* d, const void* dy, const void* w_dgrad, void* dx, const void* addend, void* stream);

/* The same data gradient with the FIRST pass of the BatchNorm backward of the layer that produced this convolution's input taken
 * in its epilogue.  dx (incl. the addend) is dz of that producer block z = SiLU(BN(y)) (classfication/models/darknet53.py:28-31,
 * 58-62: what autograd's native_batch_norm_backward + SiLU backward reduce over the batch): per row block and channel the
 * epilogue adds up dU = dz * SiLU'(y * scale + shift) and dU * (y - mean) * rstd from the values it stores, reading y (dense
 * [B*H*W][Cin], the producer's pre-BN output) once.  partial: [fva_bn_partial_rows(fva_conv_dgrad_stat_rows(d))][2][Cin] floats (the rows
 * beyond fva_conv_dgrad_stat_rows(d) are fva_bn_bwd_finalize's scratch), fixed order -- feed it to
 * fva_bn_bwd_finalize (partial_rows = the rows allocated) in place of fva_bn_silu_bwd_reduce's table.  Valid only when dx IS the whole dz (the
 * producer's output has no other consumer than this convolution and, through `addend`, the residual identity). */
typedef struct {
    const void* y;
    const float *scale, *shift, *mean, *rstd;
    float* partial;
    int64_t* acc;        /* when not NULL the sums are ADDED to this accumulator (the producer layer's backward one, see "BatchNorm statistics
                            WITHOUT a finalize launch") and `partial` is not used */
    int32_t acc_replicas;
} fva_bn_bwd_fuse;
int fva_conv_dgrad_bnstats(const fva_conv_desc* d, const void* dy, const void* w_dgrad, void* dx, const void* addend,
                           const fva_bn_bwd_fuse* fuse, void* stream);
int32_t fva_conv_dgrad_stat_rows(const fva_conv_desc* d);

/* dw (fp32, OIHW) (+)= sum_pixels dy x.  Deterministic: split-K partial tiles go to `workspace`
 * (fva_conv_wgrad_workspace() bytes) and are reduced in fixed order. */
int fva_conv_wgrad(const fva_conv_desc* d, const void* x, const void* dy, float* dw_oihw, int accumulate,
                   void* workspace, int64_t workspace_bytes, void* stream);
int64_t fva_conv_wgrad_workspace(const fva_conv_desc* d);
/* The split-K plan of the weight gradients, process-wide: 0 = for a launch that has the chip to itself (default), 1 = for launches
 * that run beside the rest of the backward pass on the side stream (half the block slots: fewer, longer blocks).  The plan fixes
 * the split factor and with it the fp32 summation order of dW: results are bit-identical between runs under the SAME plan, and
 * differ in the last bits between plans.  Returns the previous setting; any other argument only queries.  The workspace size
 * covers both. */
int fva_conv_wgrad_plan(int beside);

/* Stem: conv 3x3 s1 p1 on fp32 NCHW images with Cin <= 3, Cout == 32 (darknet53.py:73 `conv0`).
 * y dense [B*H*W][Cout] dtype + BN partial stats;  wgrad from dy dense [B*H*W][Cout] (pad 0).
 * bf16 with W a multiple of 16 runs on MFMA from a bf16 NHWC4 copy of the images that the call builds in `workspace`
 * (fva_stem_fwd_workspace() bytes; 0 for the other cases, which use the exact fp32 direct kernel). */
int fva_stem_fwd(int dtype, const float* images_nchw, const float* w_oihw, void* y, float* stats_partial,
                 void* workspace, int64_t workspace_bytes, int B, int Cin, int H, int W, int Cout, void* stream);
int64_t fva_stem_fwd_workspace(int dtype, int B, int H, int W);
int32_t fva_stem_stat_blocks(int dtype, int B, int H, int W);
int32_t fva_stem_fused_blocks(int B, int H, int W);   /* partial rows written by fva_stem_fused modes 0 and 2 */
int fva_stem_wgrad(int dtype, const float* images_nchw, const void* dy, float* dw_oihw, int accumulate,
                   void* workspace, int64_t workspace_bytes, int B, int Cin, int H, int W, int Cout, void* stream);
int64_t fva_stem_wgrad_workspace(int B, int Cin, int H, int W, int Cout);
/* bf16 alternative on the MFMA weight-gradient kernel, from the NHWC4 image copy that fva_stem_fwd left in its workspace and
 * a halo dY [B][H+2][W+2][32]: dw_raw [32][16][3] fp32 = [co][kw*4 + ci][kh] (the caller keeps kw < 3, ci < Cin). */
int fva_stem_wgrad_mfma(const void* images_nhwc4, const void* dy_halo, float* dw_raw, void* workspace, int64_t workspace_bytes,
                        int B, int H, int W, void* stream);
int64_t fva_stem_wgrad_mfma_workspace(void);
/* bf16 training form that never stores conv0's pre-BN output: the four BatchNorm / SiLU passes recompute it on MFMA from the
 * NHWC4 image copy (fva_stem_pack; fva_stem_fwd_workspace() bytes).  mode 0: partial sums of y, y^2 -> part; 1: z = SiLU(BN(y))
 * -> halo buffer out [B][H+2][W+2][32]; 2: partial sums of dU, dU*xhat from dz (dense [B*H*W][32]) -> part; 3: dY -> halo
 * buffer out.  part: fva_stem_fused_blocks() rows of [2][32] filled here, ALLOCATED with
 * fva_bn_partial_rows(fva_stem_fused_blocks()) rows, reduced by fva_bn_finalize / fva_bn_bwd_finalize. */
int fva_stem_pack(const float* images_nchw, void* images_nhwc4, int64_t bytes, int B, int Cin, int H, int W, void* stream);
int fva_stem_fused(int mode, const void* images_nhwc4, const float* w_oihw, const void* dz, const float* scale, const float* shift,
                   const float* save_mean, const float* save_rstd, const float* coef, void* out, float* part, int B, int Cin, int H,
                   int W, void* stream);

/* Head: biased 1x1 conv to N = A*(5+C) channels (detection/head/yolov3head.py:50,60;
 * demos/yolov3_u/models/yolov3.py:119-135).  Output fp32, dense [B*H*W][N] (pixel-major, N contiguous):
 * the library's permuted [B,A,H,W,5+C] (yolov3head.py:63) and the demo's NCHW are strided views of it. */
int fva_head_fwd(const fva_conv_desc* d, const void* x, const void* w_fwd, const float* bias, float* out, void* stream);
/* dhead fp32 [B*H*W][N] * (*grad_scale, device scalar, may be NULL = 1) -> dy (dtype) as a halo buffer
 * [B][H+2][W+2][Npad] (border 1, pad columns N..Npad-1 zero) ready for fva_conv_dgrad / fva_conv_wgrad with
 * Cout = Npad, and dbias[N] (+)= column sums (deterministic two-stage reduce whose first stage rides in the pass that writes dy;
 * workspace >= 4*N*4096 bytes). */
int fva_head_bwd_prepare(int dtype, const float* dhead, const float* grad_scale, void* dy, float* dbias,
                         int accumulate, void* workspace, int B, int H, int W, int N, int Npad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (training + eval) fused with SiLU and the residual add.  Replaces nn.BatchNorm2d +
 * nn.SiLU (+ `identity + conv2`) in ConvBlock3x3 / ConvBlock1x1 / ResidualBlock (darknet53.py:11-17,28-31,58-62).
 * ---------------------------------------------------------------------------------------------- */
/* Reduce conv partial stats -> batch mean / biased var; update running stats (momentum, unbiased var) and
 * num_batches_tracked += 1 (both optional: NULL skips); emit save_mean, save_rstd and the fused
 * scale = gamma*rstd, shift = beta - mean*scale.
 * stats_partial must hold fva_bn_partial_rows(nblocks) rows of [2][C] floats: the conv kernels fill the first
 * nblocks rows; tables of >= 1024 rows are first folded in parallel into the extra rows (scratch).  partial_rows = the rows
 * the caller allocated: a table that is too short is refused (FVA_ERR_WORKSPACE) instead of written past. */
int32_t fva_bn_partial_rows(int32_t nblocks);
int fva_bn_finalize(float* stats_partial, int32_t nblocks, int32_t partial_rows, int64_t count, int32_t C,
                    const float* gamma, const float* beta, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked, float momentum, float eps, float* save_mean, float* save_rstd,
                    float* scale, float* shift, void* stream);
/* Eval mode: scale/shift from running stats. */
int fva_bn_eval_coeffs(int32_t C, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, void* stream);
/* z = silu(y*scale + shift) (+ residual); writes the whole halo buffer z[B][H+2p][W+2p][C] incl. zero
 * border.  residual (optional) has the layout of z with border res_pad. */
int fva_bn_silu_apply(int dtype, const void* y, const float* scale, const float* shift, const void* residual,
                      int res_pad, void* z, int z_pad, int B, int H, int W, int C, void* stream);
/* ---- BatchNorm statistics WITHOUT a finalize launch (round 4) ------------------------------------------------------------------
 * The convolution's tiles ADD their per-channel partial sums into a fixed-point accumulator (two int64 words per sum: integer
 * addition is associative, so the total is the same bits whatever order the tiles arrive in -- deterministic run to run) and the
 * pass that consumes the statistics finalises them in its own prologue: every block computes mean / rstd / scale / shift of all
 * channels once (the arithmetic of fva_bn_finalize), block 0 also writes them out for the backward pass and updates the running
 * statistics (nn.BatchNorm2d in training mode, classfication/models/darknet53.py:11-12).  Replaces the 197 latency-bound finalize /
 * pre-reduce launches of a YOLOv3 step, each a dependent step of the chain.
 *   An accumulator is int64 [replicas][FVA_BN_ACC_WORDS][C] -- per channel the high and low words of the two sums and a count of
 *   non-finite partials (a channel that received one finalises to NaN, as a floating-point sum would) -- and must be ZERO when its first
 *   producer runs.  `replicas` (a power of two <= FVA_BN_ACC_MAX_REPLICAS; the same number for every producer and consumer of an
 *   accumulator): atomics on one address are served one after the other (~10 ns each), so a layer whose convolution runs thousands of
 *   tiles spreads them over several copies (block b adds to copy b mod replicas; about one copy per 65536 output pixels keeps the queue
 *   per address below 5 us) and the consumer adds the copies up.  A layer keeps one accumulator per direction (forward: sums of y and
 *   y^2; backward: sums of dU and dU * xhat), both with the same `replicas`.  A consumer cannot zero the accumulator it reads (its other
 *   blocks may not have read it yet), so each consumer zeroes the OTHER direction's (`zero`, may be NULL): the forward consumer clears
 *   the backward sums of the previous step, the backward consumer clears the forward sums.  fva_bn_acc_finalize, the only reader of
 *   its launch, zeroes both.  An accumulator nobody zeroed (a forward pass without backward) is the caller's to clear.
 * Forward producers: fva_conv_fwd_acc (= fva_conv_fwd with the accumulator in place of the table), fva_conv1x1_fwd_apply_acc;
 * forward consumers: fva_bn_silu_apply_acc, fva_conv1x1_fwd_apply_acc (of the block BEFORE it), fva_bn_acc_finalize.
 * Backward producers: fva_conv_dgrad_bnstats with fva_bn_bwd_fuse::acc set, fva_bn_silu_bwd_reduce_acc; consumer: fva_bn_silu_bwd_apply_acc. */
#define FVA_BN_ACC_WORDS 5
#define FVA_BN_ACC_MAX_REPLICAS 32
typedef struct {
    int64_t* acc;
    int64_t* zero;                          /* may be NULL: the other direction's accumulator, returned to zero by this launch */
    int32_t replicas;
    const float *gamma, *beta;
    float *running_mean, *running_var;      /* may be NULL */
    int64_t* num_batches_tracked;           /* may be NULL */
    float momentum, eps;
    float *save_mean, *save_rstd, *scale, *shift;   /* outputs, [C] each */
} fva_bn_fwd_acc;
typedef struct {
    int64_t* acc;
    int64_t* zero;                          /* may be NULL */
    int32_t replicas;
    const float* gamma;
    float *dgamma, *dbeta;                  /* outputs (+= when accumulate) */
    int32_t accumulate;
} fva_bn_bwd_acc;
int fva_conv_fwd_acc(const fva_conv_desc* d, const void* x, const void* w_fwd, void* y, int64_t* acc, int32_t replicas, void* stream);
int fva_bn_silu_apply_acc(int dtype, const void* y, const fva_bn_fwd_acc* acc, const void* residual, int res_pad, void* z, int z_pad,
                          int B, int H, int W, int C, void* stream);
/* The accumulator finalised by a small launch of its own (writes the four outputs, updates the running statistics, zeroes the
 * accumulator): for a consumer that cannot do it in its prologue -- the thin tile of the fused 1x1 form, foreign code. */
int fva_bn_acc_finalize(const fva_bn_fwd_acc* acc, int64_t M, int C, void* stream);
/* fva_conv1x1_fwd_apply with this layer's statistics added to acc_out, and the block before described by `prev`: prev->acc != NULL: its
 * statistics are finalised in this launch's prologue (Cout = 128: the wide tile; thinner layers run fva_bn_acc_finalize first, inside this
 * call); prev->acc == NULL: prev->scale / prev->shift are final already. */
int fva_conv1x1_fwd_apply_acc(const fva_conv_desc* d, const void* y_prev, const fva_bn_fwd_acc* prev, const void* residual, int32_t res_pad,
                              void* z, const void* w_fwd, void* y, int64_t* acc_out, int32_t replicas_out, void* stream);

/* Backward, pass 1: partial sums over pixels of dU = dz*silu'(u) and dU*xhat (u = y*scale+shift). */
int fva_bn_silu_bwd_reduce(int dtype, const void* dz, const void* y, const float* scale, const float* shift,
                           const float* save_mean, const float* save_rstd, float* partial, int32_t nblocks,
                           int64_t M, int C, void* stream);
int32_t fva_bn_bwd_blocks(int dtype, int64_t M, int C);
/* The accumulator forms of the two backward passes (see "BatchNorm statistics WITHOUT a finalize launch"): pass 1 adds its sums to
 * acc; pass 2 takes dgamma, dbeta and its coefficients from the accumulator in its prologue (no fva_bn_bwd_finalize). */
int fva_bn_silu_bwd_reduce_acc(int dtype, const void* dz, const void* y, const float* scale, const float* shift,
                               const float* save_mean, const float* save_rstd, int64_t* acc, int32_t replicas, int64_t M, int C, void* stream);
int fva_bn_silu_bwd_apply_acc(int dtype, const void* dz, const void* y, const float* scale, const float* shift,
                              const float* save_mean, const float* save_rstd, const fva_bn_bwd_acc* acc, void* dy, int dy_pad,
                              int B, int H, int W, int C, void* stream);
/* Backward, finalize: dgamma, dbeta (+)= and the per-channel coefficients of pass 2.  partial: the table of
 * fva_bn_silu_bwd_reduce or of fva_conv_dgrad_bnstats, ALLOCATED with fva_bn_partial_rows(nblocks) rows: a long table (1024 rows
 * or more) is folded in parallel first, into doubles kept behind the nblocks rows the producer fills; partial_rows = the rows
 * allocated (checked: FVA_ERR_WORKSPACE). */
int fva_bn_bwd_finalize(float* partial, int32_t nblocks, int32_t partial_rows, int64_t M, int C, const float* gamma,
                        const float* save_rstd, float* dgamma, float* dbeta, int accumulate, float* coef,
                        void* stream);
/* Backward, pass 2: dy = gamma*rstd*(dU - dbeta/n - xhat*dgamma/n) written as halo buffer (border dy_pad). */
int fva_bn_silu_bwd_apply(int dtype, const void* dz, const void* y, const float* scale, const float* shift,
                          const float* save_mean, const float* save_rstd, const float* coef, void* dy, int dy_pad,
                          int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FPN glue and layout conversion.  Replaces nn.Upsample(scale_factor=2,'nearest') + torch.cat
 * (yolov3neck.py:71,105,110; demos/yolov3_u/models/yolov3.py:96,100).
 * ---------------------------------------------------------------------------------------------- */
/* out[B][2h+2][2w+2][Cup+Cskip] (pad 1).  up: [B][h+2pu][w+2pu][Cup]; skip: [B][2h+2ps][2w+2ps][Cskip].
 * up_first != 0 -> channel order [up | skip] (library), else [skip | up] (demo). */
int fva_upsample2_concat_fwd(int dtype, const void* up, int up_pad, const void* skip, int skip_pad, void* out,
                             int B, int h, int w, int Cup, int Cskip, int up_first, void* stream);
/* dcat dense [B][2h][2w][Cup+Cskip] -> dup dense [B][h][w][Cup] (2x2 sums) and dskip dense [B][2h][2w][Cskip]. */
int fva_upsample2_concat_bwd(int dtype, const void* dcat, void* dup, void* dskip, int B, int h, int w, int Cup,
                             int Cskip, int up_first, void* stream);
/* Arbitrary-stride fp32/bf16 [B,C,H,W] tensor -> halo NHWC buffer of `dtype` (foreign inputs). */
int fva_pack_nchw(int dtype, const void* src, int src_is_bf16, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                  void* dst, int dst_pad, int B, int C, int H, int W, void* stream);
/* Cast / re-layout dense or halo NHWC -> dense NHWC of another dtype (gradient hand-off at the API edge). */
int fva_cast_nhwc(const void* src, int src_dtype, int src_pad, void* dst, int dst_dtype, int dst_pad,
                  int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Target assignment + loss, library surface.  Replaces Yolov3Loss.build_target / forward
 * (loss/yolov3_loss.py:29-124) with BiCrossEntropyLoss (loss/classification_loss.py:42-65),
 * CIOULoss (loss/iou_loss.py:88-107) and cal_iou/CIOU/DIOU/xyxy_iou (detection/tools/IOU.py).
 * Head tensors are addressed through explicit element strides so any view works.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    float* data;          /* fp32 head tensor of this level */
    float* grad;          /* fp32 gradient buffer with the SAME strides (may be NULL: loss only) */
    int64_t sb, sa, sy, sx, sk; /* element strides of (batch, anchor, grid_y, grid_x, channel) */
    int32_t B, A, H, W, K;      /* K = 5 + num_classes */
    float anchor_w[8], anchor_h[8]; /* PIXEL-unit anchors of this level (A <= 8) */
    float stride;               /* backbone stride of this level */
} fva_head_level;

/* Matcher (build_target, yolov3_loss.py:75-124).  targets [T][6] fp32.  Outputs per level, capacity T*A rows
 * in the reference's row order (target-major, anchor-minor): count[1] i32, b/gx/gy/a/cls i64 [cap],
 * xywh [cap][4] f32, anc [cap][2] f32.  Integer outputs are bit-exact with the reference. */
typedef struct {
    int32_t* count;
    int64_t *b, *gx, *gy, *a, *cls;
    float *xywh, *anc;
} fva_match_out;
int fva_yolov3_match(const float* targets, int32_t T, const fva_head_level* level, const fva_match_out* out, void* stream);

/* Loss forward + analytic backward for all levels in one call (yolov3_loss.py:29-72).
 * loss_out[4] = {total, box, conf, cls} (total already * ratios * B); grads (if level.grad != NULL) are
 * d total / d head ACCUMULATED into level.grad, which the caller zero-fills first (the objectness channel
 * of every cell is stored, matched rows are added).  workspace: fva_yolov3_loss_workspace(). */
int fva_yolov3_loss(const float* targets, int32_t T, const fva_head_level* levels, int32_t nlevels,
                    float ratio_box, float ratio_conf, float ratio_cls, float* loss_out,
                    void* workspace, int64_t workspace_bytes, void* stream);
int64_t fva_yolov3_loss_workspace(int32_t T, const fva_head_level* levels, int32_t nlevels);

/* Data-parallel form of the same loss.  The reference wraps the model in nn.DataParallel (demos/yolov3_u/train.py:85) and
 * evaluates yolov3_loss.py:29-72 ONCE on the batch gathered from all N replicas: its per-match means divide by the match count
 * of the whole job and its result is multiplied by the job's batch size.  With one process per GPU each rank calls this entry on
 * its own images and targets with norm_counts[nlevels] = the per-level match counts summed over all ranks (device memory: run
 * fva_yolov3_match per level, all-reduce the three counts) and norm_batch = N * B: loss_out[0] is then this rank's SHARE of that
 * loss and level.grad its gradient, so that a SUM all-reduce of the parameter gradients (and of loss_out[0]) reproduces the
 * reference's step.  norm_counts == NULL: plain fva_yolov3_loss. */
int fva_yolov3_loss_dp(const float* targets, int32_t T, const fva_head_level* levels, int32_t nlevels,
                       float ratio_box, float ratio_conf, float ratio_cls, const int32_t* norm_counts, int32_t norm_batch,
                       float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);

/* x[n] (fp32, 16-byte aligned) *= *scale (device scalar), in place; an empty launch when the scalar is exactly 1.  The chain rule of a
 * loss whose gradient buffers were filled in its forward pass: autograd hands `loss.backward()` an upstream gradient of one, and the
 * 3 x 91 MB multiply that `grad * gout` would be is what the backward pass starts with (loss/yolov3_loss.py:29-72 via autograd). */
int fva_scale_by_device_scalar(float* x, int64_t n, const float* scale, void* stream);

/* Stand-alone BiCrossEntropyLoss (loss/classification_loss.py:36-65) forward + dl/dy.  y [numel] fp32 logits (or probabilities:
 * already_sigmoid) seen as rows of C classes; target = one-hot of label[numel / C] (int64) or, label == NULL, the dense float
 * target [numel]; weights: NULL, one value, or numel values.  loss_out[1] = sum of the weighted element losses (/ numel when
 * mean); grad (optional, [numel]) = d(sum of weighted element losses)/dy, NOT divided by numel.  workspace: 1024 floats.
 * Deterministic (fixed-order partial sums). */
int fva_bce_loss(const float* y, const int64_t* label, const float* dense_target, const float* weights, int64_t weights_numel,
                 int64_t numel, int32_t C, int32_t already_sigmoid, int32_t mean, float* loss_out, float* grad, float* workspace,
                 void* stream);

/* Losses of the two-stage head (demos/faster_rcnn/models/rpn.py:8-64,303-312; fast.py:173-201), value + gradient in one launch.
 * fva_row_loss: logits [R][C] fp32 with int64 labels[R]; mode 0 = F.cross_entropy(reduction='mean'), mode 1 = the RPN's FocalLoss
 * (-(1 - p_t)^gamma * log p_t over softmax probabilities, alpha 1, mean); grad (optional) [R][C] = d loss / d logits;
 * workspace: R floats.  fva_smooth_l1: F.smooth_l1_loss(pred, target, reduction='mean') (beta 1) over n elements; grad (optional)
 * [n] = d loss / d pred; workspace: 1024 floats.  Deterministic (fixed-order sums). */
int fva_row_loss(const float* logits, const int64_t* labels, int32_t R, int32_t C, int32_t mode, float gamma, float* loss_out, float* grad,
                 float* workspace, void* stream);
int fva_smooth_l1(const float* pred, const float* target, int64_t n, float* loss_out, float* grad, float* workspace, void* stream);

/* The two demo losses are one pipeline with two box terms: best-anchor assignment, class BCE-with-logits (mean over T * C), IoU>0.5
 * ignore mask and masked objectness BCE are shared.  Both check their arguments, every level and the workspace size before the first
 * device call; T >= 1.  level.anchor_* are FEATURE-scale here and level.stride is unused.
 *
 * fva_demo_loss (demos/yolov3_u/utils/lossv3.py:18-119): box term BCE(xy) + MSE(wh).
 * loss_out[5] = {total, xy, wh, cls, conf} (unweighted parts, as the reference prints them; total = 2 xy + wh + cls + conf). */
int fva_demo_loss(const float* targets, int32_t T, const fva_head_level* levels, int32_t nlevels, float* loss_out,
                  void* workspace, int64_t workspace_bytes, void* stream);
int64_t fva_demo_loss_workspace(int32_t T, const fva_head_level* levels, int32_t nlevels);

/* fva_demo_ciou_loss (demos/yolov3_huaweiShip/utils/lossv3.py:35-120): the same pipeline with the box term
 * mean over T of 1 - CIoU(pred, target; 'xywh', eps 1e-7), pred = (sigmoid(z_xy) + cell, exp(z_wh) * anchor), with the
 * demo's CIoU (fva_iou_pairwise kind 3, variant 1).  Arguments and argument rules as fva_demo_loss; the workspace size is the same.
 * loss_out[4] = {box + cls + conf, box, cls, conf}; level.grad receives d (box + cls + conf) / d head: the box part in
 * channels 0..3 of the matched (cell, anchor), the objectness part in channel 4, the class part in channels 5.. */
int fva_demo_ciou_loss(const float* targets, int32_t T, const fva_head_level* levels, int32_t nlevels, float* loss_out,
                       void* workspace, int64_t workspace_bytes, void* stream);
int64_t fva_demo_ciou_loss_workspace(int32_t T, const fva_head_level* levels, int32_t nlevels);

/* level->grad[b, a, y, x, k] *= (k < 4 ? *g_box : k == 4 ? *g_conf : *g_cls), in place through the level's strides; the three scalars
 * are device memory and are not read on the host.  The chain rule of fva_demo_ciou_loss, whose three parts are separately
 * differentiable but write disjoint channel groups of ONE stored gradient.  No memory traffic when all three are exactly 1. */
int fva_scale_head_groups(const fva_head_level* level, const float* g_box, const float* g_cls, const float* g_conf, void* stream);

/* IoU family on device (detection/tools/IOU.py, BOX.py).  kind: 0 IoU 1 GIoU 2 DIoU 3 CIoU;
 * mode: 0 xyxy 1 xywh 2 wh; variant: 0 library 1 demo (iou.py centre sums / minus sign).
 * pairwise: out[N] and (optional) grad_a[N][4 or 2] = d out / d a in the caller's box parametrisation (ties
 * split as torch.maximum/minimum do, CIoU alpha constant); batch: out[N][M]. */
int fva_iou_pairwise(int kind, int mode, int variant, const float* a, const float* b, float* out, float* grad_a, int64_t N,
                     float eps, void* stream);
int fva_iou_batch(int kind, int mode, int variant, const float* a, const float* b, float* out, int64_t N, int64_t M, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Validation side (scope row f-2): eval decode, candidate selection, non-maximum suppression.
 * ---------------------------------------------------------------------------------------------- */
/* Un-letterbox mapping of the demo's postProcess (demos/yolov3_u/inference.py:90-106). */
typedef struct {
    float resize_ratio, pad_left, pad_top; /* x_ori = (x - pad_left) / resize_ratio */
    float ori_w, ori_h;                    /* clamp bounds of the original image */
    float min_wh;                          /* boxes with w <= min_wh or h <= min_wh are dropped (5 in the reference) */
} fva_letterbox;
/* Decode the head tensors of all levels into out [B][rows_per_image][K] fp32 (level after level).
 * variant 0 -- Yolov3.forward eval branch (detection/models/yolov3.py:35-53): rows of a level ordered (a, y, x);
 *   xy = (sigmoid(t) + cell) * stride, wh = exp(t) * anchor (PIXEL anchors), everything else sigmoid.
 * variant 1 -- postProcess (demos/yolov3_u/inference.py:58-88): rows ordered (y, x, a);
 *   xy = (2 sigmoid(t) - 0.5 + cell) * stride, wh = (2 sigmoid(t))^2 * anchor * stride (FEATURE anchors).
 *   With lb != NULL rows additionally go through :90-106: un-letterbox, clamp, xywh -> clamped xyxy in columns 0..3;
 *   rows the reference drops (w or h <= min_wh) keep their place with objectness -1.
 * variant 2 -- postProcess of the second demo (demos/yolov3_huaweiShip/inference.py:107-136): rows ordered (y, x, a);
 *   xy = (sigmoid(t) + cell) * stride, wh = exp(t) * anchor * stride (FEATURE anchors); lb != NULL as for variant 1. */
int fva_yolo_decode(const fva_head_level* levels, int32_t nlevels, int32_t variant, const fva_letterbox* lb,
                    float* out, int64_t rows_per_image, void* stream);

typedef struct {
    int32_t box_mode;    /* 0: rows carry xywh (converted with x -/+ w/2), 1: rows carry xyxy */
    int32_t score_mode;  /* 0: score = max_c(cls_c * obj) (NMS.py:13-16, nms.py:76-82); 1: score = obj (nms.py:24-36) */
    int32_t rethreshold; /* 1: also drop candidates with max_c(cls_c * obj) <= conf_thres (nms.py:84) */
    int32_t max_det;     /* detections kept per image */
    int32_t max_nms;     /* > 0: only the max_nms best candidates enter NMS (nms.py:40-42: 30000) */
    float conf_thres, iou_thres;
    float class_gap;     /* 0: class-agnostic (NMS.py); 4096: boxes shifted by category * gap (nms.py:45-46) */
} fva_nms_params;
/* Stage 1: rows with objectness > conf_thres become candidates, in row order (what boolean-mask indexing gives).
 * pred [B][R][K] fp32; counts [B] i32; cand: opaque buffer of fva_nms_candidates_workspace(B, R) bytes. */
int64_t fva_nms_candidates_workspace(int32_t B, int32_t R);
int fva_nms_candidates(const float* pred, int32_t B, int32_t R, int32_t K, const fva_nms_params* p, void* cand,
                       int64_t cand_bytes, int32_t* counts, void* stream);
/* Stage 2: torchvision.ops.nms on every image's candidates (greedy, highest score first, suppress when
 * inter / (area_a + area_b - inter) > iou_thres; score ties broken by candidate order).  nmax >= max(counts)
 * (the caller reads counts back: the reference's boolean indexing synchronises at the same point).
 * out [B][max_det][6] = x1, y1, x2, y2, score, category; out_rows [B][max_det] = source row in pred;
 * keep_counts [B]. */
int64_t fva_nms_select_workspace(int32_t B, int32_t nmax);
int fva_nms_select(const void* cand, const int32_t* counts, int32_t B, int32_t R, int32_t nmax, const fva_nms_params* p,
                   void* workspace, int64_t workspace_bytes, float* out, int32_t* out_rows, int32_t* keep_counts,
                   void* stream);

/* Validation mAP, the matching of metrics/map.py:17-83 for a whole batch in one launch and without a host read-back.
 * det [B][max_det][6] = x1, y1, x2, y2, score, category and kept [B] (DEVICE int32) are fva_nms_select's out and keep_counts;
 * targets [T][6] = image index, category, x1, y1, x2, y2 in pixels, in any order (rows whose image index is not one of 0..B-1 are
 * ignored; T may be 0); thr [n_thr] is a HOST array of IoU thresholds, 1 <= n_thr <= 16, read before the call returns.
 *   1. a prediction picks, among the targets of its image with an equal category (compared as floats) and IoU > (float)thr[0],
 *      the one with the highest IoU -- the lowest target row when two are equal;
 *   2. a target goes to the lowest-indexed prediction that picked it; every other prediction gets nothing;
 *   3. bit k of flags [B][max_det] (uint16) is (double)IoU > thr[k] for a winner and 0 otherwise.
 * The IoU has the bits of fva_iou_batch (kind 0, mode 0, eps) with the target as the first box.  Rows at or beyond kept[b] are
 * never read and their flags are 0.  workspace: T int32, no initial value needed (may be NULL when T is 0). */
int fva_map_match(const float* det, const int32_t* kept, int32_t B, int32_t max_det, const float* targets, int32_t T,
                  const double* thr, int32_t n_thr, float eps, int32_t* workspace, uint16_t* flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Input side (scope row f-3): decoded uint8 RGB (HWC) images -> the [B][3][H][W] fp32 input batch in one launch.
 * A "paste job" resizes one source image with OpenCV's 8-bit INTER_LINEAR arithmetic (an exact 2x decimation is
 * area-averaged, as cv2.resize does) to dst_w x dst_h, optionally mirrors it, and places it at (left, top) of canvas
 * `b`; pixels no job covers take `fill`.  Every byte then goes through lut[channel][value] (the caller tabulates
 * x/255 or (x/255 - mean)/std exactly as the reference computes it).  Replaces cv2.resize + Padding + np.fliplr/flipud
 * + Normalization + transpose + stack (datasets/detection_dataloader.py:44-103, datasets/common/padding.py,
 * datasets/common/augmentation.py:298-376) and ResizeByMax/Padding/flips/Mosaic01 (demos/yolov3_u/data_gen.py).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t src_offset;      /* byte offset of this image's [src_h][src_w][3] pixels in `src` */
    int32_t src_h, src_w;
    int32_t dst_h, dst_w;    /* size after the resize */
    int32_t top, left;       /* where the resized image lands on its canvas */
    int32_t flip_h, flip_v;  /* mirror the resized image (cv2.flip 1 / 0) */
    int32_t src_pitch;       /* bytes between source rows; 0 = src_w * 3 (a sub-image of a wider canvas otherwise) */
    int32_t reserved;
    double scale_x, scale_y; /* 1.0 / ((double)dst / src), as cv2.resize derives them */
} fva_paste_job;
/* jobs: DEVICE array; job_start: DEVICE int32[B+1], canvas b owns jobs job_start[b] .. job_start[b+1]-1, pasted in
 * that order (later jobs overwrite earlier ones); lut: DEVICE float[3][256]; out: [B][3][H][W] fp32. */
int fva_paste_resize_normalize(const uint8_t* src, const fva_paste_job* jobs, const int32_t* job_start, int32_t B,
                               int32_t H, int32_t W, int32_t fill, const float* lut, float* out, void* stream);
/* The same placement without the value table: out [B][H][W][3] uint8 (an intermediate image that a later call resizes
 * again -- the demo resizes every image to input_size before Mosaic01 resizes it to input_size/2). */
int fva_paste_resize_u8(const uint8_t* src, const fva_paste_job* jobs, const int32_t* job_start, int32_t B, int32_t H,
                        int32_t W, int32_t fill, uint8_t* out, void* stream);

/* Colour / blur extras of the demo's training image path (demos/yolov3_u/data_gen.py:26-33,120-146), on uint8 canvases
 * [B][H][W][3] resident in device memory (the output of fva_paste_resize_u8).  One job per canvas image. */
typedef struct {
    int32_t h, w;        /* valid region of the canvas image, anchored at its top-left corner */
    int32_t clahe;       /* 1: HistEqualize -- CLAHE (clip limit 2.0, 8 x 8 tiles) on the luma of OpenCV's 8-bit YUV */
    int32_t hsv;         /* 1: HueSaturationValue -- the image's three 256-byte tables applied in OpenCV's 8-bit HSV (H < 180) */
    int32_t blur;        /* fva_colour_blur_shuffle_normalize: 0 none, 1 cv2.blur 3x3, 2 cv2.medianBlur 3, 3 cv2.GaussianBlur 3x3 sigma 0 */
    int32_t perm[3];     /* fva_colour_blur_shuffle_normalize: output channel c is input channel perm[c] (ChannelShuffle) */
} fva_colour_job;
/* In place on the valid region of every canvas: [CLAHE] then [HSV tables].  jobs: DEVICE array [B]; hsv_luts: DEVICE bytes
 * [B][3][256] (hue, saturation, value tables; read only for jobs with hsv = 1); max_h / max_w: largest valid region;
 * workspace: fva_colour_workspace(B) bytes (the 64 tile tables of every image). */
int64_t fva_colour_workspace(int32_t B);
int fva_colour_clahe_hsv(uint8_t* canvases, int32_t B, int32_t H, int32_t W, const fva_colour_job* jobs, int32_t max_h, int32_t max_w,
                         const uint8_t* hsv_luts, uint8_t* workspace, void* stream);
/* canvases [B][H][W][3] uint8 -> out [B][3][H][W] fp32: per image a 3x3 blur (or none) over the whole canvas, the channel
 * permutation, then lut[channel][value] (x / 255 as the reference computes it: ToTensorV2 + `/ 255.`). */
int fva_colour_blur_shuffle_normalize(const uint8_t* canvases, int32_t B, int32_t H, int32_t W, const fva_colour_job* jobs,
                                      const float* lut, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer: torch.optim.Adam semantics (demos/yolov3_u/train.py:68), multi-tensor.
 * ptrs: device array [4][n] of {param, grad, exp_avg, exp_avg_sq} fp32 pointers; sizes: device int64[n].
 * step is the 1-based step count; lr/betas/eps/weight_decay as torch (L2-in-gradient decay).
 * ---------------------------------------------------------------------------------------------- */
int fva_adam_step(const void* const* ptrs, const int64_t* sizes, int32_t n, int64_t max_size, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* stream);
/* The same update with the step count and the learning rate in device memory, for a training step captured in a HIP graph
 * (utils/fit.py:52-66 replayed as one launch): state_dev[3] doubles = {step count, lr / (1 - beta1^step), sqrt(1 - beta2^step)};
 * the call first advances state_dev[0] by one and recomputes the two bias-corrected factors from *lr_dev (a device float the
 * host may rewrite between replays: LR schedules), then updates the tensors.  Same arithmetic as fva_adam_step. */
int fva_adam_step_dev(const void* const* ptrs, const int64_t* sizes, int32_t n, int64_t max_size, const float* lr_dev, float beta1,
                      float beta2, float eps, float weight_decay, double* state_dev, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer: torch.optim.SGD semantics (demos/faster_rcnn/train.py:91-109: momentum 0.937, Nesterov, parameter groups) with the
 * demo's global gradient-norm clipping (demos/faster_rcnn/cfg/_fit.py:6-17) on the device; multi-tensor, every group in one launch.
 * The work is split into chunks of fva_sgd_chunk_elems() elements, one block each:
 *   tab_dev: int64 [6][n] in device memory = param | grad | momentum buffer (0: none, plain SGD) fp32 pointers | element count |
 *            parameter-group index (row of hyper_dev) | slot in fresh_dev;
 *   chunks_dev: int64 [nchunks] = (tensor index << 32) | chunk number within the tensor (built once by the host);
 *   hyper_dev: float [groups][5] = lr, weight_decay, momentum, 1 - dampening, nesterov (0 or 1), read at run time (a captured HIP
 *            graph follows later host rewrites of the table: LR schedules);
 *   fresh_dev: int32 per slot, non-zero while a momentum buffer has no history (the update sets buf = g, torch's clone).
 * Pointers may be any 4-byte aligned address (16-byte vector path where a tensor's pointers allow it). */
int fva_sgd_chunk_elems(void);
/* partial_dev: double [nchunks] scratch; out_dev[0] = fp32 global L2 norm of every grad in the table, out_dev[1] = the reference's
 * coefficient clip_norm / max(norm, clip_norm) computed in double as Python does, rounded to fp32 (Python max: a NaN norm gives NaN, an infinite one 0).  Fixed summation order (fp64
 * per chunk, chunk order across chunks): bit-identical from run to run.  No host synchronisation. */
int fva_sgd_clip_coef(const int64_t* tab_dev, int32_t n, const int64_t* chunks_dev, int32_t nchunks, double* partial_dev,
                      double clip_norm, float* out_dev, void* stream);
/* p -= lr * step(coef * grad) in torch's order (weight decay into the gradient, momentum buffer, Nesterov); coef_dev: device
 * scalar (out_dev + 1 of fva_sgd_clip_coef) or NULL for 1.  The gradients themselves are not rewritten.  clear_fresh != 0: after
 * the update, zero the fresh flags of the table's slots (their buffers now have history). */
int fva_sgd_step(const int64_t* tab_dev, int32_t n, const int64_t* chunks_dev, int32_t nchunks, const float* hyper_dev,
                 int32_t* fresh_dev, int32_t clear_fresh, const float* coef_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exponential moving average of the weights (fastvision_amd.ModelEMA: the averaged model a YOLO trainer validates and checkpoints),
 * multi-tensor, counter and weight on the device (a captured training step replays it).  One call = one update:
 *   a one-thread tick computes, in double, k = state_dev[0] + 1, state_dev[0] = k, d = decay * (1 - exp(-k / tau)) (d = decay when
 *   tau == 0), state_dev[1] = w = 1 - d;  then one block per chunk applies  e = fmaf((float)w, p - e, e)  to the fp32 tensors (one fp32
 *   subtraction, one fused multiply-add) and copies the other tensors byte for byte.
 *   tab_dev: int64 [4][n] in device memory = EMA tensor pointer | model tensor pointer | count | kind; kind 0 = fp32 lerp, count in
 *            elements, any 4-byte aligned pointers (16-byte vector path where both pointers allow it); kind 1 = raw copy model ->
 *            EMA, count in bytes, any pointers (integer, bool and non-fp32 float buffers such as num_batches_tracked);
 *   chunks_dev: int64 [nchunks] = (tensor << 32) | chunk number, a chunk being fva_ema_chunk_elems() fp32 elements (kind 0) or four
 *            times as many bytes (kind 1);
 *   state_dev: double [2] = {updates done, weight of the current update}.
 * decay must lie in [0, 1), tau must be >= 0.  No atomics, no host synchronisation, nothing read back. */
int fva_ema_chunk_elems(void);
int fva_ema_update(const int64_t* tab_dev, int32_t n, const int64_t* chunks_dev, int32_t nchunks, double decay, double tau,
                   double* state_dev, void* stream);

/* Gradient bucket fill for the data-parallel all-reduce (parallel.GradientReducer; the reference's nn.DataParallel gathers
 * gradients tensor by tensor, demos/yolov3_u/train.py:85): dst[offs[t] + i] = src_t[i], converted to dst_dtype (FVA_F32 or
 * FVA_BF16), for n fp32 source tensors in one launch.  table_dev: 3n int64 in device memory = source pointers | element counts |
 * element offsets into dst; a null pointer or zero count skips the tensor.  max_size sizes the grid. */
int fva_gather_cast(const int64_t* table_dev, int32_t n, int64_t max_size, void* dst, int dst_dtype, void* stream);

/* ---- VGG blocks of the two-stage head's backbone (demos/faster_rcnn/models/vgg.py: Conv2d + bias -> ReLU,
 * MaxPool2d(2, 2); no BatchNorm) ---------------------------------------------------------------------------------------------
 * fva_conv_fwd_bias_act: z = act(conv(x) + bias[n]) straight into the halo buffer z (border zeroed), act 1 = ReLU, 2 = none;
 *   its backward uses fva_conv_dgrad / fva_conv_wgrad on dY from
 * fva_bias_relu_bwd: dY = dZ * (Z > 0) (dZ dense NHWC, Z the forward's halo output) into the halo buffer dY, and partial
 *   [fva_bias_relu_bwd_rows()][C] column sums of dY that fva_colsum adds up in fixed order (= dbias; scratch may be NULL).
 * fva_maxpool2_fwd: 2x2 / stride 2 max of the halo tensor x [B][H+2p][W+2p][C] into the halo tensor out [B][H/2+2q][W/2+2q][C]
 *   (floor mode; border zeroed).  fva_maxpool2_bwd: dz dense [B][H/2][W/2][C] -> dx dense [B][H][W][C]; the gradient goes to the
 *   first maximum of each window in scan order. */
int fva_conv_fwd_bias_act(const fva_conv_desc* d, const void* x, const void* w_fwd, const float* bias, int32_t act, void* z, int32_t z_pad,
                          void* stream);
int32_t fva_bias_relu_bwd_rows(int B, int H, int dy_pad);
int fva_bias_relu_bwd(int dtype, const void* dz, const void* z, int z_pad, void* dy, int dy_pad, float* partial, int B, int H, int W, int C,
                      void* stream);
int32_t fva_colsum_scratch_rows(int32_t rows);   /* rows of [C] floats fva_colsum wants as scratch for its two-pass form (0: none) */
int fva_colsum(const float* partial, int32_t rows, int C, float* out, float* scratch, void* stream);
/* Fully connected layers of the Fast head (Linear -> ReLU, demos/faster_rcnn/models/vgg.py classifier): dY = dZ * (Z > 0)
 * (relu = 0: dY = dZ) over rows [R][C] (dY rows dy_stride elements apart: the interior column of a halo buffer [1][R+2][3][C], which
 * is what fva_conv_wgrad / fva_conv_dgrad read) and per block of 32 rows the column sums of dY: partial [fva_rows_relu_bwd_rows(R)][C],
 * added up by fva_colsum (= dbias).  The GEMMs themselves are 1x1 convolutions over R "pixels" (fva_conv_fwd_bias_act, fva_conv_dgrad,
 * fva_conv_wgrad). */
int32_t fva_rows_relu_bwd_rows(int32_t R);
int fva_rows_relu_bwd(int dtype, const void* dz, const void* z, void* dy, int64_t dy_stride, float* partial, int32_t R, int32_t C, int32_t relu,
                      void* stream);
int fva_maxpool2_fwd(int dtype, const void* x, int x_pad, void* out, int out_pad, int B, int H, int W, int C, void* stream);
int fva_maxpool2_bwd(int dtype, const void* dz, const void* x, int x_pad, void* dx, int B, int H, int W, int C, void* stream);

/* ---- RPN proposal rows (two-stage head) ------------------------------------------------------------------------
 * filter_proposals of demos/faster_rcnn/models/rpn.py:162-186 up to the per-image selection: cls [B][H][W][A][2] logits,
 * deltas [B][H][W][A][4], anchors_wh [A][2] (already divided by the backbone stride; anchor centres are the cell indices) ->
 * out [B][H*W*A][6] = clamped x1, y1, x2, y2, softmax foreground score, 1.0: the rows fva_nms_candidates / fva_nms_select
 * take (box_mode 1, score_mode 1, max_nms = rpn_pre_nms_top_n, max_det = rpn_post_nms_top_n). */
int fva_rpn_decode(const float* cls, const float* deltas, const float* anchors_wh, float* out, int32_t B, int32_t H, int32_t W,
                   int32_t A, void* stream);

/* Second-stage head outputs of a whole batch -> the rows fva_nms_candidates takes (box_mode 1, score_mode 1), in ONE launch:
 * Fast.forward's eval branch and postProcess up to the NMS call (demos/faster_rcnn/models/fast.py:93-101,265-286,
 * demos/faster_rcnn/inference.py:87-118).  cls [K][C+1] logits (column 0 = background); box [K][4], or [K][(C+1)*4] with
 * multi_reg = 1 (the four of the row's first-maximum LOGIT are used); proposals [K][4] xywh in feature cells, image after image;
 * row_start [B+1] i32 on the device: image b owns rows row_start[b] .. row_start[b+1]-1, at most R of them (the caller's promise;
 * rows past R are not decoded, and a range that leaves [0, K) reads nothing).  pred [B][R][5+C] fp32, every element written:
 *   d = box * (0.1, 0.1, 0.2, 0.2); x = d0*pw + px, y = d1*ph + py, w = exp(d2)*pw, h = exp(d2)*ph (d2 twice, as the reference);
 *   score / category = value / first index of the maximum softmax probability; xywh * stride; then with lb == NULL the clamps
 *   of postProcess with ratio 1, pads 0 and bounds in_w / in_h (the input-pixel frame), with lb [B] (device) image b's
 *   (x - pad_left) / resize_ratio etc. against ori_w / ori_h (lb[b].min_wh is not read: min_wh is the argument);
 *   row = clamped x1, y1, x2, y2, score, then 1.0 in column 5 + category - 1 and 0 elsewhere.
 * A row is DROPPED -- written as 0, 0, 0, 0, -1, 0, ... so that no threshold passes it -- when it lies at or past its image's
 * count, when its category is background (a tie with background included), or when !(w > min_wh && h > min_wh).
 * K = 0 is allowed (cls, box, proposals may be NULL): every row is dropped. */
int fva_fast_decode(const float* cls, const float* box, const float* proposals, const int32_t* row_start, int32_t K, int32_t B,
                    int32_t R, int32_t C, int32_t multi_reg, float stride, float in_w, float in_h, float min_wh,
                    const fva_letterbox* lb, float* pred, void* stream);

/* RPN anchor / ground-truth matcher: the labelling inside RPN.computet_loss (demos/faster_rcnn/models/rpn.py:209-277).
 * anchors_xywh [Na][4] in feature cells (make_anchors_xywh, flattened (y, x, a)); targets [T][6] = image index, class, normalised
 * xywh (scaled by the map size here, rpn.py:257).  labels [B][Na] i32: >= 0 index of the matched box WITHIN its image's boxes,
 * -1 negative (best IoU < neg_thr), -2 ignored; every box then claims its best anchor, later boxes overriding earlier ones.
 * An image without boxes gets -2 everywhere.  workspace: T int32 (best anchor per box row). */
int fva_rpn_match(const float* anchors_xywh, int32_t Na, const float* targets, int32_t T, int32_t B, int32_t feature_h,
                  int32_t feature_w, float pos_thr, float neg_thr, int32_t* labels, int32_t* workspace, void* stream);

/* Fast head: proposal / ground-truth labelling of select_positive_negative_samples (demos/faster_rcnn/models/fast.py:100-127)
 * for ONE image: proposals_xywh [N][4]; targets [T][6] as above but with xywh already in feature cells (fast.py:217), only the
 * rows of `image` count.  labels [N] i32: >= 0 matched box (best IoU >= pos_thr), -1 negative (neg_floor <= best IoU <
 * neg_thr; the reference's floor is 0.1), -2 ignored. */
int fva_fast_match(const float* proposals_xywh, int32_t N, const float* targets, int32_t T, int32_t image, float pos_thr,
                   float neg_thr, float neg_floor, int32_t* labels, void* stream);

/* ---- RoIAlign (two-stage head) -----------------------------------------------------------------------------
 * torchvision.ops.roi_align as the reference calls it (demos/faster_rcnn/models/fast.py:227-231,258): rois [K][5] = (batch
 * index, x1, y1, x2, y2), out [K][C][PH][PW] fp32 (the order torch.flatten(.., 1) feeds the classifier), aligned = False,
 * sampling_ratio <= 0 = adaptive grid.  feat: halo NHWC [B][H+2*feat_pad][W+2*feat_pad][C] of dtype.  Backward: grad_out in
 * the same [K][C][PH][PW] layout is scattered (float atomics) into dfeat, dense fp32 NHWC [B][H][W][C], which the caller
 * zeroes first.  K = 0 is a no-op.  A box whose batch index is not in [0, B) -- NaN included -- pools nothing: its out rows are
 * written as zeros, and it adds nothing to dfeat. */
int fva_roi_align_fwd(int dtype, const void* feat, int feat_pad, const float* rois, int K, float* out, int B, int H, int W, int C,
                      int PH, int PW, float spatial_scale, int sampling_ratio, void* stream);
int fva_roi_align_bwd(const float* grad_out, const float* rois, int K, float* dfeat, int B, int H, int W, int C, int PH, int PW,
                      float spatial_scale, int sampling_ratio, void* stream);

/* ---- Classification top of Darknet-53 (classfication/models/darknet53.py:65-137 with including_top; loss/classification_loss.py:8-33;
 * metrics/accuracy.py) ----------------------------------------------------------------------------------------------------------
 * fva_gap_fwd: nn.AdaptiveAvgPool2d((1, 1)) + flatten.  x: NHWC [B][H+2*x_pad][W+2*x_pad][C] of dtype (x_pad 1: a halo buffer, 0:
 * dense); out fp32 [B][C] = the mean over the H*W pixels, summed in fp32 in a fixed order (no atomics: run-to-run bit-identical).
 * fva_gap_bwd: dx (dtype, dense NHWC [B][H][W][C]) = g[b][c] / (H*W), g fp32 [B][C].
 * fva_softmax_ce: CrossEntropyLoss, -sum(onehot(label) * log_softmax(z), 1) * w, over logits fp32 [R][C]; labels [R] int64
 * (FVA_LABEL_I64) or fp32 holding integer values (FVA_LABEL_F32); weights fp32 [R] or NULL (= 1).  loss_out[0] = the row losses
 * summed in double in a fixed order, divided by R for FVA_REDUCE_MEAN (not by the sum of the weights) or not for FVA_REDUCE_SUM;
 * grad (optional, [R][C]) = w_r * (softmax(z_r) - onehot) (times 1/R for the mean).  workspace: fva_softmax_ce_workspace(R) bytes.
 * A label that is < 0, >= C or (fp32) not an integer cannot raise on the device: that row's loss and gradient are NaN, so loss_out
 * is NaN, and no memory is indexed with it; the other rows' gradients are unaffected.
 * fva_top1_accuracy: out[0] = (number of rows whose argmax equals the label) / R, fp32.  logits [R][C] of logits_dtype (FVA_F32 /
 * FVA_BF16); argmax as torch.argmax (first index among equal maxima; a NaN is the maximum, the first NaN wins); an out-of-range
 * label simply never matches.  workspace: R int32.  Deterministic. */
typedef enum { FVA_LABEL_I64 = 0, FVA_LABEL_F32 = 1 } fva_label_dtype;
typedef enum { FVA_REDUCE_MEAN = 0, FVA_REDUCE_SUM = 1 } fva_reduction;
int fva_gap_fwd(int dtype, const void* x, int x_pad, int B, int H, int W, int C, float* out, void* stream);
int fva_gap_bwd(int dtype, const float* g, int B, int H, int W, int C, void* dx, void* stream);
int64_t fva_softmax_ce_workspace(int32_t R);
int fva_softmax_ce(const float* logits, const void* labels, int label_dtype, const float* weights, int32_t R, int32_t C, int32_t reduction,
                   float* loss_out, float* grad, void* workspace, void* stream);
int fva_top1_accuracy(const void* logits, int logits_dtype, const void* labels, int label_dtype, int32_t R, int32_t C, float* out,
                      void* workspace, void* stream);

/* ---- VGG classifiers (classfication/models/vgg.py:24-48: Conv2d(bias) -> BatchNorm2d -> ReLU blocks, AdaptiveAvgPool2d((7, 7)) + flatten,
 * Dropout) -----------------------------------------------------------------------------------------------------------------------
 * BatchNorm + ReLU, the three streaming passes of the SiLU path with the activation exchanged (table form: the statistics come from
 * fva_conv_fwd + fva_bn_finalize, the backward sums go through fva_bn_bwd_finalize; C / (16-byte chunk) a power of two <= 256):
 *   fva_bn_relu_apply       z = max(0, y * scale + shift) from the dense convolution output y [B*H*W][C] into the halo buffer
 *                           z [B][H+2p][W+2p][C], zero border included (p = z_pad, 0 or 1).  A NaN stays a NaN.
 *   fva_bn_relu_bwd_reduce  partial [fva_bn_bwd_blocks()][2][C] = per-block sums of dU = dz * (u > 0) and dU * xhat, u = y * scale +
 *                           shift recomputed from y (never from the rounded z), xhat = (y - mean) * rstd.  Fixed order, no atomics.
 *   fva_bn_relu_bwd_apply   dy = a * dU + k1 * y + k2 (= gamma * rstd * (dU - dbeta / n - xhat * dgamma / n); coef = the [3][C] table of
 *                           fva_bn_bwd_finalize) as a halo buffer with zero border: the operand of fva_conv_dgrad / fva_conv_wgrad.
 * The convolution bias in front of BatchNorm cancels in z in training mode, so the convolution runs without it; it stays visible in two
 * places: running_mean tracks mean(y) + b (fva_bn_bias_running_mean: running_mean += momentum * b, after fva_bn_finalize) and in eval mode
 * it folds into the shift (fva_bn_eval_coeffs_bias: scale = gamma / sqrt(running_var + eps), shift = beta + (b - running_mean) * scale). */
int fva_bn_relu_apply(int dtype, const void* y, const float* scale, const float* shift, void* z, int z_pad, int B, int H, int W, int C,
                      void* stream);
int fva_bn_relu_bwd_reduce(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                           const float* save_rstd, float* partial, int32_t nblocks, int64_t M, int C, void* stream);
int fva_bn_relu_bwd_apply(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                          const float* save_rstd, const float* coef, void* dy, int dy_pad, int B, int H, int W, int C, void* stream);
int fva_bn_bias_running_mean(int32_t C, float* running_mean, const float* bias, float momentum, void* stream);
int fva_bn_eval_coeffs_bias(int32_t C, const float* gamma, const float* beta, const float* rm, const float* rv, const float* bias, float eps,
                            float* scale, float* shift, void* stream);

/* ---- BatchNorm backward with FROZEN statistics (the module in eval mode, its convolution and affine parameters training; version 7) ----
 * scale / shift (fva_bn_eval_coeffs[_bias]) do not depend on the batch, so the two passes above collapse into one over dz and y (dense
 * NHWC [B*H*W][C]):
 *   dy = scale * dU,  dU = dz * act'(y * scale + shift)     halo buffer [B][H+2p][W+2p][C] with its zero border, p = dy_pad (0 or 1)
 *   partial != NULL: one row [2][C] per block of the launch (fva_bn_frozen_bwd_blocks() rows; fixed order, no atomics) holding
 *   s1 = sum dU and s2 = sum dU * (y - m) * r, with m, r from fva_bn_frozen_stats: m = running_mean (- bias), r = 1 / sqrt(running_var + eps).
 *   partial == NULL (neither gamma nor beta asks for a gradient): only dy is written; m and r are not read.
 * C / (16-byte chunk) a power of two <= 256.  fva_bn_frozen_bwd_finalize folds the table (allocated with
 * fva_bn_partial_rows(nblocks) rows) into dbeta = s1, dgamma = s2 and dbias = scale * s1 (the gradient of a convolution bias in front
 * of the BatchNorm); each of the three may be NULL. */
int32_t fva_bn_frozen_bwd_blocks(int dtype, int B, int H, int W, int C, int dy_pad);
int fva_bn_silu_frozen_bwd(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* m, const float* r,
                           float* partial, void* dy, int dy_pad, int B, int H, int W, int C, void* stream);
int fva_bn_relu_frozen_bwd(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* m, const float* r,
                           float* partial, void* dy, int dy_pad, int B, int H, int W, int C, void* stream);
int fva_bn_frozen_bwd_finalize(float* partial, int32_t nblocks, int32_t partial_rows, int C, const float* scale, float* dgamma, float* dbeta,
                               float* dbias, void* stream);
int fva_bn_frozen_stats(int32_t C, const float* rm, const float* rv, const float* bias, float eps, float* m, float* r, void* stream);
/* nn.AdaptiveAvgPool2d((7, 7)) + torch.flatten(x, 1).  x: NHWC [B][H+2*x_pad][W+2*x_pad][C] of dtype; out [B][C*49] of dtype in the
 * order c * 49 + i * 7 + j; windows floor(i*H/7) .. ceil((i+1)*H/7) as torch defines them, any H, W >= 1; C a multiple of the 16-byte
 * chunk.  Backward (gather form, no atomics): g [B][C*49] of dtype -> dx dense NHWC [B][H][W][C] of dtype.  One launch each;
 * run-to-run bit-identical. */
int fva_adaptive_avgpool7_fwd(int dtype, const void* x, int x_pad, int B, int H, int W, int C, void* out, void* stream);
int fva_adaptive_avgpool7_bwd(int dtype, const void* g, int B, int H, int W, int C, void* dx, void* stream);
/* nn.Dropout over n contiguous elements of dtype (n a multiple of the 16-byte chunk): out = x * keep / (1 - p), 0 < p < 1 (p = 0 and eval
 * mode are the identity: the caller launches nothing).  keep comes from Philox-4x32-10 keyed by (seed, call counter, element index);
 * state = int64[4] in DEVICE memory: {seed, call counter, 0, 0}.  The launch reads seed and counter and advances the counter itself
 * (word 2 is its block count, zero between launches), so a captured graph draws a new mask on every replay without the host.
 * All launches that share one state must be on ONE stream (or ordered by events): a launch reads the counter its predecessor wrote.
 * No mask is stored: fva_dropout_bwd gives dx = dout / (1 - p) where out != 0, else 0 (exact behind a ReLU). */
int fva_dropout_fwd(int dtype, const void* x, void* out, int64_t n, float p, int64_t* state, void* stream);
int fva_dropout_bwd(int dtype, const void* dout, const void* out, void* dx, int64_t n, float p, void* stream);

/* ---- ResNet classifiers (classfication/models/resnet.py; version 9) ---------------------------------------------------------------
 * Streaming passes around the existing convolutions; dtype FVA_F32 / FVA_BF16, C a multiple of the 16-byte chunk (4 / 8 elements) up to
 * 2048, borders 0 or 1, fixed summation order, no float atomics (run-to-run bit-identical).
 *
 * fva_stem7_patches: the 7x7 / stride 2 / pad 3 stem (resnet.py:136-140).  x: fp32 NCHW [B][Cin][H][W]; P: dense [B*OH*OW][Kp] of dtype,
 *   OH = (H - 1) / 2 + 1, Kp = fva_stem7_kp(dtype, Cin) = Cin * 49 rounded up to a whole 128-byte k-tile of the implicit GEMM, 32 columns in
 *   fp32 and 64 in bf16 (0 for a bad dtype or a Cin outside 1..1024); column ci * 49 + kh * 7 + kw
 *   holds x[b][ci][2 oy - 3 + kh][2 ox - 3 + kw], taps outside the image and the columns from Cin * 49 on are zero.  The stem is then the
 *   1x1 convolution over P (fva_conv_fwd / fva_conv_wgrad with ksize 1, Cin = Kp, H = OH, W = OW, in_pad 0); the first Cin * 49 columns
 *   of its dW [Cout][Kp] are the weight gradient in OIHW order.
 * fva_maxpool3s2_fwd / _bwd: nn.MaxPool2d(3, 2, 1) (resnet.py:142-144), any H, W >= 1, OH = (H - 1) / 2 + 1.  x: halo [B][H+2p][W+2p][C];
 *   out: halo [B][OH+2q][OW+2q][C] with its zero border.  Taps outside the image count as -inf and are never read; a NaN in a window
 *   makes the output NaN.  Backward (gather form, no argmax tensor): dz dense [B][OH][OW][C] -> dx dense [B][H][W][C]; a pixel takes dz
 *   of the (at most four) windows in which torch's scan (kh, then kw ascending) ends on it -- the first maximum --, recomputed from x.
 * fva_subsample2_fwd / _bwd: xs[b][i][j][c] = x[b][2i][2j][c] (resnet.py:49, :106: the stride of the 1x1 shortcut), H and W even.
 *   x halo, xs dense [B][H/2][W/2][C].  Backward: dxs dense -> dx dense [B][H][W][C], dxs at the even positions and WRITTEN zeros
 *   elsewhere (the `addend` of the main branch's fva_conv_dgrad).
 * fva_bn_add_relu_*: z = max(0, u), u = y * scale + shift + R (resnet.py:64-71, :117-124), y dense [B*H*W][C].  Exactly one of
 *   r      the identity: a halo tensor [B][H+2p][W+2p][C], p = r_pad; R = r                                       (form 1)
 *   y_d    the dense output of the shortcut convolution, with scale_d / shift_d; R = y_d * scale_d + shift_d      (form 2)
 *   is non-NULL.  u is recomputed in fp32 from the stored operands in all three passes (never read from the rounded z); a NaN stays a NaN.
 *   _apply       z as a halo buffer [B][H+2q][W+2q][C] with its zero border, q = z_pad.  Eval mode: the coefficients of fva_bn_eval_coeffs.
 *   _bwd_reduce  dU = dz * (u > 0), dz dense.  partial [fva_bn_add_relu_bwd_blocks()][2][C] = per-block sums of dU and dU * xhat; form 2
 *                also partial_d [..][2][C] = sums of dU (the same numbers) and dU * xhat_d, xhat_d = (y_d - mean_d) * rstd_d.  Each table
 *                goes through fva_bn_bwd_finalize as it is (allocate fva_bn_partial_rows(blocks) rows).
 *   _bwd_apply   dy = a * dU + k1 * y + k2 from coef (fva_bn_bwd_finalize's [3][C] table), a halo buffer with zero border, p = dy_pad;
 *                fp32 tensors form the sum in double.  Form 1 also writes dr = dU dense [B*H*W][C] (the identity's gradient); form 2 also
 *                dy_d = a_d * dU + k1_d * y_d + k2_d from coef_d, a halo buffer like dy. */
int32_t fva_stem7_kp(int dtype, int Cin);
int fva_stem7_patches(int dtype, const float* x, void* P, int B, int Cin, int H, int W, void* stream);
int fva_maxpool3s2_fwd(int dtype, const void* x, int x_pad, void* out, int out_pad, int B, int H, int W, int C, void* stream);
int fva_maxpool3s2_bwd(int dtype, const void* dz, const void* x, int x_pad, void* dx, int B, int H, int W, int C, void* stream);
int fva_subsample2_fwd(int dtype, const void* x, int x_pad, void* xs, int B, int H, int W, int C, void* stream);
int fva_subsample2_bwd(int dtype, const void* dxs, void* dx, int B, int H, int W, int C, void* stream);
int fva_bn_add_relu_apply(int dtype, const void* y, const float* scale, const float* shift, const void* r, int r_pad, const void* y_d,
                          const float* scale_d, const float* shift_d, void* z, int z_pad, int B, int H, int W, int C, void* stream);
int32_t fva_bn_add_relu_bwd_blocks(int dtype, int64_t M, int C);
int fva_bn_add_relu_bwd_reduce(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                               const float* save_rstd, const void* r, int r_pad, const void* y_d, const float* scale_d, const float* shift_d,
                               const float* save_mean_d, const float* save_rstd_d, float* partial, float* partial_d, int32_t nblocks, int B, int H,
                               int W, int C, void* stream);
int fva_bn_add_relu_bwd_apply(int dtype, const void* dz, const void* y, const float* scale, const float* shift, const float* save_mean,
                              const float* save_rstd, const float* coef, const void* r, int r_pad, const void* y_d, const float* scale_d,
                              const float* shift_d, const float* save_mean_d, const float* save_rstd_d, const float* coef_d, void* dy, void* dy_d,
                              int dy_pad, void* dr, int B, int H, int W, int C, void* stream);

/* ---- Grouped 3x3 convolution (classfication/models/resnext.py:40, conv2 of the ResNeXt bottleneck; version 10) ------------------------
 * 3x3, padding 1, stride 1 or 2, Cin == Cout == C, bias-free.  Contract: C = groups * Cg with Cg in {4, 8, 16, 32, 64}, C % 64 == 0,
 * C <= 2048; stride 2 needs even H and W; dtype FVA_F32 / FVA_BF16; in_pad and dy_pad in 1 ... 8.  Anything else returns FVA_ERR_ARG with a
 * message (fva_last_error) and launches nothing.  OH = (H - 1) / stride + 1.
 *   x   halo NHWC [B][H + 2 in_pad][W + 2 in_pad][C] (zero border)       y    dense [B*OH*OW][C]
 *   dy  halo NHWC [B][OH + 2 dy_pad][OW + 2 dy_pad][C] (zero border: what fva_bn_relu_bwd_apply writes)
 *   dx  dense [B][H][W][C]                                               dw   fp32 [C][Cg][3][3], the parameter's own shape
 *   w_oihw: the fp32 master weight [C][Cg][3][3] as it stands; bf16 tensors multiply its bf16 rounding.  No packed copy exists and
 *   nothing is cached between calls.
 *   stats_partial: [fva_bn_partial_rows(fva_gconv_stat_blocks(d))][2][C], per block of 256 output pixels the sums of y and y^2 (of the
 *   unrounded accumulators, in pixel order); fva_bn_finalize takes it unchanged.  NULL: no statistics (eval mode).
 *   fva_gconv_wgrad: workspace of fva_gconv_wgrad_workspace(d) bytes (0 for a descriptor outside the contract); FVA_ERR_WORKSPACE if short.
 * No float atomics, fixed summation order: every launch gives the same bits twice.  fp32 tensors accumulate in double and round once.
 * All three run on plain FMA kernels at both strides (grouped.hip); the matrix-unit path for bf16 at stride 1 is fva_gconv_mfma_* below. */
typedef struct { int32_t dtype, B, H, W, C, groups, stride, in_pad, dy_pad; } fva_gconv_desc;   /* 3x3, padding 1, Cin == Cout == C */
int     fva_gconv_fwd(const fva_gconv_desc*, const void* x, const float* w_oihw, void* y, float* stats_partial, void* stream);
int32_t fva_gconv_stat_blocks(const fva_gconv_desc*);
int     fva_gconv_dgrad(const fva_gconv_desc*, const void* dy, const float* w_oihw, void* dx, void* stream);
int     fva_gconv_wgrad(const fva_gconv_desc*, const void* x, const void* dy, float* dw_oihw, void* workspace, int64_t workspace_bytes, void* stream);
int64_t fva_gconv_wgrad_workspace(const fva_gconv_desc*);

/* ---- The same convolution on the matrix units (grouped_mfma.hip; version 11) ------------------------------------------------------------
 * A second path beside fva_gconv_*, for the layers that carry ResNeXt's time: dtype FVA_BF16, stride 1, in_pad == dy_pad == 1, the C / Cg
 * contract above, B (H + 2)(W + 2) < 2^31, and a map whose staging fits 64 KB of LDS (W <= 70).  fva_gconv_mfma_serves answers 1 / 0 for a
 * descriptor (pure host, sets no error); every other entry point refuses a descriptor it answers 0 for with FVA_ERR_ARG and a message that
 * names this contract, and launches nothing (the size functions return 0).  Tensors as above: x / dy halo (border 1, zero), y / dx dense,
 * dw fp32 [C][Cg][3][3].  The caller chooses the path; nothing falls back.
 *   fva_gconv_mfma_pack: the fp32 master weight -> two bf16 tables (round to nearest even: the values the plain path multiplies), forward
 *   and data gradient, fva_gconv_mfma_pack_bytes(d) bytes EACH.  One small launch, meant to run in front of every forward (nothing is
 *   cached or keyed on the parameter: a captured step replays it on the weights the optimizer has just written).  Table layout
 *   [C / 16 slabs][steps][64 lanes][8 elements], the A fragments of v_mfma_f32_16x16x32_bf16: lane l, element j is row m = l % 16 (channel
 *   c = 16 slab + m, whose output the row computes), k = 8 (l / 16) + j.
 *     Cg >= 32: steps = 9 Cg / 32, step = tap * (Cg / 32) + h, the row's partner channel is kc = 32 h + k of c's group (first channel gb):
 *               forward w[c][kc][tap], data gradient w[gb + kc][c - gb][8 - tap].
 *     Cg <= 16: steps = 5, tap = 2 step + k / 16, the partner is channel kc = k % 16 of the slab; zero unless tap < 9 and kc / Cg == m / Cg
 *               (the block diagonal): forward w[c][kc % Cg][tap], data gradient w[16 slab + kc][m % Cg][8 - tap].
 *   fva_gconv_mfma_fwd: stats_partial [fva_bn_partial_rows(fva_gconv_mfma_stat_blocks(d))][2][C]: one row per block of 256 consecutive
 *   PADDED positions (b, yy, xx over [B][H + 2][W + 2]), the sums of y and y^2 over the block's real pixels from the unrounded
 *   accumulators; fva_bn_finalize takes it unchanged with count = B H W.  NULL: no statistics (eval mode).
 *   fva_gconv_mfma_wgrad: workspace of fva_gconv_mfma_wgrad_workspace(d) bytes (fp32 partials per run of positions, added in their order by
 *   a second launch); FVA_ERR_WORKSPACE if short.
 * Arithmetic: the products of two bf16 values are exact in fp32; they are accumulated in fp32 in a fixed order (no atomics: the same bits
 * on every run), the statistics in double.  y and dx are rounded to bf16 once.  Cg < 16 multiplies a slab of 16 / Cg groups by a
 * block-diagonal fragment, so a NON-FINITE input in one group reaches the other groups of its 16-channel slab through zero times infinity
 * (NaN); the plain path does not do this.  The weight gradient sums over the padded positions: dy's zero border adds exact zeros, and a
 * non-finite x next to it would not. */
int     fva_gconv_mfma_serves(const fva_gconv_desc*);
int64_t fva_gconv_mfma_pack_bytes(const fva_gconv_desc*);
int     fva_gconv_mfma_pack(const fva_gconv_desc*, const float* w_oihw, void* wpack_fwd, void* wpack_dgrad, void* stream);
int32_t fva_gconv_mfma_stat_blocks(const fva_gconv_desc*);
int     fva_gconv_mfma_fwd(const fva_gconv_desc*, const void* x, const void* wpack_fwd, void* y, float* stats_partial, void* stream);
int     fva_gconv_mfma_dgrad(const fva_gconv_desc*, const void* dy, const void* wpack_dgrad, void* dx, void* stream);
int64_t fva_gconv_mfma_wgrad_workspace(const fva_gconv_desc*);
int     fva_gconv_mfma_wgrad(const fva_gconv_desc*, const void* x, const void* dy, float* dw_oihw, void* ws, int64_t ws_bytes, void* stream);

/* ---- Label smoothing, MixUp and CutMix (not in the reference: the standard recipe of its classifiers; version 12) -------------------
 * fva_mix_plan: a ONE-THREAD tick kernel that decides, on the device, what the next batch gets.  state = int64[4] in DEVICE memory,
 * {seed, call counter, 0, 0} (the protocol of fva_dropout_fwd): the launch reads seed and counter and advances the counter itself, so a
 * captured graph draws a new plan on every replay and the host never reads anything back.  All launches that share one state must be
 * on ONE stream.  Random words: Philox-4x32-10 keyed by the seed's two halves; block j = philox(counter = (j, 0, call counter lo, hi)),
 * word i of the tick = word i % 4 of block i / 4.  A uniform is u(word) = ((word >> 8) + 0.5f) * 2^-24 in fp32 arithmetic: exact for
 * word >> 8 < 2^23, the sum rounded to even above (fp32 has no half there), so u lies in (0, 1] and is never 0.
 *   word 0   apply at all iff u < prob
 *   word 1   CutMix iff (mixup_alpha > 0 and cutmix_alpha > 0 and u < switch_prob) or (only cutmix_alpha > 0); MixUp iff not CutMix and
 *            mixup_alpha > 0; both alphas 0: mode 0
 *   word 2   rx = (uint64(word) * W) >> 32        word 3   ry = (uint64(word) * H) >> 32          (exact integer arithmetic)
 *   words 4 + 2 i, 5 + 2 i (i = 0, 1, ...)   the i-th pair (U, V) of Johnk's method for lam_raw ~ Beta(alpha, alpha), alpha = the chosen
 *            mode's: X = U^(1/alpha), Y = V^(1/alpha); accept the first pair with X + Y <= 1 and return X / (X + Y); when X + Y == 0
 *            (underflow) the log-space form lx = log(U) / alpha, ly = log(V) / alpha, each minus their maximum, exp(lx - log(exp(lx) +
 *            exp(ly))) -- what numpy's RandomState.beta runs for a, b <= 1.  Evaluated in double from the fp32 uniforms and rounded ONCE
 *            to fp32.  After 512 rejected pairs (probability below 2^-512) lam_raw = 0.5.
 * Words 0 ... 3 are always consumed; a tick that does not apply draws no pair.  0 <= alpha <= 1 (alpha > 1: FVA_ERR_ARG), prob and
 * switch_prob in [0, 1], H, W >= 1 with H * W < 2^31.
 * The plan: mode (0 none, 1 MixUp, 2 CutMix), lam_raw, lam and, for CutMix, torchvision's box: r = 0.5f * sqrtf(1 - lam_raw),
 * hw = (int)(r * W), hh = (int)(r * H) (fp32), x1 = max(rx - hw, 0), x2 = min(rx + hw, W), y1, y2 likewise,
 * lam = 1.f - (float)((x2 - x1) * (y2 - y1)) / (float)(W * H).  MixUp: lam = lam_raw, no box (zeros).  Mode 0: lam = lam_raw = 1.
 *
 * fva_mix_apply: out of place over planar [B][C][H][W] of dtype (FVA_F32 / FVA_BF16); the plan is read on the device.  The partner of
 * image b is (b - 1 + B) % B (batch.roll(1, 0)).  Mode 1: out = fmaf(lam, x_b, (1 - lam) * x_partner) in fp32, rounded once to dtype;
 * mode 2: the partner's pixel inside [y1, y2) x [x1, x2), a bit-exact copy elsewhere; mode 0, and B == 1 in every mode: a bit-exact
 * copy.  16-byte accesses when C * H * W and W are multiples of the 16-byte chunk and both pointers are 16-byte aligned, one element
 * per thread otherwise; 64-bit element offsets.  B <= 65535.
 *
 * fva_softmax_ce_soft: fva_softmax_ce with the target q = (1 - smoothing) * t + smoothing / C, where t is
 *   (a) onehot(y_r)                                              plan == NULL, dense == NULL
 *   (b) lam * onehot(y_r) + (1 - lam) * onehot(y_((r-1+R) % R))  plan != NULL: lam is read from the plan on the device
 *   (c) dense[r][:], fp32 [R][C] (torch's probability targets)   dense != NULL (labels ignored; with a plan: FVA_ERR_ARG)
 * row loss = w_r * (sum(q) * lse - sum_k q_k z_k) = -w_r * sum_k q_k log_softmax(z)_k (sum(q) = 1 for (a) and (b), so lse - sum q z),
 * grad = scale * w_r * (softmax * sum(q) - q); reduction, weights, workspace (fva_softmax_ce_workspace) and the fixed-order double sum
 * as fva_softmax_ce.  An invalid label makes every row that uses it NaN and no other: row r and, under (b), row r + 1; no memory is
 * indexed with it.  smoothing in [0, 1].  With smoothing == 0 and form (a), value and gradient equal fva_softmax_ce bit for bit.
 *
 * fva_topk_accuracy: out[0] = (rows with #{j : z_j beats z_y} < k) / R; "beats" is the order of fva_top1_accuracy's argmax (a NaN is
 * largest, among equals the smaller index wins), so k = 1 equals fva_top1_accuracy exactly; k >= 1; a label out of range (or not an
 * integer) never hits.  workspace: R int32. */
typedef struct {
    int32_t mode;              /* 0 none, 1 MixUp, 2 CutMix */
    float lam_raw, lam;
    int32_t rx, ry, x1, y1, x2, y2;
} fva_mix_plan_t;
int fva_mix_plan(int64_t* state, float mixup_alpha, float cutmix_alpha, float prob, float switch_prob, int32_t H, int32_t W,
                 fva_mix_plan_t* plan, void* stream);
int fva_mix_apply(int dtype, const void* x, void* out, const fva_mix_plan_t* plan, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
int fva_softmax_ce_soft(const float* logits, const void* labels, int label_dtype, const float* dense, const float* weights, int32_t R,
                        int32_t C, int32_t reduction, float smoothing, const fva_mix_plan_t* plan, float* loss_out, float* grad,
                        void* workspace, void* stream);
int fva_topk_accuracy(const void* logits, int logits_dtype, const void* labels, int label_dtype, int32_t R, int32_t C, int32_t k, float* out,
                      void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTVISION_AMD_H */
