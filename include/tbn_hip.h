/* libtbn_hip.so -- C-ABI of the MI355X (gfx950) TBN hot path.
 *
 * The reference (tridivb/attention_based_tbn) is pure Python on torch.nn and has no native
 * interface; this is the boundary a maintainer binds with ctypes.  Every
 * entry point lists the reference code it replaces.
 *
 * Conventions
 *   - plain C: raw device pointers (fp32 unless noted), explicit sizes / pitches, `void* stream`
 *     is a hipStream_t (pass PyTorch's current stream); no torch types, no allocation, no
 *     synchronisation, no global device state inside -- the caller owns every buffer including
 *     workspaces (sizes from the *_bytes / *_floats queries);
 *   - returns 0 on success, <0 on error (TBN_ERR_*); message via tbn_last_error() (thread-local);
 *     never throws; re-entrant; results are deterministic (no float atomics);
 *   - activations are NHWC with an explicit pitch `ld` (floats between pixels) so operators read
 *     and write channel slices of concat buffers; conv weights are [Cout][R][S][Cin], i.e. the
 *     memory of an OIHW torch parameter in channels_last format.
 */
#ifndef TBN_HIP_H
#define TBN_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TBN_ERR_ARG (-1)
#define TBN_ERR_LAUNCH (-2)
#define TBN_ERR_UNSUPPORTED (-3)

/* library version in the low 16 bits; bit 16 (0x10000) is set by a -DTBN_EXPERIMENT=1 build, the only build that reads
 * A/B environment knobs (the shipped library reads no environment variable at all) */
int tbn_version(void);
/* Feature bits of this build, for callers that bind the C-ABI directly: flag bits a library does not know are ignored by
 * its launchers, so ask before relying on one.  TBN_CAP_CONV_BF16X: the split-bf16 convolution math (flags 32 / 64 of
 * tbn_conv2d_fwd / tbn_conv_desc, TBN_BACKBONE_CONV_BF16X6 / _BF16X3) is honoured.  The low 16 bits of tbn_version() name
 * the plan-cache format (TBN_PLAN_CACHE file names, the committed bench plans) and do not move with added features; a
 * library without this symbol has none of them.  Replaces nothing in the reference. */
#define TBN_CAP_CONV_BF16X 1
/* bit 2: pre-split bf16 weight planes are honoured -- conv flag 128 with the pointwise (1x1) split-bf16 kernel,
 * tbn_conv_split_weights / tbn_backbone_split_weights, TBN_BACKBONE_CONV_BF16X_ALL and tbn_backbone_params.weight_planes */
#define TBN_CAP_CONV_BF16X_PLANES 2
/* bit 3: tbn_frames_to_tensor_crops (several crop windows, optionally paired with their mirror images, in one launch) */
#define TBN_CAP_FRAMES_CROPS 4
/* bit 4: the general attention core (tbn_mha_fwd / tbn_mha_bwd: any number of queries, up to 1024 keys, any head_dim) and
 * the attention-weight softmax (tbn_attn_weights_fwd / tbn_attn_weights_bwd) */
#define TBN_CAP_ATTN_GENERAL 8
/* bit 5: the attention-weight regularisers (tbn_attn_reg_fwd / tbn_attn_reg_bwd: prior, contrast and entropy losses) */
#define TBN_CAP_ATTN_REG 16
/* bit 6: the audio data layer (tbn_stft_windows: windows cut inside the STFT launch, log-mel mode; tbn_attn_prior_loud) */
#define TBN_CAP_AUDIO_LAYER 32
/* bit 7: the stem entries (tbn_stem_geometry / tbn_stem_workspace_floats / tbn_stem_conv_fwd / tbn_stem_conv_wgrad) */
#define TBN_CAP_STEM_OPS 64
/* bit 8: the batched training-BN entries (tbn_bn_stats_partials / tbn_bn_fwd_batch / tbn_bn_bwd_batch / tbn_bn_bwd_partial_floats) */
#define TBN_CAP_BN_BATCH_OPS 128
int tbn_capabilities(void);
const char* tbn_last_error(void);

/* measurement aid (bench.py roofline): while enabled, every conv-GEMM launch (forward / data-grad /
 * weight-grad implicit GEMMs) is bracketed by hipEvents recorded on the launch stream; entries
 * aggregate, per kernel instantiation, the launch count, summed event time and summed algorithmic
 * FLOPs (2*M*Cout*R*S*Cin of the convolution; padding / zero-insertion work is not counted).
 * tbn_profile_num_entries() synchronises the recorded events.  enable(2) keys entries per layer
 * ("kernel | fwd/dgrad/wgrad <conv name>") instead of per kernel instantiation. */
int tbn_profile_enable(int on);
int tbn_profile_reset(void);
int tbn_profile_num_entries(void);
int tbn_profile_entry(int i, char* name, int name_len, long* launches, double* total_ms, double* total_flops);
/* summed ALGORITHMIC HBM bytes of entry i: per launch the input read once + weights once + output written once (conv /
 * data gradient), dy + x read once + dW written once (weight gradient) -- the denominator of the traffic ratio */
int tbn_profile_entry_bytes(int i, double* total_alg_bytes);
/* measurement aid (bench.py `box.mfma_calibration`): ONE launch of a pure v_mfma_f32_32x32x2_f32 register loop
 * (`workgroups` x 4 waves x `iters` x 16 MFMAs, no memory traffic; sink: any device float, never written) so that a bench
 * line can state what the box it ran on sustains on the instruction the roofline is priced in.  *flops = the MFMA FLOPs of
 * the launch.  Replaces nothing in the reference (which publishes no hardware figures). */
int tbn_diag_mfma_burst(float* sink, int workgroups, int iters, double* flops, void* stream);

/* ---- BN-Inception backbone engine -------------------------------------------------------------
 * replaces: BNInception.features() as instantiated by reference core/models/bn_inception.py:38-107
 * (graph core/models/bn_inception_audio.py:58-404,437-1003 with the 7x7 stem), called from
 * TBNModel.forward core/models/model.py:211-213, and its autograd backward (core/tools/train.py:81).
 * A plan is host-only metadata for one (in_channels, frames, H, W). */
typedef struct tbn_backbone_plan tbn_backbone_plan;

typedef struct {
  char name[64];          /* reference module name, e.g. "inception_3a_1x1" (+"_bn" for its BatchNorm) */
  int cin, cout, ksize, stride, pad;
  size_t weight_offset;   /* floats into the flat weight array: this conv's [cout][k][k][cin] block */
  size_t channel_offset;  /* floats into each flat per-channel array (bias, gamma, beta, mean, var) */
} tbn_conv_info;

typedef struct {
  const float* weight;        /* flat conv weights, tbn_backbone_weight_floats() */
  const float* bias;          /* flat conv biases, tbn_backbone_channel_floats() */
  const float* gamma;         /* BatchNorm weight */
  const float* beta;          /* BatchNorm bias */
  float* running_mean;        /* updated in training mode (momentum) */
  float* running_var;
  float momentum;             /* 0.1 */
  float eps;                  /* 1e-5 */
  void* side_stream;          /* optional second hipStream_t (caller-owned) for tbn_backbone_forward / _backward: BRANCH MODE.
                                 The four branches of an inception block only meet at the concat (reference
                                 core/models/bn_inception_audio.py:437-1003, torch.cat at :485-493 and in every block after);
                                 with a side stream the 3x3 / pool_proj chain of each block runs on it beside the
                                 1x1 -> double_3x3 chain on the launch stream (forked after the 1x1 group's BatchNorm, joined
                                 at the end of the block), so one chain's BN / pool passes sit under the other's GEMMs.
                                 Every layer runs the kernel the serial program would launch for it alone -- sibling-pair
                                 launches (3x3 | double_3x3_1 in one grid) are replaced by the two tuned single launches --
                                 so with pairing off the two programs agree bit for bit (tests/test_branch_gpu.py).  Joined before the
                                 call returns.  NULL = one chain.  Ignored (serial program) while the launch stream is
                                 being captured: forks inside a capture are what aux_stream's note below is about. */
  int flags;                  /* TBN_BACKBONE_RIDERS (1): training passes of the one-chain program put the BN apply / BN-backward
                                 apply of a block's INDEPENDENT column ranges into the grid of a sibling GEMM launch instead of
                                 their own launches -- forward: `1x1` beside `3x3 | double_3x3_1`, `3x3` and `pool_proj` beside
                                 `double_3x3_2`; backward: `1x1`, `3x3`, `pool_proj` beside the data gradient of `double_3x3_2`
                                 (reference dataflow core/models/bn_inception_audio.py:437-1003: these branches only meet at the
                                 concat, :485-493).  Same device code as the stand-alone passes: results are bit-identical with the
                                 flag off (tests/test_riders_gpu.py).  Ignored in branch mode and while the opt-in profiler brackets
                                 the conv launches. */
  const void* weight_planes;  /* TBN_BACKBONE_CONV_BF16X_ALL only (never read without that flag, so callers built against the
                                 shorter struct keep working): the bf16 planes of the flat weights,
                                 tbn_backbone_weight_planes_bytes() bytes filled by tbn_backbone_split_weights() with the same np */
} tbn_backbone_params;
#define TBN_BACKBONE_RIDERS 1
#define TBN_BACKBONE_STEM_WGRAD_LAST 2   /* one-chain backward without aux stream: the weight gradients of conv2_3x3 and
                                            conv2_3x3_reduce are issued after conv1's pooled BN backward instead of before it
                                            (same kernels, bit-identical results; a scheduling choice between the replicas'
                                            streams) */
#define TBN_BACKBONE_WEIGHTS_FLIPPED 4   /* tbn_backbone_backward only: the flipped / transposed data-gradient weights in the
                                            workspace are current (tbn_backbone_flip_weights ran on this workspace, on the same
                                            stream, after the matching forward and the weights have not changed since): the pass
                                            does not launch the flip itself */
#define TBN_BACKBONE_CONV_BF16X6 8       /* tbn_backbone_forward(training = 0) only: split-bf16 convolution math.  Every conv of the
                                            plan that is 3x3 / stride 1 / pad 1 with cin a multiple of 32 on a map at most 64 wide (in this
                                            graph: every 3x3 / stride 1 layer, cin 64 ... 192) runs on the bf16 MFMA with
                                            six plane products (tbn_conv2d_fwd flag 32: fp32 in / out, error below the fp32
                                            accumulation's own) and the eval epilogue, as a single launch with the layer's tuned
                                            LDS-halo tile or a size heuristic; every other layer, and every layer when training = 1,
                                            runs exactly as without the flag.  The plan blob, its size and fingerprint and the
                                            workspace size do not depend on it; tbn_backbone_autotune / _backward ignore it.
                                            replaces: the 3x3 nn.Conv2d forwards of core/models/bn_inception_audio.py:24-401 under
                                            model.eval() / torch.no_grad() (core/tools/test.py:67-87) */
#define TBN_BACKBONE_CONV_BF16X3 16      /* the same with three plane products (flag 64: relative error < 1.25 * 2^-16 per product);
                                            exclusive with TBN_BACKBONE_CONV_BF16X6 (both: TBN_ERR_ARG) */
#define TBN_BACKBONE_CONV_BF16X_ALL 32   /* with _BF16X6 or _BF16X3 and training = 0 (ignored otherwise): the weights come from
                                            tbn_backbone_params.weight_planes (NULL: TBN_ERR_ARG) -- pre-split once instead of per
                                            tap and tile inside the kernels -- and the mode also covers every 1x1 / stride 1 GEMM
                                            (cin a multiple of 32: all of them, the merged sibling groups with their pooled
                                            pool_proj part and conv2_3x3_reduce included) through the pointwise split-bf16 kernel
                                            (conv flag 128), as single launches with the eval epilogue.  The stem, the four
                                            stride-2 3x3 layers and a conv2_3x3 on a map wider than 64 stay on the fp32 MFMA.
                                            Plan blob, fingerprint, autotune and workspace size do not depend on it.
                                            replaces: the 1x1 and 3x3 nn.Conv2d forwards of core/models/bn_inception_audio.py:24-401
                                            under model.eval() / torch.no_grad() (core/tools/test.py:67-87) */

typedef struct {
  float* dweight;             /* same layout as weight; fully overwritten */
  float* dbias;
  float* dgamma;              /* may be NULL */
  float* dbeta;               /* may be NULL */
  int bn_grad_layers;         /* 0 none, 1 first BN only ("partialbn", model.py:164-176), 2 all */
  void* aux_stream;           /* optional second hipStream_t (caller-owned): weight-gradient GEMMs run on it,
                                 overlapping the data-gradient / BN-backward chain; joined before return.  NULL = serial.
                                 Not inside a stream capture: tbn_backbone_backward returns TBN_ERR_UNSUPPORTED when its
                                 launch stream is capturing and aux_stream != NULL.  The fault being fenced off is a NESTED
                                 fork (a stream that itself joined the capture through an event wait forks the aux stream):
                                 hipStreamEndCapture of ROCm 7.x then recurses until the stack overflows.  A single-level
                                 fork from the capture's ORIGIN stream captures fine, but HIP offers no query that tells an
                                 origin stream from a forked one, so the guard refuses that case too -- broader than the
                                 fault, by necessity.  The Python host passes NULL while capturing (serial launches). */
  void (*bucket_cb)(void* user, size_t first_float, size_t num_floats);
                              /* optional (NULL: none).  Gradient buckets for data parallelism (reference: the per-backward
                                 reduce_add_coalesced of nn.DataParallel, core/models/model_builder.py:73-75): called on the
                                 CALLING thread, twice per backward pass, as soon as every launch that writes
                                 dweight[first_float, first_float + num_floats) has been enqueued -- first the weights of
                                 inception_5a..5b, then those of inception_4a..4e (a suffix of the flat tensor each time;
                                 plan order = memory order).  Work the callback enqueues behind the launch stream (an
                                 RCCL all-reduce of that slice) then overlaps the rest of the pass; the remaining prefix
                                 (stem, 3a..3c) is final when the function returns.  The split depends on the graph
                                 only: identical on every replica.  With aux_stream the launch stream is first made to
                                 wait for the weight gradients issued so far.  Not called inside a stream capture. */
  void* bucket_user;
} tbn_backbone_grads;

/* TBN_ERR_UNSUPPORTED for input sizes on which the reference graph itself is inconsistent (its torch.cat of the stride-2
 * branches and the ceil-mode pool of inception_3c / 4e raises) and for frame counts that would make any one tensor of the
 * pass 2 GiB or larger (32-bit byte offsets under the hardware range check: 511 spectrograms of 256x256 or 668 frames of
 * 224x224 per call at most; eval callers chunk the frames, a training step needs a smaller per-GPU batch). */
int tbn_backbone_plan_create(int in_channels, int frames, int height, int width, tbn_backbone_plan** plan);
void tbn_backbone_plan_destroy(tbn_backbone_plan* plan);
int tbn_backbone_num_convs(const tbn_backbone_plan* plan);                       /* 69 */
int tbn_backbone_conv_info(const tbn_backbone_plan* plan, int idx, tbn_conv_info* info);
size_t tbn_backbone_weight_floats(const tbn_backbone_plan* plan);
size_t tbn_backbone_channel_floats(const tbn_backbone_plan* plan);
size_t tbn_backbone_workspace_bytes(const tbn_backbone_plan* plan, int training);
int tbn_backbone_out_shape(const tbn_backbone_plan* plan, int* h, int* w, int* c);
/* 2 when the plan holds a branch-mode program (tbn_backbone_params.side_stream is honoured), else 1 */
int tbn_backbone_num_streams(const tbn_backbone_plan* plan);
/* Opt-in kernel timeline (diagnostics; scripts/step_timeline.py reads the file): while enabled every launch of the library
 * carries a pair of events on its dispatch packet; tbn_timeline_dump synchronises the device and writes one CSV row per
 * launch (Kernel_Name, Queue_Id = stream, Start_Timestamp, End_Timestamp in ns on a common clock).  Unlike an external
 * tracer it leaves the host's launch rate alone, so the overlap of the modality streams is the un-traced step's.
 * enable(1) clears earlier records.  The reference has no counterpart (its only timing: core/tools/train.py:339-351). */
int tbn_timeline_enable(int on);
int tbn_timeline_dump(const char* path);
/* diagnostics: how many conv launches of the plan's LAST training forward / backward pass carried a rider
 * (tbn_backbone_params.flags & TBN_BACKBONE_RIDERS): 2 / 1 per average-pool inception block, 1 / 1 per stride-2 block */
int tbn_backbone_rider_launches(const tbn_backbone_plan* plan, int* forward, int* backward);
/* test / debug aid: location of one conv's tensors inside the workspace (floats). kind 0: z =
 * relu(bn(conv)) destination slice, 1: BN input y (overwritten by dy in backward), 2: gradient
 * wrt z (offset -1 when it is the caller-supplied dfeatures), 3: the conv's whole input buffer, 4: its training-mode
 * BatchNorm coefficients as 4 rows x cout (batch mean | 1/std | scale | shift).  Kind 0 of a conv whose max pool runs
 * inside its BN apply (conv1_7x7_s2, conv2_3x3 in training) fails with TBN_ERR_UNSUPPORTED: that z is never written --
 * it is relu(fma(y, scale, shift)) of kinds 1 and 4. */
int tbn_backbone_tensor_info(const tbn_backbone_plan* plan, const char* conv_name, int kind, long* offset, int* rows,
                             int* cols, int* ld);
/* test / diagnostics aid: the launch choices the plan holds for one conv (after tbn_backbone_autotune: the tuned ones,
 * before: the size heuristics).  Forward choices are kept PER MODE (`training` selects which); the data-gradient ones
 * only exist for training.  out[0..7]  = forward: kernel variant (0 register-staged implicit GEMM, 1 LDS-halo, 2 LDS-DMA,
 * 3 split-K tile), M tile, N tile, LDS stages, issued as a sibling pair (0 / 1; on the pair's first member), pair variant,
 * pair M tile, pair N tile; out[8..15] = the same for the data gradient (zeros when the layer has none / training == 0). */
int tbn_backbone_launch_info(const tbn_backbone_plan* plan, const char* conv_name, int training, int* out16);
/* The tuned launch choices of a plan as a relocatable blob in HOST memory (what tbn_backbone_autotune decides: per GEMM the
 * forward choice per mode, the data-gradient choice, sibling pairing, the weight-gradient tile -- no addresses), so that a
 * plan tuned once can be moved between processes: `DataParallel` broadcasts rank 0's blobs and every replica runs the same
 * kernels, as the reference's nn.DataParallel replicas do by construction (core/models/model_builder.py:73-75,
 * core/models/dataparallel.py:4-6).  export_bytes is a function of the plan's problem only; import validates the header
 * (same in_channels / frames / H / W) and every field against what the launchers accept, and leaves the plan untouched
 * when it refuses.  fingerprint = 64-bit FNV-1a of the blob (bench.py prints it per backbone). */
size_t tbn_backbone_plan_export_bytes(const tbn_backbone_plan* plan);
int tbn_backbone_plan_export(const tbn_backbone_plan* plan, void* buf, size_t bytes);
int tbn_backbone_plan_import(tbn_backbone_plan* plan, const void* buf, size_t bytes);
unsigned long long tbn_backbone_plan_fingerprint(const tbn_backbone_plan* plan);
/* x_nchw: (frames, in_channels, H, W) contiguous, as the reference passes it (model.py:213).
 * training=1: batch-statistics BN, keeps activations in the workspace for backward, updates
 * running stats; training=0: running-stat BN folded into the conv epilogue.
 * *features_out points INTO the workspace: NHWC (frames, h, w, 1024). */
int tbn_backbone_forward(const tbn_backbone_plan* plan, int training, const float* x_nchw,
                         const tbn_backbone_params* params, void* workspace, size_t workspace_bytes,
                         float** features_out, void* stream);
/* Weight planes for TBN_BACKBONE_CONV_BF16X_ALL (np = 6 | 3 plane products, i.e. three | two planes): one HBM-bound launch
 * that splits, in the layout of tbn_conv_split_weights, the weights of every GEMM of the plan with ksize 1 or 3, stride 1 and
 * cin a multiple of 32 -- a merged multi-part 1x1 GEMM as ONE tensor of its parts' rows in the engine's own part order, which
 * is their order in the flat weight array.  The buffer is the caller's (16-B aligned; size and layout depend on the graph and
 * np only -- 0 for another np -- never on frames or input size, so one buffer serves every plan of a backbone; a 3x3 layer
 * that a wide map keeps on the fp32 kernel still has its planes written); split again whenever the weights change.  tbn_backbone_workspace_bytes is unaffected.
 * replaces: nothing in the reference (cuDNN reads the fp32 nn.Conv2d weights of bn_inception_audio.py:24-401 directly). */
size_t tbn_backbone_weight_planes_bytes(const tbn_backbone_plan* plan, int np);
int tbn_backbone_split_weights(const tbn_backbone_plan* plan, const float* weight, int np, void* planes, void* stream);
/* optional one-time tuning of the per-layer GEMM tiles on the real shapes (times each candidate with
 * hipEvents).  The ONLY entry point that synchronises the stream; clobbers the activations held in
 * `workspace`, so call it between steps (e.g. right after the first forward of a new plan). */
int tbn_backbone_autotune(tbn_backbone_plan* plan, int training, const tbn_backbone_params* params, void* workspace,
                          size_t workspace_bytes, void* stream);
/* dfeatures: NHWC (frames, h, w, 1024) gradient of *features_out; needs the workspace of the
 * matching training forward untouched. */
int tbn_backbone_backward(const tbn_backbone_plan* plan, const float* dfeatures,
                          const tbn_backbone_params* params, const tbn_backbone_grads* grads, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The first launch of tbn_backbone_backward on its own: the flipped / transposed copy of every data-gradient weight
 * (what autograd's conv backward gets from cuDNN implicitly; reference: loss.backward(), core/tools/train.py:86) into the
 * training workspace.  It depends on the weights only, so a caller with several backbones on several streams can issue it on
 * each backbone's stream right after the streams were joined for the heads -- it then runs beside the heads' small kernels
 * instead of between them and the first backward GEMM -- and pass TBN_BACKBONE_WEIGHTS_FLIPPED to the backward pass. */
int tbn_backbone_flip_weights(const tbn_backbone_plan* plan, const tbn_backbone_params* params, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- single operators (same kernels the engine uses; used by the heads and the parity tests) ---- */

/* nn.Conv2d forward, NHWC.  epilogue: 0 = +bias (optional ReLU / accumulate via flags: 1 accumulate
 * into out, 2 ReLU); 1 = bias-FREE conv output plus per-channel (sum, sumsq) partials for a following
 * training-mode BN (stat_partial[tbn_conv2d_stat_tiles()][2][cout]) -- a per-channel constant cancels in
 * batch-stat BN, so `bias` is ignored here and only enters the running mean (tbn_backbone_* does that);
 * 2 = relu(conv * scale + shift) for eval BN (`bias` ignored: fold it into shift = beta + (bias-mean)*scale).
 * replaces: each nn.Conv2d of bn_inception_audio.py:24-401 (cuDNN).  cin must be a multiple of 32, ksize <= 3 (the
 * 7x7 stem exists only inside tbn_backbone_*: it reads a space-to-depth image the engine lays out itself).
 * flags also selects the kernel variant (test / tuning aid; 0 = generic): 4 = LDS-halo (3x3 / stride 1 / pad 1 only),
 * 8 = LDS-DMA staging, 16 = 32-row tiles whose four waves split K (statistics partial rows are then per 32*mt output
 * rows, tiles mt, nt in {1,2}).  Without a variant flag, epilogue-0 / -2 launches of at most 128 tiles and k*k*cin >= 256
 * (the head Linear layers, M = 96 rows) take the split-K tile kernel by themselves; every variant is deterministic.
 * Split-bf16 math (opt-in; replaces the same nn.Conv2d forward under model.eval() / torch.no_grad(), reference
 * core/tools/test.py:67-87): flag 32 = bf16x6, 64 = bf16x3.  fp32 operands are split into three / two bf16 planes while they
 * are staged into LDS and the six (i + j <= 2) / three (i + j <= 1) plane products run on v_mfma_f32_32x32x16_bf16 into one
 * fp32 accumulator: bf16x6 reproduces a * b to about 2^-25 relative, bf16x3 to < 1.25 * 2^-16.  3x3 / stride 1 / pad 1, map
 * width <= 64, epilogue 0 or 2, tiles mt in {1,2} x nt in {1..4} only: any other geometry, epilogue 1, a data gradient, a
 * pair launch, both bits, or a combination with 4 / 8 / 16 fails with TBN_ERR_UNSUPPORTED / TBN_ERR_ARG and a message naming
 * bf16x -- never a silent fp32 launch.  The profiler keys these launches as conv_bf16x6_kernel<..> / conv_bf16x3_kernel<..>.
 * Flag 128 (only with 32 or 64; alone: TBN_ERR_ARG): `weight` points at PRE-SPLIT bf16 weight planes written by
 * tbn_conv_split_weights with the matching np, not at fp32 weights.  3x3 / stride 1 / pad 1 (same limits): the same kernel with
 * its weight tile copied from the planes, bit-identical to the launch without 128 at the same tile (profiler key
 * conv_bf16x6_planes_kernel<..>).  1x1 / stride 1 / pad 0 with cin a multiple of 32: the pointwise split-bf16 kernel, a plain
 * [pixels x cin] . [cin x cout] GEMM with no map-width limit, the activation tile split while staged, epilogue 0 / 2, tiles
 * mt in {1,2} x nt in {1..4} (conv_bf16x6_pw_kernel<..>).  Everything else with 128 -- stride != 1, cin not a multiple of
 * 32, epilogue 1, a data gradient, a pair launch, a combination with 4 / 8 / 16 -- is refused with a message naming bf16x. */
int tbn_conv2d_fwd(const float* in, int in_ld, const float* weight, const float* bias, float* out, int out_ld,
                   int n, int h, int w, int cin, int cout, int ksize, int stride, int pad, int epilogue, int flags,
                   const float* scale, const float* shift, float* stat_partial, void* stream);
int tbn_conv2d_stat_tiles(int n, int h, int w, int cin, int cout, int ksize, int stride, int pad);
/* bf16 weight planes of ONE conv weight tensor [cout][ksize][ksize][cin] (ksize 1 or 3 -- the layers the split-bf16 kernels
 * take -- and cin a multiple of 32) for conv flag 128; np = 6
 * writes three planes (bf16x6), np = 3 two (bf16x3):  hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to
 * nearest even -- the values the split-bf16 kernels compute while staging fp32 weights.
 * LAYOUT: one record per (cout row, tap, 32-channel chunk), record index = (row * ksize * ksize + tap) * (cin / 32) + chunk,
 * i.e. (float index of the chunk's first weight) / 32; a record is [hi 32 | mid 32 | (lo 32)] bf16 = 192 B (np 6) / 128 B
 * (np 3), element c of a plane = channel 32 * chunk + c.  That is the kernels' LDS row image minus its 16-B pad, so a weight
 * tile row reaches LDS as 12 / 8 plain 16-byte copies.  Bytes: cout * ksize^2 * cin * 6 (np 6) / * 4 (np 3); the query returns
 * 0 for arguments the split refuses.  `planes` is caller-owned and 16-B aligned.
 * replaces: nothing in the reference (its nn.Conv2d weights, bn_inception_audio.py:24-401, go to cuDNN as fp32). */
size_t tbn_conv_weight_planes_bytes(int cout, int ksize, int cin, int np);
int tbn_conv_split_weights(const float* weight, int cout, int ksize, int cin, int np, void* planes, void* stream);
/* tuning / test aid: as tbn_conv2d_fwd (epilogue 0 or 1) with an explicit tile: the workgroup computes
 * (128*mt) x (32*nt) outputs, mt in {1,2}, nt in {1..4}; (0,0) = built-in heuristic */
int tbn_conv2d_fwd_tile(const float* in, int in_ld, const float* weight, const float* bias, float* out, int out_ld,
                        int n, int h, int w, int cin, int cout, int ksize, int stride, int pad, int epilogue, int flags,
                        float* stat_partial, int mt, int nt, void* stream);
/* data gradient: din (n,h,w,cin) = conv_transpose(dout).  workspace: cout*k*k*cin floats. */
int tbn_conv2d_dgrad(const float* dout, int dout_ld, const float* weight, float* din, int din_ld, int n, int h, int w,
                     int cin, int cout, int ksize, int stride, int pad, int accumulate, float* workspace,
                     void* stream);
/* ---- one convolution launch in full detail (test / tuning aid) --------------------------------
 * Reaches every kernel variant, tile, epilogue and the fused BN-backward reduce that the backbone engine's autotuner
 * can put on a layer -- including the forms the plain entry points above never select by themselves: explicit tiles of
 * the parity-phase launch of a strided data gradient, data-gradient / eval epilogues of the LDS-halo / LDS-DMA /
 * split-K tile kernels, the reduce epilogue, and two sibling convolutions in ONE launch.
 * replaces: the same nn.Conv2d forward / backward of bn_inception_audio.py:24-401 as tbn_conv2d_*. */
typedef struct {
  const float* y;         /* BN input of the producer layer at its column 0 (pitch y_ld), output pixel order */
  int y_ld;
  int col_begin;          /* first output column of this layer (multiple of 32, ascending, disjoint) */
  int channels;
  int stat_offset;        /* this layer's channel 0 inside the red_stats arrays */
  float* partial;         /* [tbn_conv_partial_rows()][2][channels]: per M tile  sum g | sum g * xhat */
} tbn_conv_red;
typedef struct {
  const float* in;        /* forward: input (n,h,w,cin); data gradient: dout (n,oh,ow,cout) */
  int in_ld;
  const float* weight;    /* [cout][k][k][cin] */
  const float* bias;      /* epilogue 0 of a forward launch; may be NULL */
  float* out;             /* forward: (n,oh,ow,cout); data gradient: din (n,h,w,cin) */
  int out_ld;
  int n, h, w, cin, cout, ksize, stride, pad;   /* geometry of the FORWARD convolution */
  int dgrad;              /* 0: forward, 1: data gradient of that convolution (workspace: cout*k*k*cin floats) */
  int epilogue;           /* forward: 0 / 1 / 2 as tbn_conv2d_fwd; data gradient: 0 */
  int flags;              /* 1 accumulate, 2 ReLU; kernel variant 4 LDS-halo, 8 LDS-DMA, 16 split-K tile (0 generic);
                             32 bf16x6 / 64 bf16x3 split-bf16 math (forward, epilogue 0 / 2; see tbn_conv2d_fwd); 128 with
                             32 / 64: `weight` points at pre-split weight planes (tbn_conv_split_weights); 256: the out2*
                             fields at the end of this struct are set (a second output destination) */
  int stages;             /* generic kernel: LDS stages 1 / 2 (0 = default) */
  const float* scale;     /* epilogue 2 */
  const float* shift;
  float* stat_partial;    /* epilogue 1: [tbn_conv_partial_rows()][2][cout] */
  int nred;               /* data gradient: fused BN-backward reduce over nred producer layers (0 = off) */
  tbn_conv_red red[4];
  const float* red_stats; /* mean | rstd | scale | shift, each red_stats_stride floats */
  int red_stats_stride;
  /* the four fields below were appended to the struct and are read ONLY when flags carries 256, so that a caller compiled
     against the shorter struct (which cannot set that bit knowingly) never has them read past its object */
  float* out2;            /* flags & 256; forward, epilogue 0 / 2: output columns >= out2_col_begin (a
                             multiple of 32, inside (0, cout)) go to out2 (pitch out2_ld, its column 0 = column out2_col_begin),
                             as the engine's merged 1x1 groups write their parts to different buffers */
  int out2_ld;
  int out2_col_begin;
  int out2_raw;           /* epilogue 2: 1 = out2 receives the bare accumulator (no scale / shift / ReLU), what the engine does
                             for a pool_proj part whose average pool follows the conv */
} tbn_conv_desc;
/* rows of stat_partial / red[i].partial that a launch with M tile `mt` writes (pair = 1: issued by tbn_conv_launch_pair); a
 * strided data gradient writes one row per M tile of every parity phase that launches (1x1 / stride 2: one parity in four;
 * accumulating, that launch refuses the reduce, which would miss the gradient already in the other pixels).
 * Every conv entry refuses an input pitch below the channels read per pixel or not a multiple of 4 floats. */
int tbn_conv_partial_rows(const tbn_conv_desc* d, int mt, int pair);
int tbn_conv_launch(const tbn_conv_desc* d, int mt, int nt, float* workspace, void* stream);
/* two independent unit-stride convolutions with the same epilogue in ONE launch (the 3x3 | double_3x3_1 siblings of an
 * inception block): variant 0 LDS-halo (both 3x3 / stride 1 / pad 1), 1 / 2 generic kernel with 1 / 2 LDS stages;
 * mt, nt in {1,2} */
int tbn_conv_launch_pair(const tbn_conv_desc* a, const tbn_conv_desc* b, int variant, int mt, int nt,
                         float* workspace_a, float* workspace_b, void* stream);

/* weight gradient: dweight [cout][k][k][cin].  workspace: tbn_conv2d_wgrad_workspace_floats(). */
size_t tbn_conv2d_wgrad_workspace_floats(int n, int h, int w, int cin, int cout, int ksize, int stride, int pad);
int tbn_conv2d_wgrad(const float* dout, int dout_ld, const float* in, int in_ld, float* dweight, int n, int h, int w,
                     int cin, int cout, int ksize, int stride, int pad, float* workspace, void* stream);
/* tuning / test aid: as tbn_conv2d_wgrad with an explicit tile: a workgroup computes (32*mt) x (32*nt) entries of one filter
 * tap, mt in {1,2,3,5}, nt in {1,2,3} without 5 x 3; (0,0) = the built-in heuristic.  Any other tile is refused, as are null
 * pointers, channel counts / pitches that are no multiples of 4 and pitches below the channel count -- before any launch.
 * workspace: tbn_conv2d_wgrad_workspace_floats() covers every tile. */
int tbn_conv2d_wgrad_tile(const float* dout, int dout_ld, const float* in, int in_ld, float* dweight, int n, int h, int w,
                          int cin, int cout, int ksize, int stride, int pad, int mt, int nt, float* workspace, void* stream);
/* host only (no launch, no device call): what tbn_conv2d_wgrad_tile would run for this problem and tile.
 * out8 = {mt, nt (the tile run), kernel mode (0 general, 2 pointwise = 1x1 / stride 1 / pad 0), splits, rows_per_split,
 * tiles_co, tiles_ci, slab lanes of the split-K reduce (0 = no split-K, 4, 16)}: the launch is
 * conv_wgrad_kernel<mt, nt, mode> on tiles_co * tiles_ci * ksize^2 * splits workgroups, then splitk_reduce_kernel<4 | 16> when
 * splits > 1.  Returns the split-K workspace floats that tile needs (>= 0), or a negative status. */
long long tbn_conv2d_wgrad_plan(int n, int h, int w, int cin, int cout, int ksize, int stride, int pad, int mt, int nt, int* out8);

/* ---- the 7x7 / stride 2 / pad 3 stem on its own (test / tuning aid) -----------------------------
 * conv1_7x7_s2 exactly as the backbone engine executes it -- the same launch sequence, built from the same statement of the
 * geometry -- for any cin in 1..16 and any h, w >= 1 (the engine itself needs 32 x 32).  x_nchw (n, cin, h, w) contiguous;
 * weight / dweight [cout][7][7][cin]; cout a multiple of 32 (the engine: 64).
 * layout: 0 = the engine's rule (space-to-depth for cin <= 3, row runs from cin = 4 on), 1 = the zero-bordered 2x2
 * space-to-depth image [n][ceil(h/2)+3][ceil(w/2)+3][4 cin] (4 filter rows of 16 cin floats, K = 64 cin), 2 = the zero-bordered
 * NHWC "row runs" image [n][2(oh-1)+8][2(ow-1)+8][cin] (7 runs of rl = 7 cin rounded up to x4 floats, K = 7 rl rounded up to x32).
 * Both layouts serve every cin.
 * tbn_stem_geometry: out8 = { layout as executed (1 | 2), image height, image width, floats per image pixel, run length,
 *   K, floats of packed weight gradient per output channel, image floats per frame }.  Host only.
 * tbn_stem_workspace_floats: floats of `workspace` (16-B aligned, caller-owned) for n frames: bordered image + packed weights
 *   + packed weight gradient + split-K slabs, each region 256-B aligned; 0 for arguments the entries refuse.  Host only.
 * tbn_stem_conv_fwd: repack, pack weights, the packed-row forward GEMM.  epilogue / bias / scale / shift / stat_partial as
 *   tbn_conv2d_fwd; tile mt in {1,2} x nt in {1..4}, or 0 x 0 = the size heuristic (statistics rows are then per 128 * mt
 *   output rows of a tile the caller does not know: size stat_partial for mt = 1, ceil(n oh ow / 128) rows, and pre-fill it);
 *   stages 1 | 2 (0 = default).
 * tbn_stem_conv_wgrad: repack, the packed-row weight gradient (+ split-K reduce), unpack.  Tile mt in {1,2,3,5} x nt in
 *   {1,2,3} without 5 x 3, or 0 x 0 = the heuristic.  Deterministic.
 * replaces: the forward / weight gradient of conv1_7x7_s2, nn.Conv2d(cin, 64, 7, stride 2, padding 3)
 * (bn_inception.py:75-77; cuDNN there). */
int tbn_stem_geometry(int cin, int h, int w, int layout, int* out8);
size_t tbn_stem_workspace_floats(int cin, int h, int w, int layout, int n, int cout);
int tbn_stem_conv_fwd(const float* x_nchw, const float* weight, const float* bias, float* out, int out_ld, int n, int h, int w,
                      int cin, int cout, int layout, int epilogue, const float* scale, const float* shift, float* stat_partial,
                      int mt, int nt, int stages, float* workspace, void* stream);
int tbn_stem_conv_wgrad(const float* dy, int dy_ld, const float* x_nchw, float* dweight, int n, int h, int w, int cin, int cout,
                        int layout, int mt, int nt, float* workspace, void* stream);

/* ---- the separable audio stem of BNInception_Audio -------------------------------------------------
 * Both stem convolutions of the one-channel spectrogram in one pass, concatenated: x (n, 1, h, w) contiguous, any h, w >= 1;
 * out NHWC (n, oh, ow, 64), oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1, pitch out_ld >= 64, a multiple of 4, out 16-B aligned.
 *   channel c < 32:  sum_t weight[c][t]      * x[2 oy - 1 + t][2 ox]      (three taps along frequency)
 *   channel 32 + c:  sum_t weight[32 + c][t] * x[2 oy][2 ox - 1 + t]      (three taps along time)
 * reads outside the image are zero.  weight / dweight [64][3]: rows 0..31 = conv1_1x3_s2.weight.view(32, 3), rows 32..63 =
 * conv1_3x1_s2.weight.view(32, 3); bias / scale / shift: 64 floats.  Plain fp32 FMAs in tap order (no MFMA: 6 multiply-adds
 * per value, the kernel streams); deterministic.
 * tbn_audio_stem_stat_rows: rows of stat_partial that epilogue 1 writes; 0 for arguments the entries refuse.  Host only.
 * tbn_audio_stem_fwd: epilogue / flags / bias / scale / shift / stat_partial as tbn_conv2d_fwd: 0 = + bias (NULL: none;
 *   flag 2: ReLU, no other flag), 1 = bias-free output plus stat_partial[(i*2 + {0,1}) * 64 + ch] = sum | sum of squares over
 *   row chunk i, the layout tbn_bn_fwd_batch reads, 2 = relu(acc * scale + shift).
 * tbn_audio_stem_wgrad: dweight from dy (n, oh, ow, 64) with pitch dy_ld (as out_ld); workspace of
 *   tbn_audio_stem_wgrad_workspace_floats floats (one [64][3] partial per workgroup, summed in fixed order in fp64; no
 *   atomics).  No data gradient (the input is a spectrogram) and no bias gradient (a BatchNorm follows) are formed.
 * replaces: the forward / weight gradient of conv1_1x3_s2 = nn.Conv2d(1, 32, (3, 1), stride 2, padding (1, 0)) and
 * conv1_3x1_s2 = nn.Conv2d(1, 32, (1, 3), stride 2, padding (0, 1)) with the torch.cat behind them
 * (bn_inception_audio.py:11-13, 16-18, 408, 411, 415; cuDNN there). */
int tbn_audio_stem_stat_rows(int n, int h, int w);
int tbn_audio_stem_fwd(const float* x, const float* weight, const float* bias, float* out, int out_ld, int n, int h, int w,
                       int epilogue, int flags, const float* scale, const float* shift, float* stat_partial, void* stream);
size_t tbn_audio_stem_wgrad_workspace_floats(int n, int h, int w);
int tbn_audio_stem_wgrad(const float* dy, int dy_ld, const float* x, float* dweight, int n, int h, int w, float* workspace,
                         void* stream);

/* ---- the operators of the VGG backbones beside the 3x3 convolutions and the Linear layers -----------
 * All fp32, deterministic (no atomics); every entry checks its arguments before any launch.
 *
 * The first convolution, 3x3 / stride 1 / pad 1 straight from the frames: x (n, cin, h, w) contiguous NCHW, cin in 1..16, any
 * h, w >= 1 with n * h * w < 2^27; weight / dweight [cout][3][3][cin] with cout = 64 (anything else: TBN_ERR_UNSUPPORTED);
 * out NHWC (n, h, w, 64), pitch out_ld >= 64, a multiple of 4, out 16-B aligned.  Reads outside the image are zero.  Plain
 * fp32 FMAs in the fixed order filter row, input channel, filter column (no MFMA: 9 cin multiply-adds per value against
 * 256 B written per pixel, the kernel streams).
 * tbn_conv3_first_stat_rows: rows of stat_partial that epilogue 1 writes; 0 for arguments the entries refuse.  Host only.
 * tbn_conv3_first_fwd: epilogue / flags / bias / scale / shift / stat_partial as tbn_audio_stem_fwd: 0 = + bias (NULL: none;
 *   flag 2: ReLU, no other flag), 1 = bias-free output plus stat_partial[(i*2 + {0,1}) * 64 + ch] = sum | sum of squares over
 *   row chunk i, the layout tbn_bn_fwd_batch reads, 2 = relu(acc * scale + shift).
 * tbn_conv3_first_wgrad: dweight from dy (n, h, w, 64) with pitch dy_ld (as out_ld); workspace of
 *   tbn_conv3_first_wgrad_workspace_floats floats (one [64][3][3][cin] partial per workgroup, summed in fixed order in fp64).
 *   No data gradient is formed: the input is frames.
 * replaces: the forward / weight gradient of features[0] = nn.Conv2d(cin, 64, 3, padding 1) of torchvision's vgg11 / vgg16
 * (_bn) as core/models/vgg.py:15-41 builds and replaces it (cuDNN there). */
int tbn_conv3_first_stat_rows(int n, int cin, int h, int w);
int tbn_conv3_first_fwd(const float* x, const float* weight, const float* bias, float* out, int out_ld, int n, int h, int w,
                        int cin, int cout, int epilogue, int flags, const float* scale, const float* shift,
                        float* stat_partial, void* stream);
size_t tbn_conv3_first_wgrad_workspace_floats(int n, int cin, int h, int w);
int tbn_conv3_first_wgrad(const float* dy, int dy_ld, const float* x, float* dweight, int n, int h, int w, int cin, int cout,
                          float* workspace, void* stream);
/* nn.MaxPool2d(2, 2) on NHWC (n, h, w, c): c a multiple of 4, h, w >= 2, floor mode -- out (n, h / 2, w / 2, c), a trailing
 * odd row / column is dropped.  Pitches are multiples of 4 and >= c, the float tensors 16-B aligned.  argmax (n, h / 2,
 * w / 2, c) uint8, unpitched, 4-B aligned, may be NULL in the forward: the tap 2 * dy + dx of the first maximum in scan order
 * (a NaN wins), the rule of tbn_maxpool3_fwd.
 * tbn_maxpool2_bwd writes EVERY element of din (n, h, w, c): dout where the element is its window's argmax, zero elsewhere
 * and in a dropped row / column; accumulate != 0 adds to din instead.  z (NULL, or the pool's own forward input with pitch
 * z_ld): the value is additionally gated by z > 0 -- the pool's backward and the ReLU mask of the layer in front of it in one
 * pass; the result equals tbn_maxpool2_bwd without z followed by tbn_relu_mask_bwd on z.
 * replaces: the nn.MaxPool2d(kernel_size=2, stride=2) layers of torchvision's vgg features (core/models/vgg.py:15-41). */
int tbn_maxpool2_fwd(const float* in, int in_ld, float* out, int out_ld, uint8_t* argmax, int n, int h, int w, int c,
                     void* stream);
int tbn_maxpool2_bwd(const float* dout, int dout_ld, const uint8_t* argmax, const float* z, int z_ld, float* din, int din_ld,
                     int n, int h, int w, int c, int accumulate, void* stream);
/* nn.AdaptiveAvgPool2d((7, 7)) + torch.flatten(x, 1): in NHWC (n, h, w, c) with pitch in_ld (a multiple of 4, >= c), c a
 * multiple of 4, any h, w >= 1; out (n, c * 49) contiguous in the order of the flattened NCHW tensor, column = ch * 49 +
 * oy * 7 + ox, so classifier.0.weight of a checkpoint is used as it is.  Windows are PyTorch's: bin i of an axis of length L
 * covers [floor(i L / 7), ceil((i + 1) L / 7)) -- replication for L < 7, overlap where 7 does not divide L.  A window is
 * summed in fp32 in row order and divided by its area; at h = w = 7 the forward is the transposition, bit for bit.
 * tbn_adaptive_avgpool7_bwd: din NHWC (pitch din_ld) = for every element the sum of dout / area over the windows that
 * contain it (summed in fp64, rounded once); accumulate != 0 adds to din instead.
 * replaces: avgpool + flatten of torchvision's VGG.forward (core/models/vgg.py:15-41). */
int tbn_adaptive_avgpool7_fwd(const float* in, int in_ld, float* out, int n, int h, int w, int c, void* stream);
int tbn_adaptive_avgpool7_bwd(const float* dout, float* din, int din_ld, int n, int h, int w, int c, int accumulate,
                              void* stream);

/* nn.Linear / nn.Conv1d(k=1) (model.py:337-386 Fusion/Classifier, model.py:62-67 pe.1, the MHA
 * projections attention.py:48-57): out[m][n] = x[m][:] . w[n][:] + bias[n].  k % 32 == 0. */
int tbn_linear_fwd(const float* x, int x_ld, const float* w, const float* bias, float* out, int out_ld, int m, int k,
                   int n, int relu, void* stream);
/* dx[m][k] (+)= dy[m][:] . w[:][k]; n % 32 == 0; workspace n*k floats */
int tbn_linear_dgrad(const float* dy, int dy_ld, const float* w, float* dx, int dx_ld, int m, int k, int n,
                     int accumulate, float* workspace, void* stream);
/* dw[n][k] = dy^T x ; dbias[n] = column sums of dy (dbias may be NULL); n % 4 == 0, k % 4 == 0 */
size_t tbn_linear_wgrad_workspace_floats(int m, int k, int n);
int tbn_linear_wgrad(const float* dy, int dy_ld, const float* x, int x_ld, float* dw, float* dbias, int m, int k,
                     int n, float* workspace, void* stream);

/* training-mode BatchNorm2d + ReLU on NHWC (p pixels x c channels), standalone form.
 * replaces nn.BatchNorm2d(...).train() + ReLU(inplace).  Workspace floats: tbn_bn_workspace_floats(). */
size_t tbn_bn_workspace_floats(int p, int c);
int tbn_bn_relu_train_fwd(const float* y, int p, int c, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, float* save_mean, float* save_rstd,
                          float* scale, float* shift, float* z, int z_ld, float* workspace, void* stream);
int tbn_bn_relu_train_bwd(const float* dz, int dz_ld, const float* y, int p, int c, const float* save_mean,
                          const float* save_rstd, const float* scale, const float* shift, float* dy, float* dgamma,
                          float* dbeta, float* workspace, void* stream);

/* training-mode BatchNorm2d + ReLU + MaxPool2d(3, stride, pad, ceil_mode) in one pass over y: z = relu(bn(y)) is pooled in
 * registers and never written (what the backbone does for conv1_7x7_s2 -> pool1 and conv2_3x3 -> pool2, the two largest
 * tensors of the network); the backward gathers dz from (dpooled, argmax) on the fly.  y: (n,h,w,c) NHWC, pooled:
 * (n,oh,ow,c) with pitch pooled_ld, argmax: n*oh*ow*c bytes.  Workspace: tbn_bn_workspace_floats(n*h*w, c).
 * replaces: BatchNorm2d.train() + ReLU + MaxPool2d of bn_inception_audio.py:21-23,28-34. */
int tbn_bn_relu_maxpool_train_fwd(const float* y, int n, int h, int w, int c, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                                  float* save_rstd, float* scale, float* shift, float* pooled, int pooled_ld,
                                  uint8_t* argmax, int oh, int ow, int stride, int pad, float* workspace, void* stream);
int tbn_bn_relu_maxpool_train_bwd(const float* dpooled, int dpooled_ld, const uint8_t* argmax, const float* y, int n, int h,
                                  int w, int c, int oh, int ow, int stride, int pad, const float* save_mean,
                                  const float* save_rstd, const float* scale, const float* shift, float* dy,
                                  float* dgamma, float* dbeta, float* workspace, void* stream);

/* ---- the batched training BN of the backbone engine on its own (test / tuning aid) -------------------
 * The launch sequence the engine runs for the BN of every conv but the fused stem pools: statistics partials (from a conv
 * epilogue, or from tbn_bn_stats_partials), then ONE finalize + ONE apply launch for up to 4 independent members (forward),
 * ONE reduce + ONE finalize + ONE apply launch (backward).  Ask tbn_capabilities() & TBN_CAP_BN_BATCH_OPS.
 * Every member: p rows x c channels, c a multiple of 4 in 4..1024; y has pitch y_ld >= c; all pitches and column offsets
 * are multiples of 4 floats and every pointer is 16-B aligned.
 * tbn_bn_stats_partials: partial[(i*2 + {0,1}) * c + ch] = sum | sum of squares of y over row chunk i; *nparts = chunks
 *   written (partial: tbn_bn_workspace_floats floats are enough).
 * tbn_bn_fwd_batch: statistics from partial[(i*2 + {0,1}) * pld + ch], i < nparts (pld >= c); writes save_mean, save_rstd,
 *   scale = gamma * rstd, shift = beta - mean * scale and z = relu(y * scale + shift) into 1..3 column segments
 *   (segment s takes the channels from seg[s].col_begin up to the next segment's col_begin; seg[s].ptr is the address of
 *   channel col_begin of row 0, seg[0].col_begin = 0).  running_mean may be NULL (running_var is then not touched either);
 *   otherwise running_mean takes mean + conv_bias (conv_bias may be NULL: y is the bias-free conv output, the reference's
 *   BN sees conv + bias) and running_var the unbiased variance, both with `momentum`.
 * tbn_bn_bwd_batch: dy = d loss / d y from dz = d loss / d z, written with pitch y_ld (dy may be y itself).  partial is
 *   scratch of tbn_bn_bwd_partial_floats floats -- or, with ext_parts > 0, holds ext_parts rows
 *   partial[(i*2 + {0,1}) * c + ch] = sum g | sum g * xhat (g = dz where z > 0, xhat = (y - mean) * rstd) made by the caller,
 *   as a data-gradient epilogue does (tbn_conv_desc.red); no reduce pass runs for that member.  coef: scratch of 3 c floats.
 *   dgamma / dbeta / dbias may be NULL; dbias receives zeros (a constant added in front of a batch-statistics BN has no
 *   gradient).
 * A batch gives every member the bits it gets as a batch of one.  Deterministic.
 * replaces: nn.BatchNorm2d(...).train() + ReLU(inplace) of bn_inception_audio.py:24-401, forward and backward. */
typedef struct {
  float* ptr;             /* address of channel col_begin of row 0 */
  int ld;                 /* floats between rows */
  int col_begin;          /* first channel that goes through this segment */
} tbn_bn_seg;
typedef struct {
  const float* y;
  int y_ld;
  int p, c;
  const float* partial;
  int pld, nparts;
  const float* gamma;
  const float* beta;
  const float* conv_bias;     /* may be NULL */
  float* running_mean;        /* may be NULL, with running_var */
  float* running_var;
  float* save_mean;
  float* save_rstd;
  float* scale;
  float* shift;
  tbn_bn_seg seg[3];          /* destinations of z */
  int nseg;
} tbn_bn_fwd_desc;
typedef struct {
  tbn_bn_seg dz[3];           /* gradient with respect to z, by column segment (read only) */
  int nseg;
  const float* y;
  float* dy;
  int y_ld;
  int p, c;
  const float* scale;         /* the four per-channel vectors tbn_bn_fwd_batch wrote */
  const float* shift;
  const float* mean;
  const float* rstd;
  float* partial;
  int ext_parts;              /* 0: partial is scratch; > 0: rows of caller-made partials */
  float* coef;
  float* dgamma;              /* may be NULL */
  float* dbeta;               /* may be NULL */
  float* dbias;               /* may be NULL */
} tbn_bn_bwd_desc;
int tbn_bn_stats_partials(const float* y, int y_ld, int p, int c, float* partial, int* nparts, void* stream);
int tbn_bn_fwd_batch(const tbn_bn_fwd_desc* members, int n, float momentum, float eps, void* stream);
size_t tbn_bn_bwd_partial_floats(int p, int c);   /* 0 for a shape the entries refuse */
int tbn_bn_bwd_batch(const tbn_bn_bwd_desc* members, int n, void* stream);

/* ---- BatchNorm with an optional residual and an optional ReLU: the join of a residual block ------------
 * z = act(y * scale + shift + res), act = ReLU (relu = 1) or identity (relu = 0), res may be NULL.  p rows x c channels,
 * c a multiple of 4 in 4..2048 (the batched entries above stop at 1024; ResNet-50/101/152 join at 2048); every tensor has its
 * own pitch (floats between rows, a multiple of 4 and at least c) and every pointer is 16-B aligned.  No capability bit and no
 * version step go with these entries (the low 16 bits of tbn_version() name the plan-cache format): callers that bind the
 * C-ABI directly detect them by symbol (dlsym of tbn_bn_res_fwd).
 * tbn_bn_res_apply: the apply pass alone with caller-given scale / shift -- the eval-mode join (scale / shift folded from the
 *   running statistics) behind a tbn_conv2d_fwd with epilogue 0 and a NULL bias.  z may be y itself.
 * tbn_bn_res_fwd: training mode.  y is the bias-free conv output, partial[(i*2 + {0,1}) * pld + ch], i < nparts, its sum |
 *   sum of squares per row chunk -- what tbn_conv2d_fwd epilogue 1 and tbn_bn_stats_partials write and tbn_bn_fwd_batch
 *   reads.  Writes save_mean, save_rstd, scale = gamma * rstd, shift = beta - mean * scale, updates running_mean /
 *   running_var (NULL: not touched) with `momentum` and the unbiased variance, then applies.  z may be y itself.
 * tbn_bn_res_bwd: with g = relu ? (z > 0 ? dz : 0) : dz -- the mask is read from the forward's STORED output z (NULL with
 *   relu = 0), so it is bit-consistent with the forward whatever was added in front of the ReLU --
 *   dres (+)= g (dres NULL: no residual; accumulate = 1 adds into it, which is how the identity path and conv1's data gradient
 *   meet at a block's input without a separate add), dy = scale * (g - mean_p(g) - xhat * mean_p(g * xhat)) with
 *   xhat = (y - mean) * rstd, i.e. the gradient with respect to y, dgamma = sum g * xhat, dbeta = sum g (either may be NULL).
 *   dy may be y itself.  workspace: tbn_bn_res_bwd_workspace_floats(p, c) floats (0 for a shape the entries refuse).
 * Deterministic (fixed-order fp64 sums of per-workgroup partials, no atomics).
 * replaces: nn.BatchNorm2d + `out += identity` + ReLU of torchvision's BasicBlock / Bottleneck and the ReLU-free
 * nn.BatchNorm2d of their downsample path, forward and backward, which the reference reaches through
 * core/models/resnet.py:15-24. */
int tbn_bn_res_apply(const float* y, int y_ld, int p, int c, const float* scale, const float* shift, const float* res,
                     int res_ld, int relu, float* z, int z_ld, void* stream);
int tbn_bn_res_fwd(const float* y, int y_ld, int p, int c, const float* partial, int pld, int nparts, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                   float* save_mean, float* save_rstd, float* scale, float* shift, const float* res, int res_ld,
                   int relu, float* z, int z_ld, void* stream);
size_t tbn_bn_res_bwd_workspace_floats(int p, int c);
int tbn_bn_res_bwd(const float* dz, int dz_ld, const float* z, int z_ld, const float* y, int y_ld, int p, int c,
                   const float* save_mean, const float* save_rstd, const float* scale, int relu, float* dy, int dy_ld,
                   float* dres, int dres_ld, int accumulate, float* dgamma, float* dbeta, float* workspace,
                   void* stream);

/* pooling (bn_inception_audio.py:21-23,86-88,155-157,394-396; ceil_mode handled by oh/ow) */
int tbn_maxpool3_fwd(const float* in, int in_ld, float* out, int out_ld, uint8_t* argmax, int n, int h, int w, int c,
                     int oh, int ow, int stride, int pad, void* stream);
int tbn_maxpool3_bwd(const float* dout, int dout_ld, const uint8_t* argmax, float* din, int din_ld, int n, int h,
                     int w, int c, int oh, int ow, int stride, int pad, int accumulate, void* stream);
int tbn_avgpool3_fwd(const float* in, int in_ld, float* out, int out_ld, int n, int h, int w, int c, int accumulate,
                     void* stream); /* 3x3 s1 p1 count_include_pad; self-adjoint => also its backward */
/* BNInception.logits override, bn_inception.py:16-35: freq_only=1 -> mean over H only (attended
 * audio, out (n,w,c)); else global mean (out (n,c)) */
int tbn_spatial_mean_fwd(const float* in, int in_ld, float* out, int out_ld, int n, int h, int w, int c,
                         int freq_only, void* stream);
int tbn_spatial_mean_bwd(const float* dout, int dout_ld, float* din, int din_ld, int n, int h, int w, int c,
                         int freq_only, void* stream);

/* ---- mid-level fusion heads ---------------------------------------------------------------- */
/* PositionalEncoding "concat" (attention.py:8-45): out[r][t][0:c]=feat, [c:c+pe_dim]=pe[:,t], zero
 * padded to out_ld. pe is (pe_dim, t) row-major. */
int tbn_pe_concat_fwd(const float* feat, int feat_ld, const float* pe, float* out, int out_ld, int r, int t, int c,
                      int pe_dim, void* stream);
/* nn.GroupNorm(groups, c) over (r, t, c) rows (model.py:62-67 pe.2).  c % groups == 0 and the channels per group
 * c / groups must be 4 * 2^k with k in 0..6 (4, 8, 16, ... 256: a group is a power-of-two run of float4 lanes inside one
 * wave); any c, t >= 1.  Anything else: TBN_ERR_ARG with a message naming groupnorm.  save_mean / save_rstd (r * groups
 * each) are the group mean and 1 / sqrt(var + eps), var = mean of the squared deviations FROM that mean (computed in a pass
 * of its own after the mean, so a large common offset of x costs no accuracy). */
int tbn_groupnorm_fwd(const float* x, float* y, const float* gamma, const float* beta, float* save_mean,
                      float* save_rstd, int r, int t, int c, int groups, float eps, void* stream);
/* dgamma_part / dbeta_part: (r, c) per-sample partials, reduce with tbn_colsum */
int tbn_groupnorm_bwd(const float* dy, const float* x, const float* gamma, const float* save_mean,
                      const float* save_rstd, float* dx, float* dgamma_part, float* dbeta_part, int r, int t, int c,
                      int groups, void* stream);
int tbn_colsum(const float* x, int x_ld, float* out, int rows, int cols, void* stream);
/* torch.nn.MultiheadAttention core for L_q = 1 (attention.py:48-57, model.py:231-237), one wave per
 * (sample, head): q (r,e) projected query (unscaled; scores = scale * q.k, scale = head_dim^-0.5);
 * kv (r,t,2e) = [k | v] projections.  drop_mask (r,heads,t) holds 0 or 1/(1-p), NULL in eval.
 * Outputs: ctx (r,e) (input of out_proj); probs, 2*r*heads*t floats = pre-dropout softmax (saved
 * for backward) followed by the post-dropout weights; avg_w (r,t) head-mean of the post-dropout
 * weights (what nn.MultiheadAttention returns).
 * Limits (forward and backward): 1 <= t <= 32 keys (the scores of a (sample, head) live in registers), e % heads == 0 and
 * head_dim = e / heads a multiple of 4 (any size: lanes walk it 256 floats at a time); anything else returns TBN_ERR_ARG
 * with a message naming mha_q1 -- core/models/attention.py sends such calls down its general path instead.
 * tbn_mha_q1_bwd: davg_w may be NULL (no gradient through the returned weights); dctx may not. */
int tbn_mha_q1_fwd(const float* q, const float* kv, const float* drop_mask, float* ctx, float* probs, float* avg_w,
                   int r, int t, int e, int heads, float scale, void* stream);
int tbn_mha_q1_bwd(const float* dctx, const float* davg_w, const float* q, const float* kv, const float* probs,
                   const float* drop_mask, float* dq, float* dkv, int r, int t, int e, int heads, float scale,
                   void* stream);
/* torch.nn.MultiheadAttention core, general shape (attention.py:48-57): l queries and t keys per sample, key and value
 * projected separately, any head_dim.  One wave per (sample, head, query); the scores of a query live in LDS.
 * q (l*r rows, row i*r + s) projected queries, unscaled (scores = scale * q.k, scale = head_dim^-0.5); k, v (t*r rows, row
 * j*r + s) projected keys / values.  Every matrix has its own leading dimension (floats between rows, >= e) and needs
 * neither contiguous nor 16-byte aligned rows: k and v may be two column ranges of one buffer.  drop_mask (r,heads,l,t)
 * holds 0 or 1/(1-p), NULL in eval.
 * Outputs: ctx (l*r rows, ctx_ld; input of out_proj); probs, 2*r*heads*l*t floats = pre-dropout softmax (r,heads,l,t),
 * saved for backward, followed by the post-dropout weights; avg_w (r,l,t) head mean of the post-dropout weights.
 * tbn_mha_bwd: dctx (l*r rows, dctx_ld); davg_w (r,l,t) may be NULL; dscores is caller-owned scratch of r*heads*l*t
 * floats (the score gradients, written by the first launch and read by the second).  dq / dk / dv are written, not
 * accumulated; the sum over the l queries into dk / dv runs inside one thread in query order (no atomics: same bits every
 * run).
 * Limits: l >= 1, 1 <= t <= 1024, r >= 1, heads >= 1, e % heads == 0 (any head_dim >= 1), r*heads*l*t < 2^31, leading
 * dimensions >= e; anything else, or a NULL required pointer, returns TBN_ERR_ARG with a message naming mha and writes
 * nothing. */
int tbn_mha_fwd(const float* q, int q_ld, const float* k, int k_ld, const float* v, int v_ld, const float* drop_mask,
                float* ctx, int ctx_ld, float* probs, float* avg_w, int l, int t, int r, int e, int heads, float scale,
                void* stream);
int tbn_mha_bwd(const float* dctx, int dctx_ld, const float* davg_w, const float* q, int q_ld, const float* k, int k_ld,
                const float* v, int v_ld, const float* probs, const float* drop_mask, float* dscores, float* dq, int dq_ld,
                float* dk, int dk_ld, float* dv, int dv_ld, int l, int t, int r, int e, int heads, float scale,
                void* stream);
/* Attention weights of the learnt single-modality and prototype variants (attention.py:60-91 UniModalAttention,
 * :94-145 PrototypeAttention) in one launch per direction -- F.softmax / F.gumbel_softmax plus the prototype mix.
 * logits (r,k) with leading dimension logits_ld; noise (r,k) contiguous Exp(1) samples or NULL; protos (k,t) row-major or
 * NULL.  g = -log(noise) (0 without noise); soft = softmax((logits + g) / tau) over k;
 * m = hard ? (onehot(argmax soft) - soft) + soft : soft, evaluated in that fp32 order (the value
 * F.gumbel_softmax(hard=True) returns), the first index winning ties; w = protos ? m @ protos : m.
 * Writes soft (r,k) (saved for backward) and w (r, protos ? t : k), both contiguous.
 * tbn_attn_weights_bwd is F.gumbel_softmax's straight-through rule (the gradient flows through soft only):
 * dm = protos ? dw @ protos^T : dw; dlogits = soft * (dm - sum_k(dm * soft)) / tau, dlogits (r,k) contiguous.
 * Limits: r >= 1, 1 <= k <= 1024, 1 <= t <= 1024 (t is ignored without protos), tau > 0; anything else, or a NULL required
 * pointer, returns TBN_ERR_ARG with a message naming attn_weights and writes nothing.  One wave per row. */
int tbn_attn_weights_fwd(const float* logits, int logits_ld, const float* noise, float tau, int hard, const float* protos,
                         float* soft, float* w, int r, int k, int t, void* stream);
int tbn_attn_weights_bwd(const float* dw, const float* soft, const float* protos, float tau, float* dlogits, int r, int k,
                         int t, void* stream);
/* The three loss terms that train the attention weights (reference core/models/model.py:299-332 and
 * core/models/contrast_loss.py:4-25: the prior criterion, ContrastLoss and the Categorical entropy with its threshold
 * switch-off) over w (r,t) with leading dimension w_ld and prior (r,t) with leading dimension prior_ld.
 *   prior term, prior_kind TBN_ATTN_PRIOR_*: NONE: off.  KL: p > 0 ? p * (log p - log(w + 1e-7)) : 0 (nn.KLDivLoss,
 *     log_target False, on log(w + 1e-7)).  MSE: (w - p)^2.  SMOOTHL1 (beta 1): |d| < 1 ? 0.5 d^2 : |d| - 0.5, d = w - p.
 *     prior_reduction TBN_ATTN_RED_*: SUM, MEAN (/ (r*t)) or BATCHMEAN (/ r, KL only: MSE / SMOOTHL1 with it are refused, as
 *     torch refuses them).
 *   contrast term (use_contrast): row term sum_t (x >= contrast_thresh ? -x : x), compared in fp32; the loss is the mean
 *     over rows (ContrastLoss with reduction mean or batchmean; its unreduced "sum" vector is not covered).
 *   entropy term (use_entropy): q = x + 1e-6, p = q / sum_t q, row term -sum_t p * log(clamp(p, eps, 1 - eps)) with
 *     eps = FLT_EPSILON (torch.distributions.Categorical(probs=q).entropy()); the loss is the mean over rows.
 *   x = w.  With log_rebind != 0 (KL only) x = log(w + 1e-7) instead: model.py:316-317 rebinds `wts` to the logarithm for
 *     the kl prior and :320-324 hand that tensor to the contrast and entropy terms; the gradient is chained through
 *     dx/dw = 1 / (w + 1e-7).
 *   total = prior_mult * prior + contrast_mult * contrast + e * entropy, e = entropy_mult except e = 0 when
 *     training && entropy_mult > 0 && entropy < entropy_thresh -- decided on the device, no host read.
 * tbn_attn_reg_fwd writes losses[4] = {prior, contrast, entropy, total} (device; a term that is off is 0) and rowterms
 * (scratch, 3*r floats: the row terms, then summed in a fixed order by one wave).  tbn_attn_reg_bwd is ONE launch: it
 * recomputes the row sums, reads the saved losses[2] to repeat the switch-off decision and the four upstream gradients
 * up[4] = d/d{prior, contrast, entropy, total} from device memory, and writes
 *   dw = (up[0] + up[3]*prior_mult) * dPrior + (up[1] + up[3]*contrast_mult) * dContrast + (up[2] + up[3]*e) * dEntropy,
 * dEntropy through the normalisation (dH/dq_j = -(log p_j + H_row) / sum q inside the clamp, the clamp's zero-gradient
 * region honoured), rows scaled by 1/r.  One wave per row, lanes stride over t (any t >= 1); no atomics: the same input
 * gives the same bits.  A NULL pointer (prior may be NULL with TBN_ATTN_PRIOR_NONE), r < 1, t < 1, a leading dimension
 * < t, an unknown kind or reduction, a prior kind without prior, MSE / SMOOTHL1 with BATCHMEAN or log_rebind without KL
 * returns TBN_ERR_ARG with a message naming attn_reg before any launch. */
#define TBN_ATTN_PRIOR_NONE 0
#define TBN_ATTN_PRIOR_KL 1
#define TBN_ATTN_PRIOR_MSE 2
#define TBN_ATTN_PRIOR_SMOOTHL1 3
#define TBN_ATTN_RED_SUM 0
#define TBN_ATTN_RED_MEAN 1
#define TBN_ATTN_RED_BATCHMEAN 2
int tbn_attn_reg_fwd(const float* w, int w_ld, const float* prior, int prior_ld, int r, int t, int prior_kind,
                     int prior_reduction, int use_contrast, float contrast_thresh, int use_entropy, float prior_mult,
                     float contrast_mult, float entropy_mult, int training, float entropy_thresh, int log_rebind,
                     float* rowterms, float* losses, void* stream);
int tbn_attn_reg_bwd(const float* up, const float* w, int w_ld, const float* prior, int prior_ld, const float* losses, int r,
                     int t, int prior_kind, int prior_reduction, int use_contrast, float contrast_thresh, int use_entropy,
                     float prior_mult, float contrast_mult, float entropy_mult, int training, float entropy_thresh,
                     int log_rebind, float* dw, int dw_ld, void* stream);
/* fixed attention (model.py:224-228): out[r][c] = sum_t feat[r][t][c] * w[r][t] */
int tbn_weighted_sum_fwd(const float* feat, const float* w, float* out, int out_ld, int r, int t, int c, void* stream);
int tbn_weighted_sum_bwd(const float* dout, int dout_ld, const float* w, float* dfeat, int r, int t, int c,
                         void* stream);
/* temporal consensus (model.py:178-203): out[b][c] = mean_n x[b*n+i][c] */
int tbn_segment_mean_fwd(const float* x, float* out, int b, int n, int c, void* stream);
int tbn_segment_mean_bwd(const float* dout, float* dx, int b, int n, int c, void* stream);
/* nn.Dropout(p) of the fusion layer (reference model.py:352-362) from a caller-drawn uniform tensor `rnd` in [0, 1):
 * mask = rnd >= p ? 1 / (1 - p) : 0, y = x * mask, both written (the mask is what backward multiplies by: tbn_mul_mask) */
int tbn_dropout_fwd(const float* x, const float* rnd, float p, float* y, float* mask, size_t count, void* stream);
/* The cross-entropy losses of up to 4 classification heads that share ONE score matrix (reference model.py:272-279: one
 * nn.CrossEntropyLoss(mean) per class key, `verb` and `noun`): head h owns columns [col0[h], col0[h] + ncls[h]) of
 * scores (batch, ld), labels[h] = int64[batch] device pointers (host array of them).  A label of -100 (the criterion's
 * default ignore_index) takes its row out of loss, gradient and mean; any other label outside [0, ncls[h]) gives NaN.
 * Writes loss[h] (device, mean over the rows not ignored, fixed summation order), rowloss (scratch, num_heads * batch floats) and dscores (batch, ld) =
 * d(sum_h loss[h]) / d(scores) for the heads' columns (other columns untouched).  tbn_ce_heads_bwd scales a head's columns
 * of dscores by upstream[h] (device) into `out` (may alias dscores): the backward for arbitrary per-head weights. */
int tbn_ce_heads_fwd(const float* scores, int ld, int batch, int num_heads, const int* col0, const int* ncls,
                     const long long* const* labels, float* rowloss, float* loss, float* dscores, void* stream);
int tbn_ce_heads_bwd(const float* dscores, int ld, int batch, int num_heads, const int* col0, const int* ncls,
                     const float* upstream, float* out, void* stream);
/* y = x * mask (dropout with a caller-generated keep/scale mask); in place allowed */
int tbn_mul_mask(const float* x, const float* mask, float* y, size_t count, void* stream);
/* dx = dy * [y > 0] (* mask if non-NULL): backward of Linear->ReLU->Dropout (model.py:337-362) */
int tbn_relu_mask_bwd(const float* dy, const float* y, const float* mask, float* dx, size_t count, void* stream);

/* ---- spectrogram --------------------------------------------------------------------------- */
/* log-power STFT of reference core/dataset/dataset.py:461-495 (librosa.stft n_fft=511, hop=120,
 * win=240 hann, centre, zero pad): wave (nseg, len) -> spec (nseg, 256, 1+(len-1)/120).
 * twiddle: tbn_stft_twiddle_floats() floats filled by tbn_stft_make_twiddle() (host fp64 -> fp32). */
size_t tbn_stft_twiddle_floats(void);
int tbn_stft_make_twiddle(float* host_buffer);
int tbn_stft_logpower(const float* wave, int nseg, int len, const float* twiddle, float* spec, float eps,
                      void* stream);
/* The same STFT kernel with the audio window cut inside the launch (reference core/dataset/dataset.py:421-459,
 * `_get_audio_segment`: `sample = aud_sample[start : start + length]`, no copy here) and a choice of representation
 * (dataset.py:461-510, `_get_spectrogram`).  Exactly one of `window_ptrs` / `wave` is non-NULL:
 *   window_ptrs  DEVICE array of nseg device pointers, the first sample of each window inside its (untrimmed) clip; any
 *                4-byte alignment.  Every window [ptr, ptr + len) must lie inside its clip -- the caller checks that, the
 *                kernel reads nothing else: the centre padding in front of and behind a window is zeros from the hardware
 *                range check, never the clip's neighbouring audio (librosa pads the trimmed sample);
 *   wave         a contiguous (nseg, len) batch, i.e. window s starts at wave + s * len (what tbn_stft_logpower takes).
 * mode TBN_STFT_LOGPOWER: out (nseg, 256, W) = log(|X|^2 + eps), W = 1 + (len - 1) / 120, bit-identical to
 *   tbn_stft_logpower on the same samples; one launch; mel_basis / power are not read.
 * mode TBN_STFT_LOGMEL (dataset.py:496-506, librosa melspectrogram + power_to_db(ref = np.max)): out (nseg, 128, W) dB =
 *   10 log10(max(1e-10, mel)) - 10 log10(max(1e-10, max of the segment)), floored at -80; mel = mel_basis (128 x 256 floats
 *   on the device, librosa.filters.mel) . |X|^2.  Two launches (the STFT writes |X|^2 into `power`, nseg * 256 * W floats
 *   of workspace; one workgroup per segment projects, reduces the maximum in a fixed order and converts); eps is not used.
 * The profiler (tbn_profile_*) counts these launches (stft_logpower_kernel<log|power>, mel_db_kernel). */
#define TBN_STFT_LOGPOWER 0
#define TBN_STFT_LOGMEL 1
int tbn_stft_windows(const float* const* window_ptrs, const float* wave, int nseg, int len, const float* twiddle,
                     float* out, float eps, int mode, const float* mel_basis, float* power, void* stream);
/* The STFT at any sampling rate (reference core/dataset/dataset.py:461-510: window = int(round(10 ms * rate)), hop =
 * int(round(5 ms * rate)), n_fft = 511 at every rate): periodic Hann(win) centred in the 511 taps (lpad = (511 - win) / 2),
 * the signal zero-padded by 255 on both sides, so tap j of frame t reads sample t * hop - win / 2 + j, and
 * W = 1 + (len - 1) / hop.  8 <= win <= 511 (librosa refuses win_length > n_fft), 1 <= hop <= win; anything else is
 * TBN_ERR_ARG before any launch.  A kernel of its own: tbn_stft_logpower / tbn_stft_windows stay the (240, 120) path.
 *   tbn_stft_rate_twiddle_floats(win)  2 * ceil(win / 8) * 256 * 8 floats (0 outside the domain);
 *   tbn_stft_rate_make_twiddle(win, host_buffer)  host, fp64 -> fp32, phase ((j + lpad) * k) mod 511 reduced in integers,
 *     layout [cos | -sin][tap / 8][bin][tap % 8] with the taps rounded up to whole groups of 8, the padding taps exact
 *     zeros; win = 240 gives tbn_stft_make_twiddle's table bit for bit;
 *   tbn_stft_rate_windows  the contract of tbn_stft_windows (a window table or a contiguous batch, both modes, the same
 *     mel / dB kernel) with `twiddle` = the table of `win` on the device.  The profiler counts stft_rate_kernel<log|power>
 *     (4 * 256 * win * W * nseg FLOP) and mel_db_kernel.  Samples that are not finite propagate into a frame from up to 7
 *     taps behind its window (the tap groups are whole groups of 8; their twiddles are zero). */
size_t tbn_stft_rate_twiddle_floats(int win);
int tbn_stft_rate_make_twiddle(int win, float* host_buffer);
int tbn_stft_rate_windows(const float* const* window_ptrs, const float* wave, int nseg, int len, int win, int hop,
                          const float* twiddle, float* out, float eps, int mode, const float* mel_basis, float* power,
                          void* stream);
/* prior_type "loud" of reference core/dataset/dataset.py:534-575 (`_get_attn_weights`) for nseg spectrograms (nseg, F, W) on
 * the device, one launch, one wave per segment: the maxima of the W / T full blocks of T frames over all F rows (a partial
 * last block is ignored), their arg-max `loc` (ties: the highest block index), then out (nseg, T) = the Gaussian `gauss`
 * (T device floats, cv2.getGaussianKernel(T, 1) rounded to float32) -- as it is when loc > T or |loc - T/2| <= 2, else rolled
 * by loc - T/2 with its minimum before index loc - 4 (if loc - 4 > 0) and from loc + 4 on (if loc + 4 < T).  A selection
 * among the T values and their minimum, no arithmetic: bit-equal to the host function.  W >= T, W <= 4096. */
int tbn_attn_prior_loud(const float* spec, int nseg, int F, int W, int T, const float* gauss, float* out, void* stream);

/* ---- audio files: decode, downmix and resample ------------------------------------------------ */
/* The waveform read of reference core/dataset/dataset.py:401-414 and preprocessing/create_audio_pickle.py:47-49,
 * librosa.load(path, sr, mono=True), for the interleaved little-endian PCM bytes of a file's data chunk on the device:
 *   decode    u8 (b - 128) / 128, s16 / 32768, s24 / 8388608, s32 / 2147483648, f32 as is (libsndfile's float32);
 *   downmix   the float32 sum of the channels in channel order, divided by the channel count (librosa.to_mono);
 *   resample  only when sr_orig != sr_new: resampy's `kaiser_best` windowed sinc (64 zero crossings, 512 table samples per
 *             crossing, rolloff 0.9475937167399596, Kaiser beta 14.769656459379492, linear interpolation in the table,
 *             step = int(min(1, sr_new / sr_orig) * 512) truncated as resampy truncates it, no gain correction), with the
 *             position of output t taken EXACTLY (t * sr_orig / sr_new in 64-bit integers) where resampy accumulates a
 *             floating-point time register; taps outside the clip are dropped;
 *   length    out_len = ceil(frames * sr_new / sr_orig) (librosa's fix_length): the at most one sample past
 *             floor(frames * sr_new / sr_orig) is exactly 0.
 * The filter weights depend on t only through t mod phases: a bank of `phases` rows of `taps` float32 weights, laid out
 * [tap][phase], computed on the host in float64 (Bessel I0 by its series) and rounded.  The two host entries below make no
 * HIP call and need no GPU: the geometry query returns taps = 2 * ceil(32769 / step), phases = sr_new / gcd and
 * floats = taps * phases (all 0 when sr_orig == sr_new: no bank), or TBN_ERR_UNSUPPORTED with a message when the bank would
 * pass 64 MiB; the builder fills host_buffer, whose size `floats` must be the geometry's.  The caller copies the bank to the
 * device.  The filter constants are restated from resampy 0.2.2 and were not checked against the library.
 * The launch entry reads pcm (pcm_bytes = frames * channels * sample width, 4-byte aligned) and writes out (out_len floats)
 * in ONE launch (profiler keys audio_load_kernel<uniform> for one phase, audio_load_kernel<phases> otherwise,
 * audio_decode_kernel when sr_orig == sr_new, where bank may be NULL).  Everything is validated on the host before the
 * launch: the format code, 1..8 channels, frames >= 1, pcm_bytes, out_len, 64-bit products, the bank pointer (TBN_ERR_ARG);
 * a ratio whose tile of outputs spans more input than the kernel stages in LDS (down-sampling beyond about 12 : 1) is
 * TBN_ERR_UNSUPPORTED.  The output-tile query is for tests: the seams of the kernel lie at its multiples.
 * There is no capability bit: callers detect the feature by the symbol. */
#define TBN_AUDIO_U8 0
#define TBN_AUDIO_S16 1
#define TBN_AUDIO_S24 2
#define TBN_AUDIO_S32 3
#define TBN_AUDIO_F32 4
int tbn_audio_bank_geometry(int sr_orig, int sr_new, int* taps, int* phases, size_t* floats);
int tbn_audio_make_bank(int sr_orig, int sr_new, float* host_buffer, size_t floats);
int tbn_audio_tile(void);
int tbn_audio_load(const void* pcm, size_t pcm_bytes, long long frames, int channels, int format, int sr_orig, int sr_new,
                   const float* bank, float* out, long long out_len, void* stream);

/* ---- train-step shell and metrics (the steps right after the path) -- */
/* Multi-tensor clip_grad_norm_ + SGD(momentum) of reference core/tools/train.py:82-94,190-202
 * (torch.nn.utils.clip_grad_norm_ norm_type 2; torch.optim.SGD dampening 0, no nesterov).  All tensors of a
 * call ride in one launch (16-byte aligned tensors move 16 B per lane, others 4 B); `momentum` buffers start as zeros (first step
 * m = d, as torch's clone).  Nothing is read back: the clip coefficient stays on the device. */
#define TBN_OPT_MAX_TENSORS 48
typedef struct tbn_opt_tensor {
  void* param;        /* fp32 parameter (may be NULL for the norm / scale entries) */
  const void* grad;   /* fp32 gradient */
  void* momentum;     /* fp32 momentum buffer (NULL when momentum == 0) */
  size_t count;       /* elements */
} tbn_opt_tensor;
/* number of per-workgroup partial sums tbn_opt_sqnorm_partials writes for these tensors */
int tbn_opt_num_partials(const tbn_opt_tensor* tensors, int num_tensors);
/* partials[i] = sum of squares of one 16384-element chunk of the gradients */
int tbn_opt_sqnorm_partials(const tbn_opt_tensor* tensors, int num_tensors, float* partials, void* stream);
/* total_norm[0] = sqrt(sum partials) (fp64, fixed order); coef[0] = min(1, max_norm / (total_norm + 1e-6)) */
int tbn_opt_clip_coef(const float* partials, int num_partials, float max_norm, float* total_norm, float* coef,
                      void* stream);
/* grad *= coef[0] in place (what clip_grad_norm_ leaves behind; skipped when coef == 1) */
int tbn_opt_scale_grads(const tbn_opt_tensor* tensors, int num_tensors, const float* coef, void* stream);
/* d = grad * grad_scale[0] (1 if NULL) + weight_decay * p ; m = momentum * m + d ; p -= lr * m */
int tbn_opt_sgd_step(const tbn_opt_tensor* tensors, int num_tensors, float lr, float momentum, float weight_decay,
                     const float* grad_scale, void* stream);
/* Multi-tensor Adam: torch.optim.Adam(lr, betas, eps, weight_decay) with amsgrad=False, maximize=False and coupled L2
 * decay, all tensors of a call in one launch (layout rules of tbn_opt_sgd_step; 28 B per element).  Per element
 *   d = grad * grad_scale[0] (1 if NULL) + weight_decay * p
 *   m = m + (1 - beta1) * (d - m)
 *   v = beta2 * v + (1 - beta2) * d * d
 *   p = p - step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)
 * The bias correction is PER TENSOR: torch counts `step` per parameter, and a parameter that had no gradient in some
 * iteration (Base_Audio under data.audio.dropout) falls behind the others; the caller forms both factors in double
 * from each tensor's own count.  1 - beta is formed in double from the shortest decimal that rounds to the float
 * argument (0.999f -> 0.999): 1 - 0.999f itself is 1.3e-5 off 1 - 0.999, which exp_avg_sq would carry.
 * exp_avg / exp_avg_sq start as zeros.  count == 0 entries and num_tensors == 0 launch nothing.
 * replaces: core/tools/train.py:202-208 (optim.Adam(model.parameters(), lr, betas=(0.9, 0.999), weight_decay)) */
typedef struct tbn_adam_tensor {
  void* param;          /* fp32 parameter */
  const void* grad;     /* fp32 gradient */
  void* exp_avg;        /* fp32 first moment */
  void* exp_avg_sq;     /* fp32 second moment */
  size_t count;         /* elements */
  float step_size;      /* lr / (1 - beta1^step), step = this tensor's count AFTER the increment */
  float inv_sqrt_bc2;   /* 1 / sqrt(1 - beta2^step) */
} tbn_adam_tensor;
int tbn_opt_adam_step(const tbn_adam_tensor* tensors, int num_tensors, float beta1, float beta2, float eps,
                      float weight_decay, const float* grad_scale, void* stream);
/* Metric._get_correct_score (core/utils/metric.py:137-157): scores (batch, classes) pitch scores_ld, target int64.
 * correct (k, batch) uint8 = [j-th ranked class == target]; pred (k, batch) int64 ranked classes (may be NULL);
 * conf_mat (classes, classes) float, conf_mat[target][top1] += 1 (may be NULL).  Ties rank the lower index first. */
int tbn_topk_correct(const float* scores, int scores_ld, const long long* target, int batch, int classes, int k,
                     unsigned char* correct, long long* pred, float* conf_mat, void* stream);
/* replaces: Metric.set_metrics + Metric._get_correct_score (core/utils/metric.py:50-106,137-157) for a whole batch in
 * ONE launch that the host never waits for.  Per head the rank of the target class in (score descending, class index
 * ascending) order -- the position tbn_topk_correct reports it at; NaN scores never rank -- decides a hit for each k of
 * topk: target in [0, classes), its score not NaN, rank < k.  hits_row is (num_heads + 1, num_topk) int32 and is ADDED
 * to: rows 0..num_heads-1 the heads, row num_heads the samples that hit in EVERY head (the reference's all_class).
 * loss_row[i] = *loss_ptrs[i] (device scalars, copied by the same launch, also when batch == 0). */
typedef struct {
  const float* scores;        /* (batch, classes), pitch scores_ld >= classes */
  int scores_ld, classes;
  const long long* target;    /* (batch,) int64 */
  float* conf_mat;            /* (classes, classes) float or NULL: conf_mat[target][top-1] += 1 */
} tbn_metric_head;
int tbn_metric_update(const tbn_metric_head* heads, int num_heads,      /* 1..4, host array, passed by value into the launch */
                      int batch, const int* topk, int num_topk,          /* host array, 1..8 values, any order, each 1..min classes */
                      const float* const* loss_ptrs, int num_losses,     /* host array of 0..8 DEVICE scalars */
                      int* hits_row,    /* device, (num_heads + 1) * num_topk ints, ADDED to; group num_heads = joint */
                      float* loss_row,  /* device, num_losses floats, written */
                      void* stream);
/* replaces: get_info's five .item() reads per clip and visualize's softmax().topk(5) (core/tools/vis.py:73-84,153-154)
 * for a whole batch in ONE launch that the host never waits for.  Per clip b and head h:
 *   top_idx[b][h][0..k)   the k best classes in (score descending, class index ascending) order -- the order of
 *                         tbn_topk_correct / tbn_metric_update; NaN never ranks; -1 once the rankable classes run out
 *   top_prob[b][h][0..k)  softmax(scores[b]) at those classes, expf(v - max) / sum; a row that holds NaN or +inf gives
 *                         NaN throughout (as torch.softmax), a -inf entry 0, a slot with index -1 NaN
 *   entropy[b]            mean over the rows b*segments .. b*segments+segments-1 of `weights` of
 *                         -sum_t w * logf(w + 1e-6f); any T >= 1
 * Every sum is taken in a fixed order, so two calls on the same inputs agree bit for bit.  batch == 0 launches nothing. */
typedef struct {
  const float* scores;        /* (batch, classes) fp32, pitch scores_ld >= classes */
  int scores_ld, classes;
} tbn_summary_head;
int tbn_clip_summary(const tbn_summary_head* heads, int num_heads,   /* 1..4, host array, passed by value into the launch */
                     int batch, int k,                               /* k in 1..8 and <= every head's classes */
                     const float* weights, int weights_ld,           /* (batch*segments, T) fp32, pitch weights_ld >= T, or NULL */
                     int segments, int T,                            /* segments >= 1 */
                     int* top_idx, float* top_prob,                  /* device, (batch, num_heads, k) each, written */
                     float* entropy,                                 /* device, (batch,), written; NULL iff weights is NULL */
                     void* stream);

/* ---- on-device visual input pipeline (the step right before the path) ---- */
/* MultiScaleCrop / Rescale (cv2.resize INTER_LINEAR, 8-bit fixed point) -> CenterCrop / crop -> RandomHorizontalFlip
 * -> Stack -> ToTensor (/255) -> Normalize of reference core/dataset/transform.py:9-543 as composed by
 * core/utils/create_dataloader.py:19-81, in one pass over the pixels.  frames: (n_img, height, width, channels)
 * uint8 on the device.  The source box (box_*) is resized to resized_w x resized_h (equal sizes: no interpolation),
 * the window (crop_x, crop_y, out_w, out_h) of that is taken, flipped horizontally if `flip`; `stack` consecutive
 * single/multi-channel images form the channels of one sample; out: (n_img/stack, channels*stack, out_h, out_w)
 * fp32 = ((v [/255]) - mean[c % n_stat]) / std[c % n_stat] (n_stat = 0: no normalisation).  The random choices
 * (crop box, flip) are the caller's: same host RNG draws as the reference. */
int tbn_frames_to_tensor(const unsigned char* frames, int n_img, int height, int width, int channels, int box_x,
                         int box_y, int box_w, int box_h, int resized_w, int resized_h, int crop_x, int crop_y,
                         int out_w, int out_h, int flip, int stack, const float* mean, const float* std_dev,
                         int n_stat, int div255, float* out, void* stream);
/* The same pass with FixedCrop (reference core/dataset/transform.py:106-179, the multi-crop test-time augmentation) in
 * place of the single window, followed by Stack (transform.py:415-461).  crop_x / crop_y: HOST arrays of n_crops window
 * origins inside the resized box, copied into the launch arguments; 1 <= n_crops <= TBN_FRAMES_MAX_CROPS, a design
 * limit (the reference has five locations).  mirror: 0 = windows as given, 1 = every window mirrored (the `flip` of
 * tbn_frames_to_tensor), 2 = every window followed by its mirror image (horizontal_flip=True), 3 = every window's
 * mirror image followed by the window (what horizontal_flip=True makes of frames that were flipped beforehand).
 * Order = the reference's: FixedCrop emits a flat list, entry j = (window * n_img + image) * F + f with F = 2 for
 * mirror >= 2 (f = 1: the second of the pair) and F = 1 otherwise; Stack makes `stack` CONSECUTIVE entries the channels
 * of one sample, so output sample s, stack slot u holds entry j = s * stack + u.  With stack > 1 and a mirror pair
 * (Flow) a sample therefore alternates plain and mirrored images of neighbouring frames -- the reference's behaviour,
 * reproduced as is.  out: (n_img * n_crops * F / stack, channels * stack, out_h, out_w) fp32.  Refused before any
 * launch: n_img * n_crops * F not a multiple of stack, a window outside the resized box, n_crops outside
 * 1..TBN_FRAMES_MAX_CROPS, and whatever tbn_frames_to_tensor refuses.  Ask tbn_capabilities() & TBN_CAP_FRAMES_CROPS. */
#define TBN_FRAMES_MAX_CROPS 16
int tbn_frames_to_tensor_crops(const unsigned char* frames, int n_img, int height, int width, int channels, int box_x,
                               int box_y, int box_w, int box_h, int resized_w, int resized_h, const int* crop_x,
                               const int* crop_y, int n_crops, int out_w, int out_h, int mirror, int stack,
                               const float* mean, const float* std_dev, int n_stat, int div255, float* out,
                               void* stream);
/* The same pass for a BATCH of clips in one launch, every clip with a geometry of its own.  Replaces reference
 * core/dataset/dataset.py:512-532 `_transform_data`, which the DataLoader applies once per sample: MultiScaleCrop and
 * RandomHorizontalFlip draw once per clip and modality, so a batch has one crop box and one flip per clip.  The
 * geometries come as a table, one row per clip; every field but first_img / out_row means what the argument of the same
 * name means to tbn_frames_to_tensor, and the result is bit-identical to that entry called once per clip with the clip's
 * row (the scale factors are the same IEEE double expression, evaluated on the device).
 *   frames       (n_img, height, width, channels) uint8 on the device; clip k owns the images
 *                [first_img, first_img + imgs_per_clip), `stack` consecutive ones form one output sample;
 *   clips_host   the table in HOST memory: everything is validated from it before any launch, because the kernel reads
 *                `frames` and writes `out` unchecked;
 *   clips_dev    the SAME bytes in device memory, the caller's own copy (as the address table of tbn_stft_windows): a
 *                workgroup reads its clip's row from here.  The launch arguments cannot hold a table of 96 clips;
 *   out          (out_rows, channels * stack, out_h, out_w) fp32; clip k writes the rows
 *                [out_row, out_row + imgs_per_clip / stack).  Rows no clip names are not touched, so several launches
 *                (one per source frame size) can fill one batch tensor.
 * Refused before any launch, with a message naming the clip: a null pointer, imgs_per_clip not a positive multiple of
 * stack, first_img < 0 or first_img + imgs_per_clip > n_img, whatever tbn_frames_to_tensor refuses for that geometry
 * (box outside the frame, window outside the resized box, out_w > 1024, missing mean / std), out_row < 0 or
 * out_row + imgs_per_clip / stack > out_rows, and two clips whose output rows overlap.  n_clips == 0 launches nothing
 * and returns 0. */
typedef struct tbn_frames_clip {
  int first_img;                        /* the clip's first image in `frames`; the clip owns imgs_per_clip images from here */
  int box_x, box_y, box_w, box_h;       /* source box, as in tbn_frames_to_tensor */
  int resized_w, resized_h;             /* == box: no interpolation */
  int crop_x, crop_y;                   /* window origin inside the resized box */
  int flip;
  int out_row;                          /* first output sample (row of `out`) this clip writes; it writes imgs_per_clip/stack rows */
  int reserved;
} tbn_frames_clip;
int tbn_frames_to_tensor_batch(const unsigned char* frames, int n_img, int height, int width, int channels,
                               const tbn_frames_clip* clips_host, const tbn_frames_clip* clips_dev, int n_clips,
                               int imgs_per_clip, int out_w, int out_h, int stack, const float* mean,
                               const float* std_dev, int n_stat, int div255, float* out, int out_rows, void* stream);

/* ---- baseline JPEG decode into device frames (the step in front of tbn_frames_to_tensor) ---------- */
/* Replaces cv2.imread of reference core/dataset/dataset.py:303-305 (RGB: 3 channels B, G, R) and :355-370 (Flow:
 * cv2.imread(path, 0), gray), i.e. libjpeg-turbo at its defaults -- ISLOW integer IDCT, "fancy" triangle upsampling,
 * fixed-point YCbCr -> RGB -- byte for byte.  The serial half (markers, Huffman) is host code and needs no GPU; the
 * half after the quantised coefficients is two kernels.  Supported: SOF0, 8-bit, Huffman, one interleaved scan; 1
 * component, or 3 components YCbCr with luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and chroma 1x1; restart intervals,
 * 0xFF00 stuffing and fill bytes before markers.  Refused with a message naming the reason (TBN_ERR_UNSUPPORTED:
 * progressive and other SOFn, arithmetic coding, 12-bit, 4 components, other sampling, several scans; TBN_ERR_ARG: a
 * missing table, a DC coefficient outside int16, a stream that ends early or meets a marker inside the scan data).
 * There is no capability bit: callers detect the feature by the symbol. */
#ifndef TBN_JPEG_GEOMETRY_DEFINED
#define TBN_JPEG_GEOMETRY_DEFINED
typedef struct tbn_jpeg_geometry {
  int width, height;          /* true image size in pixels */
  int components;             /* 1 (gray) or 3 (YCbCr) */
  int hsamp[3], vsamp[3];     /* sampling factors per component (a 1-component file: 1 x 1) */
  int blocks_w[3], blocks_h[3]; /* 8x8-block extents of each component plane, padded to whole MCUs */
  int restart_interval;       /* MCUs between restart markers, 0: none (informational, not compared) */
  size_t coef_count;          /* int16 coefficients of one image: 64 * sum(blocks_w * blocks_h) */
} tbn_jpeg_geometry;
#endif
/* HOST.  Parses SOI, APPn / COM (skipped), DQT, SOF0, DHT, DRI and SOS of `size` untrusted bytes and fills `out`.
 * replaces: the header half of cv2.imread, core/dataset/dataset.py:305, :360, :365 */
int tbn_jpeg_parse(const unsigned char* data, size_t size, tbn_jpeg_geometry* out);
/* HOST, thread-safe (no global state; the error string is thread-local).  Decodes the scan into
 * coef[expect->coef_count]: QUANTISED coefficients in natural (de-zigzagged) order, per component plane
 * [block_row][block_col][64], planes one after the other; and quant[components * 64]: the image's quantisation tables
 * per component in natural order (per image: a batch may mix qualities).  Refuses an image whose size, component
 * count or sampling differs from `expect`.  Writes nothing outside coef[0, coef_count) and quant[0, components * 64).
 * replaces: the entropy-decoding half of cv2.imread, core/dataset/dataset.py:305, :360, :365 */
int tbn_jpeg_entropy_decode(const unsigned char* data, size_t size, const tbn_jpeg_geometry* expect, int16_t* coef,
                            uint16_t* quant);
/* bytes of workspace tbn_jpeg_reconstruct needs for n_img images of this geometry (the uint8 component planes,
 * block-padded: coef_count bytes per image); 0 for a geometry it would refuse */
size_t tbn_jpeg_workspace_bytes(const tbn_jpeg_geometry* geometry, int n_img);
/* DEVICE.  n_img images of ONE geometry: coef_dev (n_img, coef_count) int16 and quant_dev (n_img, components, 64)
 * uint16 in the layouts of tbn_jpeg_entropy_decode, both and the workspace 16-byte aligned.  Kernel A: dequantisation
 * and the ISLOW 8x8 IDCT into the workspace planes.  Kernel B: h2v1 / h2v2 fancy upsampling of the chroma's true
 * downsampled extent, YCbCr -> B, G, R, interleaved and cropped: frames_dev (n_img, height, width, out_channels) uint8.
 * out_channels 3: B, G, R; a 1-component file is replicated to the three channels (cv2.imread(path)).  out_channels
 * 1: a 3-component file delivers its luma plane and its chroma is not reconstructed (cv2.imread(path, 0)).  Integer
 * arithmetic that wraps: corrupt coefficients give garbage pixels, never a fault; every address depends on the
 * geometry alone.  replaces: the reconstruction half of cv2.imread, core/dataset/dataset.py:305, :360, :365 */
int tbn_jpeg_reconstruct(const int16_t* coef_dev, const uint16_t* quant_dev, int n_img,
                         const tbn_jpeg_geometry* geometry, int out_channels, unsigned char* frames_dev,
                         void* workspace, void* stream);

/* ---- JPEG Huffman decoding on the device (opt-in; the default is tbn_jpeg_entropy_decode on host threads) ---------- */
/* A Huffman stream has no sync points but synchronises itself: a decoder started at a wrong bit usually falls onto true
 * codeword boundaries after a few symbols (Weissenberger & Schmidt, ICPP 2018 and HiPC 2021).  The unstuffed scan is cut
 * into intervals (the whole scan, or one restart interval) and every interval into subsequences of S bits, one lane
 * each; every lane decodes from a guessed state (bit, block of the MCU, zigzag index), hands the state it ends in to
 * the next lane, and the rounds repeat until no lane's start changes -- at most as many rounds as lanes, and at that
 * fixed point the result IS the sequential decode.  csrc/tbn_jpeg_sync.h has the record layout and the decoder core.
 * There is no capability bit: callers detect the feature by the symbol.
 * bytes of the record of a file of `file_size` bytes with `n_intervals` intervals (ceil(MCUs / restart interval), or 1),
 * a multiple of 16 */
size_t tbn_jpeg_scan_pack_bytes(size_t file_size, int n_intervals);
/* HOST, thread-safe.  Parses as tbn_jpeg_entropy_decode does and, instead of decoding, packs what the device decoder
 * reads into record[0, record_bytes) (16-byte aligned; pinned memory if it is to be copied asynchronously): a header,
 * the image's own Huffman tables in lookup form, the interval table (start bit, bit length), and the entropy-coded
 * bytes with 0xFF00 stuffing, fill bytes and RSTn markers removed (the markers' order is checked; a missing EOI is
 * refused).  quant[components * 64]: as tbn_jpeg_entropy_decode writes it.  *n_intervals: the image's interval count;
 * *used: the bytes of the record written.  An image of more than `max_intervals` intervals (the device decoder takes at
 * most 1024) is NOT packed: the return is 0 and *used is 0.  Refusals: the codes and the wording of
 * tbn_jpeg_entropy_decode.  Writes nothing outside record[0, record_bytes) and quant[0, components * 64). */
int tbn_jpeg_scan_pack(const unsigned char* data, size_t size, const tbn_jpeg_geometry* expect, void* record,
                       size_t record_bytes, int max_intervals, uint16_t* quant, int* n_intervals, size_t* used);
/* bytes of workspace tbn_jpeg_entropy_decode_dev needs (16 per image: the subsequence size it chose, lanes, rounds,
 * whether the scan was staged in LDS, as uint32); 0 for a geometry it would refuse */
size_t tbn_jpeg_entropy_workspace_bytes(const tbn_jpeg_geometry* geometry, int n_img);
/* DEVICE.  n_img images of ONE geometry.  packed_dev[0, packed_bytes): the records (16-byte aligned);
 * offsets_dev[n_img]: byte offset of each image's record, a multiple of 16, or 0xFFFFFFFF for an image without one
 * (status 64, nothing written for it but zeros).  subseq_bits: S; 0 = 1024, else a multiple of 32, >= 64; it grows in
 * steps of 32 for an image whose lanes would otherwise exceed 1024.  One workgroup per image, one launch (after a
 * hipMemsetAsync of coef_dev): relaxation rounds, block-count scan, validation, the write pass, DC prefix sums.
 * coef_dev (n_img, coef_count) int16, 16-byte aligned: the layout of tbn_jpeg_entropy_decode, what tbn_jpeg_reconstruct
 * takes.  status_dev[n_img]: 0 = decoded, identical to tbn_jpeg_entropy_decode's coefficients; otherwise bits 1: invalid
 * code, 2: AC run leaves the block, 4: an interval's block total differs from the geometry's, 8: an interval ends more
 * than 7 bits after its last block or runs out of bits, 16: DC outside int16, 32: inconsistent record, 64: no record --
 * such an image is for the host stage (its coefficients here are unspecified).  info_dev (n_img, 2): lanes, rounds.
 * A corrupt stream costs a status, never an access outside the image's coefficients.  Strictness: stray bytes between
 * the last block and the next marker are judged by the host stage according to its refill state; this path may accept
 * such a file where the host stage refuses it, never the reverse without a non-zero status. */
int tbn_jpeg_entropy_decode_dev(const void* packed_dev, size_t packed_bytes, const uint32_t* offsets_dev, int n_img,
                                const tbn_jpeg_geometry* geometry, int subseq_bits, int16_t* coef_dev, int* status_dev,
                                int* info_dev, void* workspace, void* stream);

/* ---- flow pickles: zip members (stored or raw deflate, RFC 1951) inflated on the device (opt-in) ---------- */
/* Replaces np.load of reference core/dataset/dataset.py:342-343 (the `flow` member of a frame_XXXXXXXXXX.npz written by
 * np.savez / np.savez_compressed): the zlib inflate and the CRC-32 check.  The zip directory and the .npy header stay host
 * work (core/dataset/npz_file.py).  The decoder core is csrc/tbn_inflate.h.  There is no capability bit: callers detect
 * the feature by the symbol.
 * One row of the member table (40 bytes):
 *   in_off, in_len   the member's compressed bytes inside `in`; in_off is a multiple of 4
 *   out_off, out_len where its inflated bytes go inside `out`, and the size the directory declares: exactly out_len
 *                    bytes are produced or the status says why not.  Rows must not overlap in `out` (not checked).
 *   crc              the directory's CRC-32 of the inflated bytes
 *   method           0 (stored: a copy) or 8 (deflate); no zlib or gzip wrapper
 *   skip             non-zero: the member takes the host path; nothing is read or written for it (status 11)
 * Limits: in_len and out_len below 2^31 (no zip64 members).
 * status[i]: 0 ok, the bytes are the member's and their CRC-32 matched; 1 reserved block type; 2 stored LEN != ~NLEN;
 * 3 code lengths (HLIT > 286, HDIST > 30, a bad repeat, an over-subscribed code, or an incomplete one where zlib refuses
 * it); 4 a symbol that does not exist (literal/length 286, 287, distance 30, 31, an unused code); 5 no end-of-block code;
 * 6 distance before the start of the output; 7 input exhausted; 8 output would pass out_len; 9 output ends short of
 * out_len; 10 CRC-32 mismatch; 11 skipped; 12 inconsistent row (a range outside the buffers, a misaligned in_off,
 * another method, a size of 2^31 or more).  With a non-zero status the member's out bytes are unspecified, but nothing
 * outside [out_off, out_off + out_len) is written and nothing outside [in_off, in_off + in_len) is read: a damaged file
 * costs a status, never a fault or a hang.  info[i]: bytes produced. */
typedef struct tbn_inflate_member {
  uint64_t in_off, out_off;
  uint32_t in_len, out_len;
  uint32_t crc;
  uint32_t method;
  uint32_t skip;
  uint32_t reserved;
} tbn_inflate_member;
/* DEVICE.  Two launches on `stream`: one wavefront per member inflates (or copies) it, then one workgroup per member
 * computes the CRC-32 of the staged bytes and folds a mismatch into the status.  in_dev[0, in_bytes): the packed
 * compressed bytes, 4-byte aligned; members_dev[n_members]: the table, in device memory, 8-byte aligned;
 * out_dev[0, out_bytes): the staging buffer; status_dev / info_dev: n_members ints each.  n_members == 0 launches nothing. */
int tbn_inflate_batch(const void* in_dev, size_t in_bytes, const tbn_inflate_member* members_dev, int n_members,
                      void* out_dev, size_t out_bytes, int* status_dev, int* info_dev, void* stream);
/* HOST, thread-safe, no GPU call: the same decoder core and the same chunked CRC run serially over the same table, all
 * pointers host memory.  The test aid of tbn_inflate_batch. */
int tbn_inflate_host(const void* in, size_t in_bytes, const tbn_inflate_member* members, int n_members, void* out,
                     size_t out_bytes, int* status, int* info);
/* Members that carry a CHUNK INDEX (written by tbn_deflate_batch_indexed below; core/dataset/npz_file.py keeps it in a zip
 * extra field): the stream is chunks of tbn_deflate_chunk() raw bytes compressed independently and joined on byte
 * boundaries, so every chunk inflates on its own -- parallelism inside a member that np.load of reference
 * core/dataset/dataset.py:342-343 has no use for.  One row of the chunk table (32 bytes), rows in member order:
 *   in_off, in_len   the chunk's compressed bytes inside `in`: ANY byte offset (only the member's in_off is aligned)
 *   out_off, out_len inside `out`: the member's out_off + chunk_no * tbn_deflate_chunk(); out_len is tbn_deflate_chunk()
 *                    but for the last chunk, which holds the rest (0 for an empty member)
 *   member           its row of the member table (method 8)
 *   last             non-zero: the member's last chunk
 * chunk_begin[n_members + 1]: member i owns chunk rows [chunk_begin[i], chunk_begin[i + 1]): max(1, ceil(out_len / chunk))
 * of them, tiling its compressed bytes and its output in order -- anything else is status 12 for the member.
 * status / info per member: status is the first non-zero chunk status in chunk order (0..12 as above; 13: a segment does
 * not end where the index says -- input left over, BFINAL in a chunk that is not the last, no BFINAL in the last one; a
 * distance before the CHUNK's first byte is 6), then the CRC-32 check of the whole member as above: status 0 means the
 * bytes are the member's whatever the index said.  info is the sum of the bytes the chunks produced.  11 for a member with
 * `skip`: its chunks do nothing.  chunk_status[2 * n_chunks]: each chunk's status, then the bytes each produced.  The
 * guarantees of tbn_inflate_batch hold per chunk: nothing outside its slice is read, nothing outside its out range written. */
typedef struct tbn_inflate_chunk {
  uint64_t in_off, out_off;
  uint32_t in_len, out_len;
  uint32_t member;
  uint32_t last;
} tbn_inflate_chunk;
/* DEVICE.  Three launches on `stream`: one wavefront per chunk inflates it; one wavefront per member folds its chunks'
 * statuses; one workgroup per member checks the CRC-32.  chunks_dev[n_chunks]: device memory, 8-byte aligned;
 * chunk_begin_dev, chunk_status_dev: 4-byte aligned; the rest as for tbn_inflate_batch.  n_members == 0 launches nothing. */
int tbn_inflate_chunks(const void* in_dev, size_t in_bytes, const tbn_inflate_member* members_dev, int n_members,
                       const tbn_inflate_chunk* chunks_dev, const uint32_t* chunk_begin_dev, int n_chunks, void* out_dev,
                       size_t out_bytes, int* status_dev, int* info_dev, int* chunk_status_dev, void* stream);
/* HOST, thread-safe, no GPU call: the test aid of tbn_inflate_chunks, all pointers host memory. */
int tbn_inflate_chunks_host(const void* in, size_t in_bytes, const tbn_inflate_member* members, int n_members,
                            const tbn_inflate_chunk* chunks, const uint32_t* chunk_begin, int n_chunks, void* out,
                            size_t out_bytes, int* status, int* info, int* chunk_status);

/* ---- flow pickles: raw deflate streams (RFC 1951) and the zip CRC-32 written on the device (opt-in) -------- */
/* Replaces the zlib run inside np.savez_compressed of reference preprocessing/create_epic_flow_pickle.py:203.  The zip
 * container and the .npy header stay host work (core/dataset/npz_file.py).  The encoder core and the stream format are
 * csrc/tbn_deflate.h: a member is cut into chunks of tbn_deflate_chunk() bytes that are compressed independently (LZ77
 * inside the chunk, stored / fixed / dynamic blocks by exact bit cost) and joined on byte boundaries; any inflate reads
 * the result.  The device and the host twin write the same bytes.  There is no capability bit: callers detect the
 * feature by the symbol.
 * One row of the member table (32 bytes):
 *   in_off, in_len   the member's raw bytes inside `raw`; in_off is a multiple of 4, in_len below 2^31
 *   out_off, out_cap where its stream goes inside `out` and how much room it has: at least tbn_deflate_bound(in_len).
 *                    Rows must not overlap in `out` (not checked).
 *   skip             non-zero: nothing is read or written for the row (status 3)
 * Status per member: 0 ok; 1 out_cap is below tbn_deflate_bound(in_len); 2 the row is inconsistent (a range outside the
 * buffers, in_len of 2^31 or more, in_off not a multiple of 4); 3 skipped.  With a non-zero status out_len and crc are 0
 * and nothing at all is written to `out` for the row; with status 0 only [out_off, out_off + out_len) is. */
typedef struct tbn_deflate_member {
  uint64_t in_off, out_off;
  uint32_t in_len, out_cap;
  uint32_t skip;
  uint32_t reserved;
} tbn_deflate_member;
/* HOST.  The chunk size of the stream format (reference preprocessing/create_epic_flow_pickle.py:203 has no such notion:
 * zlib compresses the member whole). */
size_t tbn_deflate_chunk(void);
/* HOST, closed form: no stream for n raw bytes is longer than n + 5 * max(1, ceil(n / tbn_deflate_chunk())).  The room
 * np.savez_compressed of reference preprocessing/create_epic_flow_pickle.py:203 leaves zlib to find. */
size_t tbn_deflate_bound(size_t n);
/* HOST, from a host copy of the table tbn_deflate_batch will get: bytes of its `workspace` (one slot per chunk).  Part of
 * replacing reference preprocessing/create_epic_flow_pickle.py:203. */
size_t tbn_deflate_workspace_bytes(const tbn_deflate_member* members, int n_members);
/* DEVICE.  Replaces the compression of reference preprocessing/create_epic_flow_pickle.py:203.  Three launches on
 * `stream`: one wavefront per chunk compresses it into its workspace slot; one workgroup per member joins the slots
 * into the member's stream and writes out_len and the status; one workgroup per member computes the CRC-32 of the raw
 * bytes.  raw_dev[0, raw_bytes): 4-byte aligned; members_dev[n_members]: device memory, 8-byte aligned;
 * out_dev[0, out_bytes); out_len_dev / crc_dev / status_dev: n_members 32-bit values each; workspace: device memory of
 * tbn_deflate_workspace_bytes(), 16-byte aligned.  n_members == 0 launches nothing. */
int tbn_deflate_batch(const void* raw_dev, size_t raw_bytes, const tbn_deflate_member* members_dev, int n_members,
                      void* out_dev, size_t out_bytes, uint32_t* out_len_dev, uint32_t* crc_dev, int* status_dev,
                      void* workspace, void* stream);
/* HOST, thread-safe, no GPU call: the same encoder core and the same chunked CRC run serially over the same table, all
 * pointers host memory, the same bytes out.  The test aid of tbn_deflate_batch and the host side of replacing reference
 * preprocessing/create_epic_flow_pickle.py:203. */
int tbn_deflate_host(const void* raw, size_t raw_bytes, const tbn_deflate_member* members, int n_members, void* out,
                     size_t out_bytes, uint32_t* out_len, uint32_t* crc, int* status);
/* DEVICE / HOST.  tbn_deflate_batch / tbn_deflate_host -- the same bytes, lengths, CRCs and statuses -- plus THE CHUNK
 * INDEX (reference preprocessing/create_epic_flow_pickle.py:203 has no such notion): chunk_end holds, for every row in
 * table order, max(1, ceil(in_len / tbn_deflate_chunk())) entries, the offset inside the row's stream at which each
 * chunk's bytes end (the last equals out_len); the entries of a skipped or refused row are 0.  The join launch writes
 * them.  chunk_end: 4-byte aligned, the sum of those counts over ALL rows long. */
int tbn_deflate_batch_indexed(const void* raw_dev, size_t raw_bytes, const tbn_deflate_member* members_dev, int n_members,
                              void* out_dev, size_t out_bytes, uint32_t* out_len_dev, uint32_t* crc_dev, int* status_dev,
                              void* workspace, void* stream, uint32_t* chunk_end_dev);
int tbn_deflate_host_indexed(const void* raw, size_t raw_bytes, const tbn_deflate_member* members, int n_members, void* out,
                             size_t out_bytes, uint32_t* out_len, uint32_t* crc, int* status, uint32_t* chunk_end);

/* ---- PNG frames into device frames (data.rgb.file_ext / data.flow.file_ext: "png") ---------- */
/* Replaces cv2.imread of reference core/dataset/dataset.py:305 (RGB: 3 channels B, G, R) and :360, :365 (Flow:
 * cv2.imread(path, 0), gray) for frames extracted as PNG -- lossless, so every byte is exact.  The container is host code
 * (csrc/tbn_png_host.h) and needs no GPU; the zlib stream is inflated on host threads or, opt-in, on the device with the
 * decoder core of tbn_inflate_batch (csrc/tbn_inflate.h); scanline unfiltering and the conversion to frame bytes are one
 * kernel.  Supported: bit depth 8, non-interlaced, colour types 0 (gray), 2 (RGB), 3 (palette), 4 (gray + alpha), 6 (RGBA);
 * alpha is dropped and ancillary chunks (tRNS, gAMA, ...) are skipped unread, as cv2.imread does at its defaults.  Refused
 * with a message naming the reason (TBN_ERR_UNSUPPORTED: bit depths 1, 2, 4, 16, Adam7 interlace, a scanline of more than
 * 16384 bytes = 4096 RGBA pixels, 2^31 or more scanline bytes; TBN_ERR_ARG: anything malformed or truncated).  There is no
 * capability bit: callers detect the feature by the symbol. */
#ifndef TBN_PNG_GEOMETRY_DEFINED
#define TBN_PNG_GEOMETRY_DEFINED
typedef struct tbn_png_geometry {
  int width, height;        /* image size in pixels */
  int colour_type;          /* 0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGBA */
  int bpp;                  /* bytes per pixel in the scanlines: 1, 3, 1, 2, 4 */
  int palette_entries;      /* entries of PLTE (colour type 3; else 0).  Per file: not compared */
  int reserved;
  size_t raw_bytes;         /* the inflated scanlines: height * (1 + width * bpp) */
  size_t idat_bytes;        /* sum of the IDAT payloads: the zlib stream.  Per file: not compared */
} tbn_png_geometry;
#endif
/* HOST, thread-safe.  Walks `size` untrusted bytes: the signature; IHDR first and 13 bytes long; chunk lengths inside the
 * file; CRC-32 of IHDR, PLTE, IDAT and IEND (ancillary chunks are skipped unread); PLTE present with 3 * (1..256) bytes
 * for colour type 3; consecutive IDAT chunks; IEND present.  Fills `out`.
 * replaces: the header half of cv2.imread, core/dataset/dataset.py:305, :360, :365 */
int tbn_png_parse(const unsigned char* data, size_t size, tbn_png_geometry* out);
/* HOST, thread-safe.  The same IHDR checks on the first 33 bytes alone (signature, IHDR and its CRC): width, height,
 * colour_type, bpp and raw_bytes of a frame whose file is not read further.
 * replaces: frame.shape of a cv2.imread result where only the size is used, core/dataset/dataset.py:305 */
int tbn_png_parse_header(const unsigned char* data, size_t size, tbn_png_geometry* out);
/* bytes tbn_png_gather writes for a zlib stream of idat_bytes: 2 + idat_bytes rounded up to 4, plus 4 */
size_t tbn_png_gather_bytes(size_t idat_bytes);
/* HOST, thread-safe.  Concatenates the IDAT payloads -- the zlib stream, split anywhere, inside its header and into empty
 * chunks too -- into zstream[2, 2 + expect->idat_bytes) (4-byte aligned, tbn_png_gather_bytes() long, pinned if it is to
 * be copied asynchronously; the rest is zeroed), so that the raw deflate data behind the 2-byte zlib header starts at
 * byte 4, a multiple of 4 as tbn_inflate_member.in_off and tbn_png_image.in_off require.  Checks the zlib header (CM 8,
 * window <= 32 K, no preset dictionary, FCHECK).  [*deflate_begin, *deflate_end) of zstream is the deflate data, *adler
 * the stream's trailing Adler-32.  palette_bgr (1024 bytes; may be NULL): 256 x 3 bytes B, G, R with unused entries
 * zero, the entry count as a little-endian uint32 at byte 768, zeros behind it.  Refuses a file whose size, colour type
 * or IDAT byte count differs from `expect`.
 * replaces: the chunk-reading half of cv2.imread, core/dataset/dataset.py:305, :360, :365 */
int tbn_png_gather(const unsigned char* data, size_t size, const tbn_png_geometry* expect, unsigned char* zstream,
                   unsigned char* palette_bgr, uint32_t* deflate_begin, uint32_t* deflate_end, uint32_t* adler);
/* the sizes at which the unfilter kernel changes its path, for tests: rows of a band (64), pixel steps between two staging
 * passes (64), the longest scanline in bytes (16384).  cv2.imread of core/dataset/dataset.py:305 has no such seams. */
int tbn_png_limits(int* band_rows, int* step_tile, int* max_row_bytes);
/* DEVICE.  n_img images of ONE geometry: raw_dev (n_img, raw_bytes), 4-byte aligned, are the inflated scanlines, each with
 * its filter byte; palette_dev (n_img, 1024) in tbn_png_gather's layout (colour type 3 only; else ignored);
 * frames_dev (n_img, height, width, out_channels) uint8.  Filters None, Sub, Up, Average (9-bit sum, floor) and Paeth
 * (ties in the order a, b, c), prior row of the first row = 0, a = c = 0 at the first pixel, arithmetic mod 256.
 * out_channels 3: gray replicated, RGB as B, G, R, alpha dropped, palette looked up.  out_channels 1: colour types 0 and 4
 * only (cv2.imread(path, 0) of a colour file goes through a conversion formula that is not reproduced: TBN_ERR_ARG).
 * status_dev[n_img]: 0 ok; 21 a filter byte above 4 (that row is taken as filter 0); 22 a palette index at or beyond the
 * entry count (that pixel is 0, 0, 0).  One wavefront per image, rows of a 64-row band on the lanes, skewed by one pixel
 * (csrc/png.hip).  Corrupt bytes cost a status or garbage pixels, never a fault: every address depends on the geometry
 * alone.  replaces: the row-reconstruction half of cv2.imread, core/dataset/dataset.py:305, :360, :365 */
int tbn_png_unfilter(const unsigned char* raw_dev, const unsigned char* palette_dev, int n_img, const tbn_png_geometry* geometry,
                     int out_channels, unsigned char* frames_dev, int* status_dev, void* stream);
/* One row of the image table of tbn_png_decode (24 bytes):
 *   in_off, in_len   the image's raw deflate data inside `in` (tbn_png_gather: zstream + *deflate_begin, of
 *                    *deflate_end - *deflate_begin bytes); in_off is a multiple of 4
 *   palette_off      its 1024-byte palette slot inside `in` (colour type 3; else ignored)
 *   adler            the stream's trailing Adler-32 */
typedef struct tbn_png_image {
  uint64_t in_off, palette_off;
  uint32_t in_len, adler;
} tbn_png_image;
/* bytes of workspace tbn_png_decode needs for n_img images of this geometry (their inflated scanlines); 0 for a geometry
 * it would refuse.  cv2.imread of core/dataset/dataset.py:305 allocates the like inside libpng. */
size_t tbn_png_workspace_bytes(const tbn_png_geometry* geometry, int n_img);
/* DEVICE (opt-in; the default inflates on host threads).  Three launches on `stream`: one wavefront per image inflates its
 * deflate data into the workspace with the decoder core of tbn_inflate_batch; one workgroup per image checks the Adler-32
 * of the inflated bytes; tbn_png_unfilter's kernel then skips every image whose status is not 0.  in_dev[0, in_bytes) and
 * the workspace: 4-byte aligned; images_dev[n_img]: device memory, 8-byte aligned.  status_dev[n_img]: 0 ok; 1..12 the
 * statuses of tbn_inflate_batch, raw_bytes being the required output length (12: the row is inconsistent); 20 Adler-32
 * mismatch; 21, 22 as above.  With a non-zero status the image's frame is unspecified -- it is for the host stage.
 * info_dev[n_img]: bytes inflated.  A damaged stream costs a status, never a fault or a hang.
 * replaces: the zlib and row-reconstruction halves of cv2.imread, core/dataset/dataset.py:305, :360, :365 */
int tbn_png_decode(const void* in_dev, size_t in_bytes, const tbn_png_image* images_dev, int n_img,
                   const tbn_png_geometry* geometry, int out_channels, unsigned char* frames_dev, void* workspace,
                   int* status_dev, int* info_dev, void* stream);
/* HOST, thread-safe, no GPU call: the same predictors, conversion, decoder core and Adler pieces run serially, all pointers
 * host memory, the same statuses and the same bytes.  The test aids of tbn_png_unfilter and tbn_png_decode (cv2.imread of
 * core/dataset/dataset.py:305 is their common reference). */
int tbn_png_unfilter_host(const unsigned char* raw, const unsigned char* palette, int n_img, const tbn_png_geometry* geometry,
                          int out_channels, unsigned char* frames, int* status);
int tbn_png_decode_host(const void* in, size_t in_bytes, const tbn_png_image* images, int n_img, const tbn_png_geometry* geometry,
                        int out_channels, unsigned char* frames, void* workspace, int* status, int* info);

#ifdef __cplusplus
}
#endif
#endif /* TBN_HIP_H */
