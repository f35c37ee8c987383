/* pacingpseudo_hip.h -- C ABI of libpacingpseudo_hip.so (MI355X / gfx950).
 *
 * The reference (zefanyang/pacingpseudo) has no native/FFI layer: its hot path dispatches stock PyTorch
 * operators from three Python modules.  This header is the drop-in boundary that replaces those operator
 * call sites for the PacingPseudo training step; every entry cites the reference call site it stands in for
 * (paths relative to the reference repository root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C types only: raw DEVICE pointers, explicit sizes / leading dimensions, `void* stream` = hipStream_t
 *     (pass torch.cuda.current_stream().cuda_stream); all work is enqueued on that stream, no implicit sync.
 *   - return value: 0 = OK, negative = library error (bad argument -1, unsupported -2, workspace -3),
 *     positive = hipError_t.  pp_last_error() returns a thread-local message for the last failure.
 *   - the library allocates nothing persistent and keeps no pointer after return; workspaces are caller-owned.
 *     Process state: a per-(kernel, device) cache of the dynamic-LDS attribute (mutex-protected), the opt-in event
 *     profiler below, and PP_* environment knobs that select between equivalent kernels (read once, never written).
 *   - activations are NHWC fp32: element (pixel p, channel c) of a tensor lives at base[p * ld + c] where
 *     p = (n*H + y)*W + x and ld >= C is the pixel stride in floats ("leading dimension").  A channel slice of a
 *     wider tensor (the concatenation buffers of the decoder) is addressed by offsetting `base` and keeping ld.
 *     C, ld multiples of 4 and 16-byte aligned bases are required (float4 accesses).
 *   - logits / scribbles / masks at the module boundary stay NCHW exactly as the reference passes them.
 *   - "groups": the weak and the strong view of one siamese step are laid back to back along the batch axis;
 *     BatchNorm statistics are taken per group (= per reference module call).
 */
#ifndef PACINGPSEUDO_HIP_H
#define PACINGPSEUDO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lazy activations (round 4) ------------------------------------------------------------------------ */
/* In train mode BatchNorm2d's batch statistics (models/unet.py:189) exist only once the whole convolution output z is
 * written, so y = LeakyReLU(BN(z)) used to cost one more pass over the tensor.  A LAZY tensor keeps z in memory together
 * with per-(group, channel) coefficient rows and every *_lazy entry point evaluates y while it loads:
 *   y = v > 0 ? v : v * slope,  v = z * scale + shift,
 *   coef[(g * 3 + 0) * ld + c] = scale, [(g * 3 + 1) * ld + c] = shift, [(g * 3 + 2) * ld + c] = slope,  g = image / (B / groups).
 * Channels that already hold final values carry the identity row (1, 0, 1).  coef == NULL (or a NULL descriptor) means
 * the tensor is an ordinary one.  A channel slice of a wider lazy tensor passes coef + c0 and keeps ld.  pp_bn_train_finalize_lazy
 * writes the rows; pp_lazy_materialize turns a lazy tensor into an ordinary one (for consumers without a *_lazy form). */
typedef struct pp_lazy_in {
  const float* coef;   /* device pointer, 16-byte aligned; NULL = not lazy */
  int ld;              /* floats per coefficient row (>= channels of the view, multiple of 4) */
  int groups;          /* statistics groups along the batch axis (divides B) */
} pp_lazy_in;

/* ---- runtime ------------------------------------------------------------------------------------------ */
/* 100 * round + revision; bumped whenever an entry point is removed or changes its arguments (600: round 6; 601: GroupNorm entry points).  The Python
 * binding refuses a library older than the header it was written against (pacingpseudo_amd/_lib.py: MIN_LIB_VERSION). */
int pp_version(void);
const char* pp_last_error(void);
int pp_device_info(int* cu_count, int* lds_per_cu_kb, char* arch, int arch_len);
/* optional profiler: HIP events around every call, accumulated per kernel family (see PP_KIND_*). */
/* Numeric mode of the forward / data-gradient matrix kernels, per process: 3 = every fp32 product as three fp16 MFMA
 * products of split operands (fp32 grade, the default), 1 = hi parts only (fp16 operands with fp32 accumulation: the mixed
 * precision mode of train_chaos.py --precision fp16; no 1e-4 parity claim).  The Winograd weight-gradient GEMM follows the
 * mode (round 4); the direct weight-gradient kernels always use 3 (1 in the 16-bit storage build, whose operands have no low part). */
int pp_set_matrix_products(int n);
int pp_get_matrix_products(void);
/* CU budget of the persistent direct weight-gradient kernels (conv weight gradient of models/unet.py:188 for the narrow layers), per
 * CALLING THREAD (round 6; a thread that never set one launches with the default): how many CUs' worth of blocks
 * pp_conv3x3_bwd_weight_f16x3 launches.  256 (default; PP_WGRAD_CUS) fills the chip; the engine sets 192 for the duration of a
 * backward pass whose weight gradients run on its second stream beside the data-gradient / BatchNorm chain and restores the
 * previous value (round 5: same-box -0.6 ms per step against 256, profiles/r05_experiments/).  pp_conv3x3_bwd_weight_workspace
 * does not depend on it (sized for the largest budget, 8 <= cus <= 1024). */
int pp_set_wgrad_cus(int cus);
int pp_get_wgrad_cus(void);
/* named ranges for `rocprofv3 --marker-trace` (roctxRangePush / Pop resolved at run time; no-ops without a roctx library):
 * the engine brackets the phases of a step (pack, forward, losses, aux path, backward decoder / aux / encoder, optimizer) */
int pp_range_push(const char* name);
int pp_range_pop(void);
int pp_prof_enable(int on);
int pp_prof_reserve(int events);                     /* pre-create the event pool (2 events per timed launch until the next collect) */
int pp_prof_select(unsigned long long kind_mask);   /* time only the families whose bit (1 << PP_KIND_*) is set; default all */
int pp_prof_collect(double* out /* [kinds][5] = launches, ms, executed flops, algorithmic bytes, algorithmic flops */,
                    int kinds);
#define PP_KIND_CONV_IGEMM 0
#define PP_KIND_CONV_WGRAD 1
#define PP_KIND_BN 2
#define PP_KIND_SPATIAL 3
#define PP_KIND_LOSS 4
#define PP_KIND_OPTIM 5
#define PP_KIND_MISC 6
#define PP_KIND_WINO_GEMM 7   /* flops booked = executed transform-domain flops (8 per pixel*cin*cout) */
#define PP_KIND_WINO_WGRAD 8
#define PP_KIND_WINO_XFORM 9
#define PP_KIND_CONV_F16X3 10  /* flops booked = executed 16-bit MFMA flops (3 per algorithmic flop) */
#define PP_KIND_WINO_GEMM_F16X3 11
#define PP_KIND_WINO_WGRAD_F16X3 12
#define PP_KIND_CONV_WGRAD_F16X3 13
#define PP_KIND_CONV_HALO_F16X3 14 /* conv3x3_halo_f16x3_kernel; kind 10 is conv3x3_igemm_f16x3_kernel */
#define PP_KIND_COUNT 15

/* ---- layout conversion at the module boundary --------------------------------------------------------- */
/* batch['image'] (N,C,H,W) -> NHWC, channels zero-padded to Cpad (train_chaos.py:269 -> models/unet.py:63). */
int pp_pack_image_nchw_to_nhwc(const float* src, int N, int C, int H, int W, float* dst, int ld_dst, int Cpad,
                               void* stream);
/* nn.Conv2d weight (O,I,3,3) -> wf[O][9][Ipad] (forward operand) and wb[I][9][O] with taps flipped (data-gradient
 * operand; may be NULL). */
int pp_pack_conv3x3_weights(const float* w_oihw, int O, int I, int Ipad, float* wf, float* wb, void* stream);

/* ---- 3x3 convolution, stride 1, padding = dilation (nn.Conv2d at models/unet.py:188, aux_path_memory.py:24) ---- */
/* out[p][n] = sum_{tap,c} in[p+off(tap)*dil][c] * wf[n][tap][c] + bias[n]  (+ previous out if accumulate) */
int pp_conv3x3_fwd(const float* in, int ld_in, int C, const float* wf, const float* bias, float* out, int ld_out,
                   int N, int B, int H, int W, int dil, int accumulate, void* stream);
/* autograd of the same Conv2d wrt its input: dx[p][c] (+)= sum_{tap,o} dz[p-off(tap)*dil][o] * W[o][c][tap] */
int pp_conv3x3_bwd_data(const float* dz, int ld_dz, int O, const float* wb, float* dx, int ld_dx, int I, int B,
                        int H, int W, int dil, int accumulate, void* stream);
/* ... and wrt its weight, written in the nn.Conv2d layout: dw[o][c][ky][kx] (+)= sum_p dz[p][o] * x[p+off][c] */
size_t pp_conv3x3_bwd_weight_workspace(int O, int Cpad, int B, int H, int W);
/* (no reference counterpart) which launch plan pp_conv3x3_bwd_weight (f16x3 = 0) or pp_conv3x3_bwd_weight_f16x3 given a dz_amax
 * (f16x3 = 1) runs for a shape with fp32 storage: a pure host query through the launchers' own plan functions, quoted by the
 * tests to show which state of a plan a case exercised.  (The halo paths depend on the calling thread's pp_set_wgrad_cus budget;
 * the 16-bit storage builds have no wgrad9 kernel and run the generic plan where this says PP_WGRAD_PATH_WGRAD9.)
 * Returns PP_WGRAD_PATH_*; out (nullable) receives 6 ints: [0] partial slabs the finalize sums, [1] units per split, [2] units in
 * the last split, [3] units in all, [4] splits that got a unit, [5] pixels in the last unit.  A unit is a chunk of 128 / 64 / 32
 * pixels (tile 32 / 64 / 128), a 64-pixel row segment (wgrad9), a wave's pixel run (c4: a split is a block of four waves), a
 * 4 x 32 pixel tile (halo: a split is a tile walker; [1] the tiles of walker 0, [2] those of the last walker that has any). */
#define PP_WGRAD_PATH_C4 1        /* Cpad == 4 first layer */
#define PP_WGRAD_PATH_WGRAD9 2    /* nine taps per staged row segment (fp32, dilation 1, W % 64 == 0, O <= 64, C <= 192) */
#define PP_WGRAD_PATH_TILE32 3    /* generic split-K kernel, 32 / 64 / 128 channel tiles */
#define PP_WGRAD_PATH_TILE64 4
#define PP_WGRAD_PATH_TILE128 5
#define PP_WGRAD_PATH_HALO 6      /* split-fp16 halo-tile walkers, one (32 x 32) channel pair per block */
#define PP_WGRAD_PATH_HALO_2X1 7  /* ... two pairs per block: two output blocks share the x patch */
#define PP_WGRAD_PATH_HALO_1X2 8  /* ... two input blocks share the dz tile (the last group half empty for 96 / 160 channels) */
int pp_conv3x3_bwd_weight_plan(int O, int Cpad, int B, int H, int W, int dil, int f16x3, int* out);
int pp_conv3x3_bwd_weight(const float* dz, int ld_dz, int O, const float* x, int ld_x, int Cpad, int I_true, int B,
                          int H, int W, int dil, float* dw_oihw, int accumulate, float* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- the same convolution on the fp16 matrix cores with split operands ("f16x3") ----------------------------- */
/* Every fp32 operand is split as x ~ hi + lo * 2^-11 (two fp16 numbers) and a*b is evaluated as ah*bh + 2^-11 *
 * (ah*bl + al*bh) with fp32 accumulation: fp32-grade results (the dropped term is 2^-22 relative) at 16x the MFMA
 * rate of the fp32 instruction.  Weights are split once by pp_pack_conv3x3_weights_f16x3 (same sizes and indexing as
 * the fp32 layouts of pp_pack_conv3x3_weights: every 4 consecutive K elements become 16 bytes [hi0..3 | lo0..3]),
 * activations while they are staged.  `in_amax` / `dz_amax`: NULL, or a device float holding max|operand|; the
 * operand is then scaled by a power of two into the fp16 range and the result scaled back (needed for gradients). */
int pp_pack_conv3x3_weights_f16x3(const float* w_oihw, int O, int I, int Ipad, void* wf16, void* wb16, void* stream);
/* the same for n layers in ONE launch (the per-layer launches sit behind one another at the start of every training step):
 * `items` is a HOST array, read during the call; fields as the arguments of pp_pack_conv3x3_weights_f16x3 */
typedef struct pp_pack_item { const float* w_oihw; int O, I, Ipad; void* wf16; void* wb16; } pp_pack_item;
int pp_pack_conv3x3_weights_f16x3_batch(const pp_pack_item* items, int n, void* stream);
int pp_conv3x3_fwd_f16x3(const float* in, int ld_in, int C, const void* wf16, const float* bias, float* out, int ld_out,
                         int N, int B, int H, int W, int dil, int accumulate, const float* in_amax, void* stream);
int pp_conv3x3_bwd_data_f16x3(const float* dz, int ld_dz, int O, const void* wb16, float* dx, int ld_dx, int I, int B,
                              int H, int W, int dil, int accumulate, const float* dz_amax, void* stream);
/* weight gradient, same workspace as pp_conv3x3_bwd_weight; shapes the split-fp16 kernel does not cover (dilation > 1,
 * channel counts that are not multiples of 32, W % 32, H % 4) and dz_amax == NULL run the fp32 kernels */
int pp_conv3x3_bwd_weight_f16x3(const float* dz, int ld_dz, int O, const float* x, int ld_x, int Cpad, int I_true, int B,
                                int H, int W, int dil, float* dw_oihw, int accumulate, float* workspace,
                                size_t workspace_bytes, const float* dz_amax, void* stream);

/* ---- the same convolution through Winograd F(2x2,3x3) (fp32, 2.25x less matrix work; wide layers) ------------ */
/* output-tile edge the library uses for an image shape: 4 = F(4x4,3x3) (36 planes) when H, W are multiples of
 * 4*dil, else 2 = F(2x2,3x3) (16 planes) */
int pp_conv3x3_wino_tile(int H, int W, int dil);
/* Uf[planes][O][I] = G g G^T, Ub[planes][I][O] = transform of the flipped kernel (data gradient); either may be NULL */
int pp_wino_pack_weights(const float* w_oihw, int O, int I, int tile, float* Uf, float* Ub, void* stream);
size_t pp_conv3x3_wino_workspace(int Cin, int Cout, int B, int H, int W, int dil);
size_t pp_conv3x3_wino_vkeep_elems(int Cin, int B, int H, int W, int dil);
/* v_keep (nullable, pp_conv3x3_wino_vkeep_elems floats): receives the transformed input so the weight gradient can reuse it */
int pp_conv3x3_wino_fwd(const float* in, int ld_in, int C, const float* Uf, const float* bias, float* out, int ld_out,
                        int N, int B, int H, int W, int dil, int accumulate, float* v_keep, void* workspace,
                        size_t workspace_bytes, void* stream);
int pp_conv3x3_wino_bwd_data(const float* dz, int ld_dz, int O, const float* Ub, float* dx, int ld_dx, int I, int B,
                             int H, int W, int dil, int accumulate, void* workspace, size_t workspace_bytes,
                             void* stream);
/* split-fp16 ("f16x3") forms of the two calls above for the F(4x4,3x3) geometry (pp_conv3x3_wino_tile == 4) with the GEMM
 * K (input channels forward, output channels in the data gradient) a multiple of 8: U from pp_wino_pack_weights_f16x3
 * (pre-split OCTETS [hi 8 x fp16 | lo 8 x fp16] along K, same sizes as the fp32 U); the input transform writes the
 * transformed input in the same layout, scaled by a power of two that is fixed BEFORE it runs: 2^-4 for activations,
 * for gradients taken from dz_amax = max |dz| (nullable device float; the BatchNorm backward kernels that write dz
 * collect it; null costs one extra pass over dz).  Workspace as for the fp32 calls. */
int pp_wino_pack_weights_f16x3(const float* w_oihw, int O, int I, int tile, void* Uf16, void* Ub16, void* stream);
/* ... and for n layers in ONE launch (tile 4; `items` is a HOST array, read during the call) */
typedef struct pp_wino_pack_item { const float* w_oihw; int O, I; void* Uf16; void* Ub16; } pp_wino_pack_item;
int pp_wino_pack_weights_f16x3_batch(const pp_wino_pack_item* items, int n, void* stream);
int pp_conv3x3_wino_fwd_f16x3(const float* in, int ld_in, int C, const void* Uf16, const float* bias, float* out,
                              int ld_out, int N, int B, int H, int W, int dil, int accumulate, float* v_keep,
                              void* workspace, size_t workspace_bytes, void* stream);
int pp_conv3x3_wino_bwd_data_f16x3(const float* dz, int ld_dz, int O, const void* Ub16, float* dx, int ld_dx, int I, int B,
                                   int H, int W, int dil, int accumulate, void* workspace, size_t workspace_bytes,
                                   const float* dz_amax, void* stream);
size_t pp_conv3x3_wino_bwd_weight_workspace(int O, int C, int B, int H, int W, int dil);
/* reduction splits the weight-gradient GEMM of this shape runs with (shape-only; quoted by the parity tests) */
int pp_conv3x3_wino_bwd_weight_splits(int O, int C, int B, int H, int W, int dil);
/* ... and the rest of that plan; returns the splits, out (nullable) receives 6 ints: [0] rows of a GEMM block (64 / 128),
 * [1] 32-tile chunks per split, [2] chunks in the last split, [3] chunks in all, [4] tiles in the last chunk, [5] tiles in all */
int pp_conv3x3_wino_bwd_weight_plan(int O, int C, int B, int H, int W, int dil, int* out);
/* v_cached (nullable): the v_keep of the forward call on the same x; when given, x is not read again */
int pp_conv3x3_wino_bwd_weight(const float* dz, int ld_dz, int O, const float* x, int ld_x, int C, int B, int H, int W,
                               int dil, float* dw_oihw, int accumulate, const float* v_cached, void* workspace,
                               size_t workspace_bytes, void* stream);
/* split-fp16 GEMM form (F(4x4,3x3) geometry, O and C multiples of 8); a cached V must have been written by a
 * pp_conv3x3_wino_fwd_f16x3 / pp_conv3x3_wino_fwd_bn(f16x3 = 1) call that received it as v_keep (pre-split octets) */
int pp_conv3x3_wino_bwd_weight_f16x3(const float* dz, int ld_dz, int O, const float* x, int ld_x, int C, int B, int H, int W,
                               int dil, float* dw_oihw, int accumulate, const float* v_cached, void* workspace,
                               size_t workspace_bytes, const float* dz_amax, void* stream);

/* ---- BatchNorm2d + LeakyReLU (models/unet.py:189-193, aux_path_memory.py:25-26) ------------------------- */
size_t pp_bn_workspace(int C, int P_per_group, int groups);
/* train mode: batch statistics per group, running-stat / num_batches_tracked update (one per group, in order),
 * save_mean / save_invstd [groups][C] and the fused coefficients scale = gamma*invstd, shift = beta - mean*scale. */
int pp_bn_train_stats(const float* z, int ld, int C, int P_per_group, int groups, float eps, float momentum,
                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, float* save_mean, float* save_invstd, float* scale,
                      float* shift, void* workspace, size_t workspace_bytes, void* stream);
/* eval mode (what train_chaos.py:370 leaves the model in): coefficients from the running statistics. */
int pp_bn_eval_coeffs(int C, int groups, float eps, const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var, float* save_mean, float* save_invstd,
                      float* scale, float* shift, void* stream);
/* ... for every BatchNorm layer of a network in ONE launch (round 6; eval mode: all coefficients are known when the step starts).
 * The rows written are bit-identical to pp_bn_eval_coeffs'. */
typedef struct pp_bn_coef_item {
  int C, groups;
  const float *gamma, *beta, *running_mean, *running_var;
  float *save_mean, *save_invstd, *scale, *shift;      /* [groups][C] each */
} pp_bn_coef_item;
int pp_bn_eval_coeffs_batch(const pp_bn_coef_item* items, int n, float eps, void* stream);
/* y = leaky_relu(z*scale + shift, slope) */
int pp_bn_lrelu_fwd(const float* z, int ld_z, const float* scale, const float* shift, float* y, int ld_y, int C,
                    int P_per_group, int groups, float slope, void* stream);
/* ... and the 2x2 max-pooled copy of y in the same pass (the train-mode forward of an encoder stage's last layer: its output
 * feeds the skip connection and nn.MaxPool2d(2, 2), models/unet.py:109,123-127); pooled is (B, H/2, W/2, C) */
int pp_bn_lrelu_fwd_pool(const float* z, int ld_z, const float* scale, const float* shift, float* y, int ld_y, float* pooled,
                         int ld_pooled, int C, int B, int H, int W, int groups, float slope, void* stream);
/* autograd of LeakyReLU(BatchNorm(z)): dz, dgamma, dbeta, and the gradient of the preceding conv bias.
 * workspace >= pp_bn_workspace(...) + 3*groups*C*sizeof(float). */
int pp_bn_lrelu_bwd(const float* dy, int ld_dy, const float* z, int ld_z, const float* scale, const float* shift,
                    const float* save_mean, const float* save_invstd, const float* gamma, int training, float* dz,
                    int ld_dz, float* dgamma, float* dbeta, float* dbias_conv, int accumulate_param_grads, int C,
                    int P_per_group, int groups, float slope, void* workspace, size_t workspace_bytes,
                    void* stream);
/* same, additionally *dz_amax = max |dz| (device float): operand scale for pp_conv3x3_bwd_data_f16x3 */
int pp_bn_lrelu_bwd_amax(const float* dy, int ld_dy, const float* z, int ld_z, const float* scale, const float* shift,
                    const float* save_mean, const float* save_invstd, const float* gamma, int training, float* dz,
                    int ld_dz, float* dgamma, float* dbeta, float* dbias_conv, int accumulate_param_grads, int C,
                    int P_per_group, int groups, float slope, void* workspace, size_t workspace_bytes,
                    float* dz_amax, void* stream);

/* Synchronised BatchNorm for data-parallel training while BN is in train mode (the reference normalises over the WHOLE
 * batch, models/unet.py:189; reference has no multi-GPU path, SURVEY.md 8(e) coupling A).  Each call above is split in
 * two so the caller can all-reduce the per-channel sums (double [groups][2][C]) over the ranks in between:
 *   forward : pp_bn_stats_sums -> all-reduce -> pp_bn_train_finalize(n = GLOBAL pixels per group)
 *   backward: pp_bn_lrelu_bwd_sums -> all-reduce of a copy -> pp_bn_lrelu_bwd_apply(local sums, global sums, global n):
 *             dz uses the global sums, dgamma / dbeta / dbias the local ones (the gradient all-reduce adds the ranks).
 * pp_bn_lrelu_bwd_apply workspace >= 6*groups*C floats + 16. */
int pp_bn_stats_sums(const float* z, int ld, int C, int P_per_group, int groups, double* sums, void* workspace,
                     size_t workspace_bytes, void* stream);
int pp_bn_train_finalize(const double* sums, int rows /* partial rows per group; 1 for pp_bn_stats_sums output */, int C,
                         int n_per_group, int groups, float eps, float momentum,
                         const float* gamma, const float* beta, float* running_mean, float* running_var,
                         int64_t* num_batches_tracked, float* save_mean, float* save_invstd, float* scale, float* shift,
                         void* stream);
/* the same, and additionally the (scale, shift, slope) rows of the layer's LAZY output tensor (pp_lazy_in above): lazy_coef
 * points at the layer's channel 0 inside rows of lazy_ld floats.  The engine then skips pp_bn_lrelu_fwd: the consumers of
 * the tensor apply BatchNorm + LeakyReLU while they load (models/unet.py:189-193 executed inside the next layer). */
int pp_bn_train_finalize_lazy(const double* sums, int rows, int C, int n_per_group, int groups, float eps, float momentum,
                              const float* gamma, const float* beta, float* running_mean, float* running_var,
                              int64_t* num_batches_tracked, float* save_mean, float* save_invstd, float* scale,
                              float* shift, float* lazy_coef, int lazy_ld, float slope, void* stream);
/* dst = LeakyReLU(BN(src)) of a lazy tensor (B images of HW pixels, C channels): for consumers without a *_lazy form */
int pp_lazy_materialize(const float* src, int ld_src, const pp_lazy_in* lazy, float* dst, int ld_dst, int C, int B, int HW,
                        void* stream);
int pp_bn_lrelu_bwd_sums(const float* dy, int ld_dy, const float* z, int ld_z, const float* scale, const float* shift,
                         const float* save_mean, const float* save_invstd, int C, int P_per_group, int groups,
                         float slope, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int pp_bn_lrelu_bwd_apply(const float* dy, int ld_dy, const float* z, int ld_z, const float* scale, const float* shift,
                          const float* save_mean, const float* save_invstd, const float* gamma, int training,
                          const double* local_sums, const double* global_sums, int n_global_per_group, float* dz,
                          int ld_dz, float* dgamma, float* dbeta, float* dbias_conv, int accumulate_param_grads, int C,
                          int P_per_group, int groups, float slope, void* workspace, size_t workspace_bytes,
                          float* dz_amax /* nullable */, void* stream);

/* ---- convolution with the BatchNorm that follows it fused into the kernel epilogue ----------------------------------
 * The reference block is conv -> BatchNorm2d -> LeakyReLU (models/unet.py:188-193).  These forward calls replace
 * pp_conv3x3_fwd[_f16x3] / pp_conv3x3_wino_fwd[_f16x3] + pp_bn_train_stats / pp_bn_lrelu_fwd where BatchNorm needs no
 * second look at the convolution output:
 *   bn_mode 1 (BN in train mode): out = z, and the kernel emits per-block (sum z, sum z^2) per channel into
 *       stats[groups][*rows_out][2][N] (double) -> pp_bn_train_finalize(stats, *rows_out, ...) -> pp_bn_lrelu_fwd.
 *       The statistics pass over z is gone.
 *   bn_mode 2 (BN in eval mode, the reference's state from epoch 1 on, train_chaos.py:370): scale / shift [N] from
 *       pp_bn_eval_coeffs are known up front, out = y = leaky_relu(z*scale + shift, slope); z never reaches HBM, and
 *       pp_bn_lrelu_bwd_eval reads the LeakyReLU branch from the sign of y.
 * Kernel variants without a fused epilogue run the unfused BatchNorm kernels inside the call: results are the same.
 * f16x3 != 0: w / U are the split-fp16 packs and the split-fp16 kernels run.  stats: >= pp_conv3x3_bn_stats_bytes. */
size_t pp_conv3x3_bn_stats_bytes(int N, int B, int H, int W, int groups);
int pp_conv3x3_fwd_bn(const float* in, int ld_in, int C, const void* wf, const float* bias, float* out, int ld_out, int N,
                      int B, int H, int W, int dil, int f16x3, const float* in_amax, int bn_mode, const float* scale,
                      const float* shift, float slope, int groups, double* stats, size_t stats_bytes, int* rows_out,
                      void* stream);
int pp_conv3x3_wino_fwd_bn(const float* in, int ld_in, int C, const void* U, const float* bias, float* out, int ld_out,
                           int N, int B, int H, int W, int dil, int f16x3, float* v_keep, void* workspace,
                           size_t workspace_bytes, int bn_mode, const float* scale, const float* shift, float slope,
                           int groups, double* stats, size_t stats_bytes, int* rows_out, void* stream);
/* Round 4, the conv -> conv halves of a DoubleConv (models/unet.py:160-170, narrow layers): pp_conv3x3_fwd_bn with a LAZY input,
 * and the split-fp16 weight gradient with a lazy x -- `in` / `x` hold the raw output z of the first convolution, BatchNorm +
 * LeakyReLU are applied while the two-half halo kernel (forward) / the halo-tile weight-gradient kernels stage their patches;
 * zero padding applies to y.  At most two statistics groups.  pp_conv3x3_lazy_ok: 1 when BOTH calls accept this layer shape
 * (C input, N output channels), else 0 -- a pure function of the shape; other shapes fail with PP_ERR_UNSUPPORTED. */
int pp_conv3x3_lazy_ok(int C, int N, int B, int H, int W, int dil);
int pp_conv3x3_fwd_bn_lazy(const float* in, int ld_in, int C, const void* wf, const float* bias, float* out, int ld_out, int N,
                           int B, int H, int W, int dil, int f16x3, const float* in_amax, int bn_mode, const float* scale,
                           const float* shift, float slope, int groups, double* stats, size_t stats_bytes, int* rows_out,
                           const pp_lazy_in* lazy_in, void* stream);
/* (16-bit storage builds, _h16 / _bf16: the lazy weight gradient stages y = lrelu(z * scale + shift) as fp16 and never stores it,
 * so in bf16 storage it is NOT bit-identical to the entry fed the stored y; the engine's 16-bit plans do not take this form
 * (engine.LAZY_HALO_H16) and the launch census does not cover it in 16-bit storage -- fp32 storage only.) */
int pp_conv3x3_bwd_weight_f16x3_lazy(const float* dz, int ld_dz, int O, const float* x, int ld_x, int Cpad, int I_true, int B,
                                     int H, int W, int dil, float* dw_oihw, int accumulate, float* workspace,
                                     size_t workspace_bytes, const float* dz_amax, const pp_lazy_in* lazy_x, void* stream);
/* autograd of LeakyReLU(BatchNorm_eval(z)) from dy and y alone, one pass: dz = scale*g, dgamma, dbeta, conv-bias grad.
 * scale = gamma*invstd [C] (pp_bn_eval_coeffs); P_total = all pixels of the launch (statistics are not per group in
 * eval mode); workspace >= pp_bn_workspace(C, P_total, 1); dz_amax nullable (max |dz| for the split-fp16 consumers). */
int pp_bn_lrelu_bwd_eval(const float* dy, int ld_dy, const float* y, int ld_y, const float* scale, const float* gamma,
                         const float* beta, float* dz, int ld_dz, float* dgamma, float* dbeta, float* dbias_conv,
                         int accumulate_param_grads, int C, int P_total, float slope, void* workspace,
                         size_t workspace_bytes, float* dz_amax, void* stream);
/* BatchNorm + LeakyReLU backward of an encoder stage's last layer with the gradient of the nn.MaxPool2d(2, 2) that follows it
 * (models/unet.py:109,123-127) folded in: dy = gradient arriving through the skip connection (B, H, W), dpool = gradient of
 * the pooled tensor (B, H/2, W/2); the kernels find each window's winner themselves (first maximum of y, PyTorch's rule) and
 * add dpool to it on the fly, so the separate pp_maxpool2_bwd pass over the skip-gradient buffer does not run.
 * pp_bn_lrelu_bwd_pool: train-mode statistics (or training = 0), arguments as pp_bn_lrelu_bwd_amax, dz_amax nullable.
 * pp_bn_lrelu_bwd_eval_pool: the one-pass eval form on the stored output y, arguments as pp_bn_lrelu_bwd_eval. */
int pp_bn_lrelu_bwd_pool(const float* dy, int ld_dy, const float* dpool, int ld_dpool, const float* z, int ld_z,
                         const float* scale, const float* shift, const float* save_mean, const float* save_invstd,
                         const float* gamma, int training, float* dz, int ld_dz, float* dgamma, float* dbeta,
                         float* dbias_conv, int accumulate_param_grads, int C, int B, int H, int W, int groups, float slope,
                         void* workspace, size_t workspace_bytes, float* dz_amax, void* stream);
int pp_bn_lrelu_bwd_eval_pool(const float* dy, int ld_dy, const float* dpool, int ld_dpool, const float* y, int ld_y,
                              const float* scale, const float* gamma, const float* beta, float* dz, int ld_dz, float* dgamma,
                              float* dbeta, float* dbias_conv, int accumulate_param_grads, int C, int B, int H, int W,
                              float slope, void* workspace, size_t workspace_bytes, float* dz_amax, void* stream);

/* ---- GroupNorm + LeakyReLU (--norm_op group; the reference's ConvLayer with norm_op = nn.GroupNorm, models/unet.py:178-193) ----
 * nn.GroupNorm(G, C, eps, affine) -> nn.LeakyReLU(slope) on N images of H*W pixels (HW = H*W), NHWC fp32 with row stride ld >= C.
 * Statistics are per (image, channel group) in train and eval mode alike.  pp_gn_stats writes per-(image, channel) rows [N][C]:
 * save_mean / save_invstd (the group's statistics, repeated for each channel of the group), save_xbar (mean over the image of
 * xhat in that channel: the backward's conv-bias term), scale = gamma * invstd, shift = beta - mean * scale.  The forward apply
 * is pp_bn_lrelu_fwd / pp_bn_lrelu_fwd_pool with P_per_group = HW and groups = N (one coefficient row per image).
 * pp_gn_lrelu_bwd: dz, dgamma, dbeta and the conv-bias gradient (sum of dz), each (accumulate_param_grads) added to or stored;
 * dz_amax nullable (max |dz|).  pp_gn_lrelu_bwd_pool: the same when the layer output also feeds a 2x2 max-pooling whose
 * gradient dpool (N, H/2, W/2) is added to each window's winner.  All three share one workspace of pp_gn_workspace bytes.
 * Deterministic (fixed-order reductions), C % 4 == 0, C <= 1024, G divides C.  fp32 storage only. */
size_t pp_gn_workspace(int C, int HW, int N);
int pp_gn_stats(const float* z, int ld, int C, int HW, int N, int G, float eps, const float* gamma, const float* beta,
                float* save_mean, float* save_invstd, float* save_xbar, float* scale, float* shift, void* workspace,
                size_t workspace_bytes, void* stream);
int pp_gn_lrelu_bwd(const float* dy, int ld_dy, const float* z, int ld_z, const float* scale, const float* shift,
                    const float* save_mean, const float* save_invstd, const float* save_xbar, const float* gamma, float* dz,
                    int ld_dz, float* dgamma, float* dbeta, float* dbias_conv, int accumulate_param_grads, int C, int HW, int N,
                    int G, float slope, void* workspace, size_t workspace_bytes, float* dz_amax, void* stream);
int pp_gn_lrelu_bwd_pool(const float* dy, int ld_dy, const float* dpool, int ld_dpool, const float* z, int ld_z,
                         const float* scale, const float* shift, const float* save_mean, const float* save_invstd,
                         const float* save_xbar, const float* gamma, float* dz, int ld_dz, float* dgamma, float* dbeta,
                         float* dbias_conv, int accumulate_param_grads, int C, int N, int H, int W, int G, float slope,
                         void* workspace, size_t workspace_bytes, float* dz_amax, void* stream);
/* BatchNorm + LeakyReLU backward of the network's FIRST layer (models/unet.py:188-193 on `input_ch` = 1, every dataset of the
 * reference) with that layer's weight gradient folded in: nobody asks for the data gradient of the first convolution, so dz had
 * one reader -- the weight gradient, the last kernel of the backward pass.  The pass that forms dz multiplies it with the 3x3
 * neighbourhood of the one-channel input x (channel 0 of an NHWC tensor with row stride ld_x, zero padding, dilation 1) and
 * leaves dW [C][1][3][3] (accumulate_dw: added to it); dz is never written.  A group is a whole number of H x W images.
 * Other arguments as pp_bn_lrelu_bwd / pp_bn_lrelu_bwd_eval; workspace >= pp_bn_lrelu_bwd_wgrad_c1_workspace (eval: groups = 1). */
size_t pp_bn_lrelu_bwd_wgrad_c1_workspace(int C, int P_per_group, int groups);
int pp_bn_lrelu_bwd_wgrad_c1(const float* dy, int ld_dy, const float* z, int ld_z, const float* scale, const float* shift,
                             const float* save_mean, const float* save_invstd, const float* gamma, int training,
                             const float* x, int ld_x, int H, int W, float* dw_o1hw, int accumulate_dw, float* dgamma,
                             float* dbeta, float* dbias_conv, int accumulate_param_grads, int C, int P_per_group, int groups,
                             float slope, void* workspace, size_t workspace_bytes, void* stream);
int pp_bn_lrelu_bwd_eval_wgrad_c1(const float* dy, int ld_dy, const float* y, int ld_y, const float* scale, const float* gamma,
                                  const float* beta, const float* x, int ld_x, int H, int W, float* dw_o1hw, int accumulate_dw,
                                  float* dgamma, float* dbeta, float* dbias_conv, int accumulate_param_grads, int C,
                                  int P_total, float slope, void* workspace, size_t workspace_bytes, void* stream);

/* ---- pooling / resampling (models/unet.py:109,144; aux_path_memory.py:52,75) ---------------------------- */
int pp_maxpool2_fwd(const float* x, int ld_x, float* y, int ld_y, int C, int N, int H, int W, void* stream);
int pp_maxpool2_bwd(const float* x, int ld_x, const float* dy, int ld_dy, float* dx, int ld_dx, int C, int N, int H,
                    int W, int accumulate, void* stream);
/* bilinear, align_corners=True, any size (nn.Upsample / F.interpolate) */
int pp_bilinear_fwd(const float* x, int ld_x, float* y, int ld_y, int C, int N, int Hi, int Wi, int Ho, int Wo,
                    void* stream);
int pp_bilinear_bwd(const float* dy, int ld_dy, float* dx, int ld_dx, int C, int N, int Hi, int Wi, int Ho, int Wo,
                    int accumulate, void* stream);
/* y[p][0:C] (+)= x[p][0:C]: torch.cat placement / scale_factor=1 up-sampling (models/unet.py:151) */
int pp_copy_slab(const float* x, int ld_x, float* y, int ld_y, int C, long long P, int accumulate, void* stream);

/* y[n][p][c] (+)= x[n][p][c] * scale[n][c]: nn.Dropout2d (aux_path_memory.py:22,31) forward and backward; the caller draws
 * the per-(sample, channel) mask = 0 or 1/(1-p) and keeps it for the backward pass */
int pp_channel_scale(const float* x, int ld_x, float* y, int ld_y, const float* scale, int C, int N, int HW,
                     int accumulate, void* stream);

/* ---- synthetic scribbles (utils/utils_artificial_scribbles.py:5-35, utils/utils_shorten_scribble_length.py:32-75) ----
 * masks: uint8 [M][H][W] (0 / non-zero), processed in place, one workgroup per mask, (H+2)*(W+2) <= 81,888 (LDS).
 * pp_skeletonize = skimage.morphology.skeletonize (2-D Zhang-Suen thinning); pp_dilate_antidiagonal =
 * scipy.ndimage.binary_dilation(seed, np.eye(3)[::-1], iterations, mask); pp_curve_endpoints marks set pixels with exactly
 * one set 8-neighbour (the union of the reference's eight end-point convolution kernels). */
int pp_skeletonize(unsigned char* masks, int M, int H, int W, void* stream);
int pp_dilate_antidiagonal(unsigned char* seeds, const unsigned char* masks, int M, int H, int W, int iterations,
                           void* stream);
int pp_curve_endpoints(const unsigned char* img, unsigned char* out, int M, int H, int W, void* stream);

/* ---- input pipeline on the device: the two-stream augmentation of datasets/chaos/chaos_dataset.py:58-90
 * with the transforms of datasets/augmentations.py and the configuration of datasets/chaos/chaos_aug_configs.py:16-86.
 * The random decisions are drawn on the host (pacingpseudo_amd/augment.py, the reference's call order); these entry
 * points apply them to a whole batch in HBM.  Images: fp32 [B][Hp][Wp] planes; rect: int [B][4] = {top, left, h, w}
 * restricting a call to one rectangle per sample (NULL = whole plane); stats: double [B][4] = {mean, std, min, max}.
 *   pp_aug_stats        np.mean / np.std / np.min / np.max of each sample (MeanStdNorm :11-21, Contrast :112-129, Gamma :131-166)
 *   pp_aug_coef         {a, b, lo, hi} of the per-sample map from the statistics, on the device; mode 0 MeanStdNorm,
 *                       1 Contrast, 2 Gamma power step, 3 Gamma retain_stats, 4 Brightness; param[n] <= -1e30: not drawn
 *   pp_aug_scalar_map   x <- clip(a x + b, lo, hi);   pp_aug_gamma   x <- ((x - min) / (max - min + eps)) ^ gamma
 *   pp_aug_add_noise    x += sigma[n] N(0, 1) (GaussianNoise :353-366), Philox-4x32-10 keyed by `seed`
 *   pp_aug_warp         Scaling :184-226, RandomRotation :278-318, Mirroring :337-351, RandomCrop :368-418 (and the
 *                       displacement field of ElasticTransform :228-276) as ONE resampling: maps[n] = 12 floats
 *                       {a00, a01, a02, a10, a11, a12, top, left, patch_h, patch_w, hs, ws}, source (y, x) = A (yo, xo, 1);
 *                       image bicubic (cubic = 1, the cv2.INTER_CUBIC kernel), bilinear (0) or nearest (2); class maps nearest
 *   pp_aug_elastic_field  gaussian_filter(U(-1, 1), sigma) * alpha per sample and axis -> disp [B][2][H][W]; sigma_alpha [B][2]
 *   pp_aug_onehot       to_one_hot_encoding :448-461, int32 class map -> fp32 [B][K][HW] */
int pp_aug_stats(const float* x, int B, int Hp, int Wp, const int* rect, double* stats, void* stream);
int pp_aug_coef(const double* stats, const double* stats0, const float* param, int mode, int B, float* coef, void* stream);
int pp_aug_scalar_map(float* x, int B, int Hp, int Wp, const float* coef, const int* rect, void* stream);
int pp_aug_gamma(float* x, int B, int Hp, int Wp, const float* coef, const int* rect, void* stream);
int pp_aug_add_noise(float* x, int B, int Hp, int Wp, const float* sigma, const int* rect, unsigned long long seed,
                     void* stream);
int pp_aug_warp(const float* img, const int* lab, const int* scb, int Hp, int Wp, float* out_img, int* out_lab, int* out_scb,
                float* out_valid, int Ho, int Wo, int B, const float* maps, const float* disp, const double* clip_stats,
                float img_pad, int lab_pad, int cubic, void* stream);
int pp_aug_elastic_field(float* disp, float* scratch, int B, int H, int W, const float* sigma_alpha, unsigned long long seed,
                         void* stream);
/* ElasticTransform's own interpolant (augmentations.py:270: scipy.ndimage.map_coordinates(order = 3, mode = 'nearest')):
 * pp_aug_spline_prefilter turns the flagged samples (use[n] != 0) of a batch into cubic B-spline coefficients -- edge padding
 * by 12, float64 recursive prefilter with scipy's 'reflect' initialisation, coef [B][Hp + 24][Wp + 24] -- and
 * pp_aug_warp_spline is pp_aug_warp with those samples' image taps evaluated from the coefficients (coordinates and the
 * class-map rounding in double; disp64, nullable, a double-precision displacement field in place of disp). */
int pp_aug_spline_prefilter(const float* img, int B, int Hp, int Wp, const float* maps, const int* use, double* coef, void* stream);
int pp_aug_warp_spline(const float* img, const int* lab, const int* scb, int Hp, int Wp, float* out_img, int* out_lab, int* out_scb,
                       float* out_valid, int Ho, int Wo, int B, const float* maps, const float* disp, const double* disp64,
                       const double* clip_stats, float img_pad, int lab_pad, int cubic, const double* spline_coef, const int* use,
                       void* stream);
int pp_aug_onehot(const int* lab, float* out, int B, int K, int HW, void* stream);
/* strong-view extras of TransformsColorBlur / Mixup / Low (chaos_aug_configs.py:88-186): GaussianBlur :82-95 (sigma_pad
 * [B][2] = {sigma, unused}, <= 0: untouched), Mixup :51-80 (x <- lam x + (1 - lam) y, lam < 0: untouched);
 * SimulationLowRes :168-182 is two pp_aug_warp calls (cubic = 2: nearest, then cubic = 1) */
int pp_aug_gaussian_blur(float* x, float* scratch, int B, int H, int W, const float* sigma_pad, void* stream);
int pp_aug_mix(float* x, const float* y, int B, int HW, const float* lam, void* stream);
/* GaussianNoise (augmentations.py:353-366) with the normal field given by the caller: x += f inside rect[n] (nullable) */
int pp_aug_add_field(float* x, const float* f, int B, int Hp, int Wp, const int* rect, void* stream);

/* ---- the `is_stride_conv` / `is_trans_conv` U-Net variants (models/unet.py:100-152) ------------------------------------ */
/* stride-2 / padding-1 3x3 convolution (EncBlock, unet.py:113-116) = the stride-1 convolution sampled at the even pixels:
 * out (N, Ho, Wo, C) = full (N, 2 Ho, 2 Wo, C)[:, ::2, ::2]; its gradients are those of the stride-1 convolution for the
 * zero-stuffed dz that pp_stride2_scatter writes */
int pp_stride2_gather(const float* full, int ld_full, float* out, int ld_out, int C, int N, int Ho, int Wo, void* stream);
int pp_stride2_scatter(const float* dz, int ld_dz, float* full, int ld_full, int C, int N, int Ho, int Wo, void* stream);
/* nn.ConvTranspose2d(Cin, Cout, k, k, bias=False) of DecBlock (unet.py:139-141), k = kernel = stride = 1 or 2, weight in
 * PyTorch's layout [Cin][Cout][k][k]; x (N, H, W, Cin) NHWC -> out (N, k H, k W, Cout); fp32 */
int pp_convtranspose_fwd(const float* x, int ld_x, int Cin, const float* w, float* out, int ld_out, int Cout, int k, int N,
                         int H, int W, void* stream);
int pp_convtranspose_bwd_data(const float* dout, int ld_dout, int Cout, const float* w, float* dx, int ld_dx, int Cin, int k,
                              int N, int H, int W, int accumulate, void* stream);
size_t pp_convtranspose_bwd_weight_workspace(int Cin, int Cout, int k, int N, int H, int W);
/* reduction splits of pp_convtranspose_bwd_weight for N*H*W input pixels (shape-only; quoted by the tests); out (nullable)
 * receives [0] pixels per split, [1] pixels in the last split */
int pp_convtranspose_bwd_weight_splits(int N, int H, int W, int* out);
int pp_convtranspose_bwd_weight(const float* dout, int ld_dout, int Cout, const float* x, int ld_x, int Cin, int k, int N, int H,
                                int W, float* dw, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- 1x1 heads: final_conv (models/unet.py:60) and aux fc_cls (aux_path_memory.py:32), NHWC -> NCHW logits ---- */
/* 1 <= K <= 32 classes (an argument error names the bound), C <= 128 and a multiple of 4 */
int pp_conv1x1_nhwc_to_nchw_fwd(const float* x, int ld_x, int C, const float* w, const float* bias, float* logits,
                                int K, int N, int HW, void* stream);
/* ... with a lazy x (the features of dec_block1 kept as raw convolution output in train-mode BN) */
int pp_conv1x1_nhwc_to_nchw_fwd_lazy(const float* x, int ld_x, int C, const float* w, const float* bias, float* logits,
                                int K, int N, int HW, const pp_lazy_in* lazy_x, void* stream);
size_t pp_conv1x1_bwd_workspace(int K, int C, int N, int HW);
int pp_conv1x1_nchw_to_nhwc_bwd(const float* dlogits, const float* x, int ld_x, int C, const float* w, float* dx,
                                int ld_dx, float* dw, float* dbias, int K, int N, int HW, int accumulate_dx,
                                int accumulate_param_grads, void* workspace, size_t workspace_bytes, void* stream);
/* ... with a lazy x: dw is taken against y = LeakyReLU(BN(x)) */
int pp_conv1x1_nchw_to_nhwc_bwd_lazy(const float* dlogits, const float* x, int ld_x, int C, const float* w, float* dx,
                                int ld_dx, float* dw, float* dbias, int K, int N, int HW, int accumulate_dx,
                                int accumulate_param_grads, void* workspace, size_t workspace_bytes, const pp_lazy_in* lazy_x, void* stream);

/* ---- losses (losses/losses.py; models/consistency_reglur_memory.py:31-97) ------------------------------ */
/* every loss entry point with a class count K takes 1 <= K <= 32 (pp_argmax_channels and pp_hd95_surface_distances: any K) */
/* torch.argmax(x, dim=1) on (N,C,HW) fp32 -> int64, first maximum wins (bit-exact pseudo-label masks) */
int pp_argmax_channels(const float* x, int N, int C, int HW, int64_t* out, void* stream);
/* sums[6] (double): pCE sum, #labelled, entropy sum, entropy denominator, consistency sum, consistency denominator.
 * cr_variant: 0 none, 1 ce_loss, 2 l1_loss, 3 l2_loss, 4 kl_loss (train_chaos.py:138), 5 bikl_loss (half of KL(q||s) + KL(s||q)),
 * 6 js_loss (Jensen-Shannon), 7 hard_ce_loss (cross entropy of the strong view against the first arg-max of the weak logits).
 * Unmasked consistency denominator: N*HW*K for 1, 4, 5 (mean over N,K,H,W), N*HW for 2, 3, 6, 7 (channels reduced first); masked:
 * max(sum(valid_mask), 1e-8) for all.  detach_weak drops the weak-logit gradient of 1, 2, 3, 5, 6; 4 ignores it, 7 has none.
 * In data-parallel runs the
 * caller all-reduces `sums` before pp_losses_finalize / pp_seg_losses_bwd so losses and gradients are global. */
size_t pp_seg_losses_workspace(int N, int HW);
int pp_seg_losses_fwd(const float* logits_w, const float* logits_s, const int64_t* target, const float* valid_mask,
                      int N, int K, int HW, int ignore_index, int do_ent, int cr_variant, double* sums,
                      void* workspace, size_t workspace_bytes, void* stream);
int pp_losses_finalize(const double* sums, int has_mask, float* loss_pce, float* loss_ent, float* loss_cr,
                       void* stream);
/* dlogits = g_pce*dpce + g_ent*dent + g_cr*dcr (g_* are device scalars = the upstream gradients of each loss) */
int pp_seg_losses_bwd(const float* logits_w, const float* logits_s, const int64_t* target, const float* valid_mask,
                      int N, int K, int HW, int ignore_index, int do_ent, int cr_variant, int detach_weak,
                      const double* sums, const float* g_pce, const float* g_ent, const float* g_cr,
                      float grad_scale, float* dlogits_w, float* dlogits_s, void* stream);
/* auxiliary head: F.interpolate(logits (N,K,h,w) -> (H,W), bilinear, align_corners) fused with partial CE.
 * sums[2] = pCE sum, #labelled.  workspace >= 16 bytes (two doubles) per block of its grid of min(1024, ceil(N * H * W / 256))
 * blocks; pp_seg_losses_workspace(N, H * W), 40 bytes per block of the same grid, covers it (how the engine sizes it). */
int pp_aux_pce_fwd(const float* lo, int N, int K, int h, int w, int H, int W, const int64_t* target,
                   int ignore_index, float* logits_up, double* sums, void* workspace, size_t workspace_bytes,
                   void* stream);
int pp_aux_pce_bwd(const float* logits_up, const int64_t* target, int ignore_index, const float* g_aux,
                   float grad_scale, const double* sums, float* dlo, int N, int K, int h, int w, int H, int W,
                   void* stream);
/* AuxPath.memory_update for batch sample 0 (aux_path_memory.py:68-116).  feat0: NHWC (h,w,hid) features of sample 0,
 * scribble0: (K+1,H,W) one-hot of sample 0, bank: [K][hid], momentum_now = (1-step/max_step)^0.9 * base.  Round 6: two launches
 * (per-slice partial sums over the scribble plane, then the first-visit / EMA rule per class) through a caller-owned workspace of
 * pp_memory_update_workspace(K, hid) bytes. */
size_t pp_memory_update_workspace(int K, int hid);
int pp_memory_update(const float* feat0, int ld, int hid, int h, int w, const float* scribble0, int K, int H, int W,
                     float* bank, float momentum_now, int cosine_mode, void* workspace, size_t workspace_bytes, void* stream);
/* the same with feat0 stored as IEEE fp16 (16-bit storage mode: the entry points of pacingpseudo_hip_h16.h) */
int pp_memory_update_h16(const void* feat0, int ld, int hid, int h, int w, const float* scribble0, int K, int H, int W,
                         float* bank, float momentum_now, int cosine_mode, void* workspace, size_t workspace_bytes, void* stream);
/* ... and as bfloat16 (round 6: the entry points of pacingpseudo_hip_bf16.h) */
int pp_memory_update_bf16(const void* feat0, int ld, int hid, int h, int w, const float* scribble0, int K, int H, int W,
                          float* bank, float momentum_now, int cosine_mode, void* workspace, size_t workspace_bytes, void* stream);
/* cross_entropy(fc_cls(memory_bank), arange(K)) and its gradient wrt the fc_cls weight [K][hid] */
int pp_memory_ce_fwd(const float* bank, const float* wfc, int K, int hid, float* loss, void* stream);
int pp_memory_ce_bwd(const float* bank, const float* wfc, int K, int hid, const float* g, float grad_scale,
                     float* dwfc, int accumulate, void* stream);
/* the loss assembly of train_chaos.py:273-310 in one launch each way: *out = t[0][0] * w[0] + t[1][0] * w[1] + ... (n <= 8
 * 0-dim device losses; `terms` and `weights` are HOST arrays, read during the call; fp32 products and sums, left to right, as the
 * chain of torch operations computes them), and gout[i] = *g * w[i]. */
int pp_weighted_sum_fwd(const float* const* terms, const float* weights, int n, float* out, void* stream);
int pp_weighted_sum_bwd(const float* g, const float* weights, int n, float* gout, void* stream);
/* utils/metrics.py:compute_dice counts: counts[n][k] = {|P&T|, |P|, |T|} with P = argmax prediction */
int pp_dice_counts(const float* logits, const float* label_onehot, int N, int K, int HW, float* counts,
                   void* stream);

/* 95 % Hausdorff distance of inference.py:217-237 (medpy.metric.binary.hd95, connectivity 1): surface extraction and
 * both directed surface-distance sets per (image, class) on the device.  pred / label: int64 class maps [N][H][W];
 * dist: [N*K][2][H*W] floats, counts: [N*K][4] ints = {|surface pred|, |surface label|, |pred|, |label|}.  The caller takes
 * numpy.percentile(95) of the two sets together (NaN when a mask is empty or full, as the reference). */
size_t pp_hd95_workspace(int N, int K, int H, int W);
int pp_hd95_surface_distances(const int64_t* pred, const int64_t* label, int N, int K, int H, int W, float spacing_y,
                              float spacing_x, float* dist, int* counts, void* workspace, size_t workspace_bytes,
                              void* stream);

/* soft Dice loss of the fully-supervised trainer (losses/losses.py:147-162, upper_bound_chaos.py:165):
 * -mean_{n,k} 2 sum p t / (sum p + sum t + 1e-5) on soft-max probabilities.  sums: double [N][K][3] = {sum p t, sum p,
 * sum t}, written by the forward call and read by the backward one; dlogits (+)= g * grad_scale * dloss/dlogits. */
size_t pp_dice_loss_workspace(int N, int K);
int pp_dice_loss_fwd(const float* logits, const float* label_onehot, int N, int K, int HW, double* sums, float* loss,
                     void* workspace, size_t workspace_bytes, void* stream);
int pp_dice_loss_bwd(const float* logits, const float* label_onehot, int N, int K, int HW, const double* sums,
                     const float* g, float grad_scale, float* dlogits, int accumulate, void* stream);

/* Gated CRF / Potts regulariser on the weak-view logits (this implementation's addition):
 *   L = (1/D) sum_n sum_i sum_j m_i m_j k_ij (1 - <p_i, p_j>),  p = softmax(logits),  j = i + (dy, dx) * dilation with
 *   dy, dx in [-radius, radius] \ (0, 0) inside the image,
 *   k_ij = exp(-(dy^2 + dx^2) / (2 sigma_xy^2)) * exp(-|x_i - x_j|^2 / (2 sigma_rgb^2))   (|.|^2 over the C image channels)
 * logits (N,K,H,W), image (N,C,H,W), valid_mask (N,1,H,W) or NULL (m = 1); 1 <= K <= 32, C <= 4, 1 <= radius <= 8,
 * 1 <= dilation <= 4, radius * dilation <= 16, sigma > 0.  pp_crf_loss_fwd writes sums[0] = numerator, sums[1] = sum m (the
 * pixel count N H W without a mask) in double, in a fixed order (no atomics); the loss is sums[0] / D with D = sums[1], clamped
 * as max(., 1e-8) with a mask -- data-parallel callers add `sums` over the ranks first.  With unit_grad (N,K,H,W) non-NULL the
 * same pass stores u = m_i p_ic (G_ic - <p_i, G_i>);  pp_crf_loss_bwd then ACCUMULATES
 *   dlogits[e] += grad_scale * g_up[0] * (-2 / D) * unit_grad[e],  e < n = N K H W
 * reading D from `sums` on the device.  No gradient flows to the image or the mask. */
size_t pp_crf_loss_workspace(int N, int H, int W);
int pp_crf_loss_fwd(const float* logits, const float* image, const float* valid_mask, int N, int K, int C, int H, int W,
                    int radius, int dilation, float sigma_xy, float sigma_rgb, float* unit_grad, double* sums,
                    void* workspace, size_t workspace_bytes, void* stream);
int pp_crf_loss_bwd(const float* unit_grad, const double* sums, int has_mask, const float* g_up, float grad_scale,
                    float* dlogits, long long n, void* stream);

/* Normalised cut on the weak-view logits (this implementation's addition), with the kernel, offsets and
 * accepted ranges of pp_crf_loss_fwd above:
 *   q_ic = sum_j m_j k_ij p_jc,  d_i = sum_j m_j k_ij,  A_nc = sum_{i in n} m_i p_ic q_ic,  V_nc = sum_{i in n} m_i p_ic d_i,
 *   NC_nc = 1 - A_nc / V_nc if V_nc > 1e-6, else 0 (an inactive class of that image: no gradient),  L = (1/D) sum_nc NC_nc, D = N K.
 * pp_nc_loss_fwd writes assoc_vol[n][c] = {A, V} and sums[0] = sum NC_nc, sums[1] = N K (exact) in double, in a fixed order (no
 * atomics); the loss is sums[0] / sums[1] -- data-parallel callers add `sums` over the ranks first.  With unit_grad (N,K,H,W)
 * non-NULL a second, streaming pass leaves u_ic = p_ic (G_ic - <p_i, G_i>) there, G_ic = m_i (a_nc q_ic + b_nc d_i), a = -2 / V,
 * b = A / V^2 (0 for an inactive class);  pp_nc_loss_bwd then ACCUMULATES
 *   dlogits[e] += grad_scale * g_up[0] * (1 / max(sums[1], 1)) * unit_grad[e],  e < n = N K H W
 * reading D from `sums` on the device.  The workspace (pp_nc_loss_workspace bytes, 16-byte aligned) holds the per-block
 * partials, (a, b) and d.  No gradient flows to the image or the mask. */
size_t pp_nc_loss_workspace(int N, int K, int H, int W);
int pp_nc_loss_fwd(const float* logits, const float* image, const float* valid_mask, int N, int K, int C, int H, int W,
                   int radius, int dilation, float sigma_xy, float sigma_rgb, float* unit_grad, double* assoc_vol, double* sums,
                   void* workspace, size_t workspace_bytes, void* stream);
int pp_nc_loss_bwd(const float* unit_grad, const double* sums, const float* g_up, float grad_scale, float* dlogits, long long n,
                   void* stream);

/* Mumford-Shah level-set loss with an anisotropic total-variation term on the weak-view logits (this implementation's addition;
 * DESIGN.md section 7).  With p = softmax(logits) over K, x the image (N,C,H,W), C <= 4, m the valid mask (NULL: 1 everywhere):
 *   S_nc = sum_{i in n} m_i p_ic,  mu_ncr = sum_{i in n} m_i p_ic x_ir / S_nc if S_nc > 1e-6 (else the class is inactive in that
 *   image: no level-set term, no level-set gradient),  e_ic = sum_r (x_ir - mu_ncr)^2,
 *   E = sum_nci m_i p_ic e_ic + tv_weight * sum_nc sum_(i,j) m_i m_j |p_ic - p_jc|   ((i, j): the vertical and horizontal neighbour
 *   pairs inside the image, each once),  L = E / D,  D = N H W, or max(sum m, 1e-8) with a mask.
 * pp_ms_loss_fwd writes stats[n][c] = {S, mu_0 .. mu_{C-1}} and sums[0] = E, sums[1] = sum m (mask) or N H W in double, in a fixed
 * order (no atomics); the loss is sums[0] / sums[1] -- data-parallel callers add `sums` over the ranks first.  With unit_grad
 * (N,K,H,W) non-NULL the energy pass also leaves u_ic = p_ic (g_ic - <p_i, g_i>) there,
 *   g_ic = m_i e_ic [active] + tv_weight * sum_{j in 4-neighbours of i inside the image} m_i m_j sign(p_ic - p_jc), sign(0) = 0
 * (the derivative through mu vanishes: mu is the m p-weighted mean);  pp_ms_loss_bwd then ACCUMULATES
 *   dlogits[e] += grad_scale * g_up[0] * (1 / D) * unit_grad[e],  e < n = N K H W
 * reading D from `sums` on the device.  Accepted: 1 <= K <= 32, 1 <= C <= 4, H, W >= 1, tv_weight >= 0 and finite.  The workspace
 * (pp_ms_loss_workspace bytes, 16-byte aligned) holds the per-block partials of both passes and the fp32 copy of the means.  No
 * gradient flows to the image or the mask. */
size_t pp_ms_loss_workspace(int N, int K, int C, int H, int W);
int pp_ms_loss_fwd(const float* logits, const float* image, const float* valid_mask, int N, int K, int C, int H, int W,
                   float tv_weight, float* unit_grad, double* stats, double* sums, void* workspace, size_t workspace_bytes,
                   void* stream);
int pp_ms_loss_bwd(const float* unit_grad, const double* sums, int has_mask, const float* g_up, float grad_scale, float* dlogits,
                   long long n, void* stream);

/* Connected components of class maps and the keep-largest-component filter of an evaluation pipeline (this implementation's
 * addition: the reference scores its raw arg-max, inference.py:159-190).  cls: int64 class maps [N][H][W].
 * Two pixels of ONE image are connected when they are neighbours -- the 4-neighbourhood for connectivity 1, the 8-neighbourhood
 * for connectivity 2 (scipy.ndimage.generate_binary_structure(2, connectivity); 1 is what hd95 uses) -- and hold the same
 * value, whatever the value: background is labelled like every class, all in one pass.
 * pp_label_components: labels[n][y][x] (int32) = the smallest row-major index y * W + x among the pixels of that pixel's
 *   component within its image: a canonical form, unique and independent of scheduling.
 * pp_keep_largest_components: for every image and every foreground class k in 1 .. K-1 the pixels of class k outside that
 *   class's largest component become 0; everything else is copied (class 0 is never filtered; a value outside [0, K) is copied
 *   and counted nowhere).  Of components of equal size the one with the smallest label is kept, i.e. the one that holds the
 *   lowest row-major pixel (numpy.argmax(numpy.bincount(scipy_labels)[1:])).  out may alias cls.  stats: int32 [N][K][2] =
 *   {components of class k before filtering, pixels kept}; {0, 0} for k = 0 and for absent classes.
 * 1 <= K <= 32, N H W < 2^31.  Both calls enqueue a launch sequence fixed by the shape (no host synchronisation, no block waits
 * for another, integer atomics only: the same bits in every run) and need pp_components_workspace(N, K, H, W) bytes
 * (pp_label_components: the value for K = 1 suffices). */
size_t pp_components_workspace(int N, int K, int H, int W);
int pp_label_components(const int64_t* cls, int N, int H, int W, int connectivity, int32_t* labels, void* workspace,
                        size_t workspace_bytes, void* stream);
int pp_keep_largest_components(const int64_t* cls, int N, int K, int H, int W, int connectivity, int64_t* out, int32_t* stats,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Test-time augmentation over flips and quarter turns (this implementation's addition: the reference scores one forward pass per
 * slice, inference.py:159-190).  op in 0 .. 7: bit 0 flips the last axis (W), bit 1 flips H, bit 2 transposes
 * them; the forward view of a[..][H][W] is built as transpose, then flip H, then flip W, and has shape (W, H) under bit 2, (H, W)
 * otherwise.  H and W are ALWAYS those of the un-viewed frame.
 * pp_tta_view: x [planes][H][W] -> out [planes][H'][W'], the forward view (planes = N * C); out must not overlap x.
 * pp_tta_accumulate: logits [N][K][H'][W'] = the network's output for view `op`; per pixel the soft-max over K (fp32, the maximum
 *   subtracted) goes to the inverse-mapped position of acc [N][K][H][W]: stored when first != 0 -- the previous contents of acc
 *   are never read, callers need not clear it -- and added otherwise, one fp32 addition per element.
 * pp_tta_finalize: acc *= 1 / views in place (views 1, 2, 4 or 8: exact) and, unless cls is null, cls [N][H][W] = the arg-max
 *   over K of the scaled values, the first maximum as in pp_argmax_channels.
 * 1 <= K <= 32, H, W >= 1 of any size, N K H W < 2^31.  One launch each, fixed by the shape and op; no atomics, no host
 * synchronisation: with the views accumulated in a fixed order the result is the same bits in every run. */
int pp_tta_view(const float* x, int planes, int H, int W, int op, float* out, void* stream);
int pp_tta_accumulate(const float* logits, int N, int K, int H, int W, int op, int first, float* acc, void* stream);
int pp_tta_finalize(float* acc, int N, int K, int H, int W, int views, int64_t* cls, void* stream);

/* Surface metrics from the distance sets of pp_hd95_surface_distances, reduced on the device (the reference's _compute_hd,
 * inference.py:239-258, and medpy's assd / a surface Dice from the same sets).  dist / counts exactly as
 * pp_hd95_surface_distances leaves them: dist [items][2][cap] floats, counts [items][4] ints.  Only
 * dist[i][0][:min(counts[i][0], cap)] (the set A, na entries) and dist[i][1][:min(counts[i][1], cap)] (B, nb entries) are read;
 * they must hold non-negative finite floats.  With n = na + nb and S the sorted multiset union of A and B,
 *   out[i] = {max(S), sum(A), sum(B), |{a <= tolerance}|, |{b <= tolerance}|, S[j], S[min(j + 1, n - 1)], n},
 *   j = floor(v), v = (double)(n - 1) * (percentile / 100.0)       (numpy.percentile's virtual index, method 'linear').
 * The maximum and the two order statistics are bit-exact elements of S (an exact radix select on the bit patterns), `<=` is taken
 * in fp32 against the fp32 tolerance, counts and n are exact as doubles, the sums are added in double in a fixed order (strided
 * per-thread partials, then a fixed tree): the same bits in every run.  An item with n == 0 writes eight zeros and reads nothing
 * of dist.  The caller forms  HD = out[0],  ASSD = (out[1] / na + out[2] / nb) / 2,  surface Dice = (out[3] + out[4]) / n,
 * percentile distance = out[5] + (out[6] - out[5]) * (v - j).
 * One launch of one block per item, fixed by `items`: no workspace, no host synchronisation, no global atomics (capturable).
 * Refused with a status and pp_last_error() before any launch: null pointers, items < 1, cap < 1, percentile outside (0, 100] or
 * not finite, tolerance negative or not finite, items * 2 * cap >= 2^31. */
int pp_surface_reduce(const float* dist, const int* counts, int items, int cap, double percentile, float tolerance,
                      double* out, void* stream);

/* Mean-field CRF refinement of a soft-max at inference, with an image-dependent pairwise term (this implementation's addition: the
 * reference scores its raw arg-max, inference.py:159-190).  logits (N,K,H,W), image (N,C,H,W), fp32.  With
 * j = i + (dy, dx) * dilation, dy, dx in [-radius, radius] \ (0, 0), j inside the image (a pixel outside adds nothing, also not to
 * the normalisers), dy and dx counted in window steps as in pp_crf_loss_fwd:
 *   kb_ij = exp(-(dy^2 + dx^2) / (2 sigma_xy^2)) * exp(-|x_i - x_j|^2 / (2 sigma_rgb^2)),  ks_ij = exp(-(dy^2 + dx^2) / (2 sigma_smooth^2))
 *   Q^0 = softmax(logits),  u = log_softmax(logits),  Sb_i = sum_j kb_ij,  Ss_i = sum_j ks_ij
 *   Q^{t+1}_i = softmax_c(u_ic + w_bilateral (sum_j kb_ij Q^t_jc) / (Sb_i + 1e-6) + w_smooth (sum_j ks_ij Q^t_jc) / (Ss_i + 1e-6))
 * (Potts compatibility, normalised messages: the weights are in logit units; every pixel updates from Q^t.)  prob (N,K,H,W)
 * receives Q^iterations; cls (N,H,W), unless null, the first-maximum arg-max of prob as it is stored.  One launch per iteration,
 * ping-pong between prob and the workspace (pp_crf_refine_workspace(N, K, H, W) bytes, required for every iteration count; it need
 * not be cleared) so that the result lands in prob whatever the parity; Q^0 is never stored.  No atomics and no dependence on the
 * launch grid: the same bits in every run, and per slice the same bits whatever the batch around it.  No host synchronisation.
 * Refused with a status and pp_last_error() before anything is enqueued: null logits / image / prob / workspace, N > 65535,
 * H > 262140, K outside 1 .. 32, C outside 1 .. 4, K H W >= 2^31, iterations outside 1 .. 64, radius outside 1 .. 8, dilation outside
 * 1 .. 4, radius * dilation > 16, a sigma that is not positive and finite, a weight that is negative or not finite, a workspace that
 * is too small, prob / workspace / cls overlapping each other or (prob, workspace) an input. */
size_t pp_crf_refine_workspace(int N, int K, int H, int W);
int pp_crf_refine(const float* logits, const float* image, int N, int K, int C, int H, int W, int iterations, int radius,
                  int dilation, float sigma_xy, float sigma_rgb, float sigma_smooth, float w_bilateral, float w_smooth,
                  float* prob, int64_t* cls, void* workspace, size_t workspace_bytes, void* stream);

/* ---- optimiser (torch.optim.Adam(lr, weight_decay) at train_chaos.py:219) ------------------------------- */
int pp_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int step, void* stream);
/* torch.optim.SGD(lr, momentum, weight_decay) (train_chaos.py:220-221, --optimizer momentum); step counts from 1 */
int pp_sgd_momentum_step(float* p, const float* g, float* momentum_buf, long long n, float lr, float momentum,
                         float weight_decay, int step, void* stream);
int pp_fill(float* p, long long n, float value, void* stream);
/* p[i] *= value (the unscaling of the gradient slab after a 16-bit-storage step, see pacingpseudo_hip_h16.h) */
int pp_scale(float* p, long long n, float value, void* stream);
/* Overflow guard of the 16-bit storage mode (the counterpart of torch.cuda.amp.GradScaler's skipped steps, with a static scale):
 * pp_scale_guard = pp_scale, and bad[0] |= 1 when a scaled gradient is not finite; the *_guard optimizer steps return without
 * touching p / m / v when skip[0] != 0 and count the skipped update in skip[1].  skip / bad: two device ints, reset by the caller. */
int pp_scale_guard(float* p, long long n, float value, int* bad, void* stream);
int pp_adam_step_guard(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int step, int* skip, void* stream);
int pp_sgd_momentum_step_guard(float* p, const float* g, float* momentum_buf, long long n, float lr, float momentum,
                               float weight_decay, int step, int* skip, void* stream);
/* The forms FusedAdam / FusedSGD call (round 5; torch.optim.Adam / SGD `step()`, train_chaos.py:315): the segment's step count is a
 * DEVICE int (step_dev[0] = updates applied so far: the bias corrections use step_dev[0] + 1, and a one-thread commit kernel
 * advances it after the update -- unless skip[0] != 0, in which case nothing is touched and, if count_skip != 0, skip[1] += 1:
 * pass count_skip = 1 for ONE segment per optimizer step).  lr_dev (nullable): the learning rate as a device scalar instead of
 * `lr`.  With both on the device a captured hipGraph of the step replays correctly (no host value baked into the launch). */
int pp_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                     float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip, void* stream);
int pp_sgd_momentum_step_dev(float* p, const float* g, float* momentum_buf, long long n, float lr, const float* lr_dev,
                             float momentum, float weight_decay, int* step_dev, int* skip, int count_skip, void* stream);
/* Global gradient-norm clipping, torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) semantics (the reference trains
 * without it, train_chaos.py:313-315; off by default here).  pp_grad_sumsq: sum of squares of g[0..n) formed in double, one double
 * per block written to partial[0 .. pp_grad_sumsq_rows(n)) -- the row count depends on n alone and nothing is added atomically,
 * so the result is the same bits in every run.  A step calls it once per active slab segment, each with its own rows of one
 * scratch array, then pp_grad_clip_finalize ONCE over all `rows`: out2[0] = total = sqrt(sum), out2[1] = coef =
 * min(1, max_norm / (total + 1e-6)) (double arithmetic, rounded once to fp32; max_norm = +inf: measure, never clip), and the
 * statistics block stats = double[4] {steps, steps with coef < 1, sum of total, max of total} is advanced -- unless skip
 * (nullable) says the overflow guard skips this step.  pp_adam_step_clip / pp_sgd_momentum_step_clip = the *_dev forms on
 * gradients fl32(g * clip_dev[0]), clip_dev = out2 + 1: what the *_dev forms compute on a slab scaled in place; g is not written. */
int pp_grad_sumsq_rows(long long n);
int pp_grad_sumsq(const float* g, long long n, double* partial, void* stream);
int pp_grad_clip_finalize(const double* partial, int rows, double max_norm, const int* skip, float* out2, double* stats,
                          void* stream);
int pp_adam_step_clip(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                      float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip, const float* clip_dev,
                      void* stream);
int pp_sgd_momentum_step_clip(float* p, const float* g, float* momentum_buf, long long n, float lr, const float* lr_dev,
                              float momentum, float weight_decay, int* step_dev, int* skip, int count_skip, const float* clip_dev,
                              void* stream);
/* Exponential moving average of the weights, kept on the device by the optimizer step itself (the reference trains without one,
 * train_chaos.py:313-315; off by default here).  ema is an fp32 slab laid out as p.  With t = the segment's update count BEFORE
 * this update (step_dev[0]; 0 for the first), d_t = min(ema_decay, (1 + t) / (10 + t)) in double and w = (float)(1 - d_t), every
 * element becomes ema + fl32(w * fl32(p - ema)): three separately rounded fp32 operations, the torch fp32 chain e + w * (p - e)
 * bit for bit.  0 < ema_decay < 1.  pp_adam_step_ema / pp_sgd_momentum_step_ema = the *_dev forms (clip_dev null) or the *_clip
 * forms (clip_dev set) whose kernel also loads ema, moves it towards the p it has just computed and stores it (8 B / parameter
 * more); a step the overflow guard skips leaves ema untouched, and t does not advance.  pp_ema_update: the same rule as a pass
 * of its own over p[0..n) (not written) and ema[0..n), t = step_dev[0] when step_dev is set, else t_host >= 0.  pp_slab_swap:
 * a[0..n) <-> b[0..n) in place (disjoint, 16-byte aligned), how the averaged weights are put where the live ones are. */
int pp_adam_step_ema(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                     float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip, float* ema,
                     double ema_decay, const float* clip_dev, void* stream);
int pp_sgd_momentum_step_ema(float* p, const float* g, float* momentum_buf, long long n, float lr, const float* lr_dev,
                             float momentum, float weight_decay, int* step_dev, int* skip, int count_skip, float* ema,
                             double ema_decay, const float* clip_dev, void* stream);
int pp_ema_update(const float* p, float* ema, long long n, double ema_decay, const int* step_dev, long long t_host, void* stream);
int pp_slab_swap(float* a, float* b, long long n, void* stream);

/* ---- diagnostics -------------------------------------------------------------------------------------------- */
/* bare v_mfma_f32_32x32x2_f32 loop: the fp32 matrix rate this device sustains at its clock under load */
int pp_mfma_probe(float* out, int blocks, int iters, double* flops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PACINGPSEUDO_HIP_H */
