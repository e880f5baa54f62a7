/* dta_hip.h - C ABI of the MI355X-native (gfx950) Hang2020 hot path.
 *
 * This is the drop-in boundary.  The reference has no native layer: its boundary is the
 * torch.nn.Module contract `cls(bands, classes)` / `forward(x)` of /root/reference/src/models/Hang2020.py
 * plus autograd + torch.optim.Adam.  Each entry point below names the reference interface it replaces; the
 * Python binding a reference maintainer adds is shown in INTEGRATION.md (ctypes, raw device pointers).
 *
 * Conventions
 *  - plain C, no C++/torch types; every pointer is a DEVICE pointer unless said otherwise
 *  - every buffer is allocated by the caller (PyTorch caching allocator) and only borrowed for the call;
 *    the library allocates nothing on the device (one documented exception: the peer-exchange object dta_xchg_*)
 *  - host-side state the library keeps (all of it per process): the thread-local text of dta_last_error(); the
 *    developer switches of the DEVELOPER library only (dta_dev_switches_enabled; the product library reads nothing from
 *    the environment); per launch site, a bit per
 *    device ordinal saying that the function's dynamic-LDS attribute has been set on that device; the optional
 *    profiling event pool of dta_profile_* (one device at a time); peer-exchange objects the caller created.  Nothing
 *    else survives a call: no caches keyed on shapes or pointers, no device allocations
 *  - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); no internal syncs
 *  - return 0 on success; otherwise non-zero and dta_last_error() describes the failure (thread-local text)
 *  - parameters/gradients use the reference's torch layouts and state_dict shapes
 */
#ifndef DTA_HIP_H
#define DTA_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DTA_ABI_VERSION 2   /* 2: DTA_MAX_YEARS 16, dta_adam_segment::lr, dta_multistage_*, 16 Adam segments per launch */

enum { DTA_F32 = 0, DTA_BF16 = 1 };               /* arithmetic type of the conv contractions */
enum { DTA_NET_HANG2020 = 0, DTA_NET_SPECTRAL = 1, DTA_NET_SPATIAL = 2, DTA_NET_VANILLA = 3 };

typedef struct dta_net_desc {
  int batch, bands, height, width, classes;
  int kind;          /* DTA_NET_* */
  int dtype;         /* DTA_F32 (exact fp32 MFMA) or DTA_BF16 (bf16 MFMA inputs, fp32 accumulate) */
  int training;      /* 1: BatchNorm batch statistics + running-stat update; 0: running statistics */
  int heads_mask;    /* bit L-1 set: compute classifier head L (Hang2020.forward only needs head 3 = 4);
                        | DTA_FORWARD_ONLY: no dta_net_backward will follow on this workspace (inference)
                        | DTA_SKIP_BLEND: Hang2020 forward leaves the sigmoid(alpha) blend to dta_net_loss (joint unused)
                        | DTA_REUSE_PACKED: inference with frozen weights (below) */
  float bn_momentum, bn_eps;
} dta_net_desc;

/* One spectral_network / spatial_network (Hang2020.py:170-240) or the vanilla_CNN conv stack (:33-53).
 * att[L][*]: spectral_attention -> {attention_conv1.weight (C,C,K), .bias, attention_conv2.weight, .bias, 0, 0}
 *            spatial_attention  -> {channel_pool.weight (1,C,1,1), .bias, attention_conv1.weight (1,1,k,k), .bias,
 *                                   attention_conv2.weight, .bias};  vanilla: all null.
 * fc_w/fc_b : classifier{L}.fc1 (vanilla: only index 2 = fc1). */
typedef struct dta_subnet_params {
  const float* conv_w[3]; const float* conv_b[3];
  const float* bn_w[3]; const float* bn_b[3];
  float* bn_rm[3]; float* bn_rv[3]; long long* bn_nbt[3];
  const float* att[3][6];
  const float* fc_w[3]; const float* fc_b[3];
} dta_subnet_params;

/* Gradient destinations, same shapes as the parameters; a null pointer skips that gradient. */
typedef struct dta_subnet_grads {
  float* conv_w[3]; float* conv_b[3];
  float* bn_w[3]; float* bn_b[3];
  float* att[3][6];
  float* fc_w[3]; float* fc_b[3];
} dta_subnet_grads;

/* heads_mask flag: the forward skips what only a backward would read (saved attention state, the bf16 input tiles) */
#define DTA_FORWARD_ONLY 8
#define DTA_SKIP_BLEND 16
/* heads_mask flag, inference only (training == 0 and DTA_FORWARD_ONLY; ignored otherwise): the conv / spectral-attention
 * weight re-layouts and the conv row tables that an earlier forward with the SAME descriptor, parameter table and workspace
 * left in the workspace are used as they are -- the caller guarantees that those weights have not changed since that
 * call and that nothing else wrote to the workspace.  The first forward on a workspace must not carry the flag.
 * (Tile prediction, reference predict.py:140-151 / main.py:165-205: one trained model, thousands of 64-crop batches --
 * the re-layout of 15 networks' weights is 19 us of a 145 us MultiStage.predict_step.)  BatchNorm running statistics,
 * biases and the classifier heads are read from the parameter table in every call either way. */
#define DTA_REUSE_PACKED 32

int dta_abi_version(void);
/* Hash of the sources this library was built from (python -m deeptreeattention_amd.build): measurement artifacts record
 * it, bench.py refuses to quote counters taken on another build. */
const char* dta_build_id(void);
const char* dta_last_error(void);

/* Bytes of scratch + saved-activation workspace dta_net_forward/backward need for `d` (same blob for both;
 * keep it alive and untouched between a training forward and its backward). */
size_t dta_net_workspace_bytes(const dta_net_desc* d);

/* Replaces Hang2020.forward (Hang2020.py:251-263), spectral_network.forward (:226-240), spatial_network.forward
 * (:190-204), vanilla_CNN.forward (:45-53) incl. every conv_module / attention / Classifier inside.
 *  nets   : 2 entries {spectral, spatial} for DTA_NET_HANG2020, otherwise 1
 *  alpha  : float64 scalar (Hang2020.alpha), HANG2020 only
 *  x      : float32 NCHW contiguous [batch][bands][height][width]
 *  scores : [net][L] -> float32 [batch][classes] outputs of the classifier heads selected by heads_mask
 *  joint  : HANG2020: sigmoid(alpha)-blended scores; VANILLA: fc1 output; else unused (may be null)
 * DTA_NET_VANILLA: the head is Linear(512, classes) as in the reference (:43), so only patches whose twice-pooled map
 * flattens to 128 * (H/4) * (W/4) = 512 features are accepted (the descriptor is rejected otherwise). */
int dta_net_forward(const dta_net_desc* d, const dta_subnet_params* nets, const double* alpha, const float* x,
                    void* workspace, float* const scores[2][3], float* joint, void* stream);

/* Replaces autograd's backward through the module above.  `workspace` is the blob the matching training (or eval)
 * forward filled.  dscores[net][L] / djoint: gradients wrt the forward outputs (null = that output unused; for
 * HANG2020 pass djoint, for the others dscores; HANG2020 with djoint == NULL and dscores set is the all-heads mode of
 * the Hang et al. multi-head loss: every listed head of both branches back-propagates, the blend and alpha do not).
 * Every non-null gradient buffer in `grads`, and `dalpha`, must arrive
 * ZERO-FILLED (split-K partial sums are accumulated with atomics); on return it holds the gradient.
 * phases: bit 0 = everything except the first conv's weight gradient, bit 1 = the first conv's weight gradient
 * (the largest and last piece); 3 = all.  Two calls (1, then 2) let the caller start the gradient all-reduce of
 * the rest (RCCL on a side stream) while the first conv's weight gradient is still being computed. */
int dta_net_backward(const dta_net_desc* d, const dta_subnet_params* nets, const double* alpha, void* workspace,
                     const float* const dscores[2][3], const float* djoint, const dta_subnet_grads* grads,
                     double* dalpha, int phases, void* stream);

/* The same two calls for a batch whose input is ALREADY the first conv's bf16 tiles (dta_preprocess_crops_tiles below:
 * raw crops -> tiles in one launch): bf16 mode, one input tensor (every kind but the ensemble), patches whose tile is a
 * single band (11x11-class).  x_tiles: bf16 [batch][ceil(bands / 16)][height * width][16], bands past `bands` zero; it
 * must stay valid and unchanged until the matching backward, which reads it again for the first conv's weight gradient. */
int dta_net_forward_tiles(const dta_net_desc* d, const dta_subnet_params* nets, const double* alpha, const void* x_tiles,
                          void* workspace, float* const scores[2][3], float* joint, void* stream);
int dta_net_backward_tiles(const dta_net_desc* d, const dta_subnet_params* nets, const double* alpha, const void* x_tiles,
                           void* workspace, const float* const dscores[2][3], const float* djoint,
                           const dta_subnet_grads* grads, double* dalpha, int phases, void* stream);

/* Data-parallel form of dta_net_backward / dta_net_backward_tiles (x_tiles NULL: the workspace's own tiles).  One extra
 * destination: dalpha_f32 (may be NULL) receives d(alpha) rounded to float32 -- ONE rounding of the finished float64 sum,
 * written by the launch that ends the call (any call with phases & 1), no float atomics: reruns give the same bits.  A
 * data-parallel caller points it at a slot of its flat float32 gradient buffer, so that alpha's gradient takes
 * part in the buffer's all-reduce without copy kernels around the collective (reference train.py:89-98 lets Lightning's
 * DDP all-reduce every parameter; here that is at most two collectives per step). */
int dta_net_backward_dp(const dta_net_desc* d, const dta_subnet_params* nets, const double* alpha, const void* x_tiles,
                        void* workspace, const float* const dscores[2][3], const float* djoint,
                        const dta_subnet_grads* grads, double* dalpha, float* dalpha_f32, int phases, void* stream);

/* dta_net_backward_dp for a caller that exchanges gradients through a peer exchange object (dta_xchg_* below) whose
 * buffer has a head / tail split (dta_xchg_set_split): the whole backward in one call, ordered so that the exchange's HEAD
 * segment -- every gradient except the first conv's weights, 76 % of the bytes -- is complete before the first conv's
 * weight-gradient launch, whose spare workgroups (the 16 CUs that launch leaves idle) then sum this rank's shard of the
 * head over the ranks through peer memory WHILE the matrix cores compute the last gradient (reference train.py:89-98:
 * DDP overlaps the gradient all-reduce with the backward).  The dta_xchg_adam_step / dta_xchg_allreduce that follows on
 * the same stream finds the head summed and only has the tail left.  grads must point into dta_xchg_grad_buffer(xchg);
 * alpha_slot: index of alpha's float32 exchange slot inside the head (or -1).  When the plan has no combined kernel
 * (fp32 mode, other shapes) this is exactly dta_net_backward_dp(phases = 3) and the exchange sums both segments itself. */
struct dta_xchg;
int dta_net_backward_xchg(const dta_net_desc* d, const dta_subnet_params* nets, const double* alpha, const void* x_tiles,
                          void* workspace, const float* const dscores[2][3], const float* djoint,
                          const dta_subnet_grads* grads, double* dalpha, struct dta_xchg* xchg, long long alpha_slot,
                          void* stream);

/* Loss head of the network whose forward just ran on `workspace`: the Hang2020 blend (Hang2020.py:260-261; the forward
 * was built with DTA_SKIP_BLEND), F.cross_entropy(scores, labels, weight) (src/main.py:78), d(loss)/d(scores) and the
 * scalar loss in ONE launch (dta_net_forward + dta_weighted_ce take three for the same).
 *  joint   : Hang2020: receives the blended scores [batch][classes] (may be NULL); other kinds: the scores to use (input)
 *  dlogits : d(loss)/d(scores) [batch][classes], may be NULL (validation)
 *  scratch : batch + 2 floats; the LAST 32-bit word must be zero on entry and is zero again on return (block counter) */
int dta_net_loss(const dta_net_desc* d, const double* alpha, void* workspace, const long long* labels, const float* weight,
                 float* joint, float* loss, float* dlogits, float* scratch, void* stream);
/* Forward AND loss of a single-score network (Hang2020, vanilla_CNN) in one call: what TreeModel.training_step does in
 * `y_hat = self.model.forward(images); loss = F.cross_entropy(y_hat, y, weight=self.loss_weight)` (reference src/main.py:77-78;
 * validation_step :88-89 with dlogits = NULL).  Same results as dta_net_forward (built with DTA_SKIP_BLEND) followed by
 * dta_net_loss.  For a training-mode Hang2020 on 11x11 patches the third stage of both branches, the two last heads, the
 * blend and the loss are ONE launch (the forward ends two launches earlier than dta_net_forward + dta_net_loss).
 *  x / x_tiles : the input as float32 NCHW [batch][bands][H][W], or (bf16 mode, x = NULL) as the first conv's tiles
 *                (dta_preprocess_crops_tiles) -- exactly one of the two
 *  labels, weight, joint, loss, dlogits, scratch : as for dta_net_loss (vanilla_CNN: joint receives the scores, required) */
int dta_net_forward_loss(const dta_net_desc* d, const dta_subnet_params* nets, const double* alpha, const float* x,
                         const void* x_tiles, void* workspace, const long long* labels, const float* weight, float* joint,
                         float* loss, float* dlogits, float* scratch, void* stream);

/* ---- Year ensemble (reference src/models/year.py:9-33): `years` (1..DTA_MAX_YEARS) spectral_networks, each on its own
 * input, run as the groups of ONE set of launches (a third of the launches of `years` separate dta_net_* calls);
 * the returned scores are the mean over the years of each year's last-head scores (year.py:30,33).
 * The reference skips a year whose whole batch tensor sums to zero (year.py:27): the caller passes only the years it
 * keeps (their params / inputs / grads, in any order), so a skipped year's BatchNorm state and gradients stay untouched.
 *  d      : kind DTA_NET_SPECTRAL; heads_mask is ignored (only the last head is evaluated)
 *  nets   : `years` entries;  x : `years` device pointers, each float32 NCHW [batch][bands][height][width]
 *  mean_scores : float32 [batch][classes] */
#define DTA_MAX_YEARS 16
size_t dta_ensemble_workspace_bytes(const dta_net_desc* d, int years);
int dta_ensemble_forward(const dta_net_desc* d, int years, const dta_subnet_params* nets, const float* const* x,
                         void* workspace, float* mean_scores, void* stream);
/* The reference's missing-year test on the device (year.py:27 `x.sum() == 0`): flags[y] = 1 when year y's tensor has a
 * non-zero element (NaN counts), else 0.  For the non-negative crops the reference's loader produces (min-max scaled to
 * [0, 1], missing years zero-filled, src/data.py:295-296) that is the same decision -- a sum of non-negative floats is
 * zero exactly when all of them are; tensors with negative entries that cancel to an exact zero sum would be skipped by
 * the reference and are kept here.  x: HOST array of `years` device pointers (16-byte aligned), n_per_year floats each.
 * clear_next (device, float[years], may be NULL): a second flag bank this call zeroes, so that a caller alternating two
 * banks never needs a clearing launch; with NULL the call clears `flags` itself first (one more tiny launch). */
int dta_year_flags(const float* const* x, int years, size_t n_per_year, float* flags, float* clear_next, void* stream);
/* dta_ensemble_forward over ALL years with the skip decided on the device: gate (device, float[years], e.g. from
 * dta_year_flags) <= 0 leaves that year out of the mean and leaves its BatchNorm running statistics / counter untouched,
 * exactly as a year the reference skips -- no host round trip.  (The skipped year's launches still run; their results are
 * never used.)  kept (device, float[2], may be NULL) receives {years kept, 1 / years kept}: the second word is the
 * gradient scale dta_weighted_ce_scaled_dev takes.  No year kept: mean_scores are NaN (the reference raises there). */
int dta_ensemble_forward_gated(const dta_net_desc* d, int years, const dta_subnet_params* nets, const float* const* x,
                               const float* gate, void* workspace, float* mean_scores, float* kept, void* stream);
/* Forward of the year ensemble AND the level's loss in one call (reference multi_stage.py:283-285: `y_hat = self.models[..]
 * .forward(images); loss = F.cross_entropy(y_hat, y, weight=self.loss_weight[..])`): dta_ensemble_forward(_gated) with the mean
 * over the kept years formed inside the loss launch instead of a launch of its own -- same values, bit for bit.
 *  gate    : float[years] year flags (dta_year_flags) or NULL = every year is kept
 *  mean_scores [batch][classes] (may be NULL), kept {kept years, 1 / kept} (may be NULL): outputs as in the gated forward
 *  dscore  : d(loss)/d(ONE year's scores) = d(loss)/d(mean) / kept years -- what dta_ensemble_backward* take; may be NULL
 *  labels / weight / loss / scratch : as for dta_net_loss.  Nothing kept: NaN loss, exact-zero dscore. */
int dta_ensemble_forward_loss(const dta_net_desc* d, int years, const dta_subnet_params* nets, const float* const* x,
                              const float* gate, void* workspace, const long long* labels, const float* weight,
                              float* mean_scores, float* kept, float* loss, float* dscore, float* scratch, void* stream);
/* Backward of the above.  dscore: d(loss)/d(one year's scores) = d(loss)/d(mean_scores) / years, float32
 * [batch][classes], shared by all years.  grads: `years` entries, every non-null buffer ZERO-FILLED on entry;
 * classifier1/2 gradients are not produced (those heads never reach the loss). */
int dta_ensemble_backward(const dta_net_desc* d, int years, const dta_subnet_params* nets, void* workspace,
                          const float* dscore, const dta_subnet_grads* grads, void* stream);
/* Same with the `phases` split of dta_net_backward (bit 0: everything but the years' first-conv weight gradients,
 * bit 1: those), so that a data-parallel caller can overlap the first gradient exchange with them. */
int dta_ensemble_backward_phased(const dta_net_desc* d, int years, const dta_subnet_params* nets, void* workspace,
                                 const float* dscore, const dta_subnet_grads* grads, int phases, void* stream);
/* Backward of dta_ensemble_forward_gated: gate (device, float[years], the flags the forward was gated by; NULL = all on)
 * <= 0 makes that year's gradients EXACT ZEROS (its score gradient is taken as zero whatever dscore holds; its launches
 * still run), as a year the reference skips has grad None (year.py:27-28).  A data-parallel rank whose batch lacks a year
 * that another rank kept thus contributes zeros to that year's gradient sum. */
int dta_ensemble_backward_gated(const dta_net_desc* d, int years, const dta_subnet_params* nets, void* workspace,
                                const float* dscore, const dta_subnet_grads* grads, const float* gate, int phases,
                                void* stream);
/* dta_ensemble_backward_gated (phases = 3) for a data-parallel caller whose gradients live in a peer exchange object with a
 * head / tail split (dta_xchg_set_split; declared below): the head -- every gradient of every year except the years'
 * first-conv weights, plus whatever the caller keeps in it (its year flags) -- is complete before the years' grouped
 * first-conv weight-gradient launch, whose spare workgroups sum this rank's shard of the head over the ranks through
 * peer memory while the matrix cores work (as dta_net_backward_xchg does for one network; reference multi_stage.py:277-288
 * under train.py:89-98's DDP).  The dta_xchg_allreduce that follows finds the head summed.  Plans without a combined
 * kernel (fp32 mode, launches that fill every CU): exactly dta_ensemble_backward_gated, the exchange sums both segments. */
struct dta_xchg;
int dta_ensemble_backward_xchg(const dta_net_desc* d, int years, const dta_subnet_params* nets, void* workspace,
                               const float* dscore, const dta_subnet_grads* grads, const float* gate, struct dta_xchg* xchg,
                               void* stream);

/* ---- Crop preprocessing on the device: replaces load_image / preprocess_image (src/utils.py:36-79: drop the first and
 * last `clip` bands when there are more than 3, float32, per-pixel min-max over the bands as
 * sklearn.preprocessing.minmax_scale(axis=1) computes it, NEAREST resize to size x size) plus the training flips
 * (src/augmentation.py:13-14: horizontal then vertical, both p=1) for a whole batch of ragged crops in one launch.
 * Output is bit-identical to the reference's CPU path.
 *  raw     : all crops of the batch back to back (device memory), element type `dtype`
 *  offsets : [batch] int64 element offset of each crop inside raw;  heights/widths : [batch] int32 (device)
 *            a crop with height or width 0 is a missing year: its output is all zeros (src/data.py:295-296)
 *  layout  : DTA_CROP_CHW = band-first [bands_raw][h][w] (what rasterio's read() / np.load return),
 *            DTA_CROP_HWC = pixel-interleaved [h][w][bands_raw] (how the crops lie on disk: TIFF PlanarConfiguration 1)
 *  out     : float32 [batch][dta_preprocess_out_bands(bands_raw, clip)][size][size] */
enum { DTA_CROP_F32 = 0, DTA_CROP_I16 = 1, DTA_CROP_U8 = 2 };
enum { DTA_CROP_CHW = 0, DTA_CROP_HWC = 1 };
typedef struct {
  int batch, bands_raw, clip, size, flip, layout, dtype;
} dta_crop_desc;
int dta_preprocess_out_bands(int bands_raw, int clip);
int dta_preprocess_crops(const dta_crop_desc* d, const void* raw, const long long* offsets, const int* heights,
                         const int* widths, float* out, void* stream);
/* Same preprocessing, written straight as the bf16 conv tiles dta_net_forward_tiles takes (the float32 batch never
 * exists): tiles bf16 [batch][ceil(out_bands / 16)][size * size][16] = the float32 results above rounded to bf16
 * (nearest even), bands past out_bands zero. */
int dta_preprocess_crops_tiles(const dta_crop_desc* d, const void* raw, const long long* offsets, const int* heights,
                               const int* widths, void* tiles, void* stream);

/* Replaces F.cross_entropy(logits, y, weight=w) forward+backward (src/main.py:78, multi_stage.py:285).
 * weight may be null (= ones, metadata.py:61).  scratch: batch+1 floats.  dlogits may be null.
 * Labels: -100 is ignored as torch's default ignore_index; any other label outside [0, classes) is a caller bug
 * (torch raises or device-asserts) and makes the loss and that row of dlogits NaN instead of being skipped silently. */
int dta_weighted_ce(const float* logits, const long long* labels, const float* weight, int batch, int classes,
                    float* loss, float* dlogits, float* scratch, void* stream);

/* The same loss in ONE launch (the last block to arrive finalises it) with a factor on the gradient only: dlogits =
 * grad_scale * d(loss)/d(logits).  The year ensemble's step uses it with grad_scale = 1 / kept years, the derivative of
 * the mean over the kept years' scores (src/models/year.py:33), so no elementwise pass follows the loss.
 * scratch: batch + 2 floats whose LAST 32-bit word is zero on entry (block counter; left zero). */
int dta_weighted_ce_scaled(const float* logits, const long long* labels, const float* weight, int batch, int classes,
                           float grad_scale, float* loss, float* dlogits, float* scratch, void* stream);
/* Same with the factor read from the device (grad_scale_dev[0]): 1 / kept years as dta_ensemble_forward_gated left it. */
int dta_weighted_ce_scaled_dev(const float* logits, const long long* labels, const float* weight, int batch, int classes,
                               const float* grad_scale_dev, float* loss, float* dlogits, float* scratch, void* stream);

/* Inference epilogue: replaces F.softmax(pred, dim=1) (src/models/multi_stage.py:302,315; src/main.py:190) and the
 * top-1/top-2 label+score extraction of src/main.py:192-205.  probs [batch][classes] may be null.
 * top_idx [batch][2] int64, top_score [batch][2] float32. */
int dta_softmax_top2(const float* logits, int batch, int classes, float* probs, long long* top_idx, float* top_score,
                     void* stream);

/* Replaces torch.optim.Adam(params, lr).step() (src/main.py:136) over one flat fp32 buffer plus the float64
 * alpha (alpha_* may be null).  step = 1-based step count; grads are multiplied by grad_scale first. */
int dta_adam_step(float* p, const float* g, float* m, float* v, size_t n, double* alpha_p, const double* alpha_g,
                  double* alpha_m, double* alpha_v, int step, float lr, float beta1, float beta2, float eps,
                  float grad_scale, void* stream);

/* optimizer.step() followed by optimizer.zero_grad() (the Lightning loop of src/main.py does both every batch) in one
 * pass: same update as dta_adam_step, then g and alpha_g are cleared, which is the state dta_net_backward expects. */
int dta_adam_step_zero_grad(float* p, float* g, float* m, float* v, size_t n, double* alpha_p, double* alpha_g,
                            double* alpha_m, double* alpha_v, int step, float lr, float beta1, float beta2, float eps,
                            float grad_scale, void* stream);

/* Data-parallel form: alpha's gradient is read from alpha_g_f32 (the exchange slot dta_net_backward_dp filled and the
 * all-reduce summed) when that is non-NULL, from alpha_g otherwise; zero_grad != 0 clears g and alpha_g after use. */
int dta_adam_step_dp(float* p, float* g, float* m, float* v, size_t n, double* alpha_p, double* alpha_g,
                     const float* alpha_g_f32, double* alpha_m, double* alpha_v, int step, float lr, float beta1, float beta2,
                     float eps, float grad_scale, int zero_grad, void* stream);

/* optimizer.step() + zero_grad() gated ON THE DEVICE (year ensembles under data parallelism, where whether a year is
 * stepped -- "some rank kept it", src/models/year.py:27 -- is only known on the device after the gradient exchange):
 * active[0] > 0: Adam step number dev_step[0] + 1 (dev_step[0] = steps this parameter group has taken so far, a device
 * counter); otherwise only the gradient buffer is cleared -- always: a group that is not stepped has no gradient (torch
 * leaves grad None), whatever zero_grad says -- and nothing else happens (no moment decay, as torch's Adam passes over
 * parameters whose grad is None).  dev_step_next (may be NULL; must not alias dev_step): receives the count after
 * this step, dev_step[0] + (active ? 1 : 0) -- callers ping-pong two counter words, so the count advances without any
 * launch of their own; pass it in ONE of the launches that share a counter.  No float64 alpha here. */
int dta_adam_step_gated(float* p, float* g, float* m, float* v, size_t n, const float* active, const int* dev_step,
                        int* dev_step_next, float lr, float beta1, float beta2, float eps, float grad_scale, int zero_grad,
                        void* stream);
/* Several parameter groups in ONE launch: the per-year optimizers of a year ensemble (reference multi_stage.py:258-275: one
 * Adam per level over all years' parameters; years the step skipped are passed over) instead of one launch per year and
 * segment.  Each segment is stepped exactly as dta_adam_step (active == NULL: host step count `step` >= 1) or as
 * dta_adam_step_gated (active != NULL: device gate + device step counter; `step` ignored) would step it; zero_grad and the
 * hyper-parameters are common.  1 <= nseg <= DTA_ADAM_MAX_SEGMENTS. */
#define DTA_ADAM_MAX_SEGMENTS 16
typedef struct dta_adam_segment {
  float* p; float* g; float* m; float* v; size_t n;
  const float* active; const int* dev_step; int* dev_step_next;   /* gated form, or all NULL */
  int step;                                                        /* host step count (ungated form) */
  float lr;                                                        /* > 0: this segment's learning rate instead of the call's (one Adam per
                                                                      level, reference multi_stage.py:258-262); 0: the call's.  A segment
                                                                      cannot ask for rate 0 by itself: a caller with a frozen segment
                                                                      passes lr = 0 to the call and a rate > 0 in every stepped segment */
} dta_adam_segment;
int dta_adam_step_multi(int nseg, const dta_adam_segment* segs, float lr, float beta1, float beta2, float eps, float grad_scale,
                        int zero_grad, void* stream);

/* ---- Multi-stage step (reference src/models/multi_stage.py:41-66: one learned_ensemble per level of the hierarchy, each with
 * its own class count; :277-288: per level weighted cross-entropy of the mean over the years; train.py:75-100 trains all
 * levels on every batch).  The levels x kept-years spectral networks run as the groups of ONE set of launches -- one forward
 * chain, ONE loss launch over the levels, one backward chain -- instead of one chain per level.  Every level's batch has
 * the same size (d->batch) and crop shape; d->classes is ignored (each level carries its own).
 *  lv[l].first / count : the level's networks are nets[first .. first + count) (likewise x, grads, gate); levels in order,
 *                        adjacent, the total at most DTA_MAX_YEARS networks
 *  gate (device, float[total], may be NULL): as for dta_ensemble_forward_gated -- a network whose flag is <= 0 is left out
 *                        of its level's mean, keeps its BatchNorm statistics and gets exact-zero gradients */
#define DTA_MAX_LEVELS 8
typedef struct dta_level {
  int classes, first, count;
  const long long* labels;   /* device int64 [batch] */
  const float* weight;       /* device float32 [classes], NULL = ones (reference multi_stage.py:67-79 loss_weight_{level}) */
  float* mean_scores;        /* out, device [batch][classes]: mean over the level's kept years (may be NULL) */
  float* kept;               /* out, device {kept years, 1 / kept years} (may be NULL) */
  float* loss;               /* out, device scalar */
  float* dscore;             /* out, device [batch][classes] = d(loss) / d(ONE kept year's scores); NULL: no gradient */
  float* scratch;            /* device, batch + 2 floats; the last word must be zero on entry and is left zero */
} dta_level;
size_t dta_multistage_workspace_bytes(const dta_net_desc* d, int levels, const dta_level* lv);
int dta_multistage_forward_loss(const dta_net_desc* d, int levels, const dta_level* lv, const dta_subnet_params* nets,
                                const float* const* x, const float* gate, void* workspace, void* stream);
/* The forward alone (reference MultiStage.predict_step, multi_stage.py:306-318: every level's model on the SAME crops -- the
 * x entries of the levels may point at the same tensors; and validation): lv[l].mean_scores receives each level's mean over its
 * kept years, lv[l].kept (may be NULL) {kept, 1 / kept}; labels / loss / dscore / scratch are not read. */
int dta_multistage_forward(const dta_net_desc* d, int levels, const dta_level* lv, const dta_subnet_params* nets,
                           const float* const* x, const float* gate, void* workspace, void* stream);
/* ... and with the inference epilogue of every level in the SAME call: each level's mean over its kept years, softmax over
 * its classes and the top-2 labels / scores (reference multi_stage.py:306-318 + main.py:190-205) in ONE launch behind the
 * forward.  probs (may be NULL, entries may be NULL) / top_idx / top_score: HOST arrays of `levels` device pointers
 * ([batch][classes] float32, [batch][2] int64, [batch][2] float32); lv[l].mean_scores (may be NULL) receives the scores. */
int dta_multistage_predict(const dta_net_desc* d, int levels, const dta_level* lv, const dta_subnet_params* nets,
                           const float* const* x, const float* gate, void* workspace, float* const* probs,
                           long long* const* top_idx, float* const* top_score, void* stream);
int dta_multistage_backward(const dta_net_desc* d, int levels, const dta_level* lv, const dta_subnet_params* nets,
                            void* workspace, const dta_subnet_grads* grads, const float* gate, void* stream);

/* ---- Hierarchical ensemble label (reference multi_stage.py:368-402 gather_predictions + :404-434 ensemble: the levels'
 * top-1 classes of a crop become ONE species label and score by a walk down the hierarchy; :436-485 evaluation_scores:
 * per-species accuracy / precision from the labels).  The hierarchy is a table: for level l and class c,
 * next[off[l] + c] is the level to consult next (always a later one) or -1, and species[off[l] + c] the species label of
 * a terminal class.  The walk starts at level 0.
 *  table (device int32): off[levels + 1], next[off[levels]], species[off[levels]]
 *  classes: every level's class count on the host (off[l + 1] - off[l]); the calls check it against their level arguments
 * Outputs per crop: ens_label int64 [batch] (-1 where a level's top-1 class is outside its range, e.g. a row of NaN),
 * ens_score float32 [batch] (the top-1 probability of the level the walk ended on: that level's top_score[:, 0], bit for
 * bit), ens_level int32 [batch] (that level).
 * labels (device int64 [batch], species labels) and confusion (device int64 [n_species][n_species], rows = label,
 * columns = prediction) come together or not at all: confusion is ACCUMULATED into with 64-bit integer atomic adds
 * (order-independent), so a caller sums over an epoch without a launch of its own; a label or prediction outside
 * [0, n_species) is skipped. */
typedef struct dta_hierarchy {
  int levels, n_species;
  int classes[DTA_MAX_LEVELS];
  const int* table;
} dta_hierarchy;
/* dta_multistage_predict with the walk in the SAME launch as the levels' softmax + top-2 (still one launch behind the
 * forward); the per-level outputs are dta_multistage_predict's, bit for bit. */
int dta_multistage_predict_ensemble(const dta_net_desc* d, int levels, const dta_level* lv, const dta_subnet_params* nets,
                                    const float* const* x, const float* gate, void* workspace, float* const* probs,
                                    long long* const* top_idx, float* const* top_score, const dta_hierarchy* table,
                                    long long* ens_label, float* ens_score, int* ens_level, const long long* labels,
                                    long long* confusion, void* stream);
/* The walk alone, on per-level [batch][2] top-2 arrays as dta_softmax_top2 / dta_multistage_predict leave them (HOST arrays
 * of `levels` device pointers; the first column is read): for levels that were predicted one by one. */
int dta_hierarchy_resolve(int levels, const long long* const* top_idx, const float* const* top_score, int batch,
                          const dta_hierarchy* table, long long* ens_label, float* ens_score, int* ens_level,
                          const long long* labels, long long* confusion, void* stream);

/* ---- Validation on the device (reference multi_stage.py:290-304 validation_step: weighted cross-entropy + softmax + the
 * metric collection of :20-28 / main.py:53-61; :323-366 and main.py:96-133 validation_epoch_end).  ONE launch per batch does,
 * for every level, the loss, the softmax, the top-2 and the metric counts, and ADDS to epoch accumulators, so that an epoch
 * needs no launch and no host read of its own:
 *  confusion : int64 [classes][classes], confusion[label][top-1 class] += 1 (64-bit integer atomics: order-independent)
 *  counts    : int64 {rows counted, top-1 hits, top-k hits, batches}
 *  loss_acc  : float64 {sum over batches of batch_loss * batch, sum of batch}: the epoch loss weighted by batch size is
 *              loss_acc[0] / loss_acc[1]; one writer per call and level, no floating-point atomics (reruns are bit-identical)
 * The caller zeroes the accumulators at the start of an epoch.  A row whose label is outside [0, classes) or whose scores
 * are NaN is left out of confusion and counts[0..2].  top_k: 1..DTA_EVAL_TOP_K_MAX; a tie goes to the lower class index, as
 * in the top-2 outputs. */
#define DTA_EVAL_TOP_K_MAX 8
typedef struct dta_eval_level {
  float* probs; long long* top_idx; float* top_score;   /* per-batch outputs [batch][classes], [batch][2], [batch][2]; probs may be NULL */
  long long* confusion; long long* counts; double* loss_acc;   /* accumulators, may each be NULL */
  int top_k;
} dta_eval_level;
/* Eval-mode forward of the levels x kept-years networks + the epilogue above, ONE chain.  d->training must be 0 and
 * d->heads_mask carry DTA_FORWARD_ONLY; DTA_REUSE_PACKED is refused (validation follows weight updates).  Of lv[l], labels,
 * loss and scratch are required, weight / mean_scores / kept are optional, dscore is not written.  Each level brings its own
 * inputs and labels (x: one tensor per network, as for dta_multistage_forward_loss).  Every argument is checked on the host
 * before anything is launched. */
int dta_multistage_validate(const dta_net_desc* d, int levels, const dta_level* lv, const dta_eval_level* ev,
                            const dta_subnet_params* nets, const float* const* x, const float* gate,
                            void* workspace, void* stream);
/* The epilogue alone on [batch][classes] scores (single models: Hang2020, metadata fusion, one year ensemble).
 * weight may be NULL (= ones); loss: device scalar; scratch: batch + 2 floats, last word zero on entry and left zero. */
int dta_eval_metrics(const float* scores, const long long* labels, const float* weight, int batch, int classes,
                     float* loss, float* scratch, const dta_eval_level* ev, void* stream);

/* ---- Peer gradient exchange: data-parallel training with one process per GPU of ONE node (reference train.py:89-98:
 * Lightning DDP all-reduces every parameter's gradient between loss.backward() and optimizer.step()).  Here the sum over
 * ranks and the Adam step are ONE launch on the caller's compute stream: every rank pulls its shard of all ranks'
 * gradient buffers through IPC-mapped peer memory (xGMI), publishes the sums in its staging area, and every rank then
 * pulls all summed shards and steps its full (replicated) optimizer state -- no collective library, no side stream, no
 * stream-event hops; sums are taken in rank order, so replicas stay bit-identical.  Waits inside the kernel are bounded:
 * a missing peer sets a status word (dta_xchg_status) instead of hanging the GPU.
 * EXCEPTION to the "allocates nothing" rule above: the exchange object owns device memory that peers map -- the flat
 * float32 gradient buffer (dta_xchg_grad_buffer; the backward entry points write the step's gradients there) and an
 * uncached signal + staging allocation.  Create it once per trainer, destroy it after a barrier over the ranks.
 *  handles: DTA_XCHG_HANDLE_BYTES per rank (dta_xchg_export writes this rank's; dta_xchg_connect takes all ranks' in
 *  rank order, gathered by the caller over any side channel, e.g. torch.distributed.all_gather_object). */
typedef struct dta_xchg dta_xchg;
#define DTA_XCHG_HANDLE_BYTES 128
#define DTA_XCHG_MAX_WORLD 8
int dta_xchg_create(int rank, int world, size_t n_floats, dta_xchg** out);
float* dta_xchg_grad_buffer(dta_xchg* x);          /* device pointer, dta_xchg_grad_capacity(x) floats, zero-filled */
size_t dta_xchg_grad_capacity(dta_xchg* x);        /* n_floats rounded up to a multiple of 4 */
int dta_xchg_export(dta_xchg* x, void* handles);
int dta_xchg_connect(dta_xchg* x, const void* all_handles);
/* Bound of every in-kernel wait (default 1800 s, a collective library's watchdog scale: rank skew of seconds is routine).
 * A wait that expires is FATAL for the exchange: the launch writes the status word and returns without applying anything,
 * and every later launch of this exchange returns at once (sticky), so a replica cannot train on past a failed exchange. */
void dta_xchg_set_timeout(dta_xchg* x, double seconds);
/* Exchange the buffer as two segments, head [0, split_floats) and tail [split_floats, n): the head can then be summed
 * ahead of the exchange launch by dta_net_backward_xchg.  Only before the first step; every rank sets the same split
 * (a multiple of 4 floats; 0 = one segment, the default). */
int dta_xchg_set_split(dta_xchg* x, size_t split_floats);
/* Grid bound of the exchange launch (default 256, one workgroup per CU); only before the first step.  Ranks that share
 * one GPU (tests) must keep world x workgroups co-resident: every rank's launch waits in-kernel for the others. */
void dta_xchg_set_max_workgroups(dta_xchg* x, int workgroups);
/* Overlapped form without a combined kernel: the reduce-scatter of the HEAD segment [0, split) of the exchange's NEXT launch
 * as a launch of its own (16 workgroups) on `stream` -- e.g. a side stream beside the caller's last gradient kernel, or the
 * compute stream itself.  The head must be complete on `stream` (kernel boundary / event); the dta_xchg_allreduce /
 * dta_xchg_adam_step that follows (ordered after this launch by the caller) then sums only the tail and gathers both.
 * One rank or no split: a no-op.  alpha_g / alpha_slot as below (the slot must lie inside the head).  This is the device
 * code dta_net_backward_xchg / dta_ensemble_backward_xchg run in the spare workgroups of the first conv's weight gradient.
 * Replaces: DDP's first gradient bucket being all-reduced while the backward still runs (reference train.py:89-98). */
int dta_xchg_reduce_head(dta_xchg* x, const double* alpha_g, long long alpha_slot, void* stream);
/* g := sum over ranks of g (all ranks end with the same bits).  alpha_g (may be NULL): this rank's float64 d(alpha); the
 * launch first stores it, rounded to float32, in slot alpha_slot of the gradient buffer, so that it takes part in the sum. */
int dta_xchg_allreduce(dta_xchg* x, const double* alpha_g, long long alpha_slot, void* stream);
/* Sum over ranks + dta_adam_step_dp's update in one launch.  p / m / v: this rank's flat buffers of
 * dta_xchg_grad_capacity(x) floats; alpha_slot: index (in floats) of alpha's exchange slot inside the gradient buffer, or
 * -1 with alpha_p NULL; alpha_g: this rank's float64 d(alpha) as the backward left it -- the launch rounds it to float32
 * into the slot before the sum (no float atomics anywhere: replicas and reruns are bit-identical) and afterwards stores
 * the summed gradient there (zero_grad = 0) or clears it.  zero_grad != 0: the gradient buffer is cleared for the next backward; else it holds the sum. */
int dta_xchg_adam_step(dta_xchg* x, float* p, float* m, float* v, size_t n, double* alpha_p, double* alpha_g,
                       long long alpha_slot, double* alpha_m, double* alpha_v, int step, float lr, float beta1, float beta2,
                       float eps, float grad_scale, int zero_grad, void* stream);
/* Self-test aid (peer_probe.py): fill the gradient buffer with a known pattern of (rank, step) BY A KERNEL on `stream`, so
 * that an exchange enqueued right behind it tests exactly what a train step relies on -- gradients written by the kernel
 * before the exchange on the same stream are visible to the peers' system-scope loads (kernel-boundary write-back). */
int dta_xchg_selftest_fill(dta_xchg* x, int step, void* stream);
/* ... and its counterpart behind the exchange: compares the buffer with the sum over ranks of step `step`'s patterns ON THE
 * DEVICE and adds the number of differing elements to a counter (dta_xchg_selftest_mismatches reads it after a
 * synchronisation).  fill -> all-reduce -> verify triples can so be enqueued back to back, with no host synchronisation
 * between steps -- what a training loop does, and what a lazily written-back buffer would not survive. */
int dta_xchg_selftest_verify(dta_xchg* x, int step, void* stream);
int dta_xchg_selftest_mismatches(dta_xchg* x);
/* 0 = every step so far completed; otherwise (phase << 8 | rank waited for) of the first timed-out wait (host-side read of
 * a pinned word, no synchronisation: a launch that timed out has written it by the time it ends; trainers poll it at the
 * start of every step). */
int dta_xchg_status(dta_xchg* x);
/* Development aid: how long workgroup 0 of the LAST exchange launch waited for the ranks to arrive and how long the
 * exchange proper took afterwards, in microseconds (pinned host words: synchronise the stream first). */
int dta_xchg_last_timing(dta_xchg* x, float* wait_us, float* exchange_us);
/* Orderly teardown in two collective steps: every rank UNMAPS its peers' buffers (dta_xchg_disconnect), the ranks meet at a
 * barrier, and only then does anybody free what the others had mapped (dta_xchg_destroy, which also disconnects when that
 * was not done).  Freeing while a peer still holds a mapping is safe for the peer, but a buffer re-created at the same address
 * right away (probe -> trainer, one trainer after another) then races with the peer's close of the old mapping: seen as
 * hipIpcGetMemHandle / stale-mapping failures with eight processes on one test GPU. */
int dta_xchg_disconnect(dta_xchg* x);
int dta_xchg_destroy(dta_xchg* x);

/* ---- stand-alone building blocks (same kernels as the network-level path) ------------------------------------ */

typedef struct dta_conv_module_desc {
  int batch, in_channels, filters, height, width;   /* filters in {32, 64, 128} */
  int pool;        /* 1: MaxPool2d(2) after ReLU (conv_module.forward(x, pool=True)) */
  int training, dtype;
  float bn_momentum, bn_eps;
} dta_conv_module_desc;

/* Replaces conv_module.forward (Hang2020.py:24-31): x NCHW float32 -> out NCHW float32 [batch][filters][H'][W'].
 * Workspace (dta_conv_module_workspace_bytes) is kept for the backward call. */
size_t dta_conv_module_workspace_bytes(const dta_conv_module_desc* d);
int dta_conv_module_forward(const dta_conv_module_desc* d, const float* conv_w, const float* conv_b, const float* bn_w,
                            const float* bn_b, float* bn_rm, float* bn_rv, long long* bn_nbt, const float* x,
                            void* workspace, float* out, void* stream);
/* dout: NCHW gradient of `out`.  dx_nhwc (optional, needs in_channels in {32,64,128}): gradient wrt x as
 * [batch][H*W][in_channels].  g_* arrive zero-filled. */
int dta_conv_module_backward(const dta_conv_module_desc* d, const float* conv_w, const float* bn_w, void* workspace,
                             const float* dout, float* dx_nhwc, float* g_conv_w, float* g_conv_b, float* g_bn_w,
                             float* g_bn_b, void* stream);

typedef struct dta_attention_desc {
  int batch, filters, height, width;   /* filters in {32, 64, 128} */
  int kind;                            /* 0 spectral_attention, 1 spatial_attention */
} dta_attention_desc;

/* Replaces spectral_attention.forward (Hang2020.py:149-168) / spatial_attention.forward (:105-124).
 * params: the module's tensors in the order of dta_subnet_params.att.  x_nhwc: [batch][H*W][filters] float32.
 * out_nchw: gated map [batch][filters][H][W]; feat: pooled features [batch][F]. */
size_t dta_attention_workspace_bytes(const dta_attention_desc* d);
int dta_attention_forward(const dta_attention_desc* d, const float* const params[6], const float* x_nhwc, void* workspace,
                          float* out_nchw, float* feat, void* stream);
/* dout_nchw / dfeat: gradients of the two outputs (either may be null).  dx_nhwc: [batch][H*W][filters].
 * grads[6] arrive zero-filled (null entries are skipped). */
int dta_attention_backward(const dta_attention_desc* d, const float* const params[6], const float* x_nhwc, void* workspace,
                           const float* dout_nchw, const float* dfeat, float* dx_nhwc, float* const grads[6], void* stream);

/* Replaces Classifier.forward / nn.Linear (Hang2020.py:63-66) and its backward.  gw / gb arrive zero-filled. */
int dta_linear_forward(const float* x, const float* w, const float* b, int batch, int in_features, int out_features,
                       float* out, void* stream);
int dta_linear_backward(const float* x, const float* w, const float* dout, int batch, int in_features, int out_features,
                        float* dx, float* gw, float* gb, void* stream);

/* Measurement aid (host-side state only): record a HIP-event pair around every launch of a kernel site, on the
 * stream the kernel is launched on.  site = DTA_SITE_* + layer (0..2); each call adds a site (up to four are timed at
 * once), -1 stops and forgets them all.  dta_profile_collect_site waits for the recorded events of one site, writes up
 * to `max` durations in milliseconds (HOST pointer) and returns the count; dta_profile_collect = the first site. */
enum { DTA_SITE_CONV_FWD = 0, DTA_SITE_CONV_WGRAD = 3, DTA_SITE_CONV_DGRAD = 6, DTA_SITE_STAGE_FWD = 9,
       DTA_SITE_STAGE_BWD = 12,
       DTA_SITE_GEMM = 15 /* +0 classifier heads forward, +1 head input gradients, +2 parameter-gradient group */ };
int dta_profile_enable(int site);
/* Time only every stride-th launch of an enabled site (default 1): an event pair costs ~5 us of stream time per launch,
 * which a throughput measurement running beside the timing should not pay on every step. */
int dta_profile_set_stride(int stride);
int dta_profile_collect(float* ms, int max);
int dta_profile_collect_site(int site, float* ms, int max);
/* Development aid.  The PRODUCT library (libdta_hip.so) reads nothing from the environment: dta_dev_switches_enabled()
 * returns 0 and dta_dev_reload_switches() fails.  The developer library (libdta_hip_dev.so: the same sources compiled with
 * -DDTA_DEV_SWITCHES) reads its switches (DTA_NO_FUSED_INPUT, DTA_NO_TAIL_MERGE, DTA_BN_INKERNEL, DTA_NO_LEAN, DTA_FANIN,
 * ...: same-box A/B runs of alternative launch plans) once at load time, and again on dta_dev_reload_switches(). */
int dta_dev_switches_enabled(void);
int dta_dev_reload_switches(void);

/* ---- site-metadata head of the fusion model (reference src/models/metadata.py:9-44) --------------------------------
 * meta = ReLU(Linear(Dropout(BatchNorm1d(Embedding(site)))))  (16 wide), out = ReLU(Linear(cat[meta, hsi_scores])).
 * Replaces the reference's torch modules `metadata` (:9-24) and the `fc1` fusion layer of `metadata_sensor_fusion` (:26-44)
 * for the train / validation step of MetadataModel (:52-83); the HSI scores come from dta_net_forward.
 * All tensors float32, row-major; site: int64 indices in [0, sites).  drop: [batch][16] dropout factors (0 or 1/(1-p)),
 * or NULL (no dropout / eval) -- drawn by the caller (torch's generator), applied here.  training != 0: batch statistics
 * (and the running statistics are updated with `momentum`), else running statistics.  The workspace
 * (dta_meta_head_workspace_bytes) carries the forward's state to the backward. */
typedef struct dta_meta_params {
  const float* emb;            /* [sites][16]   metadata_model.embedding.weight */
  const float* bn_w; const float* bn_b;   /* [16]  metadata_model.batch_norm.weight / bias */
  float* bn_rm; float* bn_rv; long long* bn_nbt;   /* running_mean / running_var [16], num_batches_tracked (may be NULL) */
  const float* mlp_w; const float* mlp_b;  /* [classes][16], [classes]   metadata_model.mlp */
  const float* fc_w; const float* fc_b;    /* [classes][2*classes], [classes]   fc1 (columns: [site scores | hsi scores]) */
} dta_meta_params;
typedef struct dta_meta_grads {   /* same shapes; zero-filled on entry (bias gradients are accumulated); NULL = not wanted */
  float* emb; float* bn_w; float* bn_b; float* mlp_w; float* mlp_b; float* fc_w; float* fc_b;
} dta_meta_grads;
size_t dta_meta_head_workspace_bytes(int batch, int classes, int sites);
/* out[batch][classes] = the fused scores (after the last ReLU) */
int dta_meta_head_forward(int batch, int classes, int sites, int training, float momentum, float eps, const dta_meta_params* p,
                          const long long* site, const float* scores, const float* drop, void* workspace, float* out,
                          void* stream);
/* unweighted cross-entropy of the fused scores (MetadataModel.training_step, metadata.py:52-63) in one launch: loss (0-d) and
 * dout[batch][classes] = d(loss)/d(the last ReLU's INPUT), i.e. the ReLU's backward is applied; scratch: batch + 2 floats,
 * word batch + 1 zero on entry (left zero).  dout may be NULL (validation). */
int dta_meta_head_loss(int batch, int classes, const float* out, const long long* labels, float* loss, float* dout, float* scratch,
                       void* stream);
/* dout = what dta_meta_head_loss wrote; writes the parameter gradients and dscores[batch][classes] = d(loss)/d(hsi scores) */
int dta_meta_head_backward(int batch, int classes, int sites, int training, const dta_meta_params* p, const long long* site,
                           const float* drop, void* workspace, const float* out, const float* dout, const dta_meta_grads* grads,
                           float* dscores, void* stream);

/* Prediction with the fusion model (eval mode: running statistics, no dropout).  The site branch then depends on the site
 * alone, so fc1's first `classes` columns contribute one bias row per site:
 *   T[s][c]   = fc_b[c] + sum_j fc_w[c][j] * ReLU(mlp_b[j] + sum_f mlp_w[j][f] * bn(emb[s][f]))      j < classes, f < 16
 *   out[b][c] = ReLU(T[site_b][c] + sum_k fc_w[c][classes + k] * scores[b][k])                       k < classes
 * dta_meta_site_table writes T and the re-laid-out HSI half of fc_w into the caller's workspace (one launch; reads the
 * running statistics, writes nothing else; any number of sites up to 2^20).  dta_meta_predict is then ONE launch per batch:
 * fused scores, softmax and top-2 (dta_softmax_top2's rule: value descending, ties to the lower class).  2 <= classes <= 1020.
 * site: int64 [batch] on the device, or NULL: every row has site `site_all` (a raster has one site), which is then checked
 * here.  A row whose site is outside [0, sites) gets top_idx -1, top_score 0 and zero out / probs rows (dta_crown_reduce's
 * empty-crown convention); nothing is read out of bounds.  out / probs [batch][classes] may be NULL.  top_idx [batch][2]
 * int64, top_score [batch][2] float32.  Each (row, class) is one float32 accumulator over k ascending, no atomics: a row's
 * bits do not depend on the batch size or on its place in the batch.  The workspace must be 16-byte aligned. */
size_t dta_meta_predict_workspace_bytes(int classes, int sites);
int dta_meta_site_table(int classes, int sites, float eps, const dta_meta_params* p, void* workspace, void* stream);
int dta_meta_predict(int batch, int classes, int sites, const void* workspace, const long long* site, long long site_all,
                     const float* scores, float* out, float* probs, long long* top_idx, float* top_score, void* stream);

/* ---- Dense per-pixel window prediction over a raster (reference src/patches.py:50-83 `bounds_to_pixel`: one 11x11 window
 * per pixel of a crown box, read with boundless=True; src/main.py:165-178).  The preprocessing above is per pixel position
 * and a size x size window resized to size x size is the identity, so the preprocessed window equals the window of the
 * preprocessed raster, bit for bit (an out-of-bounds pixel, zero-filled by the reference's reader, stays zero).
 *
 * dta_raster_normalise: the clipped per-pixel min-max of dta_preprocess_crops (same float32 rounding, same `tiny` rule,
 * NaNs passed over) for a whole band-first raster raw[bands_raw][height][width] of element type `dtype` (DTA_CROP_*), once.
 *  tiles == 0: out = float32 [C][height][width], C = dta_preprocess_out_bands(bands_raw, clip)
 *  tiles != 0: out = bf16 channel chunks [ceil(C / 16)][height * width][16], rounded as dta_preprocess_crops_tiles rounds,
 *              bands past C zero. */
int dta_raster_normalise(const void* raw, int bands_raw, int height, int width, int clip, int dtype, int tiles, void* out,
                         void* stream);
/* n windows of size x size (4..253, what the networks take) out of the float32 raster [bands][height][width]:
 * origins [n][2] int32 = (row, col) of each window's top-left corner in raster pixels, device memory; negative origins and
 * windows that run past the raster are allowed, positions outside the raster are zero.  out: float32 [n][bands][size][size]
 * (16-byte aligned). */
int dta_gather_windows(const float* raster, int bands, int height, int width, const int* origins, int n, int size,
                       float* out, void* stream);
/* The same out of the bf16 chunk form, written as the tiles dta_net_forward_tiles takes:
 * tiles bf16 [n][ceil(bands / 16)][size * size][16].  raster and tiles 16-byte aligned. */
int dta_gather_windows_tiles(const void* raster, int bands, int height, int width, const int* origins, int n, int size,
                             void* tiles, void* stream);
/* Per-crown mean of per-window probability rows (reference src/main.py:165-205: the pixel crops of a crown).  Rows arrive
 * grouped by crown: crown k owns rows offsets[k] .. offsets[k + 1] - 1 of probs [rows][classes] (offsets: int64
 * [n_crowns + 1], non-decreasing, device memory).  Each class is summed in row order in float32 and divided by the count
 * (no atomics: reruns are bit-identical).  mean [n_crowns][classes]; top_idx [n_crowns][2] int64 / top_score [n_crowns][2]
 * = the two largest entries of the mean, ties to the lower class as dta_softmax_top2; count [n_crowns] int32.  An empty
 * crown: count 0, labels -1, scores and mean 0.  The offsets live on the device, so this call does NOT check them: that
 * they are non-decreasing and end within the rows of probs is the caller's to guarantee (dense.crown_reduce does). */
int dta_crown_reduce(const float* probs, const long long* offsets, int n_crowns, int classes, float* mean,
                     long long* top_idx, float* top_score, int* count, void* stream);


/* ---- Dense multi-stage prediction: the levels x years networks of a multi-stage model on the windows of the years'
 * rasters (dta_multistage_predict_ensemble on gathered batches), and ONE species label per crown.
 *
 * dta_gather_windows_years: dta_gather_windows for every year of an ensemble in ONE launch.  rasters / outs: HOST arrays of
 * `years` (1..DTA_MAX_YEARS) device pointers, every raster float32 [bands][height][width], every out float32
 * [n][bands][size][size]; origins and size are shared.  A NULL raster is a missing year: nothing is written for it (the
 * caller points that year's network input at a zero buffer of its own) and its flag stays 0; at least one year must be
 * present.  For a present year the bytes written are dta_gather_windows'.
 * flags [years] float32 ends as what dta_year_flags says about the years' batches: 1 where a year's batch has a non-zero
 * element (NaN counts), else 0 -- taken from the values while they are written, so no batch is read back.  Bank protocol
 * of dta_year_flags: flags must be zero on entry; with clear_next (the other bank, [years]) the call zeroes that bank for
 * the next call, with clear_next == NULL the call clears flags itself first.  Plain stores only: no atomics. */
int dta_gather_windows_years(const float* const* rasters, int years, int bands, int height, int width, const int* origins,
                             int n, int size, float* const* outs, float* flags, float* clear_next, void* stream);
/* ---- Crops of crown boxes out of the resident raster: the reference's production prediction path (src/patches.py:5-30
 * `crop` cuts a crown's bounding box out of the tile, src/utils.py:59-79 `load_image` preprocesses it and resizes it to
 * size x size with NEAREST).  The preprocessing is per pixel position and a NEAREST resize only selects pixels, so the
 * resized, preprocessed crop of a box is an index selection from the normalised raster, bit for bit what
 * dta_preprocess_crops[_tiles] writes for the host-sliced raw crop.
 *
 * boxes [n][4] int32 = (row0, col0, row1, col1), half-open, in raster pixels, device memory; h = row1 - row0,
 * w = col1 - col0.  Output pixel (i, j) of crop k reads raster pixel
 *   (row0 + min(floor(i * float32(h / size)), h - 1), col0 + min(floor(j * float32(w / size)), w - 1))
 * -- the float32 arithmetic of ATen's nearest index, the one dta_preprocess_crops resizes with (an integer i * h / size is
 * not the same function).  flip != 0: output pixel (i, j) takes the resized pixel (size - 1 - i, size - 1 - j), both
 * training flips after the resize (dta_crop_desc.flip).  A box with h <= 0 or w <= 0 gives an all-zero crop (the
 * reference dataset's fill for a missing crop, data.py:295-296).  A source position outside the raster reads 0: a box
 * that was not clipped to the raster never reads out of bounds (clip boxes on the host to get the reference's
 * intersection; dense.crop_boxes).  size 1..4096; n >= 1.
 *
 * dta_gather_crops:        float32 raster [bands][height][width] -> out float32 [n][bands][size][size]
 * dta_gather_crops_tiles:  bf16 chunks [ceil(bands / 16)][height * width][16] -> tiles bf16 [n][ceil(bands / 16)][size * size][16]
 * dta_gather_crops_years:  dta_gather_crops for every year of an ensemble in ONE launch, all years the same boxes; rasters /
 *                          outs / flags / clear_next exactly as dta_gather_windows_years takes them (a NULL raster: a
 *                          missing year, nothing written, flag 0; flags from the values on their way out, NaN counts as
 *                          non-zero; the bank protocol of dta_year_flags).
 * raster and out / tiles 16-byte aligned.  Pure copies: no atomics, reruns are bit-identical. */
int dta_gather_crops(const float* raster, int bands, int height, int width, const int* boxes, int n, int size, int flip,
                     float* out, void* stream);
int dta_gather_crops_tiles(const void* raster, int bands, int height, int width, const int* boxes, int n, int size, int flip,
                           void* tiles, void* stream);
int dta_gather_crops_years(const float* const* rasters, int years, int bands, int height, int width, const int* boxes,
                           int n, int size, int flip, float* const* outs, float* flags, float* clear_next, void* stream);
/* One species per crown out of per-window, per-level probabilities, in ONE launch: for every level what dta_crown_reduce
 * gives on probs[l] [rows][table->classes[l]] (mean[l] [n_crowns][classes_l] -- `mean` or single entries may be NULL --,
 * top_idx[l] / top_score[l] [n_crowns][2], bit for bit; count [n_crowns] once), then what dta_hierarchy_resolve gives on
 * those per-level top-1 columns: ens_label int64 / ens_score / ens_level int32 [n_crowns].  The meaning of a crown with
 * several windows is THIS library's: the mean over the crown's windows per level, then the walk (the reference has one row
 * per crown at this point; for one window per crown the two agree exactly).  An empty crown: count 0, per-level labels -1,
 * ens_label -1, ens_level 0, ens_score 0.
 * probs / mean / top_idx / top_score: HOST arrays of `levels` device pointers.  window_labels (device int64 [rows], the
 * windows' own ens_label) and votes (device int32 [n_crowns][n_species]) come together or not at all: votes[k][s] = the
 * number of crown k's windows whose label is s (labels outside [0, n_species) are not counted); every row is zeroed by the
 * workgroup that owns it, then counted with integer adds.  No floating-point atomics: reruns are bit-identical.
 * As for dta_crown_reduce the offsets live on the device and are NOT checked here (dense.crown_resolve does). */
int dta_crown_resolve(int levels, const float* const* probs, const long long* offsets, int n_crowns,
                      const dta_hierarchy* table, float* const* mean, long long* const* top_idx, float* const* top_score,
                      int* count, long long* ens_label, float* ens_score, int* ens_level, const long long* window_labels,
                      int* votes, void* stream);

/* ---- Dense prediction with the first conv computed ONCE PER RASTER instead of once per window.  The first 3x3 conv sits
 * in front of every pool, so its output at a window position depends only on the raster pixel p under that position and on
 * which taps fall outside the window: one of nine classes, (top / middle / bottom row) x (left / middle / right column).
 *   T[q][dy][dx][n]  = sum_k w[n][k][dy+1][dx+1] * x[k][q]                 (one GEMM over the raster's pixels; 0 outside it)
 *   A[p][rc][cc][n]  = bias[n] + sum_{dy in R(rc)} sum_{dx in R(cc)} T[p + (dy, dx)][dy][dx][n]
 *   R(top / left) = {0, +1},  R(middle) = {-1, 0, +1},  R(bottom / right) = {-1, 0}
 *   conv1(window at origin o)[i][j][n] = A[o + (i, j)][rc(i)][cc(j)][n],   rc(i) = top if i == 0, bottom if i == 10, else middle
 * This is exact.  Only 11x11 windows; d->kind DTA_NET_HANG2020 (64 columns: spectral | spatial branch, as the forward
 * concatenates them), DTA_NET_SPECTRAL or DTA_NET_SPATIAL (32 columns).  Of d these calls read kind, dtype and bands (the
 * raster's NORMALISED band count); the raster is in the form of its dtype: DTA_BF16 the chunk form of dta_raster_normalise
 * (tiles != 0), DTA_F32 the float32 planes.
 *
 * The table: [(height + 2) * (width + 2) + 1][9][cols] -- the positions of the raster extended by a one-pixel ring,
 * row-major, then one "far outside" row (a position two or more pixels outside has every tap on zero input: the bias), the
 * class index rc * 3 + cc -- stored as the forward stores its first conv's output: IEEE half in bf16 mode, float32 in fp32
 * mode.  Each element is ONE float32 accumulator: the bias first, then the taps in ascending (dy, dx); no atomics.
 * dta_conv1_table_bytes: the sizes of the scratch (the weight image and T, only needed during dta_raster_conv1_table) and
 * of the table.  A 256x256 raster with 64 columns: 151 MB of scratch, 77 MB of table in half. */
int dta_conv1_table_bytes(const dta_net_desc* d, int height, int width, size_t* scratch_bytes, size_t* table_bytes);
/* nets: the network's parameter table (2 entries for Hang2020, else 1); reads conv_w[0] and conv_b[0] of each.  raster,
 * scratch and table 16-byte aligned.  Three launches (weight image, tap GEMM, class sums), once per raster and weight state. */
int dta_raster_conv1_table(const dta_net_desc* d, const dta_subnet_params* nets, const void* raster, int height, int width,
                           void* scratch, void* table, void* stream);
/* The first conv's output of n windows: row m * 121 + i * 11 + j of y0 ([n * 121][cols], row stride cols) receives the cols
 * values of A[o_m + (i, j)][rc(i)][cc(j)] -- a pure copy in 16-byte pieces, so y0 holds the table's bits.  origins [n][2]
 * int32 (row, col) as for dta_gather_windows: anywhere, negative or past the raster.  y0: normally workspace + offset of
 * dta_conv1_output_range for a descriptor of batch n. */
int dta_gather_conv1_windows(const dta_net_desc* d, const void* table, int height, int width, const int* origins, int n,
                             void* y0, void* stream);
/* Where the forward keeps its first conv's output inside the workspace of `d`: byte offset and size
 * (batch * height * width rows of cols elements in the storage format above). */
int dta_conv1_output_range(const dta_net_desc* d, size_t* offset, size_t* bytes);
/* dta_net_forward for a workspace whose first-conv output is ALREADY in place (dta_gather_conv1_windows): no input, no
 * input pack job, no row table and no conv launch for the first layer; everything behind it is dta_net_forward's.  Eval
 * mode (training == 0) with DTA_FORWARD_ONLY, 11x11 patches, kinds as above; anything else is refused.  With
 * DTA_REUSE_PACKED the usual contract holds, with one addition: this call does not leave the first layer's row table in
 * the workspace: a dta_net_forward / dta_net_forward_tiles carrying DTA_REUSE_PACKED must still follow one of those two
 * calls WITHOUT the flag on that workspace (this call with the flag may follow any of the three without it). */
int dta_conv1_forward(const dta_net_desc* d, const dta_subnet_params* nets, const double* alpha, void* workspace,
                          float* const scores[2][3], float* joint, void* stream);

/* ---- ... for a multi-stage model (dta_multistage_*: levels x years spectral networks, every level's year-y network on
 * year y's raster): ONE table per year with the levels side by side, ONE gather launch per batch for all levels x years,
 * then the grouped forward behind its first convs.  d is the multi-stage descriptor (kind DTA_NET_SPECTRAL, 11x11).
 *
 * A year's table: [(height + 2) * (width + 2) + 1][9][levels * 32], columns 32 l .. 32 l + 31 the first conv of level l's
 * year-y network -- each 32-column slice holds the bits dta_raster_conv1_table gives for that network alone; storage as
 * above.  Its mask: one byte per table position, 1 where the raster pixel under it has a non-zero stored element (NaN
 * counts; for a bf16 raster the bf16 values), 0 on the ring and in the far-outside row.  A missing year (raster == NULL)
 * gets a table of the far-outside row alone ([9][levels * 32]: the biases -- what the first conv gives on an all-zero
 * input) and a mask of one zero byte.
 * Sizes per raster pixel: 9 x 32 x levels x 2 B of table in half (4 B in fp32), and 9 x 32 x levels x 4 B of T in the
 * scratch, which the years share (build them one after the other on one stream).  5 levels at 256x256: 189 MB of table
 * per year plus 377 MB of scratch.
 * dta_conv1_multistage_table_bytes: height == width == 0 asks for a missing year's sizes (no scratch). */
int dta_conv1_multistage_table_bytes(const dta_net_desc* d, int levels, int height, int width, size_t* scratch_bytes,
                                     size_t* table_bytes, size_t* mask_bytes);
/* nets: `levels` parameter tables, level l's year-y network at nets[l] (conv_w[0] and conv_b[0] are read).  raster: the
 * year's normalised raster in the form of d->dtype, or NULL for a missing year (height, width and scratch are then not
 * used).  raster, scratch and table 16-byte aligned.  Four launches (weight image, tap GEMM, class sums, mask). */
int dta_conv1_multistage_raster_table(const dta_net_desc* d, int levels, const dta_subnet_params* nets, const void* raster,
                                      int height, int width, void* scratch, void* table, unsigned char* mask, void* stream);
/* Where the grouped forward keeps its first convs' outputs inside the workspace of dta_multistage_workspace_bytes: group g
 * (network lv[l].first + year) at offset + g * group_stride, [batch * 121][32] in the storage format above; bytes =
 * group_stride * networks. */
int dta_conv1_multistage_output_range(const dta_net_desc* d, int levels, const dta_level* lv, size_t* offset,
                                      size_t* group_stride, size_t* bytes);
/* The first convs of n (<= d->batch) windows for every level x year in ONE launch: level l's 32 columns of
 * A_y[o_m + (i, j)][rc(i)][cc(j)] go to row m * 121 + i * 11 + j of group lv[l].first + y in `workspace` (a pure copy in
 * 16-byte pieces; every level must have `years` networks).  tables / masks: HOST arrays of `years` device pointers as
 * dta_conv1_multistage_raster_table left them; present: HOST array, present[y] == 0 marks a missing year's one-row table
 * (every position reads it); at least one year must be present.  height / width: the present years' rasters.
 * flags [years] float32: 1 where any position of the batch's windows has its mask byte set, else 0 -- for an fp32 raster
 * exactly what dta_year_flags says about the float32 batch dta_gather_windows_years would have written.  Bank protocol
 * of dta_gather_windows_years (flags zero on entry; clear_next zeroed for the next call, or NULL: flags cleared first).
 * Plain stores only: no atomics. */
int dta_conv1_multistage_gather_windows(const dta_net_desc* d, int levels, const dta_level* lv, int years,
                                        const void* const* tables, const unsigned char* const* masks, const int* present,
                                        int height, int width, const int* origins, int n, void* workspace, float* flags,
                                        float* clear_next, void* stream);
/* dta_multistage_predict / dta_multistage_predict_ensemble for a workspace whose first-conv outputs are ALREADY in place
 * (dta_conv1_multistage_gather_windows): no inputs, no input pack job, no row table and no conv launch for the first
 * layer of any group; everything behind it, the epilogue included, is the code of those two calls.  Eval mode
 * (training == 0) with DTA_FORWARD_ONLY and 11x11 patches only.  DTA_REUSE_PACKED: dta_conv1_forward's contract (these calls
 * do not leave the first layer's row table behind). */
int dta_conv1_multistage_predict(const dta_net_desc* d, int levels, const dta_level* lv, const dta_subnet_params* nets,
                                 const float* gate, void* workspace, float* const* probs, long long* const* top_idx,
                                 float* const* top_score, void* stream);
int dta_conv1_multistage_predict_ensemble(const dta_net_desc* d, int levels, const dta_level* lv, const dta_subnet_params* nets,
                                          const float* gate, void* workspace, float* const* probs, long long* const* top_idx,
                                          float* const* top_score, const dta_hierarchy* table, long long* ens_label,
                                          float* ens_score, int* ens_level, const long long* labels, long long* confusion,
                                          void* stream);

/* ---- Species abundance with uncertainty: trees per species over predicted crowns, and the reference's confusion
 * resampling of that count (src/multinomial.py:28-35, 61-77, run 100 times by sample_multinomial.py; abundance.py's
 * value_counts is dta_abundance_counts).  Per iteration t and crown i of n:
 *   counter = (first_iteration + t) * n + i                                       (64 bits, modulo 2^64)
 *   mix(z)  : z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^ (z >> 31)
 *   r_keep / r_draw = mix(counter * 0x9E3779B97F4A7C15 + mix(seed * 0x9E3779B97F4A7C15 + stream + 1)) >> 40, stream 0 / 1
 *   keep    = !(float(r_keep) * 2^-24 >= score[i])        (a NaN score keeps; score == NULL: every crown keeps)
 *   drawn   = the number of entries of table[label[i]] that are <= r_draw
 *   counts[t][keep ? label[i] : drawn] += 1
 * A label outside [0, species) counts in bin `species` whatever its score (DEAD, the walk's unresolved -1); a crown with
 * mask[i] == 0 (mask may be NULL: none) is counted nowhere.  table: uint32 [species][species], row p for a crown predicted
 * as p: non-decreasing thresholds in units of 2^-24 whose last entry is 2^24 (deeptreeattention_amd/abundance.py:
 * sampling_table builds it on the host from a confusion matrix; the rows are NOT checked here).
 * counts: int64 [iterations][species + 1], OVERWRITTEN in full by the call (not added to; nothing has to be cleared).
 * Integer sums only, no atomics on global memory: reruns are bit-identical, and equal the host definition
 * (abundance.resample_np) bit for bit.  Two launches: every iteration in one, then the sum of the workgroups' partial
 * histograms, which live in `workspace` (dta_abundance_workspace_bytes(n, species, iterations) bytes, 8-byte aligned;
 * 0 and dta_last_error() for a bad shape).  n >= 1, 1 <= species <= DTA_ABUNDANCE_MAX_SPECIES, iterations >= 0
 * (0: nothing is launched).  stream: a hipStream_t, as everywhere here. */
#define DTA_ABUNDANCE_MAX_SPECIES 256
size_t dta_abundance_workspace_bytes(long long n, int species, int iterations);
int dta_abundance_resample(const long long* label, const float* score, const unsigned char* mask, long long n,
                           const unsigned int* table, int species, int iterations, unsigned long long seed,
                           unsigned long long first_iteration, long long* counts, void* workspace, size_t workspace_bytes,
                           void* stream);
/* The plain count: counts int64 [species + 1], the same bins and mask, overwritten in full; the workspace of
 * dta_abundance_workspace_bytes(n, species, 1). */
int dta_abundance_counts(const long long* label, const unsigned char* mask, long long n, int species, long long* counts,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- Abundance per tile and map cell (the reference counts a site tile by tile: src/multinomial.py:run resamples one
 * tile, abundance.py:read_shp counts one, src/neon_paths.py:bounds_to_geoindex says which 1 km tile a crown belongs to).
 * deeptreeattention_amd/abundance.py: cells_np, the group= forms of counts_np / resample_np and summary_np are the
 * definitions and the kernels equal them bit for bit.
 *
 * dta_abundance_cells: cell[i] = row * cols + col of crown box i, rows growing with northing, or -1 outside the
 * cols x rows grid.  boxes: double [n][4] (xmin, ymin, xmax, ymax) on the device; origin: double [2] on the HOST.  All
 * arithmetic in double, every operation rounded on its own (no FMA).  Per axis, with (lo, hi) the box's two coordinates:
 *   DTA_CELLS_GEOINDEX  e = trunc((lo + hi) / 2), toward zero as Python's int();  k = floor_div(e - origin, size) in
 *                       integers: the reference's rule with origin 0 and size 1000.  size and origin must be integers
 *                       (size <= 2^31-1, |origin| < 2^53); a centre that is not finite or not below 2^53 gives -1
 *   DTA_CELLS_CENTRE    k = floor(((lo + hi) * 0.5 - origin) / size), any finite origin and positive size
 * One launch.  Refused before it: a null boxes / origin / cell, n < 1, cols or rows < 1, another rule, a size that is not
 * positive and finite, an origin that is not finite, a non-integer size or origin under DTA_CELLS_GEOINDEX. */
#define DTA_CELLS_GEOINDEX 0
#define DTA_CELLS_CENTRE 1
int dta_abundance_cells(const double* boxes, long long n, int rule, const double* origin, double size, int cols, int rows,
                        long long* cell, void* stream);

/* dta_abundance_resample_grouped: dta_abundance_resample per cell in one call.  counts: int64 [iterations][groups]
 * [species + 1]; plane g is dta_abundance_resample with mask[i] && group[i] == g on the same n, seed and first_iteration:
 * the counter of a draw is the crown's index in the WHOLE input, so a crown draws the same species whichever cell it is
 * counted in.  A crown whose group is outside [0, groups) is counted nowhere.
 * The caller orders the crowns by cell: group_sorted int64 [n], the groups ascending, and order int64 [n], the crown at
 * each sorted position (torch.sort(group, stable=True) gives both; the sums are integers, so the order among equal groups
 * changes nothing).  An order entry outside [0, n) is counted nowhere.  Nothing is read back from the device: a workgroup
 * owns a FIXED slice of sorted positions (the slices of dta_abundance_resample) and 8 iterations, whatever the cells'
 * sizes, and walks the runs of equal cell inside its slice; a crown is read once per 8 iterations.
 * counts is OVERWRITTEN in full (cleared by a memset on `stream` in front of the kernels; empty cells are zeros; the
 * caller clears nothing); a cell may lie in several slices, so its partial counts are added with 64-bit integer atomics:
 * any order gives the same sums, reruns are bit-identical.  No float atomics.  workspace:
 * dta_abundance_grouped_workspace_bytes(n, species, iterations, groups) bytes (0 and dta_last_error() for a bad shape),
 * 8-byte aligned, written in full before it is read: nothing in it survives a call.  1 <= groups <= 2^31-2; the other
 * bounds are dta_abundance_resample's.  Three stream operations: the memset, a gather of the crowns into cell order, the
 * resampling. */
size_t dta_abundance_grouped_workspace_bytes(long long n, int species, int iterations, long long groups);
int dta_abundance_resample_grouped(const long long* label, const float* score, const unsigned char* mask,
                                   const long long* group_sorted, const long long* order, long long n, long long groups,
                                   const unsigned int* table, int species, int iterations, unsigned long long seed,
                                   unsigned long long first_iteration, long long* counts, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* The plain count per cell: counts int64 [groups][species + 1], overwritten in full; the workspace of
 * dta_abundance_grouped_workspace_bytes(n, species, 1, groups). */
int dta_abundance_counts_grouped(const long long* label, const unsigned char* mask, const long long* group_sorted,
                                 const long long* order, long long n, long long groups, int species, long long* counts,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* dta_abundance_summary: mean and quantiles over the iterations of a resampled table, grouped or not.  table: int64
 * [iterations][entries] on the device; mean: double [entries]; out_quantiles: double [quantiles][entries].  Per entry:
 *   mean = (double)(integer sum over the iterations) / (double)iterations
 *   quantile j: a, b = the lower[j]-th and min(lower[j] + 1, iterations - 1)-th smallest value (0-based), d = b - a,
 *               frac[j] >= 0.5 ? b - d * (1 - frac[j]) : a + d * frac[j]      every operation rounded on its own (no FMA)
 * lower / frac: HOST arrays: floor(q * (iterations - 1)) and the remainder, formed by the caller in double (NumPy's linear
 * rule; abundance.summary_np is the definition).  One launch: a workgroup stages iterations x 64 adjacent entries in LDS
 * and one lane sorts one column, which bounds iterations by DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS (128 KB of the 160 KB).
 * Refused before the launch: a null table / mean (lower / frac / out_quantiles with quantiles > 0), iterations outside
 * 1..DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS, entries < 1, quantiles outside 0..DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES, a lower
 * outside [0, iterations) or a frac outside [0, 1). */
#define DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS 256
#define DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES 16
int dta_abundance_summary(const long long* table, int iterations, long long entries, const int* lower, const double* frac,
                          int quantiles, double* mean, double* out_quantiles, void* stream);

/* ---- Crown height filter: the canopy-height statistic of every crown box of a resident CHM raster, and the reference's keep
 * rules on it (src/CHM.py:9-14 non_zero_99_quantile, run per crown through rasterstats.zonal_stats; :58-95 height_rules;
 * src/predict.py:35-42 find_crowns: CHM_height > 3).  chm: float32 [height][width] on the device.  boxes: int32 [n][4] =
 * (row0, col0, row1, col1), half-open, any int32 values: each box is clipped to the raster.  Per crown i:
 *   kept   = the cells v of the clipped box with v >= floor, one float32 comparison (drops NaN, nodata, everything under it)
 *   count  = the number of kept values; 0: out_height = NaN
 *   virt   = float32(count - 1) * (float32(q) / float32(100));  lo = floor(virt);  t = virt - lo;  hi = min(lo + 1, count - 1)
 *   a, b   = the lo-th and hi-th smallest kept value (0-based), selected exactly;  d = b - a
 *   out_height = t >= 0.5 ? b - d * (1 - t) : a + d * t        every operation rounded to float32 on its own (no FMA):
 * np.nanpercentile's result on float32 input, bit for bit (deeptreeattention_amd/canopy.py: crown_height_np is the definition).
 * A clipped box of more than 2^24 cells is refused on the device, where the boxes live: out_count = -1, out_height = NaN,
 * out_keep = 0.  The rule, in double after exact widening (chm = out_height):
 *   mode 1  keep = chm > min_height                                   (a NaN height is dropped)
 *   mode 2  with h = field_height[i], in this order: chm NaN: 0; h NaN: 1; chm < min_chm: 0;
 *           chm > h: !(chm - h >= max_diff); otherwise: !(h - chm >= limit)
 * out_keep: 0 / 1 bytes [n], NULL exactly when rule is NULL or its mode is 0; field_height: double [n] on the device, read
 * in mode 2 only.  Every output element is overwritten.  Two launches (one wave per crown of up to DTA_CROWN_WAVE_CELLS
 * clipped cells; one workgroup per larger crown), no workspace, no atomics on global memory: the result of a crown depends
 * on its own box alone.  Refused on the host, before any launch: a null chm / boxes / out_height / out_count, n < 1,
 * height or width < 1, height * width over int32, q outside [0, 100] or NaN, floor not > 0 (kept values must order by their
 * bit patterns), an unknown mode, mode 2 without field_height, a keep buffer without a rule and the reverse. */
#define DTA_CROWN_WAVE_CELLS 1024
typedef struct {
  int mode;          /* 0 none, 1 min height, 2 height rules */
  double min_height; /* mode 1 */
  double min_chm, max_diff, limit;   /* mode 2 */
} dta_height_rule;
int dta_crown_height(const float* chm, int height, int width, const int* boxes, long long n, float q, float floor,
                     const double* field_height, const dta_height_rule* rule, float* out_height, int* out_count,
                     unsigned char* out_keep, void* stream);

/* ---- Alive/dead crown filter: the data preparation in front of the reference's alive/dead classifier and the score behind
 * it (src/models/dead.py: utm_dataset.__getitem__ -- the crown's box plus one metre read from the RGB tile, ToTensor,
 * Normalize, Resize([224, 224]) per crown on a CPU worker; predict_dead -- label = argmax, score = max of
 * softmax(sigmoid(logits))).  The classifier itself is the caller's network between the two calls.
 *
 * Crops.  raster: uint8 [channels][height][width] on the device, 1 to 4 channels.  boxes: int32 [n][4] = (row0, col0, row1,
 * col1), half-open, any int32 values.  Per crown: the box is grown by `pad` pixels on every side and clipped to the raster
 * (origin (r0, c0), h rows, w columns); with S = size, every operation in float32 and rounded on its own, except the source
 * position sy * (i + 0.5) - 0.5, which is one fused multiply-add (as torch's CPU interpolate computes it):
 *   p(c, y, x) = (float(raster[c][r0 + y][c0 + x]) / 255 - mean[c]) / std[c]
 *   sy = float(h) / float(S);  fy = max(sy * (i + 0.5) - 0.5, 0);  y0 = min(int(fy), h - 1);  y1 = min(y0 + 1, h - 1);  ly = fy - y0
 *   (the same for the columns: sx, fx, x0, x1, lx)
 *   out(c, i, j) = (1 - ly) * ((1 - lx) * p(c,y0,x0) + lx * p(c,y0,x1)) + ly * ((1 - lx) * p(c,y1,x0) + lx * p(c,y1,x1))
 * which is bilinear interpolation with align_corners = False and no antialiasing, also where the box is larger than S x S
 * (deeptreeattention_amd/dead.py: crops_np is the definition).  out: [n][channels][S][S] of `dtype` (one rounding of the
 * float32 result for the 16-bit types), in that order in memory, or as [n][S][S][channels] when channels_last != 0.
 * out_valid: 0 / 1 bytes [n]: 0 for a box with row1 <= row0 or col1 <= col0 and for one whose grown box misses the raster;
 * such a crown's outputs are zeros.  Every output element is overwritten.  One launch of at most DTA_RGB_CROPS_MAX_GROUPS
 * workgroups, no workspace, no atomics.  mean, std: HOST arrays of `channels` floats.  Refused on the host, before any
 * launch: a null pointer, n < 1 or over int32, channels outside 1..4, height or width < 1, channels * height * width over
 * int32, size outside 1..DTA_RGB_CROPS_MAX_SIZE, pad < 0, an unknown dtype, a zero std, a NaN mean or std, an out pointer
 * that is not aligned to its element. */
enum { DTA_ELEM_F32 = 0, DTA_ELEM_BF16 = 1, DTA_ELEM_F16 = 2 };
#define DTA_RGB_CROPS_MAX_GROUPS 1024
#define DTA_RGB_CROPS_MAX_SIZE 512
int dta_rgb_crops(const unsigned char* raster, int channels, int height, int width, const int* boxes, long long n, int size,
                  int pad, const float* mean, const float* std, int dtype, int channels_last, void* out,
                  unsigned char* out_valid, void* stream);
/* The score.  logits: [rows][2] of `dtype` (DTA_ELEM_*) on the device, the classifier's output for one batch.  In float32:
 * s = 1 / (1 + exp(-logit));  p = softmax(s) over the two classes;  out_score[offset + r] = max(p),
 * out_label[offset + r] = 1 if p[1] > p[0] else 0 (a tie is 0, as np.argmax).  offset: where the batch starts in the result
 * arrays of the whole tile, so a driver writes every batch straight into them.  One launch.  Refused before it: a null
 * pointer, rows < 1, offset < 0, an unknown dtype. */
int dta_dead_head(const void* logits, int dtype, long long rows, long long offset, long long* out_label, float* out_score,
                  void* stream);

/* ---- Training the alive/dead classifier from a resident image pool (train_dead.py; src/models/dead.py: AliveDead -- an
 * ImageFolder of small RGB images, ToTensor, Normalize, Resize([224, 224]), RandomHorizontalFlip, and the loss
 * F.cross_entropy(F.sigmoid(logits), y)).  deeptreeattention_amd/dead.py: pool_batch_np, flips_np and loss_np are the
 * definitions.
 *
 * dta_image_pool_batch: one batch, crops and labels, in ONE launch.
 *   data:   uint8 [data_bytes] on the device: every image planar [channels][h][w], back to back
 *   table:  int64 [n][4] on the device: (offset of the image in data, h, w, label); n: 1..DTA_EPOCH_ORDER_MAX_N
 *   index:  the images of the batch, on the device: int32 (index64 == 0) or int64 [start + count] at least, read at
 *           start .. start + count - 1 -- so an epoch's order (dta_epoch_order) is read in place --, or NULL: image start + b
 *   flip:   0 / 1 bytes [count] on the device, per place of the batch, or NULL for none.  hash_flips != 0 (then flip must be
 *           NULL): image i is flipped where  mix(((epoch * n + i) mod 2^64) * 0x9E3779B97F4A7C15 + mix(seed *
 *           0x9E3779B97F4A7C15 + DTA_DEAD_FLIP_STREAM + 1)) >> 40  <  2^23: a function of the image, not of its place
 *   out:    [count][channels][size][size] of `dtype` (DTA_ELEM_*), or [count][size][size][channels] when channels_last != 0:
 *           place b holds dta_rgb_crops' crop of the whole image (box (0, 0, h, w), pad 0) -- the same arithmetic, the same
 *           bits --, with its columns reversed where the image is flipped (output column j takes the values of column
 *           size - 1 - j)
 *   out_labels: int64 [count]: the images' labels
 * An index outside 0..n-1 (and a table row that does not lie inside data) gives a crop of zeros and label -1; nothing is
 * read for it.  At most DTA_RGB_CROPS_MAX_GROUPS workgroups, no workspace, no atomics.  mean, std: HOST arrays of `channels`
 * floats.  Refused on the host, before any launch: a null data, table, mean, std, out or out_labels, n or data_bytes out
 * of range, channels outside 1..4, count < 1, start < 0, start + count > n without an index, flip together with hash_flips,
 * size outside 1..DTA_RGB_CROPS_MAX_SIZE, an unknown dtype, a zero std, a NaN mean or std, an out pointer that is not
 * aligned to its element (16-byte stores are used where out is 16-byte aligned and the line length allows it). */
#define DTA_DEAD_FLIP_STREAM 3       /* the hash stream of the flips (csrc/hash_dev.h lists the streams in use) */
#define DTA_DEAD_ORDER_LEVEL 63      /* the level id dead.ImagePool.loader gives dta_epoch_order: stream 16 + 63 */
int dta_image_pool_batch(const unsigned char* data, long long data_bytes, const long long* table, long long n, int channels,
                         const void* index, int index64, long long start, long long count, const unsigned char* flip,
                         int hash_flips, unsigned long long seed, unsigned long long epoch, int size, const float* mean,
                         const float* std, int dtype, int channels_last, void* out, long long* out_labels, void* stream);
/* dta_dead_loss: the loss of one batch, its gradient and the confusion counts in ONE launch of one workgroup.
 * logits: [rows][2] of `dtype` on the device; labels: int64 [rows].  Per row with a label in {0, 1}, in float32:
 *   s = 1 / (1 + exp(-l));  m = max(s0, s1);  lse = m + log(exp(s0 - m) + exp(s1 - m));  loss_row = lse - s[y]
 *   p = exp(s - lse);  d_l[c] = (p[c] - [c == y]) * s[c] * (1 - s[c]) / B_valid
 * out_loss[0]: the float64 sum of loss_row (per lane in row order, then a fixed tree: a rerun gives the same bits) over
 * B_valid, rounded to float32 once; 0 where B_valid = 0.  out_dlogits: float32 [rows][2], zeros for the other rows.
 * out_counts: int64 [5]: conf[label][argmax l, a tie giving 0] as four, then the rows whose label is outside {0, 1}.
 * accumulator: NULL, or DTA_DEAD_ACC_WORDS 8-byte words on the device that the caller zeroed once: a float64 loss sum,
 * then int64 rows, conf[2][2], bad; this call's sums are added (launches of one stream follow each other).  No atomics.
 * Refused before the launch: a null logits, labels, out_loss, out_dlogits or out_counts, rows outside
 * 1..DTA_DEAD_LOSS_MAX_ROWS, an unknown dtype, an accumulator that is not 8-byte aligned. */
#define DTA_DEAD_ACC_WORDS 7
#define DTA_DEAD_LOSS_MAX_ROWS 16777216
int dta_dead_loss(const void* logits, int dtype, const long long* labels, long long rows, float* out_loss, float* out_dlogits,
                  long long* out_counts, void* accumulator, void* stream);

/* ---- Reflectance cube to resident raster: the array work of the reference's generate_raster (src/Hyperspectral.py:152-219:
 * band selection, window, transpose to band-first) and of load_image's preprocessing (src/utils.py:36-57) in one pass over a
 * pixel-interleaved cube, as a NEON reflectance tile is stored ([rows][cols][426] int16).  For every pixel of the column
 * window and every k < bands:
 *   v[k] = float(strip[row][col0 + x][band_index[k]])
 *   out  = dta_raster_normalise's arithmetic on v[0 .. bands) -- the same float32 roundings, the same `tiny` rule, NaNs passed
 *          over by the min and the max -- so the result is bit for bit what dta_raster_normalise(clip = 0) gives for the
 *          selected, transposed bands.  band_index is the caller's whole selection: a band mask with load_image's 10 + 10
 *          clip already applied (deeptreeattention_amd/reflectance.py: reflectance_np is the definition).
 * strip: [rows][width_src][bands_src] of `dtype` (DTA_CROP_*) on the device; band_index: int32 [bands] on the device, any
 * order, repeats allowed, every value in [0, bands_src) (a value outside is clamped into the range, never followed).
 * out: the WHOLE raster of out_height x cols pixels, float32 [bands][out_height][cols] (tiles == 0) or the bf16 chunk form
 * [ceil(bands / 16)][out_height * cols][16] of dta_raster_normalise (bands past `bands` in the last chunk are zero).  The
 * call writes the raster rows out_row0 .. out_row0 + rows - 1 and nothing else, so a tile can be taken strip by strip
 * through a bounded raw buffer.  One launch, no workspace, no atomics; no byte outside strip[0 .. rows * width_src *
 * bands_src) is read.  Refused on the host, before any launch: a null pointer; a size below 1, col0 < 0 or out_row0 < 0;
 * col0 + cols > width_src; out_row0 + rows > out_height; an unknown dtype; out_height * cols >= 2^31; a strip or out that
 * is not 16-byte aligned; bands_src or bands over DTA_REFLECTANCE_MAX_BANDS. */
#define DTA_REFLECTANCE_MAX_BANDS 1024
typedef struct dta_reflectance_desc {
  int bands_src;    /* bands per pixel of the cube */
  int width_src;    /* pixels per cube row */
  int rows;         /* rows in this strip */
  int col0, cols;   /* column window; cols == raster width */
  int dtype;        /* DTA_CROP_* as dta_raster_normalise */
  int tiles;        /* 0: float32 [C][H][W]; else bf16 [ceil(C/16)][H*W][16] */
  int out_height;   /* rows of the whole resident raster */
  int out_row0;     /* first raster row this strip writes */
} dta_reflectance_desc;
int dta_reflectance_normalise(const dta_reflectance_desc* d, const void* strip, const int* band_index, int bands, void* out,
                              void* stream);

/* ---- Site boundary clip: which points, crown boxes and raster cells lie inside a polygon (the reference's
 * gpd.clip(crowns, boundary) in abundance.py:24-35, create_prediction_shp.py:33-41 and src/multinomial.py:16-19).
 * edges: double [n_edges][4] (ax, ay, bx, by) on the device, every ring of the (Multi)Polygon closed, any orientation, `org`
 * already subtracted; the region is the even-odd interior of all rings together.  org: double [2] on the HOST, subtracted
 * from every query coordinate first.  All arithmetic in double, every product and every difference rounded on its own (no
 * FMA, no division); deeptreeattention_amd/boundary.py: contains_np / boxes_np / rasterise_np are the definition and the
 * kernels equal them bit for bit.
 *   point p, edge k:  straddle = (ay > py) != (by > py);  dx = bx - ax;  dy = by - ay;  l = (px - ax) * dy;
 *                     r = (py - ay) * dx;  left = dy > 0 ? l < r : l > r;  inside = parity of (straddle & left) over the
 *                     edges; a NaN coordinate gives 0
 *   box (x0, y0, x1, y1):  code 0 if a coordinate is not finite or x1 < x0 or y1 < y0.  Edge k touches the filled rectangle
 *                     unless both of its ends are on the outer side of one box side (ax < x0 && bx < x0, ...) or the four
 *                     corner signs s(c) = dx * (cy - ay) - dy * (cx - ax) are all > 0 or all < 0.  code = 1 if any edge
 *                     touches, else 2 if (x0, y0) is inside, else 0
 *   pixel box (row0, col0, row1, col1) with transform (x0, a, y0, e) (double [4] on the HOST; rasterio's
 *                     Affine(a, 0, x0, 0, e, y0)):  x = x0 + col * a, y = y0 + row * e, then min / max per axis
 *   raster cell (r, c):  the point (x0 + (c + .5) * a, y0 + (r + .5) * e)
 * out: bytes, every element overwritten (points, raster: 0 / 1; boxes: the code).  One launch each, no workspace, no
 * atomics on global memory.  Refused on the host, before any launch: a null edges / org / queries / out; n < 1 or
 * n >= 2^31; n_edges outside 3 .. 2^20; height or width < 1, height * width over int32; both or neither of geo_boxes and
 * pixel_boxes; pixel_boxes without transform, geo_boxes with one; a non-finite org or transform; a == 0 or e == 0. */
#define DTA_BOUNDARY_EDGE_CHUNK 1024        /* edges staged through LDS at a time */
#define DTA_BOUNDARY_MAX_EDGES (1 << 20)
int dta_boundary_points(const double* edges, int n_edges, const double* org, const double* points, long long n,
                        unsigned char* out, void* stream);
int dta_boundary_boxes(const double* edges, int n_edges, const double* org, const double* geo_boxes, const int* pixel_boxes,
                       const double* transform, long long n, unsigned char* out, void* stream);
int dta_boundary_raster(const double* edges, int n_edges, const double* org, int height, int width, const double* transform,
                        unsigned char* out, void* stream);

/* ---- Train/test plot split search: the reference's train_test_split (src/data.py:165-236), which runs sample_plots
 * (:108-162) config["iterations"] times on a dask cluster and keeps the split with the most test species.  Everything
 * depends on integer tables over plots x species (deeptreeattention_amd/split.py builds them; search_np there is the
 * definition, and the kernels equal it bit for bit):
 *   A individuals, B individuals with at least one row that is not "fixed", R rows (individual x year)
 *   rows:   int [candidates][3][SP] on the device: A, B, R of each candidate plot, SP = species rounded up to a multiple of 4,
 *           the padding zero
 *   totals: int [2][SP] on the device: totA and totR, the sums of A and R over ALL plots
 *   floor:  double [species] on the HOST: max((double)totA[s] * 0.05, (double)min_test)
 * Iteration t (t = 0 .. iterations - 1) orders the candidates ascending by (draw32, j) with
 *   draw32 = mix(((first_iteration + t) * candidates + j) * 0x9E3779B97F4A7C15 + mix(seed * 0x9E3779B97F4A7C15 + 1)) >> 32
 * (all modulo 2^64; mix as for dta_abundance_resample), or, where `orders` (int [iterations][candidates] on the device) is
 * given, by row t of it, which the CALLER has checked to be a permutation (an entry outside 0 .. candidates - 1 is only
 * kept from leaving the table).  Then
 *   cnt = 0; wanted[s] = 1; inc[p] = 0
 *   for p in that order:  if any s has A[p][s] > 0 and wanted[s]:  inc[p] = 1; cnt += A[p]; wanted[s] = !((double)cnt[s] > floor[s])
 *   T[s] = (sum of B over inc)[s] >= min_test  &&  totA[s] - cnt[s] >= min_train
 *   species[t] = popcount(T);  train_rows[t] = sum over T of (totR[s] - (sum of R over inc)[s]);  test_plots[t] = popcount(inc)
 *   membership[t][p] = inc[p] and taxa[t][s] = T[s], bytes, where those pointers are not null
 *   best = { t, species[t], train_rows[t], test_plots[t] } of the lexicographic maximum of (species, train_rows), the
 *          smallest t on a full tie
 * Two launches (one wavefront per iteration; one workgroup for the best), no workspace, no atomics; every output element
 * is overwritten.  Refused on the host, before any launch: a null rows / totals / floor / species / train_rows /
 * test_plots / best; species outside 1 .. DTA_SPLIT_MAX_SPECIES; candidates outside 1 .. DTA_SPLIT_MAX_CANDIDATES (the
 * sort keeps 8 bytes per candidate, rounded up to a power of two, in LDS: 32 KB per wavefront at 4096, five wavefronts per
 * compute unit; twice that would be the 64 KB a workgroup gets by default and leave two); iterations < 0 (0 launches
 * nothing and writes nothing); min_train or min_test below 1; rows or totals not 16-byte aligned; a floor that is not finite. */
#define DTA_SPLIT_MAX_SPECIES 256
#define DTA_SPLIT_MAX_CANDIDATES 4096
int dta_split_search(const int* rows, const int* totals, int candidates, int species, const double* floor, int min_train,
                     int min_test, int iterations, unsigned long long seed, unsigned long long first_iteration,
                     const int* orders, int* out_species, long long* out_train_rows, int* out_test_plots, long long* best,
                     unsigned char* membership, unsigned char* taxa, void* stream);

/* ---- Field stems to crown boxes: which predicted crown box a field-measured stem gets and which stem a box keeps (the
 * reference's process_plot with create_boxes and choose_box, src/generate.py:62-153, and the last line of points_to_crowns,
 * :239).  deeptreeattention_amd/stems.py: assign_np is the definition and the kernels equal it bit for bit.  Both tables
 * are SORTED BY PLOT and every index below is a row of the sorted tables:
 *   boxes:       double [n_boxes][4] (xmin, ymin, xmax, ymax) on the device; box_start: int [plots + 1] on the device, the
 *                boxes of plot p are the rows box_start[p] .. box_start[p + 1] - 1
 *   points:      double [n_points][2] (x, y); point_plot: int [n_points], the plot code of every stem; point_start: int
 *                [plots + 1] as box_start; height: double [n_points], NaN where not measured; chm: the same or NULL
 * Stem i of plot p (all in double, every product, sum and difference rounded on its own, no FMA):
 *   candidates:  the boxes j of plot p with xmin <= px <= xmax and ymin <= py <= ymax (closed; false with a NaN)
 *   missing:     a stem without a candidate; its fallback box is (px - size, py - size, px + size, py + size) with the index
 *                n_boxes + i, a candidate of every MISSING stem of plot p that lies in it
 *   choice:      the candidate with the smallest d2 = (cx - px) * (cx - px) + (cy - py) * (cy - py), cx = (xmin + xmax) * 0.5,
 *                cy = (ymin + ymax) * 0.5; a NaN d2 counts as +inf; the lowest index among equals
 *   one stem per box, G = the stems with the same choice:  |G| = 1 keeps it.  Else S = the stems of G at the largest height
 *                that is not NaN; if |S| > 1 and chm is given, S = those of S at the largest chm that is not NaN; the lowest
 *                index of S is kept, and nobody if S is empty
 *   choice_out:  long long [n_points], the chosen index or -1
 *   status_out:  bytes: 0 dropped for a taller stem, 1 kept with a predicted box, 2 kept with a fallback box, 3 dropped, S is
 *                empty, 4 no box: a coordinate that is not finite or a plot code outside 0 .. plots - 1
 *   crowns_out:  double [n_points][4], the chosen box or NaN
 * Three launches on `stream` (one stem per lane; the rows a workgroup's stems can meet are staged through LDS,
 * DTA_STEMS_CHUNK at a time), no workspace beyond choice_out, no atomics; every output element is overwritten.  An entry of
 * box_start / point_start is clamped into its table before use: nothing is read outside a table whatever the arrays hold.
 * n_boxes == 0 is legal (every stem falls back; boxes must still not be NULL).  Refused on the host, before any launch: a
 * null pointer other than chm; n_points < 1 or >= 2^31; n_boxes < 0 or >= 2^31; plots < 1; a size that is not finite or
 * <= 0. */
#define DTA_STEMS_CHUNK 1024                /* boxes or stems staged through LDS at a time */
int dta_stems_assign(const double* boxes, const int* box_start, long long n_boxes, const double* points, const int* point_plot,
                     const int* point_start, const double* height, const double* chm, long long n_points, int plots,
                     double size, long long* choice_out, unsigned char* status_out, double* crowns_out, void* stream);

/* ---- The resident training set: the crops of a whole data set once on the device, a shuffled order per level and epoch,
 * and the batches of every level x year of a train step in one launch (the reference's TreeDataset, src/data.py:239-310,
 * five of them over the same individuals in src/models/multi_stage.py:82-219).  deeptreeattention_amd/treedata.py:
 * epoch_order_np and batch_np are the definitions and the kernels equal them bit for bit.
 *
 * dta_epoch_order: the order of `levels` (1..DTA_MAX_LEVELS) views in ONE launch.  n: HOST array, the entries of each view,
 * 1..DTA_EPOCH_ORDER_MAX_N; level_ids: HOST array of the levels' stream numbers, each 0..DTA_EPOCH_ORDER_MAX_LEVEL_ID - 1,
 * or NULL for 0, 1, ...; orders: HOST array of device pointers, int [n[l]] each.  Entry i of level l has the key
 *   key_i = mix(((epoch * n[l] + i) mod 2^64) * 0x9E3779B97F4A7C15 + mix(seed * 0x9E3779B97F4A7C15 + S + 1)) >> 32,
 *   S = DTA_EPOCH_ORDER_STREAM + level_ids[l]          (mix as for dta_abundance_resample; streams 0 and 1 are its and
 *                                                       dta_split_search's)
 * and orders[l] holds the entries sorted ascending by (key_i, i): orders[l][#{j : (key_j, j) < (key_i, i)}] = i.  About
 * n^2 compares per level (the keys stream through LDS, hashed on the way), which is what bounds n: 2^20 entries are 1.1e12
 * compares.  No atomics, every element of a table written once.  Refused on the host, before the launch: a null n or orders
 * or table, levels or a level id out of range, an n outside 1..DTA_EPOCH_ORDER_MAX_N. */
#define DTA_EPOCH_ORDER_MAX_N 1048576
#define DTA_EPOCH_ORDER_STREAM 16
#define DTA_EPOCH_ORDER_MAX_LEVEL_ID 64
int dta_epoch_order(int levels, const long long* n, const int* level_ids, unsigned long long seed, unsigned long long epoch,
                    int* const* orders, void* stream);
/* dta_pool_batches: one step's batch of every level and year in ONE launch.
 *   pool:   [pool_rows][years][bands][size][size] on the device, float32 (DTA_F32) or bf16 (DTA_BF16: widened exactly on
 *           the way out); a missing (individual, year) slot holds zeros
 *   lv:     HOST array of `levels` (1..DTA_MAX_LEVELS; levels * years <= DTA_MAX_YEARS networks) entries.  Position p
 *           (0 .. count - 1) of level l brings view entry e = order[start + p] (order NULL: e = start + p) and pool row
 *           rows[e]; flip != 0: the size * size pixels of every plane reversed, which is both training flips together
 *           (src/augmentation.py:13-14)
 *   outs:   HOST array of levels * years device pointers, level-major: float32 [count_l][bands][size][size], 16-byte aligned
 *   out_labels / out_rows of a level: long long [count]: labels[e] and rows[e] (labels and out_labels may both be NULL)
 *   flags:  float [levels * years], level-major: ends as 1 where that batch has a non-zero element (NaN counts, -0.0 does
 *           not), taken from the values on their way out, else stays 0.  The bank protocol of dta_gather_windows_years: flags
 *           zero on entry; clear_next (the other bank) is zeroed for the next call, or NULL: flags is cleared here first.
 *           Plain stores only: no atomics.
 * Every read is guarded on the device: an order entry outside 0 .. n - 1 or a row outside 0 .. pool_rows - 1 writes an
 * all-zero crop (and -1 for an entry that does not exist), so the call cannot read outside the pool or the tables whatever
 * they hold.  Pure copies: reruns are bit-identical.  Refused on the host, before the launch: a null pool / lv / outs /
 * flags / rows / out_rows / out; labels without out_labels or the reverse; a dtype other than the two; levels, years,
 * pool_rows, bands or size out of range; a level with n < 1, start < 0, count < 1 or start + count > n; an out that is not
 * 16-byte aligned. */
typedef struct {
  const int* order;           /* int [n] on the device (dta_epoch_order), or NULL: the identity */
  const long long* rows;      /* [n] on the device: view entry -> pool row */
  const long long* labels;    /* [n] on the device, or NULL */
  long long n;                /* entries of the view */
  long long start;            /* first position of this step's batch */
  int count;                  /* crops of this step's batch */
  int flip;                   /* both training flips */
  long long* out_labels;      /* [count] or NULL */
  long long* out_rows;        /* [count] */
} dta_pool_level;
int dta_pool_batches(const void* pool, int dtype, long long pool_rows, int years, int bands, int size, int levels,
                     const dta_pool_level* lv, float* const* outs, float* flags, float* clear_next, void* stream);
/* dta_pool_batches_keep: dta_pool_batches with an optional per-level year mask.  year_keep: HOST array of `levels` device
 * pointers, each unsigned char [n][years] over the VIEW's entries, or NULL for a level without a mask; a NULL year_keep is
 * dta_pool_batches itself.  Where year_keep[l][e * years + y] is 0 the crop of (entry e, year y) is written as zeros and
 * does not set the year's flag, exactly as a missing year does.  Everything else as above. */
int dta_pool_batches_keep(const void* pool, int dtype, long long pool_rows, int years, int bands, int size, int levels,
                          const dta_pool_level* lv, const unsigned char* const* year_keep, float* const* outs, float* flags,
                          float* clear_next, void* stream);

/* ---- The five level data sets of the reference's MultiStage.create_datasets (src/models/multi_stage.py:82-219) and the
 * loss_weight_<level> buffers of its __init__ (:62-79), from one resident integer table.  deeptreeattention_amd/levels.py:
 * build_np is the definition (it states the rule in full) and the kernels equal it bit for bit.
 *
 * All tables are on the device.  Records r = 0 .. records - 1 in frame order; individuals i coded in order of first
 * appearance.  ind[r], year[r] (0 .. years - 1): the record's individual and year slot; sp[i] (0 .. species - 1): the species
 * label; rank[i]: the place of i's name among all names sorted as strings; first[i]: i's first record; m[i]: its records;
 * present[i][y]: 1 when a record of (i, y) exists.  cls[s]: one of DTA_LEVEL_HEAD .. DTA_LEVEL_PLAIN; lmap[l][s]: the level
 * label of species s in level l, or -1; species_order[s]: the rank of the taxon name.  record_key: int [records], the place
 * of a record in an explicit shuffle of its species' records, or NULL for the hashed one:
 *   key_r = mix(((epoch * records + r) mod 2^64) * 0x9E3779B97F4A7C15 + mix(seed * 0x9E3779B97F4A7C15 + DTA_LEVEL_STREAM + 1)) >> 32
 * Outputs per level l: rows[l], labels[l] (long long [capacity[l]]) and year_keep[l] (unsigned char [capacity[l]][years]):
 * the kept individuals in data set order -- an entry whose place is at or above capacity[l] is not written; n[l]: how many
 * the level keeps; num_classes[l]: the level labels present among the kept records; loss_weight (train only): float
 * [DTA_LEVEL_COUNT][species + 1], the weights of labels 0 .. num_classes[l] - 1 and zeros after them.
 * workspace: dta_level_workspace_bytes(...) bytes, 16-byte aligned (0: sizes out of range).  At most four launches and one
 * memset on the stream, no allocation, no host synchronisation.  Integer atomics only (sums and one max, whose result does
 * not depend on their order): reruns are bit-identical.  About individuals^2 * 6 + records^2 compares.  Every table read is
 * guarded on the device: a code outside its table belongs to no level.  Refused on the host, before a launch: a null
 * argument or table, sizes out of range, train other than 0 / 1, a negative ceiling, min_loss_weight outside 0..1, a
 * capacity outside 0..individuals, a workspace that is too small or misaligned. */
#define DTA_LEVEL_COUNT 5
#define DTA_LEVEL_STREAM 2
#define DTA_LEVEL_MAX_SPECIES 4096
#define DTA_LEVEL_HEAD 0
#define DTA_LEVEL_CONIFER 1
#define DTA_LEVEL_OAK 2
#define DTA_LEVEL_PLAIN 3
typedef struct {
  long long individuals, records;
  int species, years;
  const int* ind;
  const int* year;
  const int* sp;
  const int* rank;
  const int* first;
  const int* m;
  const unsigned char* present;
  const int* cls;
  const int* lmap;
  const int* species_order;
  const int* record_key;
} dta_level_tables;
typedef struct {
  int train;
  long long other_sampling_ceiling, evergreen_ceiling, oaks_sampling_ceiling;
  double min_loss_weight;
  unsigned long long seed, epoch;
} dta_level_config;
typedef struct {
  long long* rows[DTA_LEVEL_COUNT];
  long long* labels[DTA_LEVEL_COUNT];
  unsigned char* year_keep[DTA_LEVEL_COUNT];
  long long capacity[DTA_LEVEL_COUNT];
  int* n;
  int* num_classes;
  float* loss_weight;
} dta_level_out;
size_t dta_level_workspace_bytes(long long individuals, long long records, int species, int years);
int dta_level_build(const dta_level_tables* tables, const dta_level_config* config, const dta_level_out* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- Field records to canopy points: which rows of a raw NEON field table survive (the reference's filter_data,
 * src/data.py:22-106) and the plot code of every stem of a contributed megaplot (megaplot.format, src/megaplot.py:28-90:
 * create_grid with gpd.sjoin, buffer_plots).  deeptreeattention_amd/field.py: filter_np and plots_np are the definitions
 * (they state the rules in full) and the kernels equal them bit for bit.
 *
 * dta_field_filter.  All tables on the device, one entry per row of the field table, in frame order:
 *   individual: int [rows], the code of the row's individual, 0 .. individuals - 1 (the rank of its name among the sorted
 *               unique names); event: int [rows], the rank of the row's event name, >= 0; height, diameter: double [rows],
 *               NaN = missing; flags: unsigned short [rows], the DTA_FIELD_* bits below, made from the table's strings.
 * reason_out[r] is the first step that drops row r, 0 = kept (keep_out[r] = 1):
 *   1 no COORDS; 2 no GROWTH; 3 no LIVE; 4 over the rows that passed 1-3 the individual has a SHADED row and no SUNNY row;
 *   5 not (height > min_height or height is NaN); 6 not (diameter > min_stem_diameter), NaN fails; 7 TAXON_EXCLUDED;
 *   8 EVENT_DROPPED; 9 not the individual's record: among the rows that passed 1-8, an individual with a height keeps the row
 *   of its maximum height (-0.0 equals +0.0), one with none the row of its largest event code, the lowest row among equals
 *   either way; 10 MULTIBOLE; 11 KNOWN_ERROR; 12 PLOT_EXCLUDED; 13 SITE_EXCLUDED.
 *   DTA_FIELD_REASON_BAD_CODE: an individual code outside 0 .. individuals - 1 or an event code below 0; such a row takes
 *   part in nothing and is counted in errors_out (int [1], may be NULL).
 * rows_out: long long [rows]: the kept rows, first those of the individuals chosen by height, ascending by individual code,
 * then those chosen by event, ascending by individual code; -1 behind them.  count_out: long long [1], how many.
 * workspace: dta_field_workspace_bytes(rows, individuals) bytes, 16-byte aligned (0: sizes out of range).  Five launches
 * and one memset on the stream, no allocation, no host synchronisation.  Integer OR / max atomics at device scope only,
 * whose result does not depend on their order: reruns are bit-identical.  Refused on the host, before a launch: a null
 * pointer other than errors_out; rows < 1 or >= 2^31; individuals < 1 or > rows; a threshold that is NaN; a workspace that
 * is too small or misaligned. */
#define DTA_FIELD_COORDS 1
#define DTA_FIELD_GROWTH 2
#define DTA_FIELD_LIVE 4
#define DTA_FIELD_SHADED 8
#define DTA_FIELD_SUNNY 16
#define DTA_FIELD_TAXON_EXCLUDED 32
#define DTA_FIELD_EVENT_DROPPED 64
#define DTA_FIELD_MULTIBOLE 128
#define DTA_FIELD_KNOWN_ERROR 256
#define DTA_FIELD_PLOT_EXCLUDED 512
#define DTA_FIELD_SITE_EXCLUDED 1024
#define DTA_FIELD_REASON_BAD_CODE 255
size_t dta_field_workspace_bytes(long long rows, long long individuals);
int dta_field_filter(const int* individual, const int* event, const double* height, const double* diameter,
                     const unsigned short* flags, long long rows, long long individuals, double min_stem_diameter,
                     double min_height, unsigned char* keep_out, unsigned char* reason_out, long long* rows_out,
                     long long* count_out, int* errors_out, void* workspace, size_t workspace_bytes, void* stream);
/* dta_megaplot_plots.  points: double [n][2] (x, y) on the device; code_out: int [n]; one launch, no workspace, no atomics.
 *   DTA_MEGAPLOT_GRID:   xs: double [nx] and ys: double [ny] on the device, ascending in steps of `cell` (the caller's
 *     np.arange(min, max + cell, cell) over the points' bounds).  Cell (i, j) has the code i * ny + j and is the closed
 *     rectangle xs[i] - cell <= x <= xs[i], ys[j] <= y <= ys[j] + cell, each bound rounded once (the reference's
 *     box(x0, y0, x0 - 40, y0 + 40) does lie to the LEFT of x0).  A point takes the lowest code among the cells that hold it
 *     (the device looks at the two columns and rows on either side of floor((x - xs[0]) / cell), with these comparisons), -1
 *     when none does or a coordinate is not finite.
 *   DTA_MEGAPLOT_BUFFER: code[j] = the highest i with (xi - xj) * (xi - xj) + (yi - yj) * (yi - yj) <= cell * cell, every
 *     product and sum rounded on its own (no FMA); -1 for a stem with a coordinate that is not finite.  n * n compares: n is
 *     at most DTA_MEGAPLOT_BUFFER_MAX.  xs and ys are not read.
 * Refused on the host, before the launch: a null points or code_out; a rule other than the two; a cell that is not finite
 * or <= 0 (or whose square is not finite, buffer rule); n < 1, n >= 2^31 (grid) or n > DTA_MEGAPLOT_BUFFER_MAX (buffer);
 * grid rule: a null table, nx or ny < 1, nx * ny >= 2^31. */
#define DTA_MEGAPLOT_GRID 0
#define DTA_MEGAPLOT_BUFFER 1
#define DTA_MEGAPLOT_BUFFER_MAX 65536
#define DTA_MEGAPLOT_CHUNK 1024             /* stems staged through LDS at a time */
int dta_megaplot_plots(const double* points, long long n, int rule, double cell, const double* xs, int nx, const double* ys,
                       int ny, int* code_out, void* stream);

/* ---- Crown-level evaluation: the reference's experiment report (MultiStage.evaluation_scores, multi_stage.py:436-485;
 * TreeModel.evaluate_crowns, main.py:265-333; site_confusion / genus_confusion / novel_prediction, src/metrics.py) as
 * functions of one grouped confusion table conf[g][t][p] = counted crowns of group g with label t and prediction p.
 * deeptreeattention_amd/evaluate.py: count_np, report_np, first_per_individual_np are the definitions and the kernels equal
 * them bit for bit.  All arrays on the device; no allocation, no host synchronisation.
 *
 * dta_eval_count.  labels, preds: long long [rows]; group: int [rows] (group_is_64 = 0) or long long [rows] (1), NULL = all
 * rows in group 0; mask: unsigned char [rows], NULL = all rows; conf: long long [groups][n_species][n_species] and tally:
 * long long [2], both ACCUMULATED into (the caller zeroes them once).  A row with mask 0 is neither counted nor tallied; a
 * row whose label or prediction is outside 0 .. n_species - 1 or whose group is outside 0 .. groups - 1 adds one to tally[1];
 * every other row adds one to conf[group][label][pred] and to tally[0].  One launch; 64-bit integer atomic adds only, so the
 * result does not depend on their order.  form: DTA_EVAL_COUNT_PLAIN, one atomic per counted row; DTA_EVAL_COUNT_COMBINE,
 * the lanes of a wave that hold the same entry are added up first (DTA_EVAL_COMBINE_ROUNDS first-lane / ballot rounds, what
 * is left goes out singly): the same table either way.  1 <= n_species <= DTA_EVAL_MAX_SPECIES, groups >= 1 and
 * groups * n_species * n_species <= 2^31 - 1 (an entry's index is an int); 1 <= rows <= 2^31 - 1.
 *
 * dta_eval_report.  conf as above (entries >= 0).  One launch of groups + 1 workgroups: workgroup g reduces plane g,
 * workgroup `groups` the sum of all planes (the pooled row).  Row r of
 *   counts  long long [groups + 1][8]: total, correct, wrong, within_site, cross_site, within_genus, cross_genus, species
 *           seen (label sum > 0);
 *   scores  double [groups + 1][4]: micro = correct / total, macro = the sum of the seen species' accuracies, added in class
 *           order, / their number, within_site / wrong, within_genus / wrong;
 *   accuracy, precision double, support long long [groups + 1][n_species] (all three or none): diagonal / label sum,
 *           diagonal / prediction sum, label sum.
 * Every quotient is one IEEE division of two integers converted to double; a zero denominator gives 0.0.  site_masks:
 * unsigned long long [n_species][site_words], 1 <= site_words <= DTA_EVAL_MAX_SITE_WORDS, bit b of a species = it occurs on
 * site b; an error (t != p) is within_site when the two masks share a bit.  genus: int [n_species]; an error is within_genus
 * when the two ids are equal.  Either may be NULL: its two counts are 0 and its share 0.0.
 *
 * dta_first_rows.  ids: int [rows] (ids_is_64 = 0) or long long [rows] (1); first_out: unsigned char [rows] = 1 where the row
 * is the lowest row of its id (the reference's groupby("individual").head(1)), 0 elsewhere and for an id outside
 * 0 .. n_ids - 1; workspace: int [n_ids].  One fill and two launches (an integer atomic min of the row, then a compare).
 *
 * dta_novel_scores.  logits: float [rows][classes], 1 <= classes <= DTA_EVAL_MAX_SPECIES.  One launch, one wave per row,
 * on dta_softmax_top2's row body: label_out long long [rows] and softmax_out float [rows] are that entry's top_idx[:, 0] and
 * top_score[:, 0] (a row with a NaN: -1 and -1.0); top_out float [rows] is the row's largest logit (NaN for a row with a NaN).
 *
 * Refused on the host, before a launch: a null pointer other than those named optional; a size outside the ranges above;
 * accuracy, precision and support not all given or all NULL; site_masks with site_words outside its range. */
#define DTA_EVAL_MAX_SPECIES 1020
#define DTA_EVAL_MAX_SITE_WORDS 4
#define DTA_EVAL_COUNT_PLAIN 0
#define DTA_EVAL_COUNT_COMBINE 1
#define DTA_EVAL_COMBINE_ROUNDS 4
int dta_eval_count(const long long* labels, const long long* preds, const void* group, int group_is_64,
                   const unsigned char* mask, long long rows, int n_species, long long groups, int form, long long* conf,
                   long long* tally, void* stream);
int dta_eval_report(const long long* conf, int n_species, long long groups, const unsigned long long* site_masks,
                    int site_words, const int* genus, long long* counts, double* scores, double* accuracy,
                    double* precision, long long* support, void* stream);
int dta_first_rows(const void* ids, int ids_is_64, long long rows, long long n_ids, unsigned char* first_out, int* workspace,
                   void* stream);
int dta_novel_scores(const float* logits, long long rows, int classes, long long* label_out, float* top_out,
                     float* softmax_out, void* stream);

/* ---- Crown boxes of a tile from a detector's per-window output: the shift by the window origin and the greedy
 * non-maximum suppression of DeepForest's predict_tile (the reference's predict_crowns, src/predict.py:112-138, and
 * predict_trees, src/generate.py:17-60).  deeptreeattention_amd/mosaic.py: nms_np and pixel_boxes_np are the definition (they
 * state the rule in full) and the kernels equal them bit for bit.  All arrays on the device.
 *
 * boxes: float [n][4] (xmin, ymin, xmax, ymax) in window pixels; scores: float [n]; window: int [n], the row of origins:
 * int [n_windows][2] (x, y), |value| < 2^24 (both NULL: the boxes are tile coordinates already); mask: unsigned char [n] or
 * NULL.  Outputs, every element of the n rows written and nothing behind them:
 *   boxes_out        float [n][4]  box + (ox, oy, ox, oy), float32 adds; unshifted for a window index out of range
 *   status_out       unsigned char [n]  DTA_MOSAIC_REFUSED: a coordinate of boxes_out or the score is not finite, xmax < xmin
 *                    or ymax < ymin, a side above max_side, a window index out of range; DTA_MOSAIC_MASKED: mask[i] == 0;
 *                    else DTA_MOSAIC_KEPT / DTA_MOSAIC_DROPPED by the greedy rule: j precedes i when score[j] > score[i], or
 *                    the scores are equal and j < i; j suppresses a later i when inter / ((area_i + area_j) - inter) >
 *                    iou_threshold in float32, each operation rounded on its own, the division correctly rounded
 *   winner_out       int [n]  a dropped box: the first kept box in the order that suppresses it; a kept box: itself; else -1
 *   pixel_boxes_out  int [n][4]  (row0, col0, row1, col1) = floor(ymin), floor(xmin), ceil(ymax), ceil(xmax) of boxes_out,
 *                    each clamped to 0 .. height / width; zeros for a row with a coordinate that is not finite or xmax < xmin
 *                    or ymax < ymin
 * The boxes that take part are binned by centre into square cells (counting sort: integer atomics for the counts and the
 * fill cursor only; the order inside a cell varies between runs and nothing depends on it).  The cell side is max_side plus
 * one pixel (or plus max_side / 1024 if that is more), doubled until there are no more cells than max(n, 64) and 2^20: two
 * boxes that overlap have centres less than max_side apart, and the float32 centre and its float32 quotient by the side are
 * together off by less than a quarter pixel for a tile of at most 2^20 pixels a side, so they lie in adjacent cells.
 * dta_mosaic_grid reports the plan.  Then `rounds` launches (negative: DTA_MOSAIC_ROUNDS) in which every undecided box looks
 * at the 3 x 3 cells around its own: dropped as soon as a preceding overlapping box is kept, kept as soon as all of them are
 * dropped (the first two by cells, DTA_MOSAIC_CHUNK boxes staged through LDS at a time; the later ones over the list of the
 * boxes the round before left undecided, one wave per box); one launch of a single workgroup that finishes what is
 * still undecided (at most one pass per undecided box, workgroup barriers only; no_tail != 0 leaves it out and such boxes
 * keep DTA_MOSAIC_UNDECIDED: for measurements); one launch for the winners.  rounds + 5 launches and one memset on the
 * stream, no allocation, no host synchronisation; reruns are bit-identical.
 * workspace: dta_mosaic_workspace_bytes(n, height, width, max_side) bytes, 16-byte aligned (0: an argument out of range).
 * Refused on the host, before a launch: a null pointer other than window / origins / mask; window without origins or the
 * reverse; n outside 1 .. 2^30; height or width outside 1 .. 2^20; max_side outside (0, 2^20]; iou_threshold outside
 * [0, 1]; rounds above DTA_MOSAIC_MAX_ROUNDS; boxes, boxes_out or pixel_boxes_out not 16-byte aligned; a workspace that is
 * too small or misaligned. */
#define DTA_MOSAIC_DROPPED 0
#define DTA_MOSAIC_KEPT 1
#define DTA_MOSAIC_MASKED 2
#define DTA_MOSAIC_REFUSED 3
#define DTA_MOSAIC_UNDECIDED 4
#define DTA_MOSAIC_CHUNK 1024               /* boxes staged through LDS at a time */
#define DTA_MOSAIC_ROUNDS 12                /* parallel rounds in front of the tail launch (profiles/README.md) */
#define DTA_MOSAIC_MAX_ROUNDS 64
typedef struct {
  int height, width;            /* the tile, pixels */
  int n_windows;                /* rows of origins (ignored without a window table) */
  float max_side;               /* no box is wider or taller: the detector's window */
  float iou_threshold;
  int rounds;                   /* parallel rounds; negative: DTA_MOSAIC_ROUNDS */
  int no_tail;                  /* 0; 1 leaves the tail launch out (measurements) */
} dta_mosaic_options;
size_t dta_mosaic_workspace_bytes(long long n, int height, int width, float max_side);
int dta_mosaic_grid(long long n, int height, int width, float max_side, float* cell, int* gx, int* gy);
int dta_mosaic(const float* boxes, const float* scores, const int* window, const int* origins, const unsigned char* mask,
               long long n, const dta_mosaic_options* opt, unsigned char* status_out, int* winner_out, float* boxes_out,
               int* pixel_boxes_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
