/* fav.h — C ABI of the MI355X-native failure-aware classification path.
 *
 * Drop-in boundary.  The reference has NO plugin / FFI API for
 * this path: its seam is a plain Python method call whose result goes straight
 * into the trust engine,
 *
 *     last_analysis = analyzer.analyze_frame(frame)         platform/backend/main.py:160
 *     anomaly_score = anomaly.compute_anomaly(...)          platform/backend/main.py:141-143,347
 *     state = engine.update(vision_status, anomaly_score, dt)   main.py:145,168,348
 *
 * so the entry points below are what a binding for that seam needs: create a
 * per-connection scorer (main.py:110-118 constructs one per WebSocket), load a
 * checkpoint, classify a batch of frames into (label, confidence), derive the
 * failure flag / anomaly score the engine consumes, destroy on disconnect
 * (main.py:310-317).  Conventions follow the reference's own: status codes and
 * sentinels instead of exceptions (video_source.py:76-78,117; main.py:233-236),
 * single caller per handle (one scorer per connection, main.py:117), caller
 * owns every buffer it passes (video_source.py:114-117 hands out copies).
 *
 * Plain C types only; nothing of torch or HIP appears in a signature (a HIP
 * stream travels as void*).  All *_dev pointers are device (HBM) addresses on
 * the handle's device.
 */
#ifndef FAV_H
#define FAV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FAV_ABI_VERSION 2

typedef struct fav_handle fav_handle;

typedef enum fav_status {
    FAV_OK = 0,
    FAV_ERR_INVALID_ARG = 1,
    FAV_ERR_BAD_BLOB = 2,
    FAV_ERR_NO_WEIGHTS = 3,
    FAV_ERR_HIP = 4,        /* a HIP runtime call failed; see fav_last_error() */
    FAV_ERR_NO_DEVICE = 5,  /* no usable gfx950 device: the path has no CPU fallback */
    FAV_ERR_UNSUPPORTED = 6
} fav_status;

/* Frame layout handed to fav_classify.  NHWC_U8 is the reference's frame
 * format (np.uint8 HxWx3, signal_analyzer.py:47-58; video_source.py:144-148);
 * NHWC_F32 carries [0,1] pixels (corrupted frames that are not 8-bit). */
typedef enum fav_layout { FAV_LAYOUT_NHWC_U8 = 0, FAV_LAYOUT_NHWC_F32 = 1 } fav_layout;
/* FAV_ARCH_VIT_B16: ViT-B/16 (BASELINE configs[4]: attention path + temperature-scaled entropy; single pass,
 * no dropout sites, no ensemble; input a multiple of 16 with at most 256 tokens).  FAV_ARCH_VIT_TINY: a
 * two-layer, 128-wide miniature of it for the parity tests. */
typedef enum fav_arch { FAV_ARCH_RESNET18_CIFAR = 0, FAV_ARCH_RESNET50 = 1, FAV_ARCH_VIT_B16 = 2, FAV_ARCH_VIT_TINY = 3 } fav_arch;
/* FAV_CONF_MUTUAL_INFO: conf = 1 - MI / ln(min(C, T)), the epistemic part of the samples' spread (fav_uncertainty below);
 * fav_create accepts it only when the head averages T >= 2 samples (MC-Dropout with an active site and round(256 p) > 0,
 * or n_members > 1) over num_classes >= 2; a single-sample handle gets there with fav_set_views, then fav_set_conf_kind. */
typedef enum fav_conf_kind { FAV_CONF_MAX_SOFTMAX = 0, FAV_CONF_ENTROPY = 1, FAV_CONF_MUTUAL_INFO = 2 } fav_conf_kind;
/* FAV_MATH_BF16: bf16 MFMA, fp32 accumulate (production).
 * FAV_MATH_F32_EXACT: same bf16 operands fed to the fp32-input MFMA, whose
 * result is a k-ordered fmaf chain; bit-reproducible against oracle/ (validation). */
typedef enum fav_math_mode { FAV_MATH_BF16 = 0, FAV_MATH_F32_EXACT = 1 } fav_math_mode;

typedef struct fav_config {
    uint32_t struct_size;   /* sizeof(fav_config), for ABI growth */
    int32_t device;         /* HIP device ordinal */
    int32_t arch;           /* fav_arch */
    int32_t num_classes;
    int32_t in_h, in_w;     /* frame size */
    int32_t max_batch;      /* largest n passed to fav_classify */
    float mean[3];          /* per-channel normalisation on [0,1] pixels */
    float stdev[3];
    int32_t n_samples;      /* MC-Dropout T; 1 = single deterministic pass */
    uint32_t site_mask;     /* bit s<n_blocks: output of residual block s; bit n_blocks: pooled features */
    float dropout_p;
    uint64_t seed;          /* Philox key */
    float temperature;      /* softmax(z / temperature) */
    int32_t conf_kind;      /* fav_conf_kind */
    float tau;              /* failure threshold: fail = conf < tau */
    int32_t math_mode;      /* fav_math_mode */
    int32_t chunk_a;        /* frames per pass through the high-resolution stages (0 = auto) */
    int32_t chunk_b;        /* frames per pass through the low-resolution stages (0 = auto) */
    int32_t regroup_block;  /* first residual block of the low-resolution group (-1 = auto) */
    int32_t n_members;      /* deep ensemble: independently trained checkpoints whose softmax is averaged
                               (1 = single model; > 1 excludes MC-Dropout) */
    /* Schedule choices (ABI 2).  0 = this build's measured default; they never change a result, only which launches compute it
     * (the library reads no environment variable). */
    int32_t tail_min_rows;  /* layers 3-4 run their one-block-per-CU fused tails when the planned launch (max_batch x T x H x W
                               rows, x members when grouped) has at least this many rows; 0 = 131 072; -1 = at any size */
    int32_t ens_grouped_max;/* deep ensemble: calls of up to this many frames run every op as ONE launch over all members;
                               0 = every call; -1 = never (one stream per member) */
    int32_t vit_streams;    /* ViT: parts of a call's batch run side by side on as many streams, 1 .. 4; 0 = 2 */
    int32_t stem_fused;     /* ImageNet stem as one launch (normalise + 7x7/2 + ReLU + max pool); 0 = yes; -1 = three launches */
} fav_config;

/* Fills *cfg with the defaults (ImageNet mean/std, T=1, no dropout, tau=0.5). */
void fav_default_config(fav_config* cfg, int32_t arch);

/* Lifecycle: create -> load_weights -> classify xN -> destroy
 * (reference lifecycle: construct on accept main.py:110-118, reset main.py:284-291,
 * drop on disconnect main.py:310-317). */
fav_status fav_create(const fav_config* cfg, fav_handle** out);
fav_status fav_load_weights(fav_handle* h, const void* blob_host, size_t size);   /* member 0 */
fav_status fav_load_member_weights(fav_handle* h, int32_t member, const void* blob_host, size_t size);
void fav_destroy(fav_handle* h);
/* Structural validation of a checkpoint blob (magic, version, layer table, every data range and its
 * alignment), without a device or a handle; fav_load_*_weights runs it first.  err (may be NULL)
 * receives a message.  The blob is file-supplied, hence untrusted. */
fav_status fav_check_blob(const void* blob_host, size_t size, char* err, size_t err_cap);
/* The static launch schedule of a configuration (ResNet archs) as text, one line per op; needs no device.
 *   "op <i> kind=<k> phase=<p> layer=<l> lc=<l> la=<l> in=<b> res=<b> out=<b> out2=<b> site=<s> relu=<r> suffix=<0|1>
 *    rese=<0|1> skipy=<0|1> esite=<s>"
 * buffers <b>: 0..4 rotating, 5 im2col matrix, -1 frames, -2 phase input, -3 phase output, -4 none.  suffix: the op's phase
 * runs once per MC-Dropout sample; rese: a fused tail takes its residual from the cached phase input and drops it itself;
 * skipy: the entry op does not store the dropped copies; esite: the first dropout site (the entry op's), -1 without MC-Dropout.
 * flags bit 0: the layer-by-layer schedule (no fused bottleneck tails).  A test / inspection hook. */
fav_status fav_plan_schedule(const fav_config* cfg, int32_t flags, char* out, size_t cap);
const char* fav_last_error(const fav_handle* h); /* h may be NULL: error of the last failed fav_create */
int32_t fav_abi_version(void);

/* Non-finite frames - the one rule of every fav_classify* and fav_op_head* entry point.  With z_t = fp32(logit_t *
 * fp32(1 / temperature)) the T scaled rows of a frame, the frame is NON-FINITE when any of its rows holds a NaN or
 * +inf among its num_classes values, or is -inf throughout (finite logits can get there: a huge logit times
 * 1 / temperature > 1 overflows).  -inf in some classes of a row is finite input: that class has probability 0 in that
 * sample.  For a non-finite frame every head writes
 *   label = 0, confidence = 0.0f, fail = 1 whatever tau is (tau = -inf included), score = 1.0f
 * and the remaining fields as stated beside fav_uncertainty, fav_pred_set and fav_calib_cell.  The other frames of the
 * call are not affected, and the call itself still returns FAV_OK. */

/* The hot path: n frames -> labels[n] (int32), conf[n] (fp32), both device
 * pointers.  Asynchronous on `hip_stream` (NULL = the default stream); results
 * are complete once the stream is synchronised.  Replaces the scorer call at
 * main.py:160 / main.py:141. */
fav_status fav_classify(fav_handle* h, const void* images_dev, int32_t n, int32_t layout,
                        int32_t* labels_dev, float* conf_dev, void* hip_stream);

/* Same, plus: first_image_index (global index of frame 0 of this call — dropout
 * masks are keyed by global frame index so a sharded batch reproduces the
 * unsharded result), fail_dev[n] (uint8: conf < tau) and
 * score_dev[n] (fp32 anomaly_score = clamp(1 - conf, 0, 1), the value fed to
 * TrustEngine.update, trust_engine.py:139).  fail_dev / score_dev may be NULL. */
fav_status fav_classify_ex(fav_handle* h, const void* images_dev, int32_t n, int32_t layout,
                           int64_t first_image_index, int32_t* labels_dev, float* conf_dev,
                           uint8_t* fail_dev, float* score_dev, void* hip_stream);

/* Same as fav_classify_ex with the two result arrays packed: records_dev[n] holds one 8-byte record per frame,
 * { int32 label, fp32 confidence } (8-byte aligned device pointer).  This is the unit the multi-GPU path exchanges
 * (one all-gather of 8 B per frame): the confidence head writes each rank's records straight
 * into its slot of the all-gather send buffer, no pack / concatenate launches in between.  The reference is a
 * single process and has no counterpart ("Distributed communication backend: None"). */
fav_status fav_classify_records(fav_handle* h, const void* images_dev, int32_t n, int32_t layout,
                                int64_t first_image_index, void* records_dev, uint8_t* fail_dev,
                                float* score_dev, void* hip_stream);

/* Uncertainty decomposition of one frame (72 bytes).  With z_t = fp32(logit_t * fp32(1/temperature)), p_t = softmax(z_t)
 * and pbar = mean_t p_t, computed exactly as for fav_classify_ex (the T samples are the MC-Dropout samples, or the members
 * of a deep ensemble; T = 1 for a single pass):
 *   label            argmax pbar, lowest index on ties (bit-identical to fav_classify_ex's label)
 *   confidence       the handle's conf_kind (kinds 0 / 1 bit-identical to fav_classify_ex's conf)
 *   mean_prob        pbar[label] (equals confidence bit for bit under FAV_CONF_MAX_SOFTMAX)
 *   prob_std         population std over the samples of p_t[label]
 *   pred_entropy     H(pbar) in nats (what FAV_CONF_ENTROPY is derived from)
 *   expected_entropy (1/T) sum_t H(p_t) in nats
 *   mutual_info      max(pred_entropy - expected_entropy, 0)
 *   agreement        #{t : argmax z_t == label} / T (per-sample argmax on z_t, lowest index on ties)
 *   top_label/prob   classes by pbar, descending, lowest index first on ties; slots past num_classes: -1 / 0
 * T = 1: expected_entropy = pred_entropy, mutual_info = 0, agreement = 1, prob_std = 0.
 * A non-finite frame (see above fav_classify): label 0, confidence 0; mean_prob, prob_std, the three entropies and
 * agreement are NaN; top_label / top_prob are -1 / 0 in all five slots. */
typedef struct fav_uncertainty {
    int32_t label; float confidence; float mean_prob; float prob_std;
    float pred_entropy; float expected_entropy; float mutual_info; float agreement;
    int32_t top_label[5]; float top_prob[5];
} fav_uncertainty;   /* 72 bytes */

/* Same schedule as fav_classify_ex; the head writes one fav_uncertainty per frame to records_dev[n] (non-NULL, 8-byte
 * aligned device pointer, e.g. a rank's slot of an all-gather buffer).  fail_dev / score_dev may be NULL. */
fav_status fav_classify_uncertainty(fav_handle* h, const void* images_dev, int32_t n, int32_t layout,
                                    int64_t first_image_index, fav_uncertainty* records_dev,
                                    uint8_t* fail_dev, float* score_dev, void* hip_stream);

/* Split-conformal prediction sets.  From pbar exactly as fav_classify_ex computes it,
 * the classes are ranked by pbar descending, lowest index first on ties (rank 0 = the label); A(c) is the mass ahead
 * of class c, one fp32 running sum of pbar in rank order (A = 0 at rank 0).  Score of class c:
 *   FAV_CP_LAC  s(c) = 1.0f - pbar[c]
 *   FAV_CP_APS  s(c) = fmaf(u, pbar[c], A(c)) + lambda * (float)max(0, rank(c) + 1 - k_reg)
 *               (lambda = 0: APS; lambda > 0: RAPS).  u = 1, or with randomized != 0 one draw per frame:
 *               Philox4x32-10, key = seed, counter = (0, global frame index, 0, 0xC0F0), u = (x0 >> 8) * 2^-24.
 * Class c is in the set iff s(c) <= qhat (qhat = +inf: every class; an empty set is legal).  The calibration score of
 * a frame with true class y is s(y), the value the membership test compares; qhat comes from calibration
 * (the ceil((n+1)(1-alpha))-th smallest score of n held-out frames).  The set then holds the true class with
 * probability >= 1 - alpha on exchangeable frames.
 * fav_conformal is rejected (FAV_ERR_INVALID_ARG) when struct_size != sizeof(fav_conformal), qhat is NaN, lambda is
 * negative or not finite, k_reg < 0, or LAC is combined with randomized != 0 or lambda != 0. */
typedef enum fav_cp_score { FAV_CP_LAC = 0, FAV_CP_APS = 1 } fav_cp_score;
typedef struct fav_conformal {
    uint32_t struct_size; int32_t score_kind; int32_t randomized; int32_t k_reg;
    float lambda; float qhat; uint64_t seed;
} fav_conformal;   /* 32 bytes */

/* One frame's prediction set (160 bytes).
 *   label / confidence  bit-identical to fav_classify_ex's (the handle's conf_kind)
 *   set_size            number of classes in the set
 *   set_mass            fp32 sum of pbar over the set (each thread's 4 ranks in order, wave butterfly, waves in order)
 *   u                   the draw used: 1 when not randomized, 0 under FAV_CP_LAC
 *   member              bit c % 32 of word c / 32 set: class c is in the set (bits of classes >= num_classes are 0)
 * A non-finite frame (see above fav_classify): label 0, confidence 0, set_size 0, set_mass 0, no member bit, u as usual;
 * its calibration score (fav_conformal_scores) is NaN. */
typedef struct fav_pred_set {
    int32_t label; float confidence; int32_t set_size; float set_mass;
    float u; int32_t reserved[3];
    uint32_t member[32];
} fav_pred_set;   /* 160 bytes */

/* Same schedule as fav_classify_ex; the head writes one fav_pred_set per frame to records_dev[n] (non-NULL, 8-byte
 * aligned device pointer, e.g. a rank's slot of an all-gather buffer).  fail_dev / score_dev (conf < tau, as
 * fav_classify_ex) may be NULL. */
fav_status fav_classify_sets(fav_handle* h, const void* images_dev, int32_t n, int32_t layout,
                             int64_t first_image_index, const fav_conformal* cp, fav_pred_set* records_dev,
                             uint8_t* fail_dev, float* score_dev, void* hip_stream);
/* Calibration: scores_dev[i] = s(labels_dev[i]) for frame i under cp (cp->qhat is not used and may be +inf);
 * NaN where the label lies outside [0, num_classes). */
fav_status fav_conformal_scores(fav_handle* h, const void* images_dev, int32_t n, int32_t layout,
                                int64_t first_image_index, const fav_conformal* cp, const int32_t* labels_dev,
                                float* scores_dev, void* hip_stream);

/* Temperature sweep: the confidence head at K trial temperatures in one launch, on
 * held-out frames whose true classes are known.  Cell (frame i, temperature k), with pbar computed exactly as
 * fav_classify_ex computes it at temperature temps[k] (inv_temp = 1.0f / temps[k]) and y = true_labels[i]:
 *   label, confidence   bit-identical to fav_classify_ex's at that temperature (the handle's conf_kind)
 *   nll                 -logf(fmaxf(pbar[y], FLT_MIN)): at most 87.34, never +inf
 *   brier               sum over c < num_classes of (pbar[c] - [c == y])^2, fp32, in a fixed order
 * y outside [0, num_classes): nll and brier are NaN, label and confidence are still written.  A non-finite frame (see
 * above fav_classify): label 0, confidence 0, nll and brier NaN at the temperatures where it is non-finite.  The mean of nll over the
 * frames is what a temperature is fitted on; label / confidence feed the reliability and risk-coverage metrics. */
#define FAV_SWEEP_MAX_TEMPS 32
typedef struct fav_calib_cell { int32_t label; float confidence; float nll; float brier; } fav_calib_cell;   /* 16 bytes */

/* The forward pass of fav_classify_ex, then the sweep head instead of the plain one: cells_dev[n][K] (non-NULL, 8-byte
 * aligned device pointer), true_labels_dev[n] (device), temps_host: K host floats, 1 <= K <= FAV_SWEEP_MAX_TEMPS, all
 * finite and > 0 (read before the call returns).  The handle's own temperature and tau are not used.  fav_get_logits
 * afterwards returns this call's logits. */
fav_status fav_classify_sweep(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                              const int32_t* true_labels_dev, const float* temps_host, int32_t K,
                              fav_calib_cell* cells_dev, void* hip_stream);
/* The handle's temperature (finite, > 0) and failure threshold tau (not NaN): they take effect for calls enqueued after
 * the setter returns; calls already enqueued keep the old value.  A rejected value leaves the handle as it was. */
fav_status fav_set_temperature(fav_handle* h, float temperature);
fav_status fav_set_tau(fav_handle* h, float tau);
/* The third live setter: the handle's fav_conf_kind, for calls enqueued after it returns.  Kinds 0 and 1 are always accepted;
 * FAV_CONF_MUTUAL_INFO needs num_classes >= 2 and a current sample count (the head's T times max(1, n_views), see
 * fav_set_views below) of at least 2.  fav_create's own rule is unchanged.  A rejected value leaves the handle as it was. */
fav_status fav_set_conf_kind(fav_handle* h, int32_t conf_kind);

/* ---- Test-time augmentation: the third source of samples beside MC-Dropout and a deep ensemble.
 * A view is pure data movement on [H][W][3] frames of either layout; every element is copied bit for bit (an fp32 NaN
 * included: sanitising stays the stem's job).  For output pixel (y, x):
 *   1. (u, v) = (y - dy, x - dx)
 *   2. the border rule, u against H and v against W.  FAV_BORDER_REFLECT101: period 2(n-1), at any distance, a dimension of
 *      1 maps to index 0 (the defocus kernel's rule); FAV_BORDER_REPLICATE: the index is clamped; FAV_BORDER_ZERO: a pixel
 *      whose u or v falls outside the frame is 0 (0.0f) in all three channels
 *   3. flip_y: u = H-1-u; flip_x: v = W-1-v
 *   4. transpose: u and v are swapped (needs H == W)
 *   5. out[y][x][c] = in[u][v][c]
 * Ranges: the three flags 0 or 1; |dy|, |dx| <= 65535; border a fav_border value; 1 <= n_views <= FAV_MAX_VIEWS. */
typedef enum fav_border { FAV_BORDER_REFLECT101 = 0, FAV_BORDER_REPLICATE = 1, FAV_BORDER_ZERO = 2 } fav_border;
typedef struct fav_view { int32_t flip_x, flip_y, transpose, dy, dx, border; } fav_view;   /* 24 bytes */
#define FAV_MAX_VIEWS 64
/* Host only, no device: the ranges above for views of H x W frames (a transpose with H != W included), the one place these
 * rules live; fav_op_views and fav_set_views call it first.  FAV_ERR_INVALID_ARG and a message in err (may be NULL) otherwise. */
fav_status fav_check_views(const fav_view* views, int32_t n_views, int32_t H, int32_t W, char* err, size_t err_cap);
/* The handle's views (copied; n_views = 0, the default: off).  Like temperature and tau they are read on the host when a call
 * is enqueued: they take effect for calls enqueued after the setter returns, and calls already enqueued keep theirs.  While
 * views are set, EVERY fav_classify* entry point (fav_classify_host, fav_conformal_scores and fav_classify_sweep included)
 *   - accepts 1 <= n with n * n_views <= max_batch (FAV_ERR_INVALID_ARG with the three numbers otherwise),
 *   - expands the n frames into n * n_views view frames, ordered [view][frame], in a buffer the handle owns (max_batch frames
 *     of the call's layout, allocated on the first such call), on the call's stream, behind the previous use of the handle.
 *     A handle that has served uint8 frames and then gets fp32 frames frees that buffer and allocates the larger one: this
 *     one call waits for the whole device (hipFree) before it enqueues anything; later calls in either layout do not,
 *   - runs the unchanged forward pass on them and the requested head on n frames with T = T_head * n_views samples: sample
 *     s = m * n_views + a is member (or pass) m under view a.  first_image_index, the conformal draw's key, stays the caller's.
 * fav_get_logits then reports T = T_head * n_views and n.  With no views set nothing changes.
 * Refused: a handle that draws dropout masks (an MC-Dropout site active with round(256 p) > 0), FAV_ERR_UNSUPPORTED - the masks
 * are keyed by batch row, and a shard-invariant key for view rows would change the mask kernels; single-pass ResNets,
 * ensembles and both ViT archs are supported.  Also refused (FAV_ERR_INVALID_ARG): what fav_check_views refuses for
 * in_h x in_w frames; in_h * in_w above (2^31 - 1) / 12; n_views > max_batch; members x n_views > 4096 (the heads' limit); and turning the views off, or down
 * to one, while the confidence kind is FAV_CONF_MUTUAL_INFO and fewer than 2 samples would be left (change the kind first). */
fav_status fav_set_views(fav_handle* h, const fav_view* views, int32_t n_views);
/* The views in force: *n_out (may be NULL) = their number, the first min(cap, number) of them copied to out (may be NULL). */
fav_status fav_get_views(const fav_handle* h, fav_view* out, int32_t cap, int32_t* n_out);

/* ---- Feature tap and feature-space OOD scoring.  Every other signal of this library is a
 * function of the logits; these two read the row the final fc GEMM reads - the FEATURE of a sample:
 *   ResNet archs   the input row of the last convolution of the schedule (the fc): the average-pool output, or the entry
 *                  dropout's output when the pooled-feature site is the first dropout site.  It is therefore POST-dropout
 *                  whenever the pooled-feature site is active.  D = 512 (ResNet-18), 2048 (ResNet-50)
 *   ViT archs      the class token behind the final LayerNorm.  D = 768 (ViT-B/16), 128 (the miniature)
 * While the tap is on, every pass copies those bf16 rows device to device into a buffer the handle owns, on the stream the
 * fc launch runs on and in front of it: per chunk at the chunk's virtual-frame offset, per ensemble member (grouped or one
 * stream a member), per stream part on the ViT path.  The buffer holds [S][n][D] rows with the sample indexing of
 * fav_get_logits (views included: S = T_head * n_views).  It is allocated by the setter, for max_batch frames; the setter may
 * synchronise, fav_classify* never allocates or synchronises for it.  The copies are booked in no kernel class.  The tap
 * changes no result.  With the tap off and no OOD model set a fav_classify* call enqueues exactly what it did before.  Turning
 * the tap off while an OOD model is set is refused (FAV_ERR_INVALID_ARG): the model reads it. */
fav_status fav_set_feature_tap(fav_handle* h, int32_t enable);
/* The features of the last fav_classify* call, converted to fp32 [S][n][D] in out_dev (16-byte aligned; may be NULL: only
 * the sizes), on hip_stream.  FAV_ERR_INVALID_ARG before the first call made with the tap on, and with the tap off. */
fav_status fav_get_features(fav_handle* h, float* out_dev, int32_t* s_out, int32_t* n_out, int32_t* d_out, void* hip_stream);

/* A class-conditional Gaussian with a tied covariance on those features (Mahalanobis distance; Lee et al. 2018), stored as a
 * whitening projection: with Sigma = U diag(lambda) U^T, P = diag(lambda^-1/2) U_k^T and M[c] = P (mu_c - mu), the distance
 * of a feature f to class c is |P (f - mu) - M[c]|^2.  All pointers are HOST pointers.
 * Ranges (fav_check_ood_model; FAV_ERR_INVALID_ARG and a message that names the field): struct_size == sizeof(fav_ood_model);
 * D a multiple of 16 in [16, 4096] (and the arch's feature width when set on a handle); 1 <= k <= 2048; 1 <= R <= 4096; every
 * value of mu, P and M finite; threshold not NaN (+inf: no frame is ever flagged); class_id >= -1. */
typedef struct fav_ood_model {
    uint32_t struct_size; int32_t D, k, R;
    const float* mu;        /* [D]    global feature mean            (host) */
    const float* P;         /* [k][D] whitening projection           (host) */
    const float* M;         /* [R][k] projected class means          (host) */
    const int32_t* class_id;/* [R]    class of each row, -1 = class-agnostic */
    float threshold;        /* ood = !(min_dist <= threshold); +inf = never */
} fav_ood_model;
/* One frame's score, 16 bytes.  Per frame i, everything fp32, every product and every sum rounded on its own (no FMA
 * contraction, no re-association):
 *   1. fbar[j]    +0, plus fp32(feat[s][i][j]) for s = 0 .. S-1 in that order, times (float)(1.0 / S)
 *   2. x[j]       fbar[j] - mu[j]
 *   3. g[r]       r < k: +0, then for j = 0 .. D-1 in that order g = g + P[r][j] * x[j]
 *   4. d[c]       c < R: +0, then for r = 0 .. k-1 in that order t = g[r] - M[c][r], d = d + t * t
 *   5. best = +inf, row = -1; for c ascending: if (d[c] < best) { best = d[c]; row = c; } - ties go to the lowest row, a NaN
 *      never wins.  min_dist = best; min_class = row < 0 ? -1 : class_id[row]
 *   6. label_dist d[c] of the lowest row whose class_id equals labels[i]; NaN when labels is NULL or no row has that class
 *   7. ood        !(min_dist <= threshold)
 * Non-finite features have no rule of their own: the chains carry them along and the strict < settles the outcome. */
typedef struct fav_ood_record { float min_dist; int32_t min_class; float label_dist; int32_t ood; } fav_ood_record;
/* Host only, no device: the ranges above (D_expected < 0: any width in range), the one place they live; fav_set_ood calls it
 * first.  err (may be NULL) receives the message. */
fav_status fav_check_ood_model(const fav_ood_model* m, int32_t D_expected, char* err, size_t err_cap);
/* The handle's OOD model (copied to the device, P and M transposed on the host; NULL: none).  Setting one turns the feature
 * tap on; clearing it turns the tap off again if this is what turned it on.  Replacing or clearing a model waits on the
 * host for the work enqueued on the handle and frees the old copy (hipFree: the whole device).  FAV_ERR_UNSUPPORTED on a
 * deep-ensemble handle: the members do not share a feature space (the tap itself works there).  A rejected call leaves the
 * handle as it was. */
fav_status fav_set_ood(fav_handle* h, const fav_ood_model* m);
/* fav_classify_ex unchanged, then the scoring head on the tapped features, all on the caller's stream: ood_dev[n] (non-NULL,
 * 8-byte aligned) gets one fav_ood_record per frame, label_dist being the distance to the class this very call wrote to
 * labels_dev.  Needs a model (FAV_ERR_INVALID_ARG otherwise).  fail_dev / score_dev may be NULL. */
fav_status fav_classify_ood(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                            int32_t* labels_dev, float* conf_dev, uint8_t* fail_dev, float* score_dev,
                            fav_ood_record* ood_dev, void* hip_stream);

/* ---- Nearest-neighbour OOD scoring (deep nearest neighbours, Sun et al. 2022): the
 * non-parametric companion of the Mahalanobis model above.  A BANK holds N L2-normalised in-distribution features as bf16
 * rows; a frame's score is the squared Euclidean distance of its normalised feature to its k-th nearest bank row.  No labels,
 * no covariance, no assumption about the shape of a class.  All pointers are HOST pointers.
 * Ranges (fav_check_knn_bank; FAV_ERR_INVALID_ARG and a message that names the field): struct_size == sizeof(fav_knn_bank);
 * D a multiple of 64 in [64, 4096] (and the arch's feature width when set on a handle); 1 <= N <= 262144; 1 <= k <=
 * min(N, 256); no row value NaN or inf; class_id NULL or every entry >= -1; threshold not NaN (+inf: no frame is ever
 * flagged).  The rows are meant to be unit vectors; this is not checked. */
typedef struct fav_knn_bank {
    uint32_t struct_size; int32_t D, N, k;
    const uint16_t* rows;    /* [N][D] bf16 bit patterns                        (host) */
    const int32_t* class_id; /* [N] class of each row, -1 = none; or NULL       (host) */
    float threshold;         /* ood = !(kth_dist <= threshold); +inf = never */
} fav_knn_bank;
/* One frame's score, 24 bytes, 8-byte aligned.  Per frame i, with the features feat[S][n][D] bf16 indexed as in
 * fav_get_features, everything fp32, every product and every sum rounded on its own (no FMA contraction):
 *   1. fbar[j]    step 1 of fav_ood_record: +0, plus fp32(feat[s][i][j]) for s = 0 .. S-1 in that order, times (float)(1.0 / S)
 *   2. ss         sixteen partial sums: p[l] = +0, then for j = l, l+16, l+32, .. in that order p[l] = p[l] + fbar[j] * fbar[j];
 *                 ss = (((p[0] + p[1]) + p[2]) + .. + p[15])
 *   3. q[j]       inv = 1.0f / sqrtf(ss), both correctly rounded; q[j] = bf16_rne(fbar[j] * inv)
 *   4. sim[b]     b < N: acc[b] + (+0.0f), where acc[b] is the production GEMM accumulator of
 *                 q . bank[b]: v_mfma_f32_16x16x32_bf16 chained from +0 over ascending k, k in the operand layout of the
 *                 convolution kernels; K is never split and never re-associated.  The + 0.0f is a conv epilogue's zero bias,
 *                 and rules out -0
 *   5. kth_sim    the k-th largest value of the multiset {sim[b]} (a value: no tie rule needed); nn_sim the largest value;
 *                 nn_row the LOWEST row that holds it; nn_class = class_id[nn_row], -1 when the bank has no class ids
 *   6. kth_dist   fmaxf(2.0f - 2.0f * kth_sim, +0.0f): the squared distance of two unit vectors; ood = !(kth_dist <= threshold)
 *   7. a DEGENERATE frame, !(ss > 0 && ss < inf) - a zero feature row, a NaN or inf feature, an overflowed square - gets
 *      kth_sim = nn_sim = kth_dist = NaN (0x7FC00000), nn_row = nn_class = -1, ood = 1, and touches no other frame of the
 *      call.  For every other frame |q[j]| <= 1 and the bank is finite, so every sim is finite. */
typedef struct fav_knn_record { float kth_dist, kth_sim, nn_sim; int32_t nn_row, nn_class, ood; } fav_knn_record;
/* Host only, no device: the ranges above (D_expected < 0: any width in range), the one place they live; fav_set_knn calls it
 * first.  err (may be NULL) receives the message. */
fav_status fav_check_knn_bank(const fav_knn_bank* bank, int32_t D_expected, char* err, size_t err_cap);
/* The handle's bank (NULL: none), as fav_set_ood in every respect: copied to the device (padded with zero rows to a multiple
 * of 64, which the GEMM's tiles want), the feature tap goes on; clearing it turns the tap off again only if a head turned it
 * on and no OOD model still reads it.  A model and a bank may be set together: the tap stays on while either is set or while
 * the caller turned it on, and fav_set_feature_tap(h, 0) is refused while either reads it.  The setter allocates the whole
 * workspace, for max_batch frames - fav_classify_knn never allocates or synchronises - and refuses a bank whose workspace
 * would exceed 1 GiB (the message carries the numbers).  Replacing or clearing a bank waits on the host for the work
 * enqueued on the handle and frees the old copy.  FAV_ERR_UNSUPPORTED on a deep-ensemble handle.  A rejected call leaves
 * the handle as it was. */
fav_status fav_set_knn(fav_handle* h, const fav_knn_bank* bank);
/* fav_classify_ex unchanged, then the k-NN head on the tapped features, all on the caller's stream: knn_dev[n] (non-NULL,
 * 8-byte aligned) gets one fav_knn_record per frame.  Needs a bank (FAV_ERR_INVALID_ARG otherwise).  fail_dev / score_dev may
 * be NULL.  The head's three launches are booked in no kernel class, like fav_classify_ood's. */
fav_status fav_classify_knn(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                            int32_t* labels_dev, float* conf_dev, uint8_t* fail_dev, float* score_dev,
                            fav_knn_record* knn_dev, void* hip_stream);

/* ---- Window-level drift detection (Rabanser et al. 2019, "Failing Loudly"): a two-sample
 * permutation test on the energy distance between a REFERENCE of R L2-normalised in-distribution features, bf16 rows, and the
 * n frames of one call - the window.  Every other output of this library describes a frame; this one describes a call.  All
 * pointers are HOST pointers.
 * Ranges (fav_check_drift_ref; FAV_ERR_INVALID_ARG and a message that names the field): struct_size == sizeof(fav_drift_ref);
 * D a multiple of 64 in [64, 4096] (and the arch's feature width when set on a handle); 2 <= R <= 2048; 1 <= n_perm <= 9999;
 * alpha in [0, 1] (a NaN is outside); no row value NaN or inf; every row's squared norm, summed in float64 over its bf16
 * values in index order, inside [0.5, 2].  A call takes 2 <= n <= 1024 frames. */
typedef struct fav_drift_ref {
    uint32_t struct_size; int32_t D, R, n_perm;
    const uint16_t* rows;    /* [R][D] bf16 bit patterns, meant to be unit vectors  (host) */
    uint64_t seed;           /* the Philox key of the permutations */
    float alpha;             /* drift = p_value <= alpha */
} fav_drift_ref;
/* One call's test, 48 bytes, 8-byte aligned.  With the features feat[S][n][D] bf16 indexed as in fav_get_features, P = n_perm:
 *   1. q[i]       the window's rows: steps 1 to 3 of fav_knn_record, unchanged.  If any frame is DEGENERATE (step 7 there) the
 *                 test is not run: statistic = NaN (0x7FF8000000000000), p_value = NaN (0x7FC00000), s_ab = s_aa = s_bb = 0,
 *                 n_exceed = -1, drift = 1, n_degenerate = their number; the permutation kernel's blocks return before they
 *                 compute anything, perm_sums is not written, and nothing a later call reads has been changed.  Otherwise
 *                 n_degenerate = 0 and:
 *   2. the pool   rows 0 .. R-1 the reference, rows R .. R+n-1 the q[i]; Np = R + n
 *   3. G[i][j]    j <= i: acc + (+0.0f), acc the production GEMM accumulator of fav_knn_record's step 4, K never split, pool
 *                 row i its activation row and pool row j its weight row.  Only j <= i is ever used: symmetry of the matrix
 *                 pipe is not assumed, it is defined away
 *   4. u[i][j]    fp32, every operation rounded on its own: d2 = fmaxf((G[i][i] + G[j][j]) - 2.0f * G[i][j], +0.0f);
 *                 dd = sqrtf(d2), correctly rounded; u[i][j] = u[j][i] = (uint32) rintf(dd * 1048576.0f) for j < i; u[i][i] = 0.
 *                 Identical rows are at distance exactly 0.  With the norm band above every u is below 2^22, and with
 *                 Np <= 3072 every sum below is below 2^45
 *   5. the sums   integers, exact, hence independent of order.  For a group B of n pool indices, A the other R:
 *                 S_BB the sum of u over the unordered pairs inside B, S_AB over the pairs across, S_AA over those inside A.
 *                 With r[i] = sum_j u[i][j] and S_tot = (sum_i r[i]) / 2: S_AB = sum_{i in B} r[i] - 2 S_BB and
 *                 S_AA = S_tot - S_BB - S_AB.  The observed group is B = {R .. Np-1}; s_ab, s_aa, s_bb are its sums
 *   6. B_p        permutation p < P: x0(i) the first word of Philox4x32-10 with counter (i, p, 0, 0x5F17) and key (seed low,
 *                 seed high); key(i) = (uint64) x0(i) << 32 | i, which are unique; B_p the n pool indices with the smallest keys
 *   7. n_exceed   T = S_AB (R n) - S_AA n^2 - S_BB R^2 as a 128-bit integer (R n (R + n) / 2 times the energy distance);
 *                 n_exceed = #{p : T_p >= T_obs}
 *   8. statistic  float64, every operation rounded on its own:
 *                 (((2.0 * S_AB) / (double)(R n) - (2.0 * S_AA) / (double)(R R)) - (2.0 * S_BB) / (double)(n n)) * 2^-20
 *                 from the observed sums: 2 E|a - b| - E|a - a'| - E|b - b'| with the V-statistic's divisors;
 *                 p_value = (float)((double)(1 + n_exceed) / (double)(P + 1)); drift = p_value <= alpha */
typedef struct fav_drift_record {
    double statistic; int64_t s_ab, s_aa, s_bb; float p_value; int32_t n_exceed, drift, n_degenerate;
} fav_drift_record;
/* Host only, no device: the ranges above (D_expected < 0: any width in range), the one place they live; fav_set_drift calls
 * it first.  err (may be NULL) receives the message. */
fav_status fav_check_drift_ref(const fav_drift_ref* ref, int32_t D_expected, char* err, size_t err_cap);
/* The handle's drift reference (NULL: none), as fav_set_knn in every respect: the feature tap goes on and is derived from the
 * three heads and the caller's own wish - a model, a bank and a reference may be set together, and fav_set_feature_tap(h, 0)
 * is refused while any of them reads the tap.  The setter allocates the whole workspace for max_batch frames (the pool
 * [pad64(R + max_batch)][D] with the reference at its front, the quantised distances of the whole pool), computes the
 * reference's own block of distances once, and synchronises; fav_classify_drift never allocates or synchronises.  A handle
 * whose max_batch lies outside [2, 1024] is refused (the message carries the numbers).  Replacing or clearing waits on the
 * host for the work enqueued on the handle and frees the old copy.  FAV_ERR_UNSUPPORTED on a deep-ensemble handle.  A
 * rejected call leaves the handle as it was. */
fav_status fav_set_drift(fav_handle* h, const fav_drift_ref* ref);
/* fav_classify_ex unchanged, then the test on the tapped features of these n frames, all on the caller's stream: drift_dev
 * (non-NULL, 8-byte aligned) gets ONE fav_drift_record: the call is the window.  Needs a reference, and n >= 2: both are
 * refused (FAV_ERR_INVALID_ARG) before anything is enqueued.  fail_dev / score_dev may be NULL.  The head's launches are
 * booked in no kernel class. */
fav_status fav_classify_drift(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                              int32_t* labels_dev, float* conf_dev, uint8_t* fail_dev, float* score_dev,
                              fav_drift_record* drift_dev, void* hip_stream);

/* ---- Class activation maps (Zhou et al. 2016).  Every signal above says WHETHER a frame can
 * be trusted; this one says WHERE in the frame the decision comes from.  On a ResNet the logit of class c is the spatial mean
 * of w_c . F(h, w) over the last feature map F, plus the bias, so M_c(h, w) = w_c . F(h, w) is an exact additive
 * decomposition of the logit over the cells of the map: no backward pass, and linear in the MC-Dropout samples, so the mean
 * map over the samples decomposes the mean logit.
 *
 * The MAP TAP.  While it is on, every pass copies the input of its average-pool launch - cn frames x Hf*Wf cells x C
 * channels, bf16 - device to device into a buffer the handle owns, on the stream of that launch and in front of it, per
 * chunk at the chunk's virtual-frame offset.  The buffer holds [S_map][n][Hf*Wf][C] with the sample indexing of
 * fav_get_logits: S_map = the MC-Dropout samples when the pool runs once a sample, 1 when it runs once a frame (the
 * pooled-feature site is the only dropout site: the map is then the same for every sample), times the views when views are
 * set.  WHICH MAPS: those the pool reads - POST-dropout for every block site, PRE-dropout for the pooled-feature site, whose
 * mask falls on the pooled feature behind the pool.
 * The setter allocates S_map * max_batch * Hf*Wf * C * 2 bytes (with A views a call takes at most max_batch / A frames) and
 * may synchronise; fav_classify* never allocates or synchronises for it.  It refuses (FAV_ERR_INVALID_ARG, the message
 * carries both numbers) a buffer above max_bytes (0: 2 GiB), and (FAV_ERR_UNSUPPORTED) a ViT arch, which has no pooled
 * convolutional map, and a deep-ensemble handle.  Turning the tap off is never refused; it waits for the work enqueued on
 * the handle and frees the buffer.  The copies are booked in no kernel class.  The tap changes no result, and it is
 * independent of the feature tap.  With the tap off a fav_classify* call enqueues exactly what it did before. */
fav_status fav_set_map_tap(fav_handle* h, int32_t enable, size_t max_bytes);
/* The maps of the last fav_classify* call made with the tap on, copied as they are - bf16 [S][n][Hf*Wf][C] - to out_dev (may
 * be NULL: only the sizes; every size pointer may be NULL), on hip_stream.  FAV_ERR_INVALID_ARG with the tap off and before
 * the first call made with it on. */
fav_status fav_get_maps(fav_handle* h, void* out_dev, int32_t* s_out, int32_t* n_out, int32_t* hf_out, int32_t* wf_out,
                        int32_t* c_out, void* hip_stream);
/* Host only, no device: what fav_set_map_tap would allocate for this configuration, from the planner - *bytes, *s_map (the
 * samples without views), *hf, *wf, *c (each may be NULL).  FAV_ERR_UNSUPPORTED for a ViT arch and for n_members > 1,
 * FAV_ERR_INVALID_ARG for a configuration the planner refuses; err (may be NULL) receives the message. */
fav_status fav_map_tap_info(const fav_config* cfg, size_t* bytes, int32_t* s_map, int32_t* hf, int32_t* wf, int32_t* c,
                            char* err, size_t err_cap);
/* The STAGE TAP: the map tap's sibling for a mid-level map.  stage is the residual stage 1 .. 4
 * (torchvision's layer1 .. layer4) on both ResNet arches; the tap holds the output of that stage's LAST block - what the next
 * stage reads, behind that block's dropout when the block's own launch draws it - as bf16 [S][n][Hf*Wf][C], indexed like the
 * map tap: every pass copies cn frames device to device BEHIND the launch that writes the block's output, at the chunk's
 * virtual-frame offset.  S = the MC-Dropout samples when that launch runs once a sample, 1 when it runs once a frame (times
 * the views).  When the block is the FIRST dropout site, its mask falls on the cached tensor in the next launch: the tap then
 * holds the output in front of it, S = 1, as the map tap does at the pooled-feature site.  Stage 4 is the buffer the average
 * pool reads: its tap is the map tap's own copy, the same bytes under every policy.
 * One stage at a time.  stage 0 turns the tap off and frees the buffer (never refused); another stage than the one in force
 * waits for the work enqueued on the handle and reallocates.  The budget is fav_set_map_tap's (0: 2 GiB).  Refused:
 * FAV_ERR_UNSUPPORTED a ViT arch and a deep-ensemble handle, as fav_set_map_tap; FAV_ERR_INVALID_ARG a stage outside [0, 4], a
 * buffer above the budget, and a stage whose map the patch head cannot take (more than 1024 cells or a side above 256: stage 1
 * of a 224 x 224 frame has 3136), the message carrying the numbers.  A refused call leaves the tap as it was.  With the tap
 * off nothing is enqueued for it; the tap changes no result and is independent of the map tap and the feature tap. */
fav_status fav_set_stage_tap(fav_handle* h, int32_t stage, size_t max_bytes);
/* fav_get_maps for the stage tap; *stage_out the stage in force.  Every size pointer and out_dev may be NULL. */
fav_status fav_get_stage_maps(fav_handle* h, void* out_dev, int32_t* stage_out, int32_t* s_out, int32_t* n_out, int32_t* hf_out,
                              int32_t* wf_out, int32_t* c_out, void* hip_stream);
/* Host only, no device: fav_map_tap_info for stage 1 .. 4 (FAV_ERR_INVALID_ARG outside).  It reports every stage's geometry,
 * also one fav_set_stage_tap would refuse for its cell count. */
fav_status fav_stage_tap_info(const fav_config* cfg, int32_t stage, size_t* bytes, int32_t* s_map, int32_t* hf, int32_t* wf,
                              int32_t* c, char* err, size_t err_cap);

/* One (frame, class) map's summary, 32 bytes, 8-byte aligned.  For frame i and class c = classes[i][k], with x the maps
 * [S][n][HW][C] and w the weight rows, everything fp32, every product and every sum rounded on its own (no FMA contraction,
 * no re-association); the partition is fixed and does not depend on the grid or the block:
 *   1. lane partials   l < 64: p[l] = +0; then for s = 0 .. S-1, for m = 0 .. C/512-1, for e = 0 .. 7, in that order, with
 *                      ch = 512 m + 8 l + e:  p[l] = p[l] + fp32(w[c][ch]) * fp32(x[s][i][hw][ch])
 *   2. six halvings    for h = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + h] for l < h.  M[hw] = p[0] * (float)(1.0 / S)
 *   3. logit_mean      +0 plus M[hw] in index order, times (float)(1.0 / HW), plus bias[c]
 *   4. peak, peak_cell best = -inf, cell = -1; for hw ascending: if (M[hw] > best) { best = M[hw]; cell = hw; } - ties go to
 *                      the lowest cell, a NaN never wins.  floor: the same from +inf with <
 *   5. pos_sum         +0 plus fmaxf(M[hw], +0) in index order.  With thr = 0.2f * peak (the 20 % rule of the CAM paper),
 *                      n_above = the number of cells with M[hw] >= thr, counted only when peak > 0 (else 0); box = the
 *                      inclusive extent of those cells, x0 | y0 << 8 | x1 << 16 | y1 << 24 with x = hw % Wf, y = hw / Wf,
 *                      -1 when n_above == 0.  It is the bounding box of ALL such cells, not of the largest connected
 *                      component
 *   6. a class id outside [0, n_classes): the slot's map is all 0x7FC00000, class_id = -1, peak_cell = -1, n_above = 0,
 *                      box = -1, the floats of the record NaN; other slots are untouched
 * Non-finite map values have no rule of their own: the chains carry them (a NaN's payload and sign are not part of the
 * contract). */
typedef struct fav_cam_record { int32_t class_id; float logit_mean, peak; int32_t peak_cell; float floor, pos_sum;
                                int32_t n_above, box; } fav_cam_record;
/* The head on the maps of the LAST fav_classify* call, with the handle's own fc weights and bias, for any classes the caller
 * names: classes_dev int32 [n][K], 1 <= K <= 8, cam_dev fp32 [n][K][Hf*Wf] (4-byte aligned), rec_dev [n][K] (8-byte aligned),
 * n the frames of that call.  One small launch on hip_stream, no second forward pass, no allocation, no synchronisation.
 * FAV_ERR_INVALID_ARG with the tap off, before the first tapped call, for a NULL or misaligned buffer and for a map outside
 * the head's ranges (fav_op_cam).  FAV_ERR_UNSUPPORTED while views are set or when the last call ran under views: a mirrored
 * or turned view's map lies in that view's frame, and averaging them mis-registers (fav_get_maps still works there). */
fav_status fav_cam(fav_handle* h, const int32_t* classes_dev, int32_t K, float* cam_dev, fav_cam_record* rec_dev,
                   void* hip_stream);
/* fav_classify_ex unchanged, then the head with K = 1 on the class this very call wrote to labels_dev (non-NULL; read on the
 * device, so nothing synchronises): cam_dev fp32 [n][Hf*Wf], rec_dev [n].  Needs the map tap on (FAV_ERR_INVALID_ARG
 * otherwise); FAV_ERR_UNSUPPORTED while views are set.  Never allocates or synchronises.  fail_dev / score_dev may be NULL.
 * The head's launch is booked in no kernel class. */
fav_status fav_classify_cam(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                            int32_t* labels_dev, float* conf_dev, uint8_t* fail_dev, float* score_dev, float* cam_dev,
                            fav_cam_record* rec_dev, void* hip_stream);

/* ---- Attention rollout (Abnar & Zuidema 2020): the ViT counterpart of the class activation map.  Average each encoder
 * layer's attention over its heads, mix in the identity for the residual connection, multiply the layers together; the class
 * token's row of the product says how much each patch fed the decision.  No backward pass.  What the tests of this library
 * verify is that algebra and its bits on synthetic checkpoints; whether the maps localise objects is a property of trained
 * weights.
 *
 * The ATTENTION TAP.  The production attention kernel keeps its probabilities in registers and never writes them.  While the
 * tap is on, every encoder layer of every part of a ViT call launches one more kernel on that part's stream, between the
 * layer's qkv GEMM and its attention launch; it reads the part's qkv rows and writes the head-mean attention of layer l into
 * a buffer the handle owns: A[L][n][T][ldT] fp32, n the frame rows of the call (frames x views when views are set, in the
 * indexing of fav_get_logits), T the tokens, ldT = 16 * ceil(T / 16) so that every row starts 16-byte aligned; columns
 * u >= T hold +0.  A part writes at its frame offset.
 * For frame i, layer l, head h < heads, query t and key u, with q_h, k_h the 64 bf16 columns of the head in qkv:
 *   1. s_h[t][u]  the production score accumulator: v_mfma_f32_16x16x32_bf16 chained from +0 over the two 32-channel steps,
 *                 K rows the A operand, the query's fragment B (oracle/fav_oracle.py: gemm_acc(q_h, k_h, "mfma"))
 *   2. p_h[t][.]  the production softmax in front of its rounding to bf16 (oracle: attn_softmax_exact): the row max of the raw
 *                 scores; e = 2^fma(s, log2(e) / 8, -(max * log2(e) / 8)) by the kernels' own exponential; the row sum from eight partial sums
 *                 (lane group (u >> 2) & 3, parity u & 1, each in ascending key order) combined as
 *                 ((s00 + s01) + (s10 + s11)) + ((s20 + s21) + (s30 + s31)); ONE 1.0f / sum, then a multiplication per
 *                 element.  Keys >= T are masked as production masks them (-inf for the max, 0 for the sum)
 *   3. A[t][u]    +0, plus p_h[t][u] for h = 0 .. heads-1 in that order, times (float)(1.0 / heads); every operation rounded
 *                 on its own
 * Non-finite qkv values have no rule of their own: the chains carry them.  Padded columns are +0 whenever the row is finite.
 * The setter allocates L * max_batch * T * ldT * 4 bytes and may synchronise; fav_classify* never allocates or synchronises
 * for the tap.  It refuses (FAV_ERR_INVALID_ARG, the message carries both numbers) a buffer above max_bytes (0: 2 GiB), and
 * (FAV_ERR_UNSUPPORTED) a ResNet arch, a deep-ensemble handle and a handle in FAV_MATH_F32_EXACT (the tap restates the
 * production score product only).  Turning the tap off is never refused; it waits for the work enqueued on the handle and
 * frees the buffer.  The tap's launches are booked in no kernel class (fav_get_profile does not see them).  The tap changes
 * no result, and it is independent of the feature tap and of the map tap.  With the tap off a fav_classify* call enqueues
 * exactly what it did before. */
fav_status fav_set_attn_tap(fav_handle* h, int32_t enable, size_t max_bytes);
/* The head-mean attention of the last fav_classify* call made with the tap on, copied as it is - fp32 [L][n][T][ld] - to
 * out_dev (may be NULL: only the sizes; every size pointer may be NULL), on hip_stream.  FAV_ERR_INVALID_ARG with the tap off
 * and before the first call made with it on.  Works under views (n = frames x views). */
fav_status fav_get_attention(fav_handle* h, float* out_dev, int32_t* l_out, int32_t* n_out, int32_t* t_out, int32_t* ld_out,
                             void* hip_stream);
/* Host only, no device: what fav_set_attn_tap would allocate for this configuration, from the planner - *bytes, *layers,
 * *tokens, *ld (each may be NULL).  FAV_ERR_UNSUPPORTED for a ResNet arch, for n_members > 1 and for FAV_MATH_F32_EXACT,
 * FAV_ERR_INVALID_ARG for a configuration the planner refuses; err (may be NULL) receives the message. */
fav_status fav_attn_tap_info(const fav_config* cfg, size_t* bytes, int32_t* layers, int32_t* tokens, int32_t* ld, char* err,
                             size_t err_cap);

/* One frame's rollout summary, 32 bytes, 8-byte aligned.  peak (byte 8) and floor (byte 16) stand where fav_cam_record has
 * them, so fav_op_cam_heatmap accepts an array of these records unchanged: that is how the overlay is made.
 * For frame i with T = gh * gw + 1 tokens and A_l = A[l][i], everything fp32, every product and every sum rounded on its own
 * (no FMA contraction, no re-association); a thread owns a column u, and the partition does not depend on the grid:
 *   1. A~_l[t][u] = 0.5f * A_l[t][u] + (t == u ? 0.5f : +0.0f).  The rows of A sum to 1 within rounding, so the rollout does
 *      not renormalise
 *   2. r[u] = A~_{L-1}[0][u]
 *   3. for l = L-2 down to first_layer: r'[u] = +0, then for t = 0 .. T-1 in that order r'[u] = r'[u] + r[t] * A~_l[t][u];
 *      r = r'.  first_layer = L-1 gives the raw last-layer class-token attention
 *   4. map M[p] = r[1 + p];  cls_mass = r[0];  patch_sum = +0 plus M[p] in index order;  n_layers = L - first_layer
 *   5. peak, peak_cell, floor as step 4 of fav_cam_record: strict scans in index order from -inf / +inf; a NaN never wins
 *   6. thr = floor + 0.5f * (peak - floor); n_above = the number of cells with M[p] >= thr, counted only when peak > floor
 *      (else 0); box as fav_cam_record over the gh x gw grid (x = p % gw, y = p / gw), -1 when n_above == 0.  (The 20 % rule
 *      of CAM would take in nearly every cell of an all-positive map, hence the midpoint.) */
typedef struct fav_rollout_record { int32_t n_layers; float cls_mass, peak; int32_t peak_cell; float floor, patch_sum;
                                    int32_t n_above, box; } fav_rollout_record;
/* The head on the attention of the LAST fav_classify* call made with the tap on: map_dev fp32 [n][gh*gw] (4-byte aligned),
 * rec_dev [n] (8-byte aligned), n the frames of that call, 0 <= first_layer < L.  One small launch on hip_stream, no second
 * forward pass, no allocation, no synchronisation.  FAV_ERR_INVALID_ARG with the tap off, before the first tapped call, for a
 * NULL or misaligned buffer and for first_layer out of range.  FAV_ERR_UNSUPPORTED while views are set or when the last call
 * ran under views: a mirrored or turned view's rollout lies in that view's frame, and averaging them mis-registers
 * (fav_get_attention still works there). */
fav_status fav_rollout(fav_handle* h, int32_t first_layer, float* map_dev, fav_rollout_record* rec_dev, void* hip_stream);
/* fav_classify_ex unchanged, then the head on this very call's attention.  Needs the attention tap on (FAV_ERR_INVALID_ARG
 * otherwise); FAV_ERR_UNSUPPORTED while views are set.  Never allocates or synchronises.  fail_dev / score_dev may be NULL.
 * The head's launch is booked in no kernel class. */
fav_status fav_classify_rollout(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                                int32_t* labels_dev, float* conf_dev, uint8_t* fail_dev, float* score_dev, int32_t first_layer,
                                float* map_dev, fav_rollout_record* rec_dev, void* hip_stream);

/* ---- Deletion / insertion curves (Petsiuk et al. 2018, RISE).  The two heads above say WHERE a
 * decision comes from; this one says whether such a map means anything for the checkpoint in use.  The cells of a map are
 * ranked, most salient first; the frames are classified again with the k_s most salient cells filled (deletion) or with only
 * those cells shown on a filled frame (insertion), for s = 0 .. S, and the probability of one class is integrated over the
 * steps.  A faithful map makes deletion fall fast (low AUC) and insertion rise fast (high AUC), both against a random ranking.
 * No labels, no boxes, no backward pass; any arch, any source of samples, any map - CAM, rollout or the caller's own.  What the
 * tests of this library verify is the algebra and its bits on synthetic checkpoints, where the SIGN of a gain carries no
 * meaning; whether a map is faithful is a property of trained weights.
 *
 * One frame's curve summary, 32 bytes, 8-byte aligned.  With p[s] = prob[s][i] the class probability of frame i at step s and
 * lab[s] = labels[s][i] the label of that pass, everything fp32, every operation rounded on its own, in this order:
 *   1. curve[i][s] = p[s]
 *   2. auc         acc = +0; for s = 0 .. S-1 in order acc = acc + (p[s] + p[s+1]); auc = acc * (float)(0.5 / S), the
 *                  constant rounded once from double
 *   3. p_first = p[0], p_last = p[S]; p_min: best = +inf, for s ascending: if (p[s] < best) best = p[s] - a NaN never wins
 *   4. flip_step   FAV_CURVE_DELETION: the first s with lab[s] != class_id; FAV_CURVE_INSERTION: the first s with
 *                  lab[s] == class_id; -1 when there is none.  flip_cells = flip_step * cells / S in integer division (the
 *                  cells occluded, or shown, at that step), or -1
 *   5. reserved = 0
 *   6. a class outside the range: class_id = -1, the four floats NaN, flip_step = flip_cells = -1; the curve row is still
 *      what the class-probability head wrote, which is NaN
 * Non-finite probabilities have no rule of their own: the chains carry them. */
typedef enum fav_curve_mode { FAV_CURVE_DELETION = 0, FAV_CURVE_INSERTION = 1 } fav_curve_mode;
typedef struct fav_curve_record { int32_t class_id; float auc, p_first; int32_t flip_step; float p_last, p_min;
                                  int32_t flip_cells, reserved; } fav_curve_record;
/* The descriptor of a handle's curves: S = steps in [1, 256]; the fill of an occluded pixel, a byte a channel for uint8 frames
 * (each <= 255) and the bits of an fp32 a channel for fp32 frames (any word). */
typedef struct fav_curve { uint32_t struct_size; int32_t steps; uint32_t fill_u8[3]; uint32_t fill_f32_bits[3]; } fav_curve;   /* 32 bytes */
/* Host only, no device: the descriptor's ranges for H x W frames of `layout`, the one place they live; fav_set_curve calls it
 * first, for both layouts.  Refused (FAV_ERR_INVALID_ARG, a message in err, which may be NULL): a NULL descriptor, a wrong
 * struct_size, steps outside [1, 256], H or W below 1, an unknown layout, H * W above (2^31 - 1) / 12, and under
 * FAV_LAYOUT_NHWC_U8 a fill_u8 above 255. */
fav_status fav_check_curve(const fav_curve* desc, int32_t H, int32_t W, int32_t layout, char* err, size_t err_cap);
/* The handle's curve descriptor (copied; NULL: none, the default).  The setter validates it and allocates everything a later
 * fav_classify_curve needs for max_batch frames, in one buffer: the occluded frames of ONE step sized for the fp32 layout, the
 * ranks [max_batch][1024], the probability and label planes [steps + 1][max_batch] and the first pass's labels and confidences.
 * It may synchronise; a refusal for lack of memory carries the size.  Replacing or clearing waits on the host for the work
 * enqueued on the handle and frees the old buffer.  FAV_ERR_UNSUPPORTED while views are set, and fav_set_views is refused
 * (FAV_ERR_UNSUPPORTED) while a descriptor is set: an occluded frame's views are not what the map was made for.  A rejected call
 * leaves the handle as it was.  With no descriptor set a fav_classify* call enqueues exactly what it did before; with one set, too. */
fav_status fav_set_curve(fav_handle* h, const fav_curve* desc);
/* The curve of n frames under one map each: map_dev fp32 [n][mh*mw] (4-byte aligned; 1 <= mh*mw <= 1024, mh, mw <= 256),
 * classes_dev int32 [n] or NULL: the class whose probability is followed - NULL: the label of the unoccluded pass, read on the
 * device, so nothing synchronises.  Outputs: curve_dev fp32 [n][steps + 1] (4-byte aligned), rec_dev [n] (8-byte aligned),
 * labels_dev / conf_dev (either may be NULL): label and confidence of the unoccluded pass, bit-identical to fav_classify_ex on
 * the same frames.  Never allocates or synchronises.  Enqueued on hip_stream, in this order:
 *   1. fav_op_rank_cells on the maps
 *   2. for every step: fav_op_occlude with s1 - s0 = 1 into the handle's buffer, the unchanged forward pass of fav_classify_ex
 *      on it, and fav_op_head_class_prob into the step's plane (the unoccluded step also runs the handle's own head for
 *      labels_dev / conf_dev).  The unoccluded step runs first - step 0 for deletion, step S for insertion - and the others
 *      follow by increasing occlusion (deletion 1 .. S, insertion S-1 .. 0)
 *   3. fav_op_curve
 * Every pass gets the SAME first_image_index.  MC-Dropout masks are keyed by the global frame index, so all steps of a frame
 * see the same masks (common random numbers): the curve then moves with the occlusion only, not with the draw.  Ensembles and
 * ViTs need nothing special: the class-probability head is a function of [T][n][ld] logits.  Afterwards fav_get_logits returns
 * the LAST pass, which is the fully occluded one, and every tap that is on holds that pass.  A class >= num_classes is outside
 * the range like a negative one.  The launches of steps 1 and 3 and the occlusions are booked in no kernel class.
 * FAV_ERR_INVALID_ARG: no descriptor set, n outside [1, max_batch], an unknown layout or mode, a map out of range, a NULL or
 * misaligned map, curve or record buffer, misaligned fp32 frames. */
fav_status fav_classify_curve(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                              const float* map_dev, int32_t mh, int32_t mw, const int32_t* classes_dev, int32_t mode,
                              int32_t* labels_dev, float* conf_dev, float* curve_dev, fav_curve_record* rec_dev,
                              void* hip_stream);

/* ---- RISE saliency (Petsiuk et al. 2018).  The classifier as a black box: the frames are
 * classified under N random smooth masks, every mask is weighted by the probability the class got under it, and the weighted
 * masks are summed.  No tap, no backward pass, no special checkpoint: the map is a function of the input alone, it exists for
 * every arch - a deep ensemble included, which has neither a map tap nor an attention tap - and for any class, and it is a
 * second, independent map to hold against CAM or rollout under the curves above.  What the tests of this library verify is the
 * algebra and its bits on synthetic checkpoints; where a map peaks is a property of trained weights.
 *
 * The descriptor: n_masks N in [1, 8192]; grid g in [1, 15]; keep in [1, 255] (a grid cell is ON with probability keep / 256);
 * seed; the fill of a masked-out pixel as in fav_curve.  Valid for frames H x W with g <= min(H, W).
 *
 * The mask is a pure integer function.  Let ch = ceil(H / g), cw = ceil(W / g), F = the low 32 bits of first_image_index + i for
 * frame i of a call, m the mask index, philox4x32_10(counter, key) the generator of the MC-Dropout masks with key = (seed's low
 * word, seed's high word), and byte b (0 .. 15) of a draw (x, y, z, w) = bits 8 (b % 4) .. 8 (b % 4) + 7 of word b / 4 - x's low
 * byte first, the order of the dropout draws:
 *   1. grid bits: the grid has (g+1) x (g+1) cells, cell j = gy * (g+1) + gx; cell j is ON (b[gy][gx] = 1) iff byte j % 16 of
 *      philox4x32_10((j / 16, F, m, 0x715E), key) is < keep
 *   2. shift: (x, y, ., .) = philox4x32_10((16, F, m, 0x715E), key); dy = mulhi32(x, ch) in [0, ch-1], dx = mulhi32(y, cw) in
 *      [0, cw-1] (mulhi32: the high word of the 64-bit product)
 *   3. bilinear upsampling with half-pixel centres, in integers.  For pixel row y: P = y + dy, num = max(2P + 1 - ch, 0),
 *      y0 = num / (2ch), fy = num % (2ch); if y0 >= g then y0 = g and fy = 0; y1 = min(y0 + 1, g).  Columns alike with cw, dx.
 *      top = (2cw - fx) b[y0][x0] + fx b[y0][x1], bot the same on row y1, num2 = (2ch - fy) top + fy bot in [0, 4 ch cw],
 *      mq = (256 num2 + 2 ch cw) / (4 ch cw) in integer division, in [0, 256]
 * The contract is the mathematical integer.  The kernels compute it in 32 bits, which holds it exactly while
 * 1026 ch cw < 2^31; fav_check_rise refuses the frames beyond (ch cw above 2093057 - at g = 1 a frame of about 1446 x 1446). */
typedef struct fav_rise { uint32_t struct_size; int32_t n_masks, grid, keep; uint64_t seed; uint32_t fill_u8[3];
                          uint32_t fill_f32_bits[3]; } fav_rise;   /* 48 bytes */
/* One frame's RISE summary, 32 bytes, 8-byte aligned.  peak (byte 8) and floor (byte 16) stand where fav_cam_record has them,
 * so fav_op_cam_heatmap accepts an array of these records unchanged.  With p[k] = prob[k][i] (plane 0 the unmasked pass, plane
 * 1 + m mask m), cls = classes[i], and for cell c = cy * mw + cx the sample pixel (yc, xc): lo = ceil(cy * H / mh),
 * hi = ceil((cy + 1) * H / mh) - 1, yc = (lo + hi) / 2 in integer division, xc alike - the middle of the pixels fav_op_occlude
 * assigns to the cell - and wq[m][c] = mq of mask m at (yc, xc); everything fp32, every operation rounded on its own:
 *   1. acc[c] = +0, cov[c] = 0; for m = 0 .. N-1 in that order: acc[c] = acc[c] + p[1 + m] * ((float)wq[m][c] * 2^-8) and
 *      cov[c] += wq[m][c] (an integer, at most 2^21)
 *   2. M[c] = cov[c] > 0 ? acc[c] / ((float)cov[c] * 2^-8) : +0 - the mean of the class probability over the masks, weighted by
 *      how much of the cell each showed.  Dividing by the coverage a cell got, not by N keep / 256, is the usual correction
 *   3. p_full = p[0]; p_mean = (+0 plus p[1 + m] in mask order) * (float)(1.0 / N), the constant rounded once from double
 *   4. peak, peak_cell, floor, n_above and box: steps 5 and 6 of fav_rollout_record over the mh x mw map (the midpoint threshold)
 *   5. a class outside the range: class_id = -1, the four floats NaN, peak_cell = -1, n_above = 0, box = -1; the map row is
 *      still what the chains give
 * Non-finite probabilities have no rule of their own: the chains carry them. */
typedef struct fav_rise_record { int32_t class_id; float p_full, peak; int32_t peak_cell; float floor, p_mean;
                                 int32_t n_above, box; } fav_rise_record;
/* Host only, no device: the descriptor's ranges for H x W frames of `layout`, the one place they live; fav_set_rise calls it
 * first, for both layouts.  Refused (FAV_ERR_INVALID_ARG, a message in err, which may be NULL): a NULL descriptor, a wrong
 * struct_size, n_masks outside [1, 8192], grid outside [1, 15] or above min(H, W), keep outside [1, 255], H or W below 1, an
 * unknown layout, H * W above (2^31 - 1) / 12, 1026 ceil(H / grid) ceil(W / grid) at 2^31 or above, and under
 * FAV_LAYOUT_NHWC_U8 a fill_u8 above 255. */
fav_status fav_check_rise(const fav_rise* desc, int32_t H, int32_t W, int32_t layout, char* err, size_t err_cap);
/* The handle's RISE descriptor (copied; NULL: none, the default).  The setter validates it and allocates everything a later
 * fav_classify_rise needs for max_batch frames, in one buffer: the masked frames of ONE pass sized for the fp32 layout, the
 * probability planes [n_masks + 1][max_batch] and the first pass's labels and confidences.  It may synchronise; a refusal for
 * lack of memory carries the size.  Replacing or clearing waits on the host for the work enqueued on the handle and frees the
 * old buffer.  FAV_ERR_UNSUPPORTED while views are set, and fav_set_views is refused (FAV_ERR_UNSUPPORTED) while a descriptor
 * is set: a masked frame's views are not what the map is made for.  Independent of the curve descriptor: both may be set.  A
 * rejected call leaves the handle as it was.  With no descriptor set a fav_classify* call enqueues exactly what it did before;
 * with one set, too. */
fav_status fav_set_rise(fav_handle* h, const fav_rise* desc);
/* The RISE map of n frames: classes_dev int32 [n] or NULL: the class whose probability weights the masks - NULL: the label of
 * the unmasked pass, read on the device, so nothing synchronises.  The map has mh x mw cells with mh <= in_h, mw <= in_w,
 * mh, mw <= 256 and mh * mw <= 1024.  Outputs: map_dev fp32 [n][mh*mw] (4-byte aligned), rec_dev [n] (8-byte aligned),
 * labels_dev / conf_dev (either may be NULL): label and confidence of the unmasked pass, bit-identical to fav_classify_ex on
 * the same frames.  Never allocates or synchronises.  Costs n_masks + 1 forward passes of the n frames.  Enqueued on hip_stream:
 *   1. the unchanged forward pass of fav_classify_ex on the frames, the handle's own head for labels_dev / conf_dev and
 *      fav_op_head_class_prob into plane 0
 *   2. for m = 0 .. n_masks-1: fav_op_rise_mask with m1 - m0 = 1 into the handle's buffer, the unchanged forward pass on it and
 *      fav_op_head_class_prob into plane 1 + m
 *   3. fav_op_rise_accumulate, told the handle's num_classes
 * Every pass gets the SAME first_image_index.  MC-Dropout masks are keyed by the global frame index, so all passes of a frame
 * see the same dropout masks (common random numbers): the probability then moves with the RISE mask only.  Several masks of one
 * frame in one batch would break exactly that, so a pass holds one mask of every frame.  Afterwards fav_get_logits returns the
 * LAST masked pass, and every tap that is on holds that pass.  A class >= num_classes is outside the range like a negative one.
 * The mask launches and the head's are booked in no kernel class.
 * FAV_ERR_INVALID_ARG: no descriptor set, n outside [1, max_batch], first_image_index < 0 or first_image_index + n > 2^32 - 1,
 * an unknown layout, a map out of range, a NULL or misaligned map or record buffer, misaligned fp32 frames or classes. */
fav_status fav_classify_rise(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                             const int32_t* classes_dev, int32_t mh, int32_t mw, int32_t* labels_dev, float* conf_dev,
                             float* map_dev, fav_rise_record* rec_dev, void* hip_stream);

/* ---- Patch-level anomaly maps (PatchCore, Roth et al. 2022).  The feature-space heads above say
 * WHETHER a frame is unlike the training data, the localisation heads WHERE the classifier's decision comes from; this one says
 * WHERE a frame is unlike the training data.  A BANK holds N L2-normalised in-distribution PATCH features - cells of the last
 * feature map - as bf16 rows; every cell of a frame's map gets the squared Euclidean distance of its normalised feature to its
 * nearest bank row.  That is an anomaly heat map, and its peak is a frame score that the average pool does not dilute.  ResNet
 * arches only (the map tap's).  All pointers are HOST pointers.
 * Ranges (fav_check_patch_bank; FAV_ERR_INVALID_ARG and a message that names the field): struct_size == sizeof(fav_patch_bank);
 * D and N as in fav_knn_bank, D also the map's channel count C when set on a handle; chunk_rows 0 (the default rule below) or a
 * multiple of 64 in [64, 262144]; no row value NaN or inf; threshold not NaN.  The rows are meant to be unit vectors; this is
 * not checked. */
typedef struct fav_patch_bank {
    uint32_t struct_size; int32_t D, N, chunk_rows;
    const uint16_t* rows;   /* [N][D] bf16 bit patterns, meant to be unit vectors (host) */
    float threshold;        /* a cell is above when dist >= threshold; +inf: never */
} fav_patch_bank;
/* One frame's summary, 32 bytes, 8-byte aligned.  peak (byte 8) and floor (byte 16) stand where fav_cam_record has them, so
 * fav_op_cam_heatmap draws the dist map from this record.  Row r = i * HW + c is frame i, cell c; the maps are x[S][n][HW][C]:
 *   1. q[r], DEGENERATE   steps 1 to 3 and 7 of fav_knn_record with feat = x read as [S][n * HW][C]: a cell is a frame there
 *   2. sim[r][b]          b < N: step 4 of fav_knn_record, unchanged: the production GEMM accumulator plus +0.0f
 *   3. nn_sim[r]          the largest sim[r][b]; nn_row[r] the LOWEST b that holds it; dist[r] = fmaxf(2.0f - 2.0f * nn_sim[r],
 *                         +0.0f).  A degenerate cell gets dist = NaN (0x7FC00000) and nn_row = -1, and touches no other cell
 *   4. the record of frame i over dist[i][0 .. HW):
 *        n_degenerate     the count of degenerate cells
 *        mean_dist        +0 plus dist[hw] in index order, times (float)(1.0 / HW); a NaN carries through
 *        peak, peak_cell, floor   step 4 of fav_cam_record: strict > from -inf, strict < from +inf, the lowest cell on a tie,
 *                         a NaN never wins (all cells degenerate: peak -inf, floor +inf, peak_cell -1)
 *        peak_row         nn_row[peak_cell], -1 when peak_cell is -1
 *        n_above, box     the cells with dist >= threshold (a NaN cell is not one) and the inclusive extent of them, packed as
 *                         in fav_cam_record over the Hf x Wf grid; -1 when n_above == 0
 *   5. nothing in a record or a map depends on chunk_rows: the maximum of (sim, -row) is associative and commutative, so the
 *      columns of the bank may be folded in any grouping. */
typedef struct fav_patch_record { int32_t n_degenerate; float mean_dist, peak; int32_t peak_cell; float floor;
                                  int32_t peak_row, n_above, box; } fav_patch_record;
/* Host only, no device: the ranges above (D_expected < 0: any width in range), the one place they live; fav_set_patch_bank
 * calls it first.  err (may be NULL) receives the message. */
fav_status fav_check_patch_bank(const fav_patch_bank* bank, int32_t D_expected, char* err, size_t err_cap);
/* The handle's patch bank (NULL: none), as fav_set_knn in every respect that is not the tap: copied to the device (padded with
 * zero rows to a multiple of 64), D checked against the map's channel count, the whole workspace allocated here for max_batch *
 * Hf * Wf cells (Hf, Wf, C from the planner, as fav_map_tap_info reports them) - fav_classify_patch never allocates or
 * synchronises - and a workspace above 1 GiB refused with the numbers in the message.  The map tap is NOT touched: it stays
 * the caller's, as for fav_cam.  Independent of the feature-space heads: a k-NN bank and a patch bank may be set together.
 * Replacing or clearing a bank waits on the host for the work enqueued on the handle and frees the old copy.
 * FAV_ERR_UNSUPPORTED on a ViT arch and on a deep-ensemble handle, as fav_set_map_tap.  A rejected call leaves the handle as it
 * was. */
fav_status fav_set_patch_bank(fav_handle* h, const fav_patch_bank* bank);
/* The head on the maps of the LAST fav_classify* call: dist_dev fp32 [n][Hf*Wf] (4-byte aligned), row_dev int32 [n][Hf*Wf]
 * (4-byte aligned) or NULL, rec_dev [n] (8-byte aligned), n the frames of that call.  No second forward pass, no allocation,
 * no synchronisation.  FAV_ERR_INVALID_ARG with the tap off, before the first tapped call, without a bank and for a NULL or
 * misaligned buffer.  FAV_ERR_UNSUPPORTED while views are set or when the last call ran under views, as fav_cam. */
fav_status fav_patch(fav_handle* h, float* dist_dev, int32_t* row_dev, fav_patch_record* rec_dev, void* hip_stream);
/* fav_classify_ex unchanged, then fav_patch on the same stream.  Needs the map tap on and a bank (FAV_ERR_INVALID_ARG
 * otherwise); FAV_ERR_UNSUPPORTED while views are set.  Never allocates or synchronises.  fail_dev / score_dev may be NULL.
 * The head's launches are booked in no kernel class. */
fav_status fav_classify_patch(fav_handle* h, const void* images_dev, int32_t n, int32_t layout, int64_t first_image_index,
                              int32_t* labels_dev, float* conf_dev, uint8_t* fail_dev, float* score_dev, float* dist_dev,
                              int32_t* row_dev, fav_patch_record* rec_dev, void* hip_stream);

/* ---- Mid-level patch maps (the rest of PatchCore).  The last map of a 224 x 224 frame has 7 x 7
 * cells of 32 x 32 pixels; PatchCore reads layer2 / layer3 instead (28 x 28 and 14 x 14 cells) and replaces every cell by the
 * aggregate of its neighbourhood before it is normalised.  A SITE says where a bank's rows come from and where the head reads:
 * stage, the residual stage 1 .. 4 whose output the STAGE TAP (above, beside the map tap) holds, and radius, the half width of
 * the neighbourhood: 0 (the cell alone), 1 (3 x 3) or 2 (5 x 5).
 * The locally aware query of a site replaces step 1 of fav_patch_record.  With x the maps [S][n][Hf*Wf][C], r = radius, for
 * frame i, cell (y, x), channel j, everything fp32, every operation rounded on its own, no re-association:
 *   1. m[y][x][j] = (+0 + x[0] + x[1] + .. + x[S-1]) * (float)(1.0 / S), s ascending: step 1 of fav_knn_record
 *   2. v[y][x][j] = +0 + m[y-r][x][j] + .. + m[y+r][x][j], dy ascending; a row outside [0, Hf) is SKIPPED, not added as zero
 *   3. a[y][x][j] = +0 + v[y][x-r][j] + .. + v[y][x+r][j], dx ascending; a column outside [0, Wf) is skipped.  No division by
 *      the count: the normalisation removes any positive scale.  A neighbourhood never crosses a frame
 *   4. steps 2, 3 and 7 of fav_knn_record on a: the sixteen strided chains of the squared norm (chain l over j = l, l + 16, ..),
 *      their sum in index order, fav_sqrtf, the correctly rounded reciprocal, q = bf16(a * inv); a cell whose ss is 0 or not
 *      finite is DEGENERATE: flag 1 and a zero row of q.  A zero cell with a non-zero neighbour is not degenerate at r >= 1
 * At radius 0 this is the k-NN head's query bit for bit (+0 + m is m, and m is never -0).  Only the algebra and the bits are
 * verified here, on synthetic checkpoints; whether mid-level maps localise better is a property of trained weights. */
typedef struct fav_patch_site { uint32_t struct_size; int32_t stage, radius; } fav_patch_site;   /* 12 bytes */
/* Host only, no device: struct_size == sizeof(fav_patch_site), stage in [1, 4], radius in [0, 2]; the message names the field. */
fav_status fav_check_patch_site(const fav_patch_site* site, char* err, size_t err_cap);
/* fav_set_patch_bank at a site.  site == NULL: fav_set_patch_bank itself, byte for byte (the map tap, the k-NN head's query
 * kernel).  With a site: D is checked against the STAGE's channel count, Hf, Wf and the workspace come from the stage's map (as
 * fav_stage_tap_info reports it; the 1 GiB limit and its message stay), fav_patch and fav_classify_patch then read the STAGE
 * TAP - which must be on and at that stage, FAV_ERR_INVALID_ARG with a message naming both stages otherwise - run
 * fav_op_patch_query with the site's radius and write dist / row as [n][Hf*Wf] of that stage.  Records, fold and score kernel
 * are unchanged.  A site {4, 0} gives the records of the plain bank.  The taps are not touched. */
fav_status fav_set_patch_bank_at(fav_handle* h, const fav_patch_bank* bank, const fav_patch_site* site);

/* ---- Greedy coreset selection (the k-centre selection of PatchCore, Roth et al. 2022).  WHICH
 * rows a patch bank or a k-NN bank holds: a uniform draw keeps rows in proportion to how often they occur, so the rare
 * in-distribution modes get no row and are then reported as anomalous; farthest-point sampling covers the feature space
 * instead.  An operator on device arrays (fav_op_coreset_select, below); no handle takes part.
 * In: rows[N][D] bf16 bit patterns, finite, meant to be unit vectors; M in [1, N]; start_row in [0, N).
 * Out: order[M] int32, the rows in the order picked; radius[M + 1] fp32.
 *   order[0] = start_row;  radius[0] = +inf;  mind[r] = +inf for every r;  no row taken
 *   for t = 1 .. M:
 *     1. c = order[t-1];  c becomes taken
 *     2. sim[r] = rows[r] . rows[c] in ONE order for every D: 64 chains, element j in chain (j / 8) % 64; a chain runs
 *        acc = acc + a[j] * b[j] in fp32 over its elements in ascending j from +0 (a product of two bf16 is exact in fp32, so
 *        a fused multiply-add gives the same bits); then six halving steps s[l] = s[l] + s[l + w] for l < w, w = 32, 16, 8, 4,
 *        2, 1; sim = s[0].  What a wave computes whose lane l reads 16 bytes at element 8 l + 512 step and ends with an xor
 *        butterfly.  A chain without elements (D < 512) stays +0
 *     3. d[r] = fmaxf(2.0f - 2.0f * sim[r], +0.0f), the product and the difference rounded on their own, as step 3 of
 *        fav_patch_record;  mind[r] = min(mind[r], d[r]) for EVERY r
 *     4. (key, row) = the lexicographic maximum of (mind[r], -r) over the rows not taken: the farthest row, the LOWEST on a
 *        tie; none when every row is taken (t = M = N only)
 *     5. radius[t] = that mind, 0.0f when none;  if t < M: order[t] = that row
 * radius[1 .. M-1] is the distance at which each centre was picked and never increases; radius[M] is the covering radius of
 * the finished selection: no row of the pool is farther than that from its nearest selected row.  A selection of M rows is a
 * prefix of every longer one from the same start_row, so one run gives the whole coverage curve.
 * The op cannot see a non-finite row: for a pool that holds a NaN or an infinity its picks are unspecified (every index it
 * writes is still a row of the pool, and it never faults); the callers refuse such rows before upload, with the check of
 * fav_check_patch_bank.
 * Ranges (fav_check_coreset, the one place they live; FAV_ERR_INVALID_ARG and a message that names the field): D a multiple of
 * 64 in [64, 4096]; N in [1, 2^24] - the pool may be larger than a bank; M in [1, min(N, 262144)]; start_row in [0, N). */
fav_status fav_check_coreset(int32_t N, int32_t D, int32_t M, int32_t start_row, char* err, size_t err_cap);   /* host only */

/* Host-buffer convenience (frames and results in host memory; synchronous). */
fav_status fav_classify_host(fav_handle* h, const void* images_host, int32_t n, int32_t layout,
                             int64_t first_image_index, int32_t* labels_host, float* conf_host,
                             uint8_t* fail_host, float* score_host);

/* Logits of the last fav_classify call, copied to logits_dev as fp32
 * [T][n][num_classes] (T = 1 without dropout).  Parity tests use it. */
fav_status fav_get_logits(fav_handle* h, float* logits_dev, int32_t* t_out, int32_t* n_out, void* hip_stream);

/* Per-kernel-class timing with HIP events on the launch stream (bench.py's
 * roofline leg).  Classes: see fav_kernel_class.  The launches that make a call's views (fav_set_views) are booked in no
 * class: the profile speaks of the forward pass and the head only. */
typedef enum fav_kernel_class {
    FAV_K_STEM = 0, FAV_K_CONV = 1, FAV_K_MAXPOOL = 2, FAV_K_AVGPOOL = 3,
    FAV_K_DROPOUT = 4, FAV_K_HEAD = 5, FAV_K_COUNT = 6
} fav_kernel_class;
typedef struct fav_profile {
    double ms[FAV_K_COUNT];        /* summed event-measured duration per class */
    double flops[FAV_K_COUNT];     /* algorithmic FLOPs launched */
    double bytes[FAV_K_COUNT];     /* algorithmic HBM bytes launched */
    int64_t launches[FAV_K_COUNT];
} fav_profile;
/* One row per op of the static schedule (valid after fav_get_profile). */
typedef struct fav_op_profile {
    int32_t op_index, kind;          /* kind: 0 stem im2col, 1 conv/fc, 2 maxpool, 3 avgpool, 4 entry dropout, 5 fused bottleneck tail, 6 entry dropout + reduce, 7 fused stem (conv + max pool) */
    int32_t H, W, Cin, Ho, Wo, Cout, kh, kw, stride;
    int32_t reserved;
    double ms, flops, bytes;
    int64_t launches;
} fav_op_profile;
fav_status fav_set_profiling(fav_handle* h, int32_t enable);
fav_status fav_get_op_profile(fav_handle* h, fav_op_profile* out, int32_t cap, int32_t* n_out);
fav_status fav_get_profile(fav_handle* h, fav_profile* out, int32_t reset); /* synchronises the device */

/* ---- Operator level (one launch each; used by the executor and by the
 * per-kernel parity tests).  All tensors NHWC, bf16 unless noted. ---- */
/* The MC-Dropout mask of one launch.  Row r of the launch is virtual frame v = v0 + r: sample t = v / n_img of frame
 * i = v % n_img.  Element e of that row draws byte e % 16 (little endian over the four words) of
 *   Philox4x32-10(counter = (e / 16, low 32 bits of (first_image_index + i), t, site), key = (low, high half of seed))
 * and is KEPT iff the byte is >= threshold; a kept value is bf16(fp32 value * scale), a dropped one +0.
 * Ranges, checked by every fav_op_* that takes a descriptor (conv2d, bottleneck_tail, avgpool, entry_dropout,
 * entry_reduce) before anything is launched - FAV_ERR_INVALID_ARG otherwise; with site < 0 no other field is read:
 *   site               0 .. 2^31 - 1, the fourth counter word
 *   threshold          0 .. 255 (0: site enabled, nothing dropped; the draw is 8 bits wide, so 256 would drop everything)
 *   scale              finite and > 0 (1 / (1 - threshold/256) keeps the expectation; the kernels multiply by what is given)
 *   n_img              >= 1
 *   v0, v0 + rows      0 <= v0 and v0 + rows <= 2^31 - 1: the kernels hold v and t in 32 bits
 *   first_image_index  any value; ONLY ITS LOW 32 BITS enter the counter, so frames 2^32 apart share their masks
 *                      (and the frame word wraps inside a launch that crosses a multiple of 2^32)
 *   seed               any value
 * fav_create refuses a dropout_p whose round(256 p) is 256. */
typedef struct fav_dropout_desc {
    int32_t site;            /* -1 = no dropout */
    uint32_t threshold;      /* drop iff 8-bit draw < threshold (= round(p * 256)) */
    float scale;             /* 1 / (1 - threshold/256) */
    uint64_t seed;
    int64_t v0;              /* virtual frame index of row 0: v = t * n_img + i */
    int32_t n_img;           /* frames per sample */
    int64_t first_image_index;
} fav_dropout_desc;

/* Ranges of a convolution, checked before anything touches the device (FAV_ERR_INVALID_ARG, message "conv: ..."):
 *   n_frames, H, W, kh, kw, stride   >= 1
 *   pad                              >= 0, with H + 2*pad >= kh and W + 2*pad >= kw (the window fits the padded frame)
 *   Cin, Cout                        multiples of 64, >= 64 (Cout 0 or negative would be an empty or a wrapped grid)
 *   relu 0, 1 or 2; out_f32 0 or 1; math_mode a fav_math_mode
 *   n_frames * Ho * Wo               <= 2^31 - 1
 * kh != kw is supported (w is [Cout][kh][kw][Cin] as for a square window). */
typedef struct fav_conv_desc {
    const void* x;           /* [n_frames][H][W][Cin] bf16, Cin % 64 == 0 */
    const void* w;           /* [Cout][kh][kw][Cin] bf16, Cout % 64 == 0 */
    const float* bias;       /* [Cout] */
    const void* res;         /* optional [n_frames][Ho][Wo][Cout] bf16 */
    void* y;                 /* [n_frames][Ho][Wo][Cout] bf16, or fp32 if out_f32 */
    int32_t n_frames, H, W, Cin, Cout, kh, kw, stride, pad;
    int32_t relu, out_f32, math_mode;   /* relu: 0 = none, 1 = ReLU, 2 = GELU (ViT MLP) */
    fav_dropout_desc drop;
} fav_conv_desc;
/* Non-finite values.  Every fav_op_* between the stem and the logits is IEEE arithmetic: a NaN
 * in x, res or made inside (+inf - inf, inf x 0) stays a NaN and +-inf behave as in float64, on every route and in both math
 * modes.  ReLU maps -inf to +0 and keeps +inf and a NaN of either sign; GELU is its fixed sequence (-inf gives NaN); a dropped
 * NaN is +0, a kept one stays NaN; the one rounding to bf16 turns a finite fp32 above the bf16 range into +-inf; the max pool
 * is NaN when any tap inside the frame is; a LayerNorm row with a non-finite value is NaN throughout; an attention query whose
 * scores hold a NaN or +inf has NaN outputs.  The NaN the device makes is 0xFFC00000 (sign set, measured on MI355X); which NaN
 * pattern comes out is not part of the contract.  A frame whose activations overflow ends in the non-finite frame rule above
 * fav_classify, whatever the batch size and the schedule fields of fav_config. */
fav_status fav_op_conv2d(const fav_conv_desc* d, void* hip_stream);

/* Bottleneck tail (one launch): conv_b 3x3/1/1 Cmid->Cmid + ReLU (skipped when wb == NULL: x is then conv_c's
 * input), conv_c 1x1 Cmid->4*Cmid + bias + residual + ReLU + dropout site -> y, and the NEXT block's conv_a
 * 1x1 4*Cmid->Nred + ReLU -> t1n (skipped when wa == NULL).  Same arithmetic, k order and rounding points as the
 * three fav_op_conv2d launches it replaces (bit-identical results); production math mode only.
 * Cmid in {64, 128}; Nred in {0, Cmid, 128}.  n_frames, H and W >= 1, else FAV_ERR_INVALID_ARG ("bottleneck tail: ...")
 * before anything touches the device. */
typedef struct fav_tail_desc {
    const void* x;                          /* [n][H][W][Cmid] bf16 */
    const void* wb; const float* bias_b;    /* [Cmid][3][3][Cmid] bf16, [Cmid] */
    const void* wc; const float* bias_c;    /* [4*Cmid][Cmid] bf16, [4*Cmid] */
    const void* res;                        /* [n][H][W][4*Cmid] bf16 */
    void* y;                                /* [n][H][W][4*Cmid] bf16 */
    const void* wa; const float* bias_a;    /* [Nred][4*Cmid] bf16, [Nred] */
    void* t1n;                              /* [n][H][W][Nred] bf16 */
    int32_t n_frames, H, W, Cmid, Nred;
    fav_dropout_desc drop;
    /* res_entry != 0 (Cmid = Nred = 64 with the 3x3, drop.site >= 0): `res` is the CACHED prefix output
     * [drop.n_img][H][W][4*Cmid] and the residual of virtual frame v is dropout_{entry_site}(res[v % n_img]) - what
     * fav_op_entry_dropout / fav_op_entry_reduce would have stored for it (same bits), computed in the epilogue instead */
    int32_t res_entry, entry_site;
} fav_tail_desc;
fav_status fav_op_bottleneck_tail(const fav_tail_desc* d, void* hip_stream);
/* Route report: the kernel instantiation that the calling thread's most recent fav_op_* launch took, as text in out
 * (NUL-terminated; FAV_ERR_INVALID_ARG, a message of its own in fav_last_error(NULL) and an empty string if cap is too
 * small - 64 bytes hold every name; the recorded route stays).  Empty after a refused call, after a fav_op_* whose launcher
 * has one kernel only (pools, heads, LayerNorm, stream-K, corruptions, ...) and after any fav_classify*, served or refused.
 * The launch site records an enum and a few ints; the text is made here.  Names, with the template arguments that tell
 * instantiations apart:
 *   conv_igemm<BM,BN,BK,NS,bf16|f32,epi0|epi1[,pp][,gelu]>   implicit-GEMM tile: rows x columns x K depth, ring stages, math
 *                                                            mode, epilogue (0 staged through LDS, 1 in registers), ping-pong
 *                                                            K loop, GELU compiled in
 *   conv3x3_halo<CIN,BN,BM,NS,bf16|f32>                      staged-patch 3x3: channels in / out, pixels per tile, weight stages
 *   proj<CIN,COUT,nwN>                                       row-owning projection shortcut, N waves
 *   tail<CMID,NRED,3x3|1x1,nwN,wc1|wc2[,rp16][,res_entry]>   bottleneck tail: with / without conv_b, waves, Wc buffers, 16 rows
 *                                                            per wave pass, residual recomputed from the cached entry tensor
 *   attention<bf16|f32,NKT[,full]>                           key tiles compiled for (13 or 16); full: exactly 13, no masking
 *   entry_reduce<C,NRED>     stem7_pool<u8|f32> */
fav_status fav_op_last_route(char* out, size_t cap);
/* Which kernel instantiation fav_op_conv2d, fav_op_bottleneck_tail or fav_op_attention would launch for these arguments: the
 * name fav_op_last_route reports after the launch, in out (NUL-terminated; 128 bytes hold every answer) - or, with
 * FAV_ERR_INVALID_ARG, the text the op refuses them with, without its "fav_op_...: " prefix.  No device is needed and nothing
 * is launched; a descriptor's pointers are tested for NULL as the op tests them and never read; fav_op_last_route keeps what
 * it held.  vit != 0: as a GEMM of the ViT encoder (its own tile rule); groups >= 1: as one launch over that many ensemble
 * members (the row thresholds count rows x members).  A test / inspection hook. */
fav_status fav_route_conv2d(const fav_conv_desc* d, int32_t vit, int32_t groups, char* out, size_t cap);
fav_status fav_route_bottleneck_tail(const fav_tail_desc* d, int32_t groups, char* out, size_t cap);
fav_status fav_route_attention(int32_t n, int32_t T, int32_t D, int32_t heads, int32_t math_mode, char* out, size_t cap);
/* frames (u8 or fp32 NHWC3) -> normalised bf16 im2col matrix [n*Ho*Wo][kpad].  n, H, W >= 1, a known layout and a window that
 * fits the padded frame, else FAV_ERR_INVALID_ARG and nothing is launched (the same holds for the pools and the entry ops below). */
fav_status fav_op_stem_im2col(const void* images, int32_t layout, int32_t n, int32_t H, int32_t W,
                              int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t kpad,
                              const float* mean3, const float* inv_std3, void* out, void* hip_stream);
/* the ImageNet stem in one launch: frames (u8 or fp32 NHWC3) -> normalise -> 7x7/2 conv to 64 channels (w [64][192] bf16,
 * k = (r*7 + s)*3 + c, zero for k >= 147) -> + bias -> ReLU -> bf16 -> 3x3/2 max pool -> out [n][Hp][Wp][64] bf16;
 * bit-identical to fav_op_stem_im2col + fav_op_conv2d + fav_op_maxpool3x3s2 */
fav_status fav_op_stem_pool(const void* images, int32_t layout, int32_t n, int32_t H, int32_t W, const void* w, const float* bias,
                            const float* mean3, const float* inv_std3, void* out, void* hip_stream);
/* 3x3 / stride 2 / pad 1 max pool, [n][H][W][C] -> [n][(H-1)/2+1][(W-1)/2+1][C]; n, H, W >= 1, C % 8 == 0.  Rounds nothing:
 * subnormals and infinities pass as they are; -0 and +0 are not ordered. */
fav_status fav_op_maxpool3x3s2(const void* x, void* y, int32_t n, int32_t H, int32_t W, int32_t C, void* hip_stream);
/* global average pool [n][HW][C] -> [n][C]: sequential fp32 sum in row order, times fp32(1 / HW), the optional dropout site, one
 * bf16 rounding; n, HW >= 1, C % 16 == 0; drop may be NULL */
fav_status fav_op_avgpool(const void* x, void* y, int32_t n, int32_t HW, int32_t C,
                          const fav_dropout_desc* drop, void* hip_stream);
/* out[v - v0][e] = dropout(x[v % n_img][e]) for v in [v0, v0 + n_out); elems_per_frame >= 16 and a multiple of 16, n_out >= 1,
 * drop->site >= 0 */
fav_status fav_op_entry_dropout(const void* x, void* out, int64_t elems_per_frame, int32_t n_out,
                                const fav_dropout_desc* drop, void* hip_stream);
/* entry dropout and the 1x1 reduce behind it in one launch (C = 256, Nred = 64):
 * y[v - v0] = dropout(x[v % n_img]) as above, t1[v - v0] = bf16(relu(conv1x1(y[v - v0], wa) + bias_a)); x [n_img][HW][C],
 * wa [Nred][C] bf16.  The executor's fusion of the MC-Dropout suffix's first two launches (no reference counterpart).
 * y may be NULL: the dropped copies are then not stored (a tail with res_entry recomputes them). */
fav_status fav_op_entry_reduce(const void* x, void* y, const void* wa, const float* bias_a, void* t1, int32_t C, int32_t Nred,
                               int32_t HW, int32_t n_out, const fav_dropout_desc* drop, void* hip_stream);
/* logits fp32 [T][n][ld] -> labels, conf (and fail/score if non-NULL).  The four fav_op_head* entry points read only
 * the first num_classes values of a row (ld - num_classes padding values may hold anything) and apply the non-finite
 * frame rule stated above fav_classify to the caller's logits. */
fav_status fav_op_head(const float* logits, int32_t T, int32_t n, int32_t num_classes, int32_t ld,
                       float temperature, int32_t conf_kind, float tau,
                       int32_t* labels, float* conf, uint8_t* fail, float* score, void* hip_stream);
/* logits fp32 [T][n][ld] -> records[n] (fav_uncertainty, 8-byte aligned), fail / score if non-NULL.  T <= 4096,
 * num_classes <= 1024; conf_kind 0, 1 or 2 (kind 2 at T = 1 or num_classes = 1: conf = 1).  fav_op_head with conf_kind 2
 * runs the same kernel (and needs T >= 2, num_classes >= 2).  Non-finite frames: the rule above fav_classify and the record's
 * fields beside fav_uncertainty. */
fav_status fav_op_head_uncertainty(const float* logits, int32_t T, int32_t n, int32_t num_classes, int32_t ld,
                                   float temperature, int32_t conf_kind, float tau, fav_uncertainty* records,
                                   uint8_t* fail, float* score, void* hip_stream);

/* logits fp32 [T][n][ld] -> the prediction sets of fav_classify_sets under cp.  records (8-byte aligned) may be NULL
 * when true_labels is given; true_labels / true_scores (both or neither): the calibration scores of
 * fav_conformal_scores.  fail / score may be NULL.  num_classes <= 1024; conf_kind 0, 1 or 2; first_image_index is
 * the global index of frame 0 (the Philox counter of a randomized cp).  Non-finite frames: the rule above fav_classify; the set
 * is empty and the calibration score NaN (beside fav_pred_set). */
fav_status fav_op_head_sets(const float* logits, int32_t T, int32_t n, int32_t num_classes, int32_t ld,
                            float temperature, int32_t conf_kind, float tau, int64_t first_image_index,
                            const fav_conformal* cp, const int32_t* true_labels, float* true_scores,
                            fav_pred_set* records, uint8_t* fail, float* score, void* hip_stream);

/* logits fp32 [T][n][ld] (device) -> cells[n][K] (fav_calib_cell, 8-byte aligned) at the K temperatures temps_host
 * (host floats, 1 <= K <= FAV_SWEEP_MAX_TEMPS, all finite and > 0), one launch that reads the logits once.  T <= 4096,
 * num_classes <= 1024; conf_kind 0, 1 or 2 (kind 2 needs T >= 2 and num_classes >= 2, as for fav_op_head).  Non-finite
 * frames: the rule above fav_classify, per temperature; nll and brier NaN (beside fav_calib_cell). */
fav_status fav_op_head_sweep(const float* logits, int32_t T, int32_t n, int32_t num_classes, int32_t ld,
                             const float* temps_host, int32_t K, int32_t conf_kind, const int32_t* true_labels_dev,
                             fav_calib_cell* cells_dev, void* hip_stream);

/* ---- ViT building blocks (BASELINE configs[4]); linear layers go through fav_op_conv2d with kh = kw = 1.
 * LayerNorm over rows of D bf16 values (row r at x + r*ldx elements; D % 4 == 0, D <= 1024), fp32 statistics,
 * y[rows][D] bf16. */
fav_status fav_op_layernorm(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t rows,
                            int32_t D, float eps, void* hip_stream);
/* Multi-head attention with 64-wide heads: qkv [n][T][3D] bf16 (Q | K | V) -> out [n][T][D] bf16,
 * softmax(Q K^T / 8) V per head, T <= 256, D = 64 * heads. */
fav_status fav_op_attention(const void* qkv, void* out, int32_t n, int32_t T, int32_t D, int32_t heads,
                            int32_t math_mode, void* hip_stream);
/* One linear layer of the encoder as the chained stream-K GEMM (gemm_streamk_kernel): y[rows][N] = act((x[rows][K] w[N][K]^T + bias) + res),
 * bf16 in and out, fp32 bias; res may be NULL or y itself (in-place residual); act 0 none, 1 ReLU, 2 GELU.  Bit-identical to
 * fav_op_conv2d with kh = kw = 1 on the same operands (the K steps are dealt out evenly over a persistent grid and a tile's partial
 * accumulator is handed on, never re-associated).  K % 32 == 0, N % 128 == 0, at least 256 tiles of 128 x 128; production math only.
 * No reference counterpart (the slot is platform/backend/main.py:160). */
typedef struct fav_linear_desc {
    const void* x; const void* w; const float* bias; const void* res; void* y;
    int64_t rows;
    int32_t K, N, act;
} fav_linear_desc;
fav_status fav_op_linear_streamk(const fav_linear_desc* d, void* hip_stream);
/* Token assembly: x[f][0] = pos[0], x[f][1 + p] = bf16(emb[f][p] + pos[1 + p]); emb [n][ntok-1][D] bf16, pos fp32. */
fav_status fav_op_vit_assemble(const void* emb, const float* pos, void* x, int32_t n, int32_t ntok, int32_t D,
                               void* hip_stream);

/* ---- SignalAnalyzer.analyze_frame as one fused pass per frame (SURVEY.md §8f row 2;
 * reference platform/backend/signal_analyzer.py:62-112): cv2.COLOR_BGR2GRAY, cv2.Laplacian
 * (ksize 1, reflect-101) variance, mean brightness, mean |gray - previous gray|, 256-bin
 * histogram entropy.  frames_bgr: [n][H][W][3] uint8 on the device, consecutive frames of
 * one stream; prev_gray: gray plane preceding frame 0 (NULL = none); last_gray_out: receives
 * the gray plane of frame n-1 (NULL = not wanted).  W % 4 == 0, H >= 3, H*W <= 150000.
 * The kernel moves four pixels per dword: frames_bgr, prev_gray and last_gray_out must be
 * 4-byte aligned and stats_dev 8-byte aligned, else FAV_ERR_INVALID_ARG and nothing is launched. */
typedef struct fav_signal_stats {
    double lap_var, mean, mean_diff;
    float entropy;
    int32_t has_prev;
    int64_t sum_lap, sum_lap2;         /* exact integer sums the doubles are derived from */
    uint32_t sum_gray, sum_absdiff;
    uint32_t hist[256];
} fav_signal_stats;
fav_status fav_op_signal_stats(const uint8_t* frames_bgr, int32_t n, int32_t H, int32_t W, const uint8_t* prev_gray,
                               uint8_t* last_gray_out, fav_signal_stats* stats_dev, void* hip_stream);

/* ---- On-device corruption generator: the reference's four vision modes
 * (platform/backend/vision_simulator.py:15, painted at platform/frontend/js/app.js:782-857) and
 * ImageNet-C style Gaussian noise, as a pure function of (seed, global frame index).
 * frames: uint8 [n][H][W][3] on the device.  out: uint8 [n][H][W][3] for modes 0..2, fp32
 * [n][H][W][3] in [0,1] for FAV_CORRUPT_GAUSSIAN. */
typedef enum fav_corrupt_mode { FAV_CORRUPT_NORMAL = 0, FAV_CORRUPT_BLANK = 1, FAV_CORRUPT_GLITCH = 2,
                                FAV_CORRUPT_GAUSSIAN = 3 } fav_corrupt_mode;
fav_status fav_op_corrupt(const uint8_t* frames, void* out, int32_t n, int32_t H, int32_t W, int32_t mode,
                          float noise_level, float brightness_gain, float gaussian_sigma, uint64_t seed,
                          int64_t first_frame_index, void* hip_stream);

/* ---- ImageNet-C style corruption family on the device: eight corruptions at severities 1..5, every one a pure function
 * of (seed, global frame index) like fav_op_corrupt.  frames: uint8 [n][H][W][3] on the device; out: fp32 [n][H][W][3] in
 * [0,1] (FAV_LAYOUT_NHWC_F32, which fav_classify* accepts), 4-byte aligned.  x_c = u8 / 255 in fp32; the definitions
 *  are this build's contract, not bit-parity with scikit-image, PIL or OpenCV:
 *   impulse    a = amount in [0,1]: channel c of a pixel is hit iff its uniform draw is below a; a hit is 0 or 1
 *   speckle    a = sigma >= 0: clamp(x + (x a) z), z standard normal (Box-Muller, as FAV_CORRUPT_GAUSSIAN)
 *   gaussian blur  a = sigma > 0: separable, R = (int)(4 a + 0.5) <= 32, replicate borders
 *   defocus    a = disk radius, (int)a in 1..12; b = alias sigma > 0; reflect-101 borders
 *   contrast   a in [0,1]: clamp((x - m_c) a + m_c), m_c the frame's channel mean
 *   pixelate   a in (0,1]: box means over max(1, (int)(H a)) x max(1, (int)(W a)) cells; W <= 2048
 *   brightness a in [0,1]: HSV value V -> min(V + a, 1)
 *   saturate   a >= 0, b in [-1,1]: HSV saturation S -> clamp(S a + b)
 * The noise kinds draw Philox4x32-10 with key = seed and counter = (pixel index in the frame, low 32 bits of
 * first_frame_index + f, stream, 0), stream 16 for impulse and 17 for speckle. */
typedef enum fav_corruption { FAV_C_IMPULSE_NOISE = 0, FAV_C_SPECKLE_NOISE = 1, FAV_C_GAUSSIAN_BLUR = 2,
    FAV_C_DEFOCUS_BLUR = 3, FAV_C_CONTRAST = 4, FAV_C_PIXELATE = 5, FAV_C_BRIGHTNESS = 6, FAV_C_SATURATE = 7,
    FAV_C_COUNT = 8 } fav_corruption;
typedef struct fav_corruption_desc { uint32_t struct_size; int32_t kind; float a, b; uint64_t seed;
    int64_t first_frame_index; } fav_corruption_desc;            /* 32 bytes */
/* host only, no device: the severity table; severity 1..5 */
fav_status fav_corruption_params(int32_t kind, int32_t severity, float* a, float* b);
/* host only: the fp32 taps the blur kernels use for (kind, a, b).
 * GAUSSIAN_BLUR: 2R+1 taps.  DEFOCUS_BLUR: (2R+1)^2 taps, row-major.
 * *radius = R; FAV_ERR_INVALID_ARG if cap is too small or the kind has no taps */
fav_status fav_corruption_taps(int32_t kind, float a, float b, float* taps, int32_t cap, int32_t* radius);
/* One launch, no allocation, no workspace, no synchronisation.  A rejected call (FAV_ERR_INVALID_ARG: a NULL pointer, n, H or
 * W below 1, a wrong struct_size, a kind outside [0, FAV_C_COUNT), a non-finite a or b, a parameter outside the range stated
 * above) launches nothing and leaves a message that names the function in fav_last_error(NULL). */
fav_status fav_op_corrupt_c(const uint8_t* frames_dev, float* out_dev, int32_t n, int32_t H, int32_t W,
                            const fav_corruption_desc* d, void* hip_stream);

/* ---- The views defined above fav_set_views, made on the device: frames [n][H][W][3] of `layout` -> out [n_views][n][H][W][3]
 * of the same element type, view a of frame i at row a*n + i.  The views travel in the kernel arguments: views_host (at most
 * 1536 bytes) is read before the call returns.  No allocation, no workspace, no synchronisation; at most two launches (the
 * views without transpose, those with).  Pointers need the element type's alignment only (any byte for uint8, 4 for fp32).
 * A refused call (FAV_ERR_INVALID_ARG: a NULL pointer, n, H or W below 1, an unknown layout, what fav_check_views refuses, a
 * misaligned fp32 pointer, H * W above (2^31 - 1) / 12, n * n_views above 2^31 - 1, out overlapping frames) launches nothing and leaves a message
 * that names the function in fav_last_error(NULL). */
fav_status fav_op_views(const void* frames_dev, void* out_dev, int32_t n, int32_t H, int32_t W, int32_t layout,
                        const fav_view* views_host, int32_t n_views, void* hip_stream);

/* ---- The scoring head defined beside fav_ood_record, on device arrays: feat_bf16 [S][n][D] bf16, mu_dev [D], Pt_dev [D][k]
 * and Mt_dev [k][R] (P and M TRANSPOSED, so that the kernel reads them along its thread index), class_id_dev [R], labels_dev
 * [n] or NULL, records_dev [n] (8-byte aligned).  One launch; no allocation, no workspace (x and g live in LDS), no
 * synchronisation; vector stores only.  A thread owns one column of the projection, then one row of the means, for the up to
 * four frames of its block; every chain runs in the contract's order.  The matrix pipe is not used: an fp32-input MFMA is an
 * fmaf chain, which rounds once where the contract rounds twice.
 * A refused call (FAV_ERR_INVALID_ARG: a NULL pointer other than labels_dev, S outside [1, 4096], n < 1, D, k or R outside
 * the ranges of fav_ood_model, a NaN threshold, a misaligned records_dev) launches nothing and leaves a message that names the
 * function in fav_last_error(NULL). */
fav_status fav_op_ood_score(const void* feat_bf16, int32_t S, int32_t n, int32_t D, int32_t k, int32_t R,
                            const float* mu_dev, const float* Pt_dev, const float* Mt_dev,
                            const int32_t* class_id_dev, const int32_t* labels_dev, float threshold,
                            fav_ood_record* records_dev, void* hip_stream);

/* ---- The k-NN head defined beside fav_knn_record, on device arrays: feat_bf16 [S][n][D] bf16, bank_dev [N][D] bf16 (16-byte
 * aligned; exactly N rows - the caller never pads), class_id_dev [N] or NULL, ws_dev a workspace of at least
 * fav_knn_workspace_bytes(n, D, N) bytes on a 256-byte boundary, records_dev [n] (8-byte aligned).  Three kernels: the query
 * kernel (q and the degenerate flags), the similarity GEMM through the convolution launcher (1x1, fp32 output, zero bias;
 * fav_op_last_route names its tile) - in two launches when N is no multiple of 64 and at least 64: the bank in place up to
 * its last whole 64 rows, the rest from a zero-padded tile in the workspace - and the radix select.  No allocation, no
 * synchronisation; vector stores only.  Padding columns and degenerate frames' rows of the workspace are never read by the
 * select.
 * A refused call (FAV_ERR_INVALID_ARG: a NULL pointer other than class_id_dev, S outside [1, 4096], n < 1, D, N or k outside
 * the ranges of fav_knn_bank, a NaN threshold, a workspace too small or misaligned, a misaligned bank_dev or records_dev)
 * launches nothing and leaves a message that names the function in fav_last_error(NULL). */
size_t fav_knn_workspace_bytes(int32_t n, int32_t D, int32_t N);   /* host only; 0 for sizes out of range */
fav_status fav_op_knn_score(const void* feat_bf16, int32_t S, int32_t n, int32_t D, const void* bank_dev, int32_t N, int32_t k,
                            const int32_t* class_id_dev, float threshold, void* ws_dev, size_t ws_bytes,
                            fav_knn_record* records_dev, void* hip_stream);

/* ---- The whole drift test defined beside fav_drift_record, on device arrays: feat_bf16 [S][n][D] bf16, ref_dev [R][D] bf16
 * (16-byte aligned; exactly R rows), ws_dev a workspace of at least fav_drift_workspace_bytes(n, D, R, n_perm) bytes on a
 * 256-byte boundary, record_dev one record (8-byte aligned), perm_sums_dev int64 [n_perm][2] (8-byte aligned) or NULL: the
 * pair (S_BB, S_AB) of every permutation.  The reference's block of distances is computed in the call: one GEMM of the whole
 * pool against itself through the convolution launcher (1x1, fp32 output, zero bias; fav_op_last_route names its tile), then
 * the quantise, row-sum, permutation (n_perm + 1 blocks) and final kernels.  No allocation, no synchronisation; vector stores
 * only.  The reference's norms are not checked here (fav_check_drift_ref is host work on host rows).
 * A refused call (FAV_ERR_INVALID_ARG: a NULL pointer other than perm_sums_dev, S outside [1, 4096], n outside [2, 1024], D, R,
 * n_perm or alpha outside the ranges of fav_drift_ref, a workspace too small or misaligned, a misaligned ref_dev, record_dev
 * or perm_sums_dev) launches nothing and leaves a message that names the function in fav_last_error(NULL). */
size_t fav_drift_workspace_bytes(int32_t n, int32_t D, int32_t R, int32_t n_perm);   /* host only; 0 for sizes out of range */
fav_status fav_op_drift_test(const void* feat_bf16, int32_t S, int32_t n, int32_t D, const void* ref_dev, int32_t R,
                             int32_t n_perm, uint64_t seed, float alpha, void* ws_dev, size_t ws_bytes,
                             fav_drift_record* record_dev, int64_t* perm_sums_dev, void* hip_stream);

/* ---- The CAM head defined beside fav_cam_record, on device arrays: maps_bf16 [S][n][Hf*Wf][C] bf16 and w_bf16 rows of ldw
 * bf16 (both 16-byte aligned), bias fp32 [n_classes], classes_dev int32 [n][K], cam_dev fp32 [n][K][Hf*Wf], rec_dev [n][K]
 * (8-byte aligned).  One launch, one block a frame, no global workspace, no allocation, no synchronisation; vector stores
 * only.  Ranges: 1 <= S <= 4096; n >= 1; 1 <= Hf*Wf <= 1024 with Hf, Wf <= 256 (the box packs a byte a coordinate); C a
 * multiple of 512, at most 4096; ldw >= C, a multiple of 8; n_classes >= 1; 1 <= K <= 8.  A refused call
 * (FAV_ERR_INVALID_ARG: a NULL pointer, a size out of range, a misaligned buffer) launches nothing and leaves a message that
 * names the function in fav_last_error(NULL). */
fav_status fav_op_cam(const void* maps_bf16, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C, const void* w_bf16,
                      int32_t ldw, const float* bias, int32_t n_classes, const int32_t* classes_dev, int32_t K, float* cam_dev,
                      fav_cam_record* rec_dev, void* hip_stream);
/* The overlay a dashboard draws: each of m maps (cam_dev fp32 [m][Hf*Wf], rec_dev [m] for its floor and peak) resized to
 * H x W and normalised to a byte, out_u8 [m][H][W].  Bilinear, half-pixel centres, clamped edges (align_corners = False).
 * Per output pixel (y, x), everything fp32, every operation rounded on its own:
 *   1. sy = fmaxf(((float)y + 0.5f) * ((float)Hf / (float)H) - 0.5f, 0);  y0 = min((int)sy, Hf - 1);  y1 = min(y0 + 1, Hf - 1);
 *      ly = sy - (float)y0;  hy = 1 - ly;  likewise sx, x0, x1, lx, hx from x, Wf and W
 *   2. top = hx * M[y0][x0] + lx * M[y0][x1];  bot = hx * M[y1][x0] + lx * M[y1][x1];  v = hy * top + ly * bot
 *   3. t = (v - floor) / (peak - floor);  byte = rintf(fminf(fmaxf(t, 0), 1) * 255) (fmaxf drops a NaN: byte 0)
 *   4. a map with !(peak > floor) - flat, all NaN, a class out of range - is all 0
 * Ranges: m >= 1; 1 <= Hf*Wf <= 1024; 1 <= H*W <= 2^31 - 1.  Refusals as fav_op_cam. */
fav_status fav_op_cam_heatmap(const float* cam_dev, const fav_cam_record* rec_dev, int32_t m, int32_t Hf, int32_t Wf,
                              int32_t H, int32_t W, uint8_t* out_u8, void* hip_stream);

/* ---- The attention tap's launch on caller buffers (the contract stands beside fav_set_attn_tap): qkv_bf16 [n][T][3 D] bf16
 * (Q | K | V, head h = columns 64 h .. 64 h + 63 of each), a_dev fp32 [n][T][ldT] with ldT = 16 * ceil(T / 16), both 16-byte
 * aligned.  One launch, no workspace, no allocation, no synchronisation; vector stores only.  Ranges: n >= 1; 2 <= T <= 256;
 * 1 <= heads <= 64; D == 64 * heads.  A refused call (FAV_ERR_INVALID_ARG) launches nothing and leaves a message that names
 * the function in fav_last_error(NULL). */
fav_status fav_op_attn_mean(const void* qkv_bf16, float* a_dev, int32_t n, int32_t T, int32_t D, int32_t heads, void* hip_stream);
/* The rollout head defined beside fav_rollout_record, on device arrays: a_dev fp32 [L][n][T][ld] with T = gh * gw + 1, map_dev
 * fp32 [n][gh*gw] (both 4-byte aligned), rec_dev [n] (8-byte aligned).  One launch, one block a frame, no workspace, no
 * allocation, no synchronisation.  Ranges: 1 <= L <= 64; 0 <= first_layer < L; n >= 1; 1 <= gh, gw <= 255 with
 * gh * gw + 1 <= 256; ld >= T, a multiple of 4.  Refusals as fav_op_attn_mean. */
fav_status fav_op_attn_rollout(const float* a_dev, int32_t L, int32_t n, int32_t gh, int32_t gw, int32_t ld, int32_t first_layer,
                               float* map_dev, fav_rollout_record* rec_dev, void* hip_stream);

/* ---- The four operations behind fav_classify_curve, on device arrays.  Each: one launch, no allocation, no workspace, no
 * synchronisation, vector stores only.  A refused call (FAV_ERR_INVALID_ARG) launches nothing and leaves a message that names
 * the function in fav_last_error(NULL).
 *
 * The ranking: map_dev fp32 [n][cells] -> rank_dev int32 [n][cells] (both 4-byte aligned), n >= 1, 1 <= cells <= 1024.
 * rank[i][c] = the number of cells of frame i that come before c in the order "more salient first".  Cell a comes before b when
 *   - a is not NaN and b is NaN, or
 *   - both are not NaN and M[a] > M[b], or
 *   - neither value is greater - equal values, +0 against -0, both NaN - and a < b.
 * So every NaN ranks behind -inf, ties go to the lower index, and the ranks of a frame are a permutation of 0 .. cells-1.  One
 * block a frame, the comparisons run from LDS. */
fav_status fav_op_rank_cells(const float* map_dev, int32_t n, int32_t cells, int32_t* rank_dev, void* hip_stream);
/* The occlusion: frames [n][H][W][3] of `layout` -> out [s1 - s0][n][H][W][3] of the same element type, the steps s0 .. s1-1
 * of S, 0 <= s0 < s1 <= S + 1.  With cells = mh * mw:
 *   1. the cell of pixel (y, x) is (y * mh / H) * mw + (x * mw / W), integer division (a map finer than the frame is legal:
 *      some cells then hold no pixel)
 *   2. k_s = s * cells / S, integer division, for s = 0 .. S: k_0 = 0, k_S = cells
 *   3. FAV_CURVE_DELETION: a pixel of step s is `fill` when rank[i][cell] < k_s, else the source pixel;
 *      FAV_CURVE_INSERTION: the source pixel when rank[i][cell] < k_s, else `fill`
 * Every copied element is copied bit for bit (an fp32 NaN keeps its payload, as in fav_op_views).  fill: three words read before
 * the call returns - under uint8 each <= 255 and its low byte is stored, under fp32 the word is the fp32's bits.  rank_dev int32
 * [n][cells] is NOT validated on the device: any value below k_s occludes, so a caller may bring a ranking that is no permutation.
 * Ranges: n, H, W >= 1; 1 <= S <= 256; 1 <= mh * mw <= 1024 with mh, mw <= 256; H * W at most (2^31 - 1) / 12;
 * n * (s1 - s0) at most 2^31 - 1; frames and out need the element type's alignment only (any byte for uint8, 4 for fp32),
 * rank_dev 4; out must not overlap frames.  The source pixels are read once, whatever s1 - s0 is. */
fav_status fav_op_occlude(const void* frames_dev, void* out_dev, int32_t n, int32_t H, int32_t W, int32_t layout,
                          const int32_t* rank_dev, int32_t mh, int32_t mw, int32_t mode, int32_t S, int32_t s0, int32_t s1,
                          const uint32_t* fill, void* hip_stream);
/* The class-probability head: logits fp32 [T][n][ld] -> prob_dev fp32 [n] and labels_dev int32 [n] (may be NULL).  pbar is
 * computed by the heads' shared core exactly as fav_classify_ex computes it; prob[i] = pbar[classes_dev[i]], labels[i] is
 * fav_classify_ex's label.  classes_dev int32 [n] may be NULL: the frame's own label - prob is then the mean_prob of
 * fav_uncertainty, bit for bit.  A class outside [0, num_classes) gives prob = NaN, the label is still written.  A non-finite
 * frame (the rule above fav_classify) gives prob = NaN and label 0.  T <= 4096, num_classes <= 1024, ld >= num_classes and a
 * multiple of 4, temperature > 0; only the first num_classes values of a row are read. */
fav_status fav_op_head_class_prob(const float* logits, int32_t T, int32_t n, int32_t num_classes, int32_t ld, float temperature,
                                  const int32_t* classes_dev, float* prob_dev, int32_t* labels_dev, void* hip_stream);
/* The curve head defined beside fav_curve_record: prob_dev fp32 [S + 1][n], labels_dev int32 [S + 1][n], classes_dev int32 [n]
 * -> curve_dev fp32 [n][S + 1] (all 4-byte aligned) and rec_dev [n] (8-byte aligned).  n >= 1, 1 <= S <= 256,
 * 1 <= cells <= 1024, mode a fav_curve_mode value.  A thread a frame.  This entry point is not told the number of classes: the
 * class outside the range is, for it, a negative one (the class-probability head has written NaN for any other, and the chains
 * carry it); fav_classify_curve passes the handle's num_classes along. */
fav_status fav_op_curve(const float* prob_dev, const int32_t* labels_dev, const int32_t* classes_dev, int32_t n, int32_t S,
                        int32_t cells, int32_t mode, float* curve_dev, fav_curve_record* rec_dev, void* hip_stream);

/* ---- The two operations behind fav_classify_rise (beside fav_op_head_class_prob above), on device arrays.  Each: one launch,
 * no allocation, no workspace, no synchronisation, vector stores only.  A refused call (FAV_ERR_INVALID_ARG) launches nothing
 * and leaves a message that names the function in fav_last_error(NULL).  desc is a host pointer read before the call returns
 * and checked by fav_check_rise for H x W frames; the mask function stands beside fav_rise.  first_image_index may be any
 * value: only its low 32 bits count, and frame i's index wraps past 2^32 with them.
 *
 * The masks applied: frames [n][H][W][3] of `layout` -> out [m1 - m0][n][H][W][3] of the same element type, the masks
 * m0 .. m1-1 of desc->n_masks, 0 <= m0 < m1 <= n_masks.  With mq the mask value of the pixel:
 *   uint8: out = (p * mq + fill * (256 - mq) + 128) >> 8 a channel, so mq = 256 copies the pixel and mq = 0 stores the fill
 *   fp32:  mq == 256 copies the source bits (a NaN keeps its payload), mq == 0 stores the fill's bits, otherwise
 *          w = (float)mq * 2^-8 and out = f + w * (p - f), the three operations rounded on their own (no FMA contraction)
 * Ranges and alignment as fav_op_occlude: n, H, W >= 1; H * W at most (2^31 - 1) / 12; n * (m1 - m0) at most 2^31 - 1; frames
 * and out need the element type's alignment only (any byte for uint8, 4 for fp32); out must not overlap frames.  The source
 * pixels are read once, whatever m1 - m0 is; the grid bits and the shift of a (frame, mask) pair are drawn once a block. */
fav_status fav_op_rise_mask(const void* frames_dev, void* out_dev, int32_t n, int32_t H, int32_t W, int32_t layout,
                            const fav_rise* desc, int64_t first_image_index, int32_t m0, int32_t m1, void* hip_stream);
/* The accumulate head defined beside fav_rise_record: prob_dev fp32 [N + 1][n] with N = desc->n_masks, classes_dev int32 [n]
 * -> map_dev fp32 [n][mh*mw] (all 4-byte aligned) and rec_dev [n] (8-byte aligned).  n >= 1; 1 <= mh <= H, 1 <= mw <= W,
 * mh, mw <= 256, mh * mw <= 1024; H and W as fav_check_rise takes them under either layout (the fill is not read).  No frame is
 * read: a block a frame derives the mask values again at the cells' sample pixels.  num_classes: a class >= num_classes is
 * outside the range like a negative one; 0: not known, only a negative class then is (the class-probability head has written
 * NaN for any other, and the chains carry it). */
fav_status fav_op_rise_accumulate(const float* prob_dev, const int32_t* classes_dev, int32_t n, const fav_rise* desc,
                                  int64_t first_image_index, int32_t H, int32_t W, int32_t mh, int32_t mw, int32_t num_classes,
                                  float* map_dev, fav_rise_record* rec_dev, void* hip_stream);

/* ---- The patch head defined beside fav_patch_record, on device arrays: maps_bf16 [S][n][Hf*Wf][C] bf16, bank_dev [N][C] bf16
 * (16-byte aligned; exactly N rows - the caller never pads), ws_dev a workspace of at least fav_patch_workspace_bytes(n * Hf *
 * Wf, C, N, chunk_rows) bytes on a 256-byte boundary, dist_dev fp32 [n][Hf*Wf] and row_dev int32 [n][Hf*Wf] or NULL (4-byte
 * aligned), rec_dev [n] (8-byte aligned).  The k-NN head's query kernel on a grid of n * Hf * Wf blocks; then, one column chunk
 * of the bank at a time, the similarity GEMM through the convolution launcher into one slab sim[n * Hf * Wf][chunk] (1x1, fp32
 * output, zero bias; fav_op_last_route names its tile; an unpadded bank's last part tile goes through a zero-padded 64-row tile
 * in the workspace) and the fold of that slab into a running (similarity, row) a cell - stream order makes reusing the slab
 * safe; then the score kernel, a block a frame.  The chunk: chunk_rows when given, else the largest multiple of 128 whose slab
 * fits 256 MiB, at least 128; either way at most N padded to 64 (fav_patch_chunk_rows).  No allocation, no synchronisation;
 * vector stores only.  Padding columns and degenerate cells' rows of the slab are never read by the fold.
 * A refused call (FAV_ERR_INVALID_ARG: a NULL pointer other than row_dev, S outside [1, 4096], n < 1, Hf*Wf outside [1, 1024] or
 * a side above 256, n*Hf*Wf above 2^31 - 1, C or N outside the ranges of fav_patch_bank, a bad chunk_rows, a NaN threshold, a
 * workspace too small or misaligned, a misaligned bank_dev, dist_dev, row_dev or rec_dev) launches nothing and leaves a message
 * that names the function in fav_last_error(NULL). */
size_t fav_patch_workspace_bytes(int32_t cells_total, int32_t D, int32_t N, int32_t chunk_rows);   /* host only; 0 for sizes out of range */
int32_t fav_patch_chunk_rows(int32_t cells_total, int32_t N, int32_t chunk_rows);   /* host only: the slab's columns; 0 out of range */
fav_status fav_op_patch_score(const void* maps_bf16, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C,
                              const void* bank_dev, int32_t N, int32_t chunk_rows, float threshold, void* ws_dev,
                              size_t ws_bytes, float* dist_dev, int32_t* row_dev, fav_patch_record* rec_dev, void* hip_stream);
/* fav_op_patch_score with one more argument, radius in [0, 2]: step 1 of fav_patch_record is then the locally aware query
 * defined beside fav_patch_site - fav_op_patch_query into the workspace - in place of the k-NN head's query kernel; everything
 * behind it is unchanged.  maps_bf16 must be 16-byte aligned here.  At radius 0 dist, row and rec are fav_op_patch_score's. */
fav_status fav_op_patch_score_at(const void* maps_bf16, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C,
                                 const void* bank_dev, int32_t N, int32_t chunk_rows, float threshold, int32_t radius,
                                 void* ws_dev, size_t ws_bytes, float* dist_dev, int32_t* row_dev, fav_patch_record* rec_dev,
                                 void* hip_stream);
/* ---- The locally aware query defined beside fav_patch_site, on device arrays: maps_bf16 [S][n][Hf*Wf][C] bf16 and q_dev bf16
 * [n*Hf*Wf][C] (both 16-byte aligned), flags_dev int32 [n*Hf*Wf].  One launch of patch_local_query_kernel, a block of 256
 * threads a frame row: 16-byte loads, several in flight a lane; a map row is read by the 2 radius + 1 blocks around it, from
 * HBM by the first of them; where a row of C channels does not fit 64 KB of LDS the block works through channel slices and the
 * sixteen chains carry on from slice to slice.  Vector stores only, no atomics, no block waits for another, no allocation, no
 * synchronisation.  A refused call (FAV_ERR_INVALID_ARG: a NULL pointer, a misaligned maps_bf16, q_dev or flags_dev, S outside
 * [1, 4096], n < 1, Hf*Wf outside [1, 1024] or a side above 256, n*Hf*Wf above 2^31 - 1, C not a multiple of 64 in [64, 4096],
 * radius outside [0, 2]) launches nothing and leaves a message that names the function in fav_last_error(NULL). */
fav_status fav_op_patch_query(const void* maps_bf16, int32_t S, int32_t n, int32_t Hf, int32_t Wf, int32_t C,
                              int32_t radius, void* q_dev, int32_t* flags_dev, void* hip_stream);

/* ---- The selection defined beside fav_check_coreset, on device arrays: rows_bf16_dev [N][D] bf16, order_dev int32 [M],
 * radius_dev fp32 [M + 1] (all three 16-byte aligned), ws_dev a workspace of at least fav_coreset_workspace_bytes(N, D, M) bytes
 * on a 256-byte boundary: mind as uint32 keys [N] and two buffers of per-block partial (key, row) pairs.  No handle.  One step
 * kernel launched M + 1 times on hip_stream, plain launches whose stream order is the only synchronisation: launch t finds the
 * centre from the partials of launch t - 1 (every block reduces them itself; block 0 stores radius[t] and order[t]), then
 * streams the pool once - N * D * 2 bytes a step - a wave a row, and leaves its own partials; launch M is one block and only
 * stores radius[M].  No allocation, no synchronisation, no atomics, no cooperative launch, no block waits for another; vector
 * stores only.  Launch 0 writes mind without reading it and every partial is written before it is read: what an earlier call
 * left in the workspace reaches no result.  The host enqueues M + 1 launches, which is what a fit-time operation costs.
 * A refused call (FAV_ERR_INVALID_ARG: anything fav_check_coreset refuses, a NULL or misaligned pointer, a workspace too
 * small) launches nothing, writes nothing and leaves a message that names the function in fav_last_error(NULL). */
size_t fav_coreset_workspace_bytes(int32_t N, int32_t D, int32_t M);   /* host only; 0 for sizes out of range */
fav_status fav_op_coreset_select(const void* rows_bf16_dev, int32_t N, int32_t D, int32_t M, int32_t start_row, void* ws_dev,
                                 size_t ws_bytes, int32_t* order_dev, float* radius_dev, void* hip_stream);

/* ---- The autoencoder anomaly sensor: the one learned model of the reference's design
 * (docs/system_notes.md 6.1: "Conv2d -> ReLU -> ConvTranspose2d", trained on normal frames only, anomaly_score =
 * MSE(recon, frame)).  It needs no classifier and has a handle of its own; nothing of fav_handle is involved.
 *
 * The model, levels L in {1, 2, 3}, widths C_l = 64 * 2^(l-1), pixels in [0, 1] (u8 / 255, fp32 sanitised as the stem does; no
 * mean or std):
 *   enc_1: Conv2d(3, 64, 3, stride 2, pad 1) + ReLU          enc_l: Conv2d(C_{l-1}, C_l, 3, stride 2, pad 1) + ReLU, l = 2 .. L
 *   dec_l: ConvTranspose2d(C_l, C_{l-1}, 2, stride 2) + ReLU, l = L .. 2          dec_1: ConvTranspose2d(64, 3, 2, stride 2) + Sigmoid
 *   recon = net(x)[..., :H, :W]
 * Grids: h_0 = H, h_l = (h_{l-1} - 1) / 2 + 1, likewise w; the decoder's output is 2^L h_L x 2^L w_L >= H x W and is cropped.
 * Every layer rounds its output to bf16 once, as every convolution of the library does.  enc_1 is fav_op_stem_im2col (3x3/2/1,
 * kpad 64, mean 0, inv_std 1) and a 1x1 fav_op_conv2d 64 -> 64 whose weight is [64][64], k = (r 3 + s) 3 + c, zero above 26;
 * enc_l is fav_op_conv2d.  A 2x2 / stride-2 transposed convolution has no overlapping windows, so dec_l, l >= 2, is a 1x1
 * fav_op_conv2d C_l -> 4 C_{l-1} whose weight row (2a + b) C_{l-1} + co holds wt[:, co, a, b] and whose bias is tiled four
 * times; its output [rows][4 C] read as [4 rows][C] feeds the next one as it is.
 * Row order.  With m = L - 1 such steps, row r of the last hidden matrix [n h_L w_L 4^m][64] has r / 4^m = (i h_L + y_L) w_L +
 * x_L and the base-4 digits d_1 .. d_m of r % 4^m, most significant first, d_j = 2 a_j + b_j; it is pixel (y, x) of the
 * 2^m h_L x 2^m w_L level-1 grid, from (y_L, x_L) by y = 2 y + a_j, x = 2 x + b_j for j = 1 .. m.
 *
 * Decode and compare, operation by operation (tests/ae_ref.py restates it; equal bits):
 *   1. acc[r][(2a + b) 3 + co], 12 columns: the production accumulator of a 1x1 convolution 64 -> 12 over the hidden rows,
 *      v_mfma_f32_16x16x32_bf16, k ascending, two issues, the accumulator starting at +0
 *   2. z = acc + bias[co], one fp32 addition
 *   3. s = 1.0f / (1.0f + exp(-z)): the library's fixed exponential sequence (the ViT path's), one addition, a correctly
 *      rounded division
 *   4. q = (int)rintf(s * 255.0f), 0 .. 255 (a NaN z: the exponential answers 0, hence 255); it is output pixel
 *      (2 y + a, 2 x + b), channel co; pixels outside H x W are dropped
 *   5. the frame's pixel in the same units: a u8 pixel as it is; fp32: rintf(min(max(sanitise(px), 0), 1) * 255.0f)
 *   6. e = q - p and e^2 in integers; every sum below is an integer sum, so its order is free
 *   7. cell in {8, 16, 32}; gh = ceil(H / cell), gw = ceil(W / cell), gh * gw <= 1024, gh and gw <= 256.  cell_sse[i][c], uint32:
 *      the sum over the cell's pixels inside the frame and their 3 channels;
 *      err_map[i][c] = (float)((double)cell_sse / ((double)(3 * pixels_inside) * 65025.0))
 *   8. the record: sse the 64-bit frame sum; mse = (float)((double)sse / ((double)(3 H W) * 65025.0)), the reference's
 *      anomaly_score on [0, 1] pixels; peak, peak_cell, floor as step 4 of fav_cam_record over err_map; n_above and box as
 *      in fav_cam_record over the cells with err_map >= threshold (-1 when there is none)
 *   9. optionally recon_u8 [n][H][W][3]: the bytes q.
 * The record is 32 bytes, 8-byte aligned; peak (byte 8) and floor (byte 16) stand where fav_cam_record has them, so
 * fav_op_cam_heatmap draws err_map from it. */
typedef struct fav_ae_record { uint32_t sse_lo; float mse, peak; int32_t peak_cell; float floor;
                               uint32_t sse_hi; int32_t n_above, box; } fav_ae_record;
typedef struct fav_ae_config {
    uint32_t struct_size;   /* sizeof(fav_ae_config) */
    int32_t in_h, in_w;     /* frame size, 1 .. 4096 each */
    int32_t levels;         /* 1 .. 3 */
    int32_t max_batch;      /* largest n passed to fav_ae_score, >= 1 */
    int32_t cell;           /* 8, 16 or 32 */
} fav_ae_config;
typedef struct fav_ae fav_ae;
/* Host only: the ranges above; each refusal (FAV_ERR_INVALID_ARG) names the field in err (may be NULL). */
fav_status fav_check_ae_config(const fav_ae_config* cfg, char* err, size_t err_cap);
/* Host only, the one place the geometry lives: h[l], w[l] for l = 0 .. levels (0 beyond), the cell grid and the bytes
 * fav_ae_create allocates for max_batch frames (two rotating activation buffers; every pointer may be NULL).  A workspace
 * above 1 GiB is refused with both numbers in the message. */
fav_status fav_ae_info(const fav_ae_config* cfg, int32_t h[4], int32_t w[4], int32_t* gh, int32_t* gw, size_t* workspace_bytes,
                       char* err, size_t err_cap);
/* Host only: structural validation of a FAVA v1 blob.  Header of 64 bytes: magic "FAVA", version 1, levels, layers = 2 levels
 * (uint32 each), the total size (uint64); then a (weight offset, bias offset) uint64 pair a layer, in the order enc_1 .. enc_L,
 * dec_L .. dec_2, dec_1; then the data, every range 64-byte aligned: bf16 weights in the device layouts above (dec_1: [12][64]),
 * fp32 biases (dec_l: the tiled 4 C_{l-1}; dec_1: 3).  FAV_ERR_BAD_BLOB for a truncated blob, a misaligned or out-of-range
 * offset, a wrong level or layer count and any non-finite value; err (may be NULL) says which. */
fav_status fav_ae_check_blob(const void* blob_host, size_t size, char* err, size_t err_cap);
/* Lifecycle: create -> load_weights -> score xN -> destroy, on the calling thread's current HIP device.  create allocates the
 * whole workspace and the weight slab; load_weights runs fav_ae_check_blob first and refuses (FAV_ERR_BAD_BLOB) a blob of
 * another level count; threshold (the cell threshold of step 8) defaults to +inf, so no cell counts as above until it is set;
 * a NaN is refused.  A rejected call leaves the object as it was; its message is in fav_last_error(NULL). */
fav_status fav_ae_create(const fav_ae_config* cfg, fav_ae** out);
fav_status fav_ae_load_weights(fav_ae* ae, const void* blob_host, size_t size);
fav_status fav_ae_set_threshold(fav_ae* ae, float threshold);
void fav_ae_destroy(fav_ae* ae);
/* n frames (1 <= n <= max_batch) -> err_map_dev fp32 [n][gh*gw], rec_dev [n] (8-byte aligned), and recon_u8_dev [n][H][W][3]
 * unless NULL.  L + 1 encoder launches, L - 1 decoder GEMMs and the two launches of fav_op_ae_decode_compare, all on
 * hip_stream; never allocates or synchronises.  FAV_ERR_NO_WEIGHTS before load_weights; FAV_ERR_INVALID_ARG for n out of range,
 * an unknown layout and a NULL or misaligned buffer (fp32 frames and err_map_dev 4 bytes, rec_dev 8), before anything is
 * launched.  Calls on one object must not overlap: they share its workspace. */
fav_status fav_ae_score(fav_ae* ae, const void* images_dev, int32_t n, int32_t layout, float* err_map_dev, fav_ae_record* rec_dev,
                        uint8_t* recon_u8_dev, void* hip_stream);
/* Steps 1 - 9 on caller buffers: hidden_bf16 [n h_L w_L 4^m][64] in the row order above and wg12_bf16 [12][64] (both 16-byte
 * aligned), bias3 fp32 [3], frames [n][H][W][3] in `layout`.  Two launches: a block a cell of a frame (it leaves the cell's
 * integer sum in err_map_dev), then a block a frame for the means and the record; cell_sse_dev (may be NULL) receives the
 * integer sums.  No allocation, no workspace, no synchronisation, no atomics, vector stores only.  Ranges: n >= 1; m 0 .. 2;
 * H, W, h_L, w_L 1 .. 4096 with 2^(m+1) h_L >= H and 2^(m+1) w_L >= W; n h_L w_L 4^m <= 2^31 - 1; the cell and grid ranges of
 * step 7; threshold not NaN.  A refused call (FAV_ERR_INVALID_ARG: one of these, a NULL pointer other than cell_sse_dev and
 * recon_u8_dev, an unknown layout, a misaligned buffer) launches nothing and leaves a message that names the function in
 * fav_last_error(NULL). */
fav_status fav_op_ae_decode_compare(const void* hidden_bf16, int32_t n, int32_t h_L, int32_t w_L, int32_t m, const void* wg12_bf16,
                                    const float* bias3, const void* frames, int32_t layout, int32_t H, int32_t W, int32_t cell,
                                    float threshold, uint32_t* cell_sse_dev, float* err_map_dev, fav_ae_record* rec_dev,
                                    uint8_t* recon_u8_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FAV_H */
