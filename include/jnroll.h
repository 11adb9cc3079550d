/*
 * jnroll.h — C ABI of libjnroll.so, the MI355X (gfx950) glimpse-rollout engine.
 *
 * The reference (jolibrain/jolineedle) has no FFI: its boundary for this path is the
 * Python operator API.  Each entry point below names the reference
 * interface it sits under (paths relative to /root/reference).  A reference-side
 * binding is a ctypes stub, shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; `*_dev` pointers are HIP device pointers owned by the caller
 *    (e.g. torch tensors' data_ptr()); `stream` is a hipStream_t passed as void*
 *    (NULL = the legacy default stream).
 *  - every function returns 0 on success or a negative JN_E* code; jn_last_error()
 *    gives the message of the calling thread's last failure.  No exceptions cross.
 *  - no hidden host synchronisation: only functions documented as "synchronises"
 *    wait for the device.
 *  - activations are fp32 (the reference is fp32 end to end); tensors exchanged at
 *    the boundary keep the reference's layouts (NCHW images/patches, [B,T] rows).
 */
#ifndef JNROLL_H
#define JNROLL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JN_ABI_VERSION 2

enum {
  JN_OK = 0,
  JN_EINVAL = -1,    /* bad argument / shape / state                     */
  JN_ENOMEM = -2,    /* device or host allocation failed                 */
  JN_EHIP = -3,      /* a HIP runtime call failed                        */
  JN_ENOTFOUND = -4, /* a required state-dict entry is missing           */
  JN_ESTATE = -5     /* call order violated (e.g. rollout before weights) */
};

/* Action-selection modes of jn_rollout (src/reinforce.py:73-90). */
enum { JN_MODE_GREEDY = 0, JN_MODE_SAMPLE = 1, JN_MODE_FORCED = 2 };

/* Which conv network a call addresses. */
enum { JN_NET_GPT_BACKBONE = 0, JN_NET_DETECTOR = 1 };

typedef struct jn_ctx jn_ctx;

/* Mirrors the fields of the reference's model_config / train_config that shape the
 * path (main.py:310-388; src/models/gpt.py:162-329).  Zero-initialise, set
 * struct_size = sizeof(jn_config). */
typedef struct jn_config {
  int32_t struct_size;
  int32_t device;               /* HIP device ordinal                                   */
  /* decision transformer: gpt.py:190-218 zoo entry already resolved */
  int32_t n_layer, n_head, n_embd;
  int32_t block_size;           /* max_seq_len T (tokens = T + 1 with the class token)  */
  int32_t n_actions;            /* 9 with --enable-stop else 8 (src/env/common.py:48-56) */
  int32_t patch_size;           /* P                                                    */
  int32_t use_pos_emb;          /* --use-positional-embedding                           */
  int32_t no_patch_emb;         /* --no-patch-embedding                                 */
  int32_t concat_emb;           /* --concat-embeddings                                  */
  int32_t decoder_pos_encoding; /* --decoder-pos-encoding                               */
  int32_t pos_emb_size;         /* rows of transformer.wpe (main.py:378)                */
  /* patch encoder `gpt_backbone` (gpt.py:261-264); width 0 = absent, the detector's
   * PAFPN encodes patches instead (gpt.py:376-380) */
  float gpt_bb_depth, gpt_bb_width;
  int32_t gpt_bb_depthwise;
  /* detector `yolox` (gpt.py:251-259); with_detector 0 = decision-only context */
  int32_t with_detector;
  float det_depth, det_width;
  int32_t det_depthwise;
  float det_conf_threshold;     /* --detector-conf-threshold                            */
  float det_nms_threshold;      /* yolox postprocess default 0.45                       */
  int32_t max_batch;            /* capacity B of env / rollout workspaces               */
  int32_t max_det_per_patch;    /* cap of kept boxes per patch (ragged output rows)     */
  int32_t act_dtype;            /* activation storage: 0 = fp32 (the reference's dtype, exact-fp32 MFMA),
                                 * 1 = bf16 (bf16 storage + bf16 MFMA, fp32 accumulate / statistics / weights) */
  int32_t gpt_wide;             /* 1: take the wide decision route for every model it admits (n_embd 64, 128, 192, 256
                                 * as well; a test and A/B switch, the Python layer sets it from JN_GPT_WIDE=1).  Ignored
                                 * for the shapes that route refuses; n_embd above 256 takes the route whatever is set */
} jn_config;

/* One state-dict entry (names of SURVEY.md §5, e.g. "gpt_backbone.backbone.stem.conv.bn.weight"). */
typedef struct jn_tensor {
  const char* name;
  const void* data;   /* HOST pointer, contiguous                      */
  int32_t dtype;      /* 0 = float32, 1 = int64                        */
  int32_t ndim;
  int64_t shape[4];
} jn_tensor;

typedef struct jn_param_info {
  char name[160];
  int32_t dtype;      /* 0 = float32, 1 = int64                        */
  int32_t ndim;
  int64_t shape[4];
  int32_t is_buffer;  /* 1 = registered buffer (running stats, masks)  */
  int32_t used;       /* 0 = listed for state-dict compatibility only  */
} jn_param_info;

/* Outputs of one rollout: ReinforceTrainer.rollout's dict (src/reinforce.py:204-215).
 * All pointers are device memory sized for T = block_size steps; entries past
 * `n_steps` (read with jn_rollout_steps) are zero/false.  NULL = not wanted. */
typedef struct jn_rollout_out {
  float* rewards_dev;        /* [B, T]                                          */
  float* returns_dev;        /* [B, T]                                          */
  float* logprobs_dev;       /* [B, T]                                          */
  float* entropies_dev;      /* [B, T]                                          */
  uint8_t* masks_dev;        /* [B, T+1]                                        */
  uint8_t* logit_masks_dev;  /* [B, T]                                          */
  int64_t* positions_dev;    /* [B, T+1, 2] (y, x)                              */
  int64_t* actions_dev;      /* [B, T]   actions taken                          */
  float* logits_dev;         /* [B, T, n_actions] last-token logits per step    */
  float* final_emb_dev;      /* [B, T+1, n_embd] token embeddings (gpt.py:534)  */
  float* patches_dev;        /* [B, T+1, 3, P, P] or NULL                       */
  float* det_boxes_dev;      /* [B, T+1, max_det_per_patch, 7] or NULL          */
  int32_t* det_counts_dev;   /* [B, T+1] kept boxes per patch (0 = reference None) */
} jn_rollout_out;

/* ---- lifetime ------------------------------------------------------------------ */
int jn_abi_version(void);
const char* jn_last_error(void);
/* GPT.__init__ (src/models/gpt.py:162-329): builds the layer plan and workspaces. */
int jn_create(const jn_config* cfg, jn_ctx** out);
int jn_destroy(jn_ctx* ctx);

/* ---- weights: nn.Module.state_dict()/load_state_dict of GPT (main.py:532-584) ---- */
int jn_param_count(const jn_ctx* ctx);
int jn_param_info_at(const jn_ctx* ctx, int index, jn_param_info* out);
/* Debugging aid, no device needed: the plan of one conv-stack forward pass of `net` over N patches (train / eval,
 * with the detection head or not, from op `first_op` on), as the pass itself forms it.  Writes up to `cap` triples
 * (route, link, deferred) to `out`, one per op, and returns the number of ops of the pass (or a negative error).
 * route: 1 stem, 2 conv (1x1 / depthwise / dense 3x3 by the op), 3 fused DWConv, 4 fused DWConv + shortcut add,
 * 5 absorbed by the fused kernel of op `link`, 6 spp, 7 upsample, 8 shortcut add, 9 predictors.  link (an op index, -1:
 * none): of route 3 / 4 the pointwise op; of an fp32 1x1 conv the upsample whose copy its kernel may write.  deferred:
 * the layer's BatchNorm table is left to its consumers in this pass. */
int jn_debug_forward_plan(const jn_ctx* ctx, int net, int N, int train, int with_head, int first_op, int32_t* out,
                          int cap);
/* Debugging aid, no device needed: the route the context's decision steps take.  0: one workgroup per agent
 * (n_embd <= 256); 1: the wide route, every Linear one GEMM over all agents (256 < n_embd <= 1024, a multiple of 64;
 * with jn_config.gpt_wide also n_embd 64, 128, 192, 256). */
int jn_debug_decision_route(const jn_ctx* ctx);
/* Uploads and pre-packs (BN folded for eval, Linear weights transposed).  Entries the
 * path does not use are ignored; a missing used entry -> JN_ENOTFOUND.  Synchronises. */
int jn_load_weights(jn_ctx* ctx, const jn_tensor* tensors, size_t n);

/* ---- environment: NeedleGeneralEnv (src/env/general_env.py) ----------------------- */
/* __init__ :15-82 + convert_bboxes_to_masks :360-379.  images [B,3,H,W] f32 stay owned
 * by the caller and must outlive the env; bboxes [B,nb,4] int64 xyxy (zero rows = pad). */
int jn_env_init(jn_ctx* ctx, const float* images_dev, const int64_t* bboxes_dev,
                int B, int H, int W, int nb, int max_ep_len, int stop_enabled, void* stream);
/* The same env over 8-bit images [B,3,H,W] u8 (what the reference's ToTensor gets from PIL), read in place: byte b
 * stands for b / 255 correctly rounded, so every result equals that of jn_env_init on u8.float().div(255).  The
 * gathers, the rollout's encoders and the training backward read the bytes (a quarter of the fp32 image's traffic). */
int jn_env_init_u8(jn_ctx* ctx, const uint8_t* images_dev, const int64_t* bboxes_dev,
                   int B, int H, int W, int nb, int max_ep_len, int stop_enabled, void* stream);
/* reset :144-170.  positions [B,2] (y,x) int64 or NULL = uniform draw from `seed`. */
int jn_env_reset(jn_ctx* ctx, const int64_t* positions_dev, uint64_t seed, void* stream);
/* step :172-233 + rewards :321-358 + terminated :235-246.  Outputs may be NULL. */
int jn_env_step(jn_ctx* ctx, const int64_t* actions_dev, float* rewards_dev,
                uint8_t* terminated_dev, uint8_t* truncated_dev, void* stream);
/* State views (device pointers into the context, valid until jn_env_init/jn_destroy):
 * what = 0 positions int64 [B,2]; 1 bbox_masks u8 [B,Gh,Gw]; 2 visited u8 [B,Gh,Gw];
 * 3 steps int32 [B]; 4 has_stopped u8 [B]; 5 the grid extents int32 [B,2] of ragged mode (jn_env_init_ragged
 * below; a null pointer in every other mode). */
int jn_env_state(jn_ctx* ctx, int what, void** ptr_dev);
/* `patches` property :285-306 — bit-exact strided copy of the current patches
 * -> out [B,3,P,P] f32. */
int jn_env_patches(jn_ctx* ctx, float* out_dev, void* stream);
/* Stand-alone gather (no context state): out[b] = images[b,:,y*P:(y+1)*P, x*P:(x+1)*P]. */
int jn_gather_patches(const float* images_dev, const int64_t* positions_dev, float* out_dev,
                      int B, int C, int H, int W, int P, void* stream);
/* ... of u8 images: out (f32) = byte / 255 correctly rounded. */
int jn_gather_patches_u8(const uint8_t* images_dev, const int64_t* positions_dev, float* out_dev,
                         int B, int C, int H, int W, int P, void* stream);
/* Trajectory form of the gather: out[n] = images[image_index[n], :, y_n*P:(y_n+1)*P, x_n*P:(x_n+1)*P] for N
 * (image, position) pairs — the patches NeedleSimpleEnv.generate_sample stacks one `get_patch` at a time
 * (src/env/simple_env.py:55-81, 472) and init_sample's detector patches (:417-419).  image_index[n] < 0 writes
 * a zero patch (a masked step of the zero-initialised sample, :380-384).  Positions must lie on the grid and
 * indices below n_images (the Python mirror asserts both, as get_patch does at :73-74). */
int jn_gather_patches_indexed(const float* images_dev, const int64_t* image_index_dev,
                              const int64_t* positions_dev, float* out_dev, int N, int n_images,
                              int C, int H, int W, int P, void* stream);
/* ... of u8 images: out (f32) = byte / 255 correctly rounded. */
int jn_gather_patches_indexed_u8(const uint8_t* images_dev, const int64_t* image_index_dev,
                                 const int64_t* positions_dev, float* out_dev, int N, int n_images,
                                 int C, int H, int W, int P, void* stream);

/* ---- image views: NeedleDataset.rotate / translate and padded_collate_fn, applied in the read ------------------
 * (src/dataset.py:95-226 rotate / translate, :274-278 their order, :308-347 bottom / right padding to one canvas.)
 * A view describes one stored image [3,Hs,Ws] (contiguous, f32 or u8) as an image on the batch's logical canvas
 * Hc x Wc: with (Hr,Wr) = (Hs,Ws) for rot 0 / 180 and (Ws,Hs) for rot 90 / 270, canvas pixel (c,Y,X) is
 *   0 when Y >= Hr or X >= Wr (padding); else with (y1,x1) = (Y - ty, X - tx): 0 outside [0,Hr) x [0,Wr) (the
 *   whole-pixel shift's zero fill); else rot 0: src[y1,x1]; 90: src[Hs-1-x1,y1]; 180: src[Hs-1-y1,Ws-1-x1];
 *   270: src[x1,Ws-1-y1] (the transpose / flip pairs of rotate); a byte b stands for b / 255 correctly rounded.
 * The augmented image is never written: the kernels that cut patches apply the mapping. */
typedef struct jn_image_view {
  const void* src;     /* device address of the stored image; stays the caller's */
  int32_t src_u8;      /* 0: f32 values, 1: u8 bytes */
  int32_t Hs, Ws;      /* stored height and width */
  int32_t rot;         /* 0, 90, 180 or 270 */
  int32_t ty, tx;      /* translation in pixels, down / right positive (bbox + translate, :212-226) */
} jn_image_view;
/* jn_env_init over B views on one canvas Hc x Wc (multiples of patch_size): views_host[B] is read from HOST
 * memory, validated (JN_EINVAL: rot outside the four values, a rotated image larger than the canvas, a canvas that
 * is no multiple of patch_size, a null source, mixed element types) and copied to the device; the context owns the
 * copy, the stored images must outlive the env.  bboxes [B,nb,4] are the boxes already transformed to the canvas.
 * Every glimpse step then gathers its B patches through the views into a staging stack the context owns (element
 * type of the sources) and the encoders read that.  jn_env_init / jn_env_init_u8 put the env back into plain mode. */
int jn_env_init_views(jn_ctx* ctx, const jn_image_view* views_host, const int64_t* bboxes_dev, int B, int Hc, int Wc,
                      int nb, int max_ep_len, int stop_enabled, void* stream);
/* jn_env_init_views for batched inference over images of unequal size: extents_host [B][2] = (gh, gw) int32, read
 * from HOST memory, gives every agent its own patch grid inside the canvas grid.  The reference pads an image it
 * infers on to ITS OWN multiple of patch_size and the agent cannot leave that image (infer.py:138-146; the B = 1 envs
 * of test(), src/reinforce.py:383-386), whereas on the canvas of padded_collate_fn every agent walks the whole canvas
 * (the training semantics, which jn_env_init_views keeps).  With extents: the step clamps to gh - 1 / gw - 1, the
 * random reset draws modulo (gh, gw), the boxes are clipped to gh*P x gw*P; the state arrays stay [B,Gh,Gw] on the
 * canvas grid, cells outside an extent are never visited and never marked.  Agent b then behaves exactly as a B = 1
 * env on image b padded on its own.  JN_EINVAL beyond jn_env_init_views' checks: an extent outside 1..Hc/P x
 * 1..Wc/P, a view with ty or tx != 0, a rotated image larger than gh*P x gw*P.  Every other jn_env_init* call clears
 * ragged mode. */
int jn_env_init_ragged(jn_ctx* ctx, const jn_image_view* views_host, const int32_t* extents_host,
                       const int64_t* bboxes_dev, int B, int Hc, int Wc, int nb, int max_ep_len, int stop_enabled,
                       void* stream);
/* NeedleGeneralEnv.get_detection_batch (src/env/general_env.py:506-546, over parse_bboxes :381-504) without its patches,
 * context-free: which cells of the patch grid the detector trains on, and every such patch's targets.  bboxes [B,nb,4]
 * int64 xyxy in image pixels, zero rows = padding; the grid is Gh x Gw cells of P px, or per image the top-left
 * gh x gw of it with extents_dev (int32 [B,2] = (gh, gw); cells outside an extent do not exist).
 *  - Cell (py, px) holds a piece of box k iff y1 // P <= py <= y2 // P and x1 // P <= px <= x2 // P (floor division,
 *    for negative coordinates too; a box with y2 // P < y1 // P touches nothing); pieces in cells outside the grid or
 *    the extent are dropped.  The piece is (max(x1, px*P) - px*P, max(y1, py*P) - py*P, min(x2, px*P + P - 1) - px*P,
 *    min(y2, py*P + P - 1) - py*P).  An all-zero row thus marks cell (0, 0) with a zero box: the reference's padding
 *    quirk (:492-502), kept.  A cell is positive when any box touches it, else empty.
 *  - Per image, in index order: its positive cells in row-major (y, x) order, then k = min(sample_neg, n_empty)
 *    negatives by a partial Fisher-Yates shuffle of the row-major list E of its empty cells: for j = 0..k-1,
 *    r = Philox4x32-10(key = seed, counter = (image, j, 0x4e454753, 0)).x, swap E[j] with E[j + r mod (n_empty - j)],
 *    emit E[j].  The draws depend on (seed, image index) only (the reference draws with torch.randperm, which no
 *    device path reproduces).
 *  - Row offsets[i] is the first row of image i, offsets[B] = n the number of rows (int32 [B+1]); n_pos int32 [B] the
 *    positive cells per image.  cells int64 [capacity,3] = (image, y, x); targets int64 [capacity,nb,5] = (0, x1, y1,
 *    x2, y2) of box k's piece in the cell, zeros where box k does not touch it (F.pad(boxes[i, y, x], (1, 0)), :544).
 *    Rows >= capacity are not written (offsets still count them); rows >= n are left alone.  capacity = B * Gh * Gw
 *    always suffices.
 * Three launches on `stream` (count, scan over B, select), no atomics: equal inputs give equal bytes.  One workgroup
 * per image keeps the image's cell lists in LDS, hence Gh * Gw <= 4096.  Does not wait for the device, except with
 * extents_dev: they are read back and checked first (one stream synchronisation).
 * JN_EINVAL, before any launch: nb < 1, P < 1, sample_neg < 0, Gh or Gw < 1, Gh * Gw > 4096, B < 0, capacity < 0, an
 * extent outside 1..Gh x 1..Gw, a null pointer (cells / targets may be NULL with capacity 0). */
int jn_detection_cells(const int64_t* bboxes_dev, const int32_t* extents_dev, int B, int nb, int Gh, int Gw, int P,
                       int sample_neg, uint64_t seed, int capacity, int64_t* cells_dev, int64_t* targets_dev,
                       int32_t* offsets_dev, int32_t* n_pos_dev, void* stream);
/* Trainer.patch_bboxes2full_image (src/trainer.py:250-280) for a whole batch, context-free: the detections of a
 * rollout (jn_rollout_out: det_boxes [B,T+1,K,7], det_counts [B,T+1], positions [B,T+1,2] (y,x), masks u8 [B,T+1])
 * become one list per image in full-image pixels.  Image b walks t = 0..S (S <= T steps were executed), skips the
 * steps with masks[b,t] == 0 and appends the step's boxes in their stored order: columns 0..3 + (x*P, y*P, x*P,
 * y*P) as one f32 add each, columns 4..6 copied.  out_boxes [B,(S+1)*K,7]: rows 0..out_totals[b]-1 of image b are
 * written, the rest is left alone; out_totals int32 [B] is all the host needs to read back. */
int jn_rollout_boxes_to_image(const float* det_boxes_dev, const int32_t* det_counts_dev, const int64_t* positions_dev,
                              const uint8_t* masks_dev, int B, int T, int S, int K, int P, float* out_boxes_dev,
                              int32_t* out_totals_dev, void* stream);
/* merge_boxes (src/utils.py:198-255) for a whole batch, context-free: boxes [B,Nmax,W] f32 with counts int32 [B]
 * (what jn_rollout_boxes_to_image writes), W = 7 or 6 for predictions (x1,y1,x2,y2,obj,cls,...) -> rows of 6
 * (x1,y1,x2,y2,max obj*cls,1); target != 0: W = 5 (cls,x1,y1,x2,y2) -> rows of 5 with a leading 0.  Box i joins the
 * lowest-numbered group that contains it and pulls every later box within `threshold` px (min of the four edge
 * distances, f32) into that group; groups come out in the order the reference opens them.  out_boxes
 * [B,Nmax,Wout]: rows 0..out_counts[b]-1 of image b are written.  rounds_dev (int32 [B], may be NULL) receives the
 * label-relaxation rounds each image took.  JN_EINVAL: Nmax > 4096 (no launch is made), another W.  Inputs are finite. */
int jn_merge_boxes(const float* boxes_dev, const int32_t* counts_dev, int B, int Nmax, int W, int target, float threshold,
                   float* out_boxes_dev, int32_t* out_counts_dev, int32_t* rounds_dev, void* stream);
/* The detector's training loss on given predictor outputs, context-free: the published YOLOX head's get_losses for one
 * class (called at src/models/yolox.py:58-73 with use_l1 = True; restated in oracle/yolox_ref.py::losses_from_raw) as
 * jn_detector_step / jn_detector_forward run it after the head, without a network around it.  raw_dev [N,A,6] f32 (reg 4,
 * obj logit, cls logit; anchors level by level, row-major), targets_dev [N,nb,5] f32 = (class, x1, y1, x2, y2) in patch
 * pixels, zero rows = padding (converted to cxcywh on the device as the training pass does).  The patch is P x P with
 * levels of stride0 < stride1 < stride2: level l holds (P / stride_l)^2 anchors, A is their sum.  Outputs: d_raw_dev
 * [N,A,6] = d loss / d raw before the 1 / max(num_fg, 1) factor, metrics_dev f32[8] as for jn_detector_step, scale_dev
 * f32[1] = loss_scale / max(num_fg, 1), the factor the predictor backward applies to d_raw.  At most 8 boxes per patch
 * (see jn_detector_step).  Allocates its scratch and waits for `stream`: an entry for tests and diagnostics, not part of
 * a training step.  JN_EINVAL: a null pointer, N < 1, nb < 1, P not a multiple of 32 or of a stride. */
int jn_yolox_loss(const float* raw_dev, const float* targets_dev, int N, int nb, int P, int stride0, int stride1,
                  int stride2, int use_l1, float loss_scale, float* d_raw_dev, float* metrics_dev, float* scale_dev,
                  void* stream);
/* jn_yolox_loss over EVERY box of a patch: same arguments, same outputs, always the wide kernel (for any nb >= 1), so
 * a patch may hold up to nb boxes and none is cut.  JN_EINVAL in addition, before anything is launched: nb >
 * JN_DETLOSS_MAX_BOXES, A > 8400 (P above 640 at strides 8 / 16 / 32).  Two calls on the same input give the same bits. */
int jn_yolox_loss_wide(const float* raw_dev, const float* targets_dev, int N, int nb, int P, int stride0, int stride1,
                       int stride2, int use_l1, float loss_scale, float* d_raw_dev, float* metrics_dev, float* scale_dev,
                       void* stream);
/* The detector's threshold / sort / NMS stage on given decoded predictions, context-free: what jn_detect runs behind
 * the head (the published postprocess with class_agnostic = True and one class, then clamp_(0, P - 1);
 * src/models/yolox.py:80-113, restated in oracle/yolox_ref.py::postprocess).  raw_dev [N,A,6] f32 = decoded rows
 * (cx, cy, w, h, obj, cls), which is what jn_detect hands back as raw_dev; A is free.  Per patch: keep the anchors with
 * obj * cls >= conf_threshold, order them by score descending (ties to the lower anchor index), greedy NMS (a box is
 * suppressed when its IoU with a kept box is > nms_threshold), clamp the edges to [0, clamp_max] AFTER the NMS.  Two
 * silent caps: only the first 2048 passing anchors in index order enter the sort, and only the first max_out survivors
 * in score order are written.  boxes_dev [N,max_out,7] = (x1, y1, x2, y2, obj, cls, 0) and counts_dev int32 [N] exactly
 * as jn_detect writes them; rows at or beyond counts[n] are left alone.  stats_dev (int32 [N,2], may be NULL): column 0
 * = the anchors with score >= conf_threshold before the 2048 cap, column 1 = the NMS survivors before max_out; a caller
 * sees a cap was reached from stats[n][0] > 2048 or stats[n][1] > max_out.  Launches on `stream` and does not wait.
 * Inputs are finite with w, h >= 0.  JN_EINVAL: a null raw / boxes / counts, N < 1, A < 1, max_out < 1.
 * jn_postprocess_all is the same stage without the first cap. */
int jn_postprocess(const float* raw_dev, int N, int A, float conf_threshold, float nms_threshold, float clamp_max,
                   int max_out, float* boxes_dev, int32_t* counts_dev, int32_t* stats_dev, void* stream);
/* jn_postprocess under the candidate policy "all": EVERY anchor with obj * cls >= conf_threshold enters the sort, so
 * the result is the published postprocess (which has no candidate cap) cut to max_out rows; everything else, the
 * arguments, the outputs, stats_dev and the launch contract, is as in jn_postprocess, and for A <= 2048 the two give the
 * same bytes.  One workgroup per patch holds the candidates in LDS, hence A <= 8400 (640 px at strides 8 / 16 / 32).
 * JN_EINVAL: as jn_postprocess, and A > 8400 (nothing is launched). */
int jn_postprocess_all(const float* raw_dev, int N, int A, float conf_threshold, float nms_threshold, float clamp_max,
                       int max_out, float* boxes_dev, int32_t* counts_dev, int32_t* stats_dev, void* stream);
/* The metrics of one teacher-forced validation batch on given logits, context-free: SupervisedTrainer.compute_metrics
 * (src/supervised.py:162-197) on the labels eval_supervised forms (:449-458).  logits_dev [B,T,nA] f32, current_actions /
 * next_actions [B,T] int64, masks u8 [B,T] (1 = token, 0 = padding).  Labels: next_actions; with on_self_trajectory != 0
 * (config.loss_mode == "on-self-trajectory") label(b,t) = next[b,t] at t = n_b - 1, n_b = the row's mask sum (n_b = 0
 * addresses column T - 1, as Python's index -1 does); elsewhere current[b,t+1] for t < T - 1 and 0 in the last column
 * (current_actions may be NULL otherwise).  Per token CrossEntropy(weight[STOP = 8] = stop_weight, reduction none);
 * metrics_dev f32[4] = action_loss (plain mean over the tokens with mask == 1, not weight-normalised), action_accuracy
 * over the same tokens (argmax, first maximum wins), episode_length (mean row sum of masks), the number of valid tokens.
 * No valid token: action_loss NaN (torch's mean of nothing) and action_accuracy 0 (the reference replaces that NaN,
 * :188-195).  Optional outputs: token_loss_out_dev f32 [B,T], predicted_out_dev u8 [B,T]; padding tokens get 0 / 0.
 * One workgroup, sums in a fixed order without atomics: two calls give equal bits.  Launches on `stream`, does not wait.
 * JN_EINVAL: a null logits / next_actions / masks / metrics, B, T or nA < 1, nA > 256. */
int jn_supervised_metrics(const float* logits_dev, const int64_t* current_actions_dev, const int64_t* next_actions_dev,
                          const uint8_t* masks_dev, int B, int T, int nA, float stop_weight, int on_self_trajectory,
                          float* token_loss_out_dev, uint8_t* predicted_out_dev, float* metrics_dev, void* stream);
/* The per-image half of mAP-50 as Trainer.compute_detection_metrics reports it (src/trainer.py:188-248; COCO
 * protocol, one class): preds [B,Nmax,W >= 5] f32 with score in column 4 and pred_counts int32 [B]; targets
 * [B,Mmax,5] f32 (cls,x1,y1,x2,y2) with target_counts int32 [B] (Mmax = 0: no targets, both may be NULL).  Per image
 * the max_det best predictions by score (ties to the lower index) are matched in that order to the untaken target of
 * highest IoU >= 0.5 (f64, ties to the higher index).  Outputs [B,max_det]: scores f64, hits int32, sel int32 (the
 * chosen row), valid up to n_pred[b] = min(count, max_det); n_gt[b] = the image's targets.  JN_EINVAL: Nmax or
 * Mmax > 4096. */
int jn_match_detections(const float* preds_dev, const int32_t* pred_counts_dev, int B, int Nmax, int W,
                        const float* targets_dev, const int32_t* target_counts_dev, int Mmax, int max_det,
                        double* scores_dev, int32_t* hits_dev, int32_t* sel_dev, int32_t* n_pred_dev, int32_t* n_gt_dev,
                        void* stream);
/* The average-precision half (same reference site): from jn_match_detections' outputs, out f64 [B] = the AP of every
 * image on its own (pooled = 0), or out f64 [1] = the AP of all B images' lists concatenated in image order
 * (pooled = 1).  Score order descending, ties in concatenation order; precision made monotone from the right and
 * sampled at thresholds_dev (f64 [n_thresholds], the caller's linspace(0, 1, 101)), summed in threshold order.  No
 * target or no prediction in a segment gives 0.  JN_EINVAL: a segment of more than 8192 slots (B * max_det when
 * pooled, else max_det), n_thresholds outside 1..256. */
int jn_average_precision(const double* scores_dev, const int32_t* hits_dev, const int32_t* n_pred_dev,
                         const int32_t* n_gt_dev, int B, int max_det, int pooled, const double* thresholds_dev,
                         int n_thresholds, double* out_dev, void* stream);
/* jn_average_precision over arbitrary runs of units: jn_match_detections' outputs over U units and seg_offsets int32
 * [NS+1] (device); segment s is the units seg_offsets[s] .. seg_offsets[s+1]-1 concatenated in unit order, out f64 [NS].
 * Same arithmetic as jn_average_precision (one segment over all units equals pooled = 1 bit for bit); n_gt of a segment
 * is the sum over its units; no target or no prediction gives 0.  max_units is the caller's bound on the units of a
 * segment (the offsets stay on the device): JN_EINVAL when max_units * max_det > 8192, and a longer segment is cut to
 * max_units.  The reference's per-image value of the multistart evaluation is one MeanAveragePrecision over that
 * image's patches (src/supervised.py:203-277). */
int jn_average_precision_segments(const double* scores_dev, const int32_t* hits_dev, const int32_t* n_pred_dev,
                                  const int32_t* n_gt_dev, int U, int max_det, const int32_t* seg_offsets_dev, int NS,
                                  int max_units, const double* thresholds_dev, int n_thresholds, double* out_dev, void* stream);
/* The pooling of the multistart evaluation (metrics_from_multiple_samples / eval_missing_patches,
 * src/supervised.py:573-625), context-free, on what a rollout of A walks leaves on the device: det_boxes f32
 * [A,T+1,K_det,7] (patch-local pixels), det_counts int32 [A,T+1], positions int64 [A,T+1,2] (y,x); tokens 0..S of a
 * walk are read (S <= T), of which walk a owns the first walk_tokens[a] (int32 [A], its own steps + 1).  Image i uses
 * the walks walk_first[i] .. walk_first[i]+walk_count[i]-1 (int32 [NI] each; one launch per n_starts prefix needs no
 * repacking).  Cell c = y*Gw + x of image i is visited when a token of a used walk stands on it (visited u8
 * [NI,Gh*Gw]); its pool is the boxes of every such token in (walk, token, stored) order, a walk that returns to a cell
 * contributing again.  Greedy NMS in (column 4 descending, pool index ascending) order: a box is suppressed when its
 * IoU with a kept box is > 0.5, the IoU in f32 with every operation rounded once (w = max(min(x2) - max(x1), 0),
 * likewise h, inter = w*h, iou = inter / ((area_a + area_b) - inter)); a NaN IoU suppresses nothing.  The survivors go
 * in that order to cell_boxes f32 [NI,Gh*Gw,max_per_cell,7], cell_counts int32 = min(survivors, max_per_cell) (0 on
 * an unvisited cell), rows beyond the count are left alone; cell_stats (int32 [NI,Gh*Gw,2], may be NULL) = pool size
 * and survivors before that cut.  max_walks is the caller's bound on walk_count.  JN_EINVAL, before any launch:
 * max_walks*(S+1)*K_det > 4096, max_per_cell < 1, NI < 1, a null pointer. */
int jn_pool_walk_detections(const float* det_boxes_dev, const int32_t* det_counts_dev, const int64_t* positions_dev,
                            const int32_t* walk_tokens_dev, const int32_t* walk_first_dev, const int32_t* walk_count_dev, int A,
                            int T, int S, int K_det, int NI, int max_walks, int Gh, int Gw, int max_per_cell,
                            float* cell_boxes_dev, int32_t* cell_counts_dev, int32_t* cell_stats_dev, uint8_t* visited_dev,
                            void* stream);
/* Context-free indexed gather through a DEVICE table of n_views views (all of one element type, already valid):
 * out[n] = canvas[image_index[n]][:, y*P:(y+1)*P, x*P:(x+1)*P], image_index[n] < 0 = zero patch.  out_u8 = 0:
 * out is f32 (bytes as b / 255); out_u8 = 1: u8 sources only, out is the transformed byte copy. */
int jn_gather_patches_views(const jn_image_view* views_dev, int n_views, const int64_t* image_index_dev,
                            const int64_t* positions_dev, void* out_dev, int out_u8, int N, int Hc, int Wc, int P,
                            void* stream);

/* ---- detection augmentation ------------------------------------- */
/* Trainer.init_detection's on-device chain (src/trainer.py:176-186, applied at src/reinforce.py:332-333 and
 * src/supervised.py:855-861, 884-885) fused into one pass: RandomPlanckianJitter (per-patch red / blue gains,
 * clamp to [0,1]) -> RandomGrayscale -> RandomGaussianBlur 3x3 (reflect border) -> RandomPlasmaShadow (shade where a
 * value-noise fractal of the patch falls below `quantity`: kornia's diamond-square map restated as a counter-based
 * fractal, csrc/kernels_aug.hip) -> RandomGaussianNoise -> RandomMotionBlur 3x3 (zero border).  patches [N,3,P,P]
 * f32 -> out (must not alias); params [N,JN_AUG_NPARAM] f32 per patch = r_gain, b_gain, gray flag, Gaussian centre
 * weight, Gaussian side weight, noise std, motion kernel k[3][3] row-major, shade intensity, shade quantity,
 * roughness, fractal stretch, pad; an op a patch did not draw is encoded as the identity
 * (1, 1, 0, 1, 0, 0, delta, 0, ...).  noise_dev: optional [N,3,P,P]
 * standard-normal field (parity runs); NULL = counter-based generator seeded by `seed`. */
#define JN_AUG_NPARAM 20
int jn_augment_patches(const float* in_dev, float* out_dev, const float* params_dev, const float* noise_dev,
                       uint64_t seed, int N, int P, void* stream);

/* ---- networks ------------------------------------------------------------------- */
/* YOLOPAFPN.forward as called at src/models/gpt.py:375 / src/models/yolox.py:55 "with the
 * current mode of the model": train = 0 uses the BatchNorm running statistics, train != 0
 * the batch statistics of these N patches (and updates the running statistics, momentum
 * 0.03).  patches [N,3,P,P] f32 NCHW; fpn outputs NCHW f32 ([N,c,P/8,P/8], /16, /32), any
 * may be NULL. */
int jn_backbone_forward(jn_ctx* ctx, int net, const float* patches_dev, int N, int train,
                        float* fpn0_dev, float* fpn1_dev, float* fpn2_dev, void* stream);
/* Reads back a tensor the engine mutates (BatchNorm "<prefix>.bn.running_mean" / "running_var")
 * into host memory, so state_dict() of the owning module stays current.  Synchronises. */
int jn_read_tensor(jn_ctx* ctx, const char* name, float* host_out, size_t numel);
/* GPT.embed_patches (src/models/gpt.py:356-384): patches [N,3,P,P] -> [N, n_embd]. */
int jn_embed_patches(jn_ctx* ctx, const float* patches_dev, int N, float* out_dev, void* stream);
/* ---- training (loss.backward() / optimizer of src/reinforce.py:341-353) ---------------------- */
/* optimizer.zero_grad(): clears the flat gradient arena. */
int jn_zero_grad(jn_ctx* ctx, void* stream);
/* Backward of the most recent train-mode jn_backbone_forward(net, patches, N, train=1): g*_dev are
 * dL/d(fpn outputs), NCHW f32.  NULL = no gradient arrives in that output from outside the network
 * (numerically a zero gradient; the backward then takes the routes of the training backward, which
 * feeds fpn[2] only).  Parameter gradients (conv weights, BN weight/bias) are ACCUMULATED into the
 * gradient arena (read with jn_read_grad). */
int jn_backbone_backward(jn_ctx* ctx, int net, const float* patches_dev, int N, const float* g0_dev,
                         const float* g1_dev, const float* g2_dev, void* stream);
/* Options of one REINFORCE iteration (src/reinforce.py:217-265, 341). */
typedef struct jn_train_opts {
  int32_t struct_size;
  int32_t reward_norm;      /* config.reward_norm: advantages = (returns - mean) / (std + 1e-8)      */
  float ret_mean, ret_std;  /* last_return_mean / last_return_std of the previous optimiser window */
  float entropy_weight;     /* --entropy-weight                                                      */
  float loss_scale;         /* 1 / gradient_accumulation                                             */
} jn_train_opts;

/* One REINFORCE iteration minus the optimiser (src/reinforce.py:326-341): train-mode rollout
 * (batch-statistics BatchNorm per glimpse step, running statistics updated), loss + metrics, and
 * loss.backward() into the gradient arena (accumulating).  metrics_dev[8] = action_loss,
 * entropy_loss, loss, returns, episode_length, steps.  Synchronises once (to read the step count). */
int jn_reinforce_step(jn_ctx* ctx, int mode, const int64_t* forced_actions_dev,
                      const int64_t* start_positions_dev, uint64_t seed, int stop_early,
                      const jn_train_opts* opts, const jn_rollout_out* out, float* metrics_dev, void* stream);
/* Autograd bridge (SURVEY.md 8b "Ownership": in training, rollout's logprobs / entropies carry a graph).  The reference
 * differentiates a loss built from the rollout dict (src/reinforce.py:326-341: rollout -> compute_metrics ->
 * (loss / ga).backward()).  jn_reinforce_forward is the train-mode rollout alone (batch-statistics BatchNorm, every
 * step's activations kept resident, or a ring of them under jn_set_activation_slots); jn_reinforce_backward is the backward of that rollout for GIVEN d loss / d logprobs
 * and d loss / d entropies ([B, T] f32, either may be NULL = zero): what a torch.autograd.Function around the rollout
 * receives.  Parameter gradients ACCUMULATE in the gradient arena.  jn_reinforce_backward synchronises once (step count). */
int jn_reinforce_forward(jn_ctx* ctx, int mode, const int64_t* forced_actions_dev, const int64_t* start_positions_dev,
                         uint64_t seed, int stop_early, const jn_rollout_out* out, void* stream);
int jn_reinforce_backward(jn_ctx* ctx, const float* dlogprobs_dev, const float* dentropies_dev, void* stream);
/* Walks that do not fit: activation replay (opt-in).  By default a train-mode rollout of the patch encoder keeps one full
 * workspace slot per glimpse step (activations of every layer at max_batch) until its backward.  With n >= 1 it keeps a
 * ring of n activation slots besides slot 0 and only the small per-step state of every step (BatchNorm tables, saved
 * mean / invstd, fp64 batch sums, the staged view columns, embed_fpn's activations); the backward walks the trajectory in
 * chunks of min(n, gradient slots) steps and re-runs the forward of a chunk from the kept statistics, bit for bit, just
 * before that chunk's backward (no BatchNorm finalize, no running-statistics update: those happened once, in the
 * rollout).  n = 0 (default): one activation slot per step, nothing is replayed.  A rollout of T <= n steps takes the
 * default path unchanged.  n < 0: JN_EINVAL.  The setter makes the state of an earlier train-mode rollout stale:
 * jn_reinforce_backward after it fails with JN_ESTATE until a new jn_reinforce_forward / jn_reinforce_step has run.  With a
 * detached encoder (no gpt_backbone: the detector's PAFPN encodes the patches and gets no policy gradient) there is no
 * encoder backward: the switch is accepted and has no effect.  The supervised step (one slot of B*T patches) is not
 * covered. */
int jn_set_activation_slots(jn_ctx* ctx, int n);
/* What a net's workspace holds now: activation slots and table slots (equal unless a ring is in use), the bytes of one
 * activation slot at max_batch, and how many glimpse steps the most recent REINFORCE backward replayed (0 for a net
 * that is not the patch encoder).  Any output may be NULL. */
int jn_activation_slots_info(const jn_ctx* ctx, int net, int* act_slots, int* table_slots, size_t* slot_bytes, int* replayed_steps);
/* The chunks in which the encoder's backward walks S executed glimpse steps, in the order it runs them (host rule, no
 * device; the backward itself calls it): chunk i covers steps t0[i] .. t0[i] + n[i] - 1, every chunk has min(act_slots,
 * g_slots) steps and the last one the rest.  act_slots = 0: every step is resident, chunks of g_slots steps, no replay.
 * Writes at most `cap` chunks and returns their number (which may exceed cap); JN_EINVAL: S < 0, act_slots < 0,
 * g_slots < 1. */
int jn_replay_chunks(int S, int act_slots, int g_slots, int* t0, int* n, int cap);
/* Debug entry of the replay: after a train-mode rollout under n = 0 (every step resident) re-runs glimpse step `step`
 * (< the executed steps) into activation slot 0 and counts the 32-bit words, over the first B patches of every buffer of
 * the patch encoder, in which the replay differs from the resident slot of that step: *n_diff, 0 = bit for bit.
 * Overwrites the eval workspace (a pending jn_supervised_backward is refused afterwards).  Synchronises. */
int jn_debug_replay_diff(jn_ctx* ctx, int step, long long* n_diff, void* stream);
/* The arena keeps tensors in kernel-friendly layouts (transposed Linear weights, tap-major conv weights, ...).  These
 * convert, ON THE DEVICE, between the arena and a caller-owned buffer of >= arena floats that holds every trainable
 * tensor in the reference's (PyTorch) layout at the SAME offset as in the arena (jn_arena_segment): the Python module's
 * param.data / param.grad are views of such buffers, so torch code (clip_grad_value_, an optimizer's state, a
 * state_dict) sees real tensors.  what = 0 parameters, 1 gradients, 2 / 3 AdamW exp_avg / exp_avg_sq (the optimiser
 * state of a checkpoint, torch.optim.AdamW.state_dict() layout per tensor).  export: arena -> buffer (accumulate != 0:
 * +=); import: buffer -> arena. */
int jn_arena_segment(jn_ctx* ctx, const char* name, size_t* off, size_t* numel);
int jn_export_arena(jn_ctx* ctx, int what, float* dst_dev, size_t numel, int accumulate, void* stream);
int jn_import_arena(jn_ctx* ctx, int what, const float* src_dev, size_t numel, void* stream);

/* --dropout (main.py:123-128 -> embd_pdrop = attn_pdrop = resid_pdrop, src/models/gpt.py:178-179): active in the
 * train-mode passes only (jn_reinforce_step / _forward, jn_supervised_step); eval entry points never drop.  The keep mask
 * of an element is a pure function of (seed + number of train-mode forwards since this call, agent, token, layer, site,
 * index) — Philox4x32-10, jn_device.h drop_scale — so the teacher-forced backward regenerates it and nothing is stored.
 * Deviation from the reference: a token's masks are drawn once, when the token is processed (KV cache),
 * whereas the reference re-draws the masks of the whole prefix at every glimpse step. */
int jn_set_dropout(jn_ctx* ctx, float p, uint64_t seed);
/* --freeze-image-processor (src/models/gpt.py:264-268: requires_grad = False on yolox.backbone.*): the optim_yolox
 * group (jn_optimizer_step_group(1)) then updates the detection head only. */
int jn_set_freeze(jn_ctx* ctx, int freeze_detector_backbone);
/* AdamW step counter of a parameter group (bias correction): read (set = 0) or restore (set != 0) — the "step" entry of
 * a torch optimizer state_dict, so that a resumed run continues where the checkpoint stopped. */
int jn_optimizer_steps(jn_ctx* ctx, int group, int* steps, int set);

/* One supervised (teacher-forced) step minus the optimiser: SupervisedTrainer.run body
 * (src/supervised.py:863-902) with the detector term off.  patches [B,T,3,P,P], current_actions /
 * next_actions [B,T] int64, classes [B] int64 (src/supervised.py:852, 866; NULL = class 0), positions [B,T,2] int64,
 * masks [B,T] u8 (1 = token, 0 = padding); B*T <=
 * max_batch.  GPT.forward runs on the full sequence in train mode (BatchNorm statistics over the B*T
 * patches), loss = CrossEntropy(weight[STOP] = stop_weight, reduction none) averaged over non-padding
 * tokens (:138-177); gradients ACCUMULATE in the arena.  logits_out_dev [B,T,n_actions] optional;
 * metrics_dev[4] = action_loss, action_accuracy, episode_length. */
int jn_supervised_step(jn_ctx* ctx, const float* patches_dev, const int64_t* current_actions_dev,
                       const int64_t* next_actions_dev, const int64_t* classes_dev, const int64_t* positions_dev,
                       const uint8_t* masks_dev, int B, int T, float stop_weight, float* logits_out_dev,
                       float* metrics_dev, void* stream);
/* Supervised autograd bridge — the two halves of jn_supervised_step around the CALLER's loss, so that the reference's
 * supervised loop runs unchanged (src/supervised.py:863-868: `action_logits, embeddings = model(patches, current_actions,
 * classes=classes, positions=positions)`, then :138-177 its cross-entropy, then :897 `loss.backward()`):
 * jn_supervised_forward = GPT.forward (src/models/gpt.py:481-534, full-sequence, train mode: BatchNorm statistics over
 * the B*T patches, running statistics updated, dropout) -> logits_out_dev [B,T,n_actions], final_emb_out_dev [B,T+1,C]
 * (optional); jn_supervised_backward = the backward of that forward for GIVEN d loss / d logits [B,T,n_actions],
 * gradients ACCUMULATE in the arena (the class token's gradient goes to row classes[b] of embed_class).  patches /
 * actions / classes / positions must stay alive until the backward; any pass over
 * the patch encoder in between makes the saved activations stale and the backward fails with JN_ESTATE. */
int jn_supervised_forward(jn_ctx* ctx, const float* patches_dev, const int64_t* current_actions_dev,
                          const int64_t* classes_dev, const int64_t* positions_dev, int B, int T, float* logits_out_dev,
                          float* final_emb_out_dev, void* stream);
int jn_supervised_backward(jn_ctx* ctx, const float* dlogits_dev, void* stream);
/* Which backward differentiates the decision transformer over a sequence of T glimpse steps (T + 1 tokens): host only, no
 * device call.  decision_route: jn_debug_decision_route of the context (0 per agent, 1 wide).  Returns 0 = none (every
 * training entry point refuses that length with JN_EINVAL), 1 = the batched backward with a head's attention tiles in LDS
 * (4 (T + 1) head_size + 2 (T + 1)^2 <= 16384 floats), 2 = the one-workgroup-per-agent kernel (per-agent route, T <= 62),
 * 3 = the batched backward with the tiled attention kernels (per-agent route, head_size <= 256, T <= 255).  The rule takes
 * the first of 1, (wide: 0), 2, 3 that admits the shape; the test hook JN_GPT_BWD_TILED=1 sends a per-agent-route shape of 1
 * or 2 to 3.  JN_EINVAL: decision_route not 0 or 1. */
int jn_gpt_backward_route(int C, int n_head, int T, int decision_route);
/* Debug entry, context-free: ONE layer's causal attention of the batched GPT backward on caller tensors — the recompute
 * (probabilities into ATT_dev [B * n_head][Lm][Lm], Y_dev [B][Lm][C] = drop(P) . V), then its backward dQKV_dev [B][Lm][3 C]
 * from dY_dev [B][Lm][C] — enqueued on `stream` (no wait).  QKV_dev [B][Lm][3 C] holds q, k, v of token (b, i) side by side,
 * head h in columns h * head_size ...; L <= Lm is the number of live tokens (stop-early): rows >= L of ATT, Y and dQKV are
 * left as they are.  Attention dropout pdrop with the key (seed, b, i, layer, 1, h * Tmax + j), Tmax >= Lm.  form 0 = the
 * LDS kernels, 1 = the tiled kernels (Lm <= 256, head_size <= 256).  The call keeps a workspace per device between calls
 * (the tiled form's dS, of ATT's shape), so calls on one device are for one stream at a time.  JN_EINVAL: a null pointer,
 * a size out of range, or a form that does not take the shape. */
int jn_gpt_attention_backward(int form, const float* QKV_dev, const float* dY_dev, int B, int n_head, int C, int Lm, int L,
                              float pdrop, uint64_t seed, int layer, int Tmax, float* ATT_dev, float* Y_dev, float* dQKV_dev,
                              void* stream);
/* The eval-mode twin of jn_supervised_step — one batch of SupervisedTrainer.eval_supervised (src/supervised.py:431-472,
 * under model.eval() and no_grad): GPT.forward on the teacher's sequences with BatchNorm running statistics and no
 * dropout, then jn_supervised_metrics on the logits.  Same tensors as jn_supervised_step; on_self_trajectory selects the
 * labels of :449-456.  Touches no statistic, weight or gradient and needs no training state; works in both activation
 * dtypes.  The encoder takes the B*T patches in flattened (b t) order in chunks of at most max_batch (ceil(B*T /
 * max_batch) conv-stack passes, where jn_gpt_forward makes T of B patches each); then the full-sequence decode over
 * T + 1 tokens (1-D positions 0..T-1, class token from `classes`).  B <= max_batch, T <= block_size; B*T is free.
 * Optional outputs: logits_out_dev [B,T,n_actions], token_loss_out_dev f32 [B,T], predicted_out_dev u8 [B,T];
 * metrics_dev f32[4] as jn_supervised_metrics.  All on `stream`, no synchronisation.  Like every eval pass it uses the
 * encoder's workspace slot 0: a pending jn_supervised_backward then fails with JN_ESTATE. */
int jn_supervised_eval(jn_ctx* ctx, const float* patches_dev, const int64_t* current_actions_dev,
                       const int64_t* next_actions_dev, const int64_t* classes_dev, const int64_t* positions_dev,
                       const uint8_t* masks_dev, int B, int T, float stop_weight, int on_self_trajectory,
                       float* logits_out_dev, float* token_loss_out_dev, uint8_t* predicted_out_dev, float* metrics_dev,
                       void* stream);
/* clip_grad_value_(clip_value) + AdamW (torch defaults) over the optim_gpt parameters
 * (src/reinforce.py:344-346, src/models/gpt.py:552-557); grad_scale multiplies the gradients first
 * (1/world_size after a SUM all-reduce). */
int jn_optimizer_step(jn_ctx* ctx, float lr, float weight_decay, float clip_value, float grad_scale, void* stream);
/* Sizes of the flat parameter/gradient arena (floats): whole arena, and its optim_gpt prefix. */
int jn_arena_info(jn_ctx* ctx, size_t* total_numel, size_t* optim_gpt_numel);
/* Use caller-owned device memory (>= arena floats, zeroed) as the gradient arena, e.g. a torch
 * tensor that is handed to one RCCL all-reduce per optimiser step. */
int jn_set_grad_arena(jn_ctx* ctx, float* grads_dev, size_t numel);
/* Current value of a trainable state-dict entry (reference layout) to host memory.  Synchronises. */
int jn_read_param(jn_ctx* ctx, const char* name, float* host_out, size_t numel);
/* param.grad of a trainable state-dict entry, in the reference's (PyTorch) layout, to host memory.
 * Synchronises. */
int jn_read_grad(jn_ctx* ctx, const char* name, float* host_out, size_t numel);

/* GPT.forward (src/models/gpt.py:481-534), eval mode.  patches [B,T,3,P,P] f32 (NULL with
 * no_patch_emb), actions [B,T] int64, positions [B,T,2] int64 (y,x; NULL unless use_pos_emb),
 * classes [B] int64 = row of embed_class behind every agent's class token (gpt.py:476-478; NULL = class 0, ids are
 * clamped to the table's 100 rows), prev_embeddings [B,Tp,C] or NULL.  Without prev_embeddings all T tokens are embedded
 * (1-D positions 0..T-1); with it only the last one is (1-D position 0, the reference's
 * recurrent quirk gpt.py:431-449) and appended.  L = prev ? Tp+1 : T+1.
 * Outputs: logits [B, L-1, n_actions], final_emb [B, L, n_embd] (either may be NULL). */
int jn_gpt_forward(jn_ctx* ctx, const float* patches_dev, const int64_t* actions_dev, const int64_t* classes_dev,
                   const int64_t* positions_dev, const float* prev_emb_dev, int B, int T, int Tp,
                   float* logits_dev, float* final_emb_dev, void* stream);
/* NeedleYOLOX.forward inference branch (src/models/yolox.py:24-57, 74-113): boxes
 * [N, max_det_per_patch, 7] (x1,y1,x2,y2,obj,cls,cls_id; clamped to [0,P-1]) + counts [N];
 * raw_dev optional [N, A, 6] decoded head output before postprocess. */
int jn_detect(jn_ctx* ctx, const float* patches_dev, int N, float* boxes_dev,
              int32_t* counts_dev, float* raw_dev, void* stream);
/* Candidate policy of the detector's threshold / sort / NMS stage wherever `ctx` runs it: jn_detect and the rollout's
 * do_detection, the eval head of jn_detector_forward, jn_detector_eval_loss.  all = 0 (the default): the first 2048
 * passing anchors in index order enter the sort (jn_postprocess).  all != 0: every passing anchor does
 * (jn_postprocess_all), which is the published postprocess up to max_det_per_patch.  Sticky until set again.
 * JN_ESTATE: the context has no detector.  JN_EINVAL: all != 0 and the detector has more than 8400 anchors (a patch
 * size above 640). */
int jn_set_det_candidates(jn_ctx* ctx, int all);

/* One training step of the detector minus the optimiser: NeedleYOLOX.forward(patches, targets) loss branch
 * (src/models/yolox.py:58-73) + loss.backward() (src/reinforce.py:336-341).  PAFPN + head forward with
 * batch-statistics BatchNorm on N patches, SimOTA assignment + IoU / objectness / class / L1 losses (YOLOX head,
 * use_l1 = True), backward; gradients are ACCUMULATED into the gradient arena (yolox.* parameters).
 * targets_dev: [N, nb, 5] float32 = (class id, x1, y1, x2, y2) in patch pixels, zero rows = padding
 * (NeedleGeneralEnv.get_detection_batch layout).  loss_scale multiplies the loss before backward
 * (1 / gradient_accumulation).  metrics_dev: float32[8] = total_loss, iou_loss (x5), conf_loss, cls_loss, l1_loss,
 * num_fg (foreground anchors per ground-truth box).
 * Box cap: a patch's boxes are its first ng rows, ng = the number of rows with a positive sum (as published).  Two
 * policies, chosen by jn_set_det_loss_boxes:
 * - the default (all = 0): the loss kernel holds 8 boxes in LDS, and a patch with ng > 8 is cut to its first 8 rows
 *   WITHOUT an error (the reference uses them all; num_fg then counts 8).  nb > 8 is accepted and exact as long as no
 *   patch has more than 8 such rows.  The Python wrappers refuse such a batch (ValueError); a C caller checks its own
 *   targets.  jn_yolox_loss is this policy.
 * - all != 0: every box is used, as the reference does.  A call with nb > 8 runs the wide kernel (jn_yolox_loss_wide),
 *   which has no cap: nothing is ever cut.  Its capacity is checked before anything is launched: nb >
 *   JN_DETLOSS_MAX_BOXES is JN_EINVAL.  A call with nb <= 8 runs the default kernel, which cannot cut it.
 * Holds for jn_detector_forward and jn_detector_eval_loss too. */
int jn_detector_step(jn_ctx* ctx, const float* patches_dev, int N, const float* targets_dev, int nb,
                     float loss_scale, float* metrics_dev, void* stream);
/* Rows of `targets` the wide detector loss accepts per patch (its boxes and candidate lists share 160 KB of LDS). */
#define JN_DETLOSS_MAX_BOXES 1024
/* Box policy of the detector loss wherever `ctx` computes it: jn_detector_step, jn_detector_forward,
 * jn_detector_eval_loss.  all = 0 (the default): at most 8 boxes per patch, see jn_detector_step.  all != 0: every box
 * of a patch takes part in the SimOTA assignment, which is the published loss.  Sticky until set again.  JN_ESTATE: the
 * context has no detector.  JN_EINVAL: all != 0 and the detector has more than 8400 anchors (a patch size above 640). */
int jn_set_det_loss_boxes(jn_ctx* ctx, int all);
/* Detector autograd bridge — NeedleYOLOX.forward(patches, targets) (src/models/yolox.py:24-91) as the two halves of
 * jn_detector_step around the CALLER's autograd, so that the reference's loop runs as written (src/reinforce.py:330-341:
 * `_, _, yolo_loss = yolox(patches_yolox, bboxes_yolox); loss += yolo_loss["total_loss"]; (loss / ga).backward()`; the
 * same in src/supervised.py:881-897).
 * jn_detector_forward: PAFPN + head in train mode on N <= max_batch patches (batch-statistics BatchNorm, running
 * statistics updated), SimOTA loss -> metrics_dev float32[8] as above.  The activations and d loss / d raw stay resident
 * as pass `pass` of `n_pass` (a detection batch above max_batch is fed in n_pass chunks, each with its own workspace
 * slot; pass 0 sizes the workspace for n_pass) until jn_detector_backward(pass).  Optional outputs of the rest of the
 * reference's forward: boxes_dev [N, max_det_per_patch, 7] + counts_dev [N] = the EVAL-mode head on the train-mode FPN
 * maps, postprocessed and clamped (yolox.py:74-91; both NULL: skipped), fpn{0,1,2}_dev = fpn_outs [N, C_i, H_i, W_i]
 * (activated, NCHW; NULL: skipped).  patches_dev must stay alive until the backward.
 * jn_detector_backward: the backward of pass `pass` for d L / d total_loss = dloss_dev[0] (device scalar, what torch hands
 * to the loss node; NULL = 1) times the host factor `scale` (the chunk's share N_pass / N_total of the batch mean);
 * yolox.* gradients ACCUMULATE in the arena.  One backward per forward; a later pass over the same slot or a second
 * backward fails with JN_ESTATE.  Independent of the REINFORCE / supervised bridges: either order of backward calls. */
int jn_detector_forward(jn_ctx* ctx, const float* patches_dev, int N, const float* targets_dev, int nb, int pass,
                        int n_pass, float* metrics_dev, float* boxes_dev, int32_t* counts_dev, float* fpn0_dev,
                        float* fpn1_dev, float* fpn2_dev, void* stream);
int jn_detector_backward(jn_ctx* ctx, int pass, const float* dloss_dev, float scale, void* stream);
/* NeedleYOLOX.forward(patches, targets) as VALIDATION calls it (src/supervised.py:465, under model.eval() and no_grad):
 * the PAFPN runs in the module's current mode — eval, running statistics, none of them written (src/models/yolox.py:54-55)
 * — and only the head goes to train mode for the loss (`self.train()`, yolox.py:62): batch statistics over the N patches,
 * and the head's running statistics move with momentum 0.03 as in any train pass (the reference's behaviour, kept).
 * N <= max_batch, fp32 activations only.  metrics_dev f32[8] as for jn_detector_step.  Optional outputs as in
 * jn_detector_forward: boxes_dev / counts_dev = the eval head on the same maps with the head statistics as just updated,
 * postprocessed and clamped (yolox.py:74-91); fpn{0,1,2}_dev = the eval-mode maps.  Works in the eval workspace, and the
 * next eval pass rebuilds its BatchNorm table.  A detector training pass that is resident (jn_detector_forward without its
 * backward yet) keeps its own workspace slot, which this call does not write: its jn_detector_backward stays valid and
 * gives the same gradient as without the call.  All on `stream`, no synchronisation. */
int jn_detector_eval_loss(jn_ctx* ctx, const float* patches_dev, int N, const float* targets_dev, int nb,
                          float* metrics_dev, float* boxes_dev, int32_t* counts_dev, float* fpn0_dev, float* fpn1_dev,
                          float* fpn2_dev, void* stream);
/* AdamW + clip on one parameter group of the arena: group 0 = optim_gpt (everything but yolox.*,
 * src/models/gpt.py:552-557), group 1 = optim_yolox (yolox.*).  jn_optimizer_step == group 0. */
int jn_optimizer_step_group(jn_ctx* ctx, int group, float lr, float weight_decay, float clip_value,
                            float grad_scale, void* stream);

/* ---- the hot loop ----------------------------------------------------------------- */
/* ReinforceTrainer.rollout (src/reinforce.py:108-215) for the env set by jn_env_init:
 * reset (positions NULL = random from seed), then up to T steps of
 * patch-encode -> GPT decode (KV cache) -> action select -> env step [-> detect],
 * all enqueued on `stream` with no host synchronisation; the returns/logit_masks
 * epilogue (:186-202) runs on device too.  forced_actions [B,T] int64 for JN_MODE_FORCED.
 * stop_early != 0 reproduces the reference's `break` when every env is done (:181-184):
 * later steps become no-ops on device. */
int jn_rollout(jn_ctx* ctx, int mode, const int64_t* forced_actions_dev,
               const int64_t* start_positions_dev, uint64_t seed, int do_detection,
               int stop_early, const jn_rollout_out* out, void* stream);
/* 1-D token positions of the following rollouts.  by_token = 0 (the default): every new token sits at position 0, the
 * recurrent forward of src/models/gpt.py:431-449 that a REINFORCE-trained policy saw.  by_token != 0: the token of
 * step t sits at position t (row t of the sinusoid table with decoder_pos_encoding, else wpe[t]) — the last row of
 * the full-prefix forward (gpt.py:331-354) that --no-recurrent-embedding selects in ReinforceTrainer.rollout
 * (gpt.py:427-428) and that SupervisedTrainer.test_model_on_env runs at every step (src/supervised.py:279-405); exact
 * in eval mode (running BatchNorm statistics, causal attention), everything else in the step unchanged.  Sticky until
 * set again.  While it is set: a rollout with a learned table and max_ep_len > pos_emb_size fails with JN_EINVAL (the
 * reference's nn.Embedding raises there), and jn_reinforce_forward / jn_reinforce_step fail with JN_ESTATE (train mode
 * re-encodes the whole prefix with BatchNorm statistics over B * (t + 1) patches, which one step cannot reproduce). */
int jn_set_rollout_positions(jn_ctx* ctx, int by_token);
/* The teacher's action set of B states, context-free (NeedleSimpleEnv.build_keypoints_trajectory and move_towards,
 * src/env/simple_env.py:590-629, 84-125).  positions_dev int64 [B,2] (y, x); visited_dev, targets_dev uint8
 * [B,Gh,Gw] (non-zero = set).  Per agent: the remaining targets are targets & ~visited, N = those at the minimum
 * Manhattan distance |dy| + |dx|, and sets_dev[b] (uint8 [B]) gets bit a for every action a = move_towards(position,
 * q), q in N, actions 0..7 in the Action order — the set the reference draws one member of with random.choice.  STOP
 * (a remaining target under the agent) sets no bit; no remaining target gives 0.  Launches on `stream`, does not wait.
 * JN_EINVAL: a null pointer, B, Gh or Gw < 1. */
int jn_teacher_actions(const int64_t* positions_dev, const uint8_t* visited_dev, const uint8_t* targets_dev, int B, int Gh,
                       int Gw, uint8_t* sets_dev, void* stream);
/* The teacher's whole walk for a batch of images, context-free: NeedleSimpleEnv.generate_sample_indices
 * (src/env/simple_env.py:481-588) without its patches, with the env's two random sources replaced by counter-based
 * draws (no device path can consume numpy's or Python's streams).  Draw k of a stream of image b is
 * Philox4x32-10(key = seed, counter = (b, k, TAG, 0)).x, k counting from 0 in the order the host code makes its calls:
 *  - stream R (TAG 0x54574B52) for `rng`: integers(lo, hi) = lo + r mod (hi - lo), one draw (n draws with size = n);
 *    choice(n) = r mod n; binomial(n, 1/2) = the set bits among n random bits, ceil(n / 32) draws, draw j supplying bits
 *    32j .. 32j + 31 and the last one only its low n - 32j bits.  In order: the negative detector cell (if the image has
 *    an empty cell), the start (y, x) unless given, the one random keypoint (y, x) when no target is left to visit, the
 *    number of detours in min_keypoints .. max_keypoints, their places, then the detours (y, x; binomial: x before y) and
 *    the STOP replacements as the walk meets them.
 *  - stream Y (TAG 0x54574B59) for the tie choice of build_keypoints_trajectory: keypoint k is element r_k mod len of the
 *    remaining target cells nearest (L1) to the previous keypoint, listed in row-major order; one draw per keypoint.
 * bboxes_dev int64 [B,nb,4] xyxy in pixels, nb >= 0; an all-zero row is padding and is skipped, and column j of both box
 * outputs is the j-th non-zero row (the other columns are zero).  A box's target cells (bbox_positions, :270-321): the
 * cells of its own range (floor division) with 20 * h * w > P * P, which is h * w / P**2 > 0.05, plus its centre's cell;
 * cells outside the Gh x Gw grid are dropped.  start_positions_dev int64 [B,2] (y, x) or NULL; a start outside the grid
 * is the caller's error (the kernel clamps it into the grid).
 * Outputs: positions int64 [B,T,2], current_actions / next_actions / labels int64 [B,T], masks f32 [B,T], local_bboxes
 * f32 [B,T,nb,6] (rows (0, x1, y1, x2, y2, 1) of NeedleSimpleEnv.local_bboxes, :231-268) — the walk's last T steps, zero
 * rows behind a shorter walk; n_steps int32 [B] the walk's length before that cut; targets uint8 [B,Gh,Gw]; offsets int32
 * [B+1], cells int64 [capacity,3] = (image, y, x) and bboxes_yolox f32 [capacity,nb,6]: per image its target cells in
 * row-major order, then the one negative cell, the (first R draw mod n_empty)-th empty cell in row-major order.  Rows
 * >= capacity are not written (offsets still count them), rows >= offsets[B] are left alone; B * Gh * Gw always suffices.
 * Three launches on `stream` (walk: one wave per image; scan; detector rows), no atomics: equal inputs give equal
 * bytes.  Does not wait for the device.  Limits: Gh * Gw <= 4096 (the walk state of an image lives in LDS), T <= 4096
 * (the LDS ring of the last T steps, 8 bytes each), max_keypoints <= 64 (the detour table, one lane per detour).
 * JN_EINVAL, before any launch: B < 0, nb < 0, P < 1, Gh or Gw < 1, Gh * Gw > 4096, T < 1, T > 4096, min_keypoints < 0,
 * max_keypoints < min_keypoints, max_keypoints > 64, capacity < 0, B * Gh * Gw > INT32_MAX, a null pointer (bboxes /
 * local_bboxes / bboxes_yolox may be NULL with nb = 0, cells / bboxes_yolox with capacity 0).  B = 0 writes offsets[0] = 0
 * and launches nothing. */
int jn_teacher_walks(const int64_t* bboxes_dev, const int64_t* start_positions_dev, int B, int nb, int Gh, int Gw, int P,
                     int T, int min_keypoints, int max_keypoints, int binomial_keypoints, uint64_t seed, int capacity,
                     int64_t* positions_dev, int64_t* current_actions_dev, int64_t* next_actions_dev, int64_t* labels_dev,
                     float* masks_dev, float* local_bboxes_dev, int32_t* n_steps_dev, uint8_t* targets_dev,
                     int64_t* cells_dev, float* bboxes_yolox_dev, int32_t* offsets_dev, void* stream);
/* Debug entry, context-free: the fused backward of ONE pointwise (1x1) BatchNorm + SiLU layer over S workspace slots of M
 * pixels each, as the conv-stack backward launches it for the layers with at most 128 channels on either side (cout and
 * cin each 16, 32, 64 or 128).  Per slot s, pixel m, with y = sc * z + sh of the layer's raw output z:
 *   g_z = k * (g * silu'(y) - c1 - (z - mean) * invstd * c2),   gx (=|+=) g_z . w (+ gadd),   gw += g_z^T . a_in,
 * a_in = fl ? silu(sc_in * x + sh_in) : x.  All fp32: g, z [S,M,cout]; x, gx and the optional gadd (NULL: none) [S,M,cin];
 * tab [S,3,cout+cin]: rows sc, sh, fl, the output channels' entries first, then the input channels' (fl of the output
 * is not read); save [S,cout,2] = (mean, invstd); consts [S,cout,3] = (c1, c2, k); w, gw [cout,cin] — gw is added to,
 * over all slots.  accumulate != 0 adds to what gx holds.  route: 0 = the launcher's choice (32-pixel tiles, two
 * workgroups per CU, for 128 input channels and 64 or 128 output channels), 1 = the 64-pixel kernel.  max_wg: 0 = the
 * launcher's rule, else a cap on the workgroups (1: one workgroup walks every tile of every slot).  Allocates its
 * workspace, waits for `stream` and frees it.  JN_EINVAL: a null pointer, S < 1, M < 1, a shape without a fused kernel,
 * route outside 0..1, max_wg < 0. */
int jn_pw_bwd_fused(const float* g_dev, const float* z_dev, const float* x_dev, const float* tab_dev, const float* save_dev,
                    const float* consts_dev, const float* w_dev, const float* gadd_dev, int accumulate, float* gx_dev,
                    float* gw_dev, int S, long long M, int cout, int cin, int route, int max_wg, void* stream);
/* Debug entries, context-free: ONE launch of a dense 3x3 kernel (pad 1, stride 1 or 2; csrc/kernels_conv3.hip) on caller
 * tensors, then a wait for `stream`.  All maps are NHWC with a leading dimension (floats, or bf16 elements, between pixels)
 * that may exceed the channel count: channels past it are neither read nor written.  H x W is always the layer's INPUT
 * map, the output map is H / stride x W / stride.  A table is f32 [3][cin]: rows scale, shift, flag; the kernels read
 * a = flag ? silu(scale * x + shift) : x, and the zero padding is applied to a.  `route` picks the kernel: 0 = the
 * launcher's own rule (what the networks get), else one kernel family, which must admit the launch.
 * Common JN_EINVAL, before any device call: a null pointer (but the optional ones), N, H, W < 1, a channel count or a
 * leading dimension that is no multiple of 4, a leading dimension below its channel count, a stride other than 1 or 2,
 * an odd H or W at stride 2, n_slots < 1, a route out of range or one whose preconditions the launch does not meet, a size
 * beyond what a debug call is for (N * H * W > 2^24, more than 4096 channels, a leading dimension above 8192, n_slots > 64).
 *
 * jn_conv3: out (=|+=) conv(a(in), w).  w f32 [9][cout][cin], tap = 3 ky + kx.  transposed != 0 (stride 1 only): the data
 * gradient of a stride-1 layer, out[y][x][n] = sum a(in)[y + 1 - ky][x + 1 - kx][k] * w[tap][k][n] with w f32 [9][cin][cout],
 * the forward layer's weight.  stats_dev: NULL, or f64 [32][2 cout] that the launch ADDS per-channel (sum, sum of squares)
 * of the output pixels into, spread over the 32 replicas.  skip_flag_dev: NULL, or a device int; the launch does nothing
 * when *skip_flag_dev >= skip_when.  n_slots > 1: slot j reads in + j * in_slot_stride and writes out + j * out_slot_stride
 * (elements; all slots share the table).  Routes: 1 = fp32 matrix pipe; 2 = three-way split operands on the bf16 pipe
 * (cin % 32 == 0; at stride 2 neither accumulate nor slots); 3 = bf16 inference kernel: in and out hold bf16, w is rounded
 * to bf16 inside the call (cin % 8 == 0; no stats, accumulate, slots or transposed).
 * jn_conv3_bwd_data_s2: data gradient of a stride-2 layer, gin [S][N,H,W,gin_ld] (=|+=) from gz [S][N,H/2,W/2,g_ld] and the
 * forward weight w [9][cout][cin].  Routes: 1 = fp32; 2 = split (cout % 32 == 0).  Allocates a workspace and frees it.
 * jn_conv3_bwd_weight: gw [9][cout][cin] += sum over slots and pixels of gz[p][o] * a(x)[p (+) tap][k]; gz [S][N,OH,OW,g_ld],
 * x [S][N,H,W,x_ld], tab [S][3][cin].  Routes: 1 = split planes with transposed LDS reads (cout % 16 == 0); 2 = split at
 * the LDS read; 3 = exact fp32 products (what JN_WW_EXACT=1 makes the rule pick).  max_wg: 0 = the launcher's rule, else
 * the number of workgroups that walk the pixel tiles of one channel block (1: one workgroup walks them all); < 0: JN_EINVAL.
 * jn_conv3_route: host only, no device call: the route (1..3, as above) the launcher's rule gives the launch.  kind 0 =
 * jn_conv3 forward, 1 = jn_conv3 transposed, 2 = jn_conv3_bwd_data_s2, 3 = jn_conv3_bwd_weight; (ld_a, ld_b) are the two
 * leading dimensions in the order of that entry's arguments.  JN_EINVAL as above. */
int jn_conv3(const void* in_dev, int in_ld, const float* tab_dev, const float* w_dev, void* out_dev, int out_ld, int N, int H,
             int W, int cin, int cout, int stride, int transposed, int accumulate, double* stats_dev, const int* skip_flag_dev,
             int skip_when, int n_slots, long long in_slot_stride, long long out_slot_stride, int route, void* stream);
int jn_conv3_bwd_data_s2(const float* gz_dev, int g_ld, const float* w_dev, float* gin_dev, int gin_ld, int N, int H, int W, int cout,
                         int cin, int accumulate, int n_slots, int route, void* stream);
int jn_conv3_bwd_weight(const float* gz_dev, int g_ld, const float* x_dev, int x_ld, const float* tab_dev, float* gw_dev, int N, int H,
                        int W, int cout, int cin, int stride, int n_slots, int route, int max_wg, void* stream);
int jn_conv3_route(int kind, int N, int H, int W, int cin, int cout, int stride, int n_slots, int ld_a, int ld_b);
/* Debug entries, context-free: ONE launch of a depthwise 3x3 kernel (pad 1, stride 1 or 2; csrc/kernels_conv.hip, the backward in
 * csrc/kernels_bwd.hip) on caller tensors, then a wait for `stream`.  Maps are NHWC with a leading dimension that may exceed the
 * channel count C: channels past it are neither read nor written.  H x W is the layer's INPUT map, of any size; the output map
 * is OH x OW = (H + stride - 1) / stride x (W + stride - 1) / stride.  Tables are f32 [3][channels], rows scale, shift, flag:
 * a = flag ? silu(scale * x + shift) : x, zero padding applied to a.  w f32 [9][C], tap = 3 ky + kx.  dtype: 0 = f32, 1 = bf16 maps.
 * Common JN_EINVAL, before any device call: a null pointer (but the optional ones), N, H, W < 1, N * H * W > 2^24, C < 4, C % 4 != 0,
 * C > 4096, a stride other than 1 or 2, a leading dimension below its channel count, no multiple of 4 or above 8192, a route out
 * of range or one whose preconditions the launch does not meet.
 *
 * jn_dw3x3: out = dwconv(a(in), w).  stats_dev: NULL, or f64 [nrep][2 C] that the launch ADDS per-channel (sum, sum of squares)
 * of the output into, spread over the nrep (1..32) replicas.  skip_flag_dev: NULL, or a device int; nothing is done when
 * *skip_flag_dev >= skip_when.  Routes: 0 = the launcher's rule, 1 = the LDS-tiled kernel (C % 16 == 0, N <= 65535), 2 = the
 * strip kernel (reads the table arrays only).
 * jn_dw3x3_route: host only: the route (1 or 2) the launcher's rule gives.
 * jn_dwpw: the eval-mode fusion out = w_pw . silu(msc * dwconv(a(in), w_dw) + msh), w_pw f32 [cout][C], mtab [3][C] (flag row not
 * read); with res_dev the bottleneck shortcut out = silu(psc * (that) + psh) + T_rtab(res), res [N,OH,OW,res_ld], rtab and ptab
 * [3][cout] (ptab's flag row not read).  JN_EINVAL also where dwpw_supported(C, cout, stride) is false: C or cout no multiple of
 * 16, C > 64, cout / 16 not 1, 2, 4 or 8 (stride 2: not 1).
 * jn_dw_bwd: the backward of one depthwise BatchNorm + SiLU layer over n_slots (1..64) workspace slots.  Per slot, with
 * y = o_sc * z + o_sh of the layer's raw output z: g_z = k * (g * silu'(y) - c1 - (z - mean) * invstd * c2); gin (=|+=) the
 * transposed depthwise conv of g_z; gw [9][C] += sum g_z * a(x) over all slots.  g [S][N,OH,OW,g_ld], z likewise, x [S][N,H,W,x_ld],
 * gin likewise; otab, itab [S][3][C] (otab's flag row not read); save [S][C][2] = (mean, invstd); consts [S][C][3] = (c1, c2, k).
 * Routes: 0 = the backward plan's choice, 1 = the fused kernel (C % 16 == 0), 2 = bn_bwd_gz, data-gradient and weight-gradient
 * kernels one after the other.  red_out_dev: NULL, or f64 [S][32][2 C] the fused kernel ADDS, per input channel,
 * (sum dx * silu'(y_in), sum dx * silu'(y_in) * y_in) into, y_in = i_sc * x + i_sh, dx the data gradient it writes (route 1 without
 * accumulate only).  use_wpart != 0: the weight gradient goes through a zeroed [32][16384] replica scratch, copied to
 * wpart_back_dev (required then) after the launch, where it must be zero again.  max_wg: 0 = the launcher's rule, else a cap on
 * the persistent workgroups per channel block and slot (route 1) or on the weight-gradient kernel's workgroups per slot (route 2).
 * Allocates its workspace, waits for `stream` and frees it. */
int jn_dw3x3(const void* in_dev, int in_ld, const float* tab_dev, const float* w_dev, void* out_dev, int out_ld, int N, int H, int W,
             int C, int stride, int dtype, double* stats_dev, const int* skip_flag_dev, int skip_when, int nrep, int route, void* stream);
int jn_dw3x3_route(int N, int C, int stride, int dtype);
int jn_dwpw(const void* in_dev, int in_ld, const float* itab_dev, const float* w_dw_dev, const float* mtab_dev, const float* w_pw_dev,
            void* out_dev, int out_ld, const void* res_dev, int res_ld, const float* rtab_dev, const float* ptab_dev, int N, int H, int W,
            int C, int cout, int stride, int dtype, const int* skip_flag_dev, int skip_when, void* stream);
int jn_dw_bwd(const float* g_dev, int g_ld, const float* z_dev, int z_ld, const float* x_dev, int x_ld, const float* otab_dev,
              const float* itab_dev, const float* save_dev, const float* consts_dev, const float* w_dev, float* gin_dev, int gin_ld,
              int accumulate, float* gw_dev, double* red_out_dev, int N, int H, int W, int C, int stride, int n_slots, int route,
              int use_wpart, float* wpart_back_dev, int max_wg, void* stream);
/* Debug entries, context-free: ONE launch of a 1x1 (pointwise) conv kernel (csrc/kernels_conv.hip, kernels_pwres.hip,
 * kernels_pwxs.hip; the weight gradient in kernels_bwd_pw.hip) on caller tensors, then a wait for `stream`.  Maps are [M][ld] with
 * M = N * H * W pixels and a leading dimension that may exceed the channel count: channels past it are neither read nor written.
 * Common JN_EINVAL, before any device call: a null pointer (but the optional ones), N, H, W or M < 1, M > 2^24, a channel count
 * below 4, above 4096 or no multiple of 4, a leading dimension below its channel count, no multiple of 4 or above 8192, n_slots
 * outside 1..64, a forced route whose kernels do not admit the launch, max_wg < 0.
 *
 * jn_pw: out (=|+=) act(T(in) . w^T + bias), T(x) = flag ? silu(scale * x + shift) : x from tab f32 [3][cin] (rows scale, shift,
 * flag).  w f32 [cout][cin]; transposed != 0: w is [cin][cout], the forward weight of the layer whose data gradient this is.
 * dtype_in / dtype_out: 0 = f32, 1 = bf16 maps; bf16_mfma != 0: the products run on the bf16 matrix pipe (required with bf16 input).
 * in_identity != 0 promises a table of flags 0 (kernels may compile the transform out).  bias_dev f32 [cout] or NULL; act 0 = none,
 * 1 = silu, 2 = relu, 3 = sigmoid.  stats_dev: NULL, or f64 [nrep][2 cout] (nrep 1..32) that the launch ADDS per-channel (sum, sum of
 * squares) of the stored fp32 values into; replicas past nrep are not touched.  skip_flag_dev: NULL, or a device int; nothing is done
 * when *skip_flag_dev >= skip_when.  n_slots > 1: slot j reads in + j * in_slot_stride, writes out + j * out_slot_stride (elements,
 * multiples of 4, at least M * ld) and reads the table rows at + j * tab_slot_stride floats each (0: one table for all).
 * up_out_dev: NULL, or f32 [N][2H][2W][up_ld] that also receives the output upsampled nearest x2 (the routes and shapes of
 * pw_fuses_upsample only: X3 128 -> 64 and 256 -> 128, XS 256 -> 128).  route: 0 = the rule of pw_route with the split planes
 * present (what the networks get), else 1 = X1 (bf16 maps, single plane), 2 = X3 (three bf16 planes), 3 = XS, 4 = WIDE (pw_dir_kernel),
 * 5 = NARROW, 6 = MFMA.  For X1 and X3 the call splits w itself with the context's splitters (flat planes, then fragment order where
 * pw_x3_fragment_order says so).  max_wg: 0 = the launcher's rule, else a cap on the x extent of the persistent grid (1: one
 * workgroup walks every pixel tile); MFMA has no persistent grid and refuses max_wg > 0.
 * defer: NULL = a plain table, else the input view's deferred BatchNorm entries (one slot only): f64 batch sums
 * [8][rep_stride] ((sum, sum of squares) of stat channel i at [2 i] of a replica), a parameter buffer with the BatchNorm weights and
 * biases, dN patches, the deferral limit dmax and 1..4 ascending channel runs: channels [c0, c1) are stat channels stat0 + (c - c0)
 * with weight / bias at params[g0 / b0 + (c - c0)] over dN * hw pixels; stat0 < 0, or dN * hw > dmax: the run reads tab.  use_runs != 0
 * hands the runs to the kernel as they are (ChanTab::r0..r3), 0 expands them into the per-channel arrays (dsrc / dhw / dgoff / dboff).
 * jn_pw_route: host only, no device call: with route = 0 the route (1..6) the rule gives that launch, else `route` itself where
 * that family's kernels admit the launch (JN_EINVAL where not); for route 6 variant_out (int32 [3], or NULL) receives pw_mfma_kernel's tile variant (CT channel tiles, KC chunk, WM pixel waves: 32 WM pixels per workgroup), else zeros.
 * jn_pw_bwd_data_x3: the data gradient of a wide layer on the split pipe (launch_pw_x3_bwd_data): gx [S][M][gx_ld] = gz [S][M][g_ld] . w,
 * w f32 [cout][cin] the forward weight, (cout, cin) one of (256, 128), (256, 256), (256, 512), (128, 256).  Allocates the transposed
 * planes and frees them.
 * jn_pw_bwd_weight: gw [cout][cin] += sum over slots and pixels of gz[m][n] * T(x)[m][k]; gz slot j at + j * gz_slot_stride floats,
 * x [S][M][x_ld], tab [S][3][cin].  use_wpart != 0 (cout * cin <= 16384, below 128 x 128): through a zeroed [32][16384] replica
 * scratch, copied to wpart_back_dev (required then) after the launch, where it must be zero again.  exact != 0 (both counts >= 128):
 * the wide kernel with exact fp32 products (what JN_WW_EXACT=1 makes the rule pick), else its split products. */
typedef struct jn_pw_run { int32_t c0, c1, stat0, g0, b0; float hw; } jn_pw_run;
typedef struct jn_pw_defer {
  const double* sums_dev; long long rep_stride; const float* params_dev;
  int32_t dN; long long dmax;
  int32_t n_runs, use_runs;
  jn_pw_run run[4];
} jn_pw_defer;
int jn_pw(const void* in_dev, int in_ld, int dtype_in, const float* tab_dev, const jn_pw_defer* defer, const float* w_dev,
          const float* bias_dev, void* out_dev, int out_ld, int dtype_out, int N, int H, int W, int cin, int cout, int bf16_mfma,
          int transposed, int in_identity, int accumulate, int act, double* stats_dev, int nrep, const int* skip_flag_dev, int skip_when,
          int n_slots, long long in_slot_stride, long long out_slot_stride, long long tab_slot_stride, float* up_out_dev, int up_ld,
          int route, int max_wg, void* stream);
int jn_pw_route(int N, int H, int W, int cin, int cout, int in_ld, int out_ld, int dtype_in, int dtype_out, int bf16_mfma, int transposed,
                int accumulate, int has_bias, int act, int n_slots, int has_up, int route, int32_t* variant_out);
int jn_pw_bwd_data_x3(const float* gz_dev, int g_ld, const float* w_dev, float* gx_dev, int gx_ld, long long M, int cout, int cin,
                      int n_slots, int max_wg, void* stream);
int jn_pw_bwd_weight(const float* gz_dev, int g_ld, const float* x_dev, int x_ld, const float* tab_dev, float* gw_dev, long long M, int cout,
                     int cin, int n_slots, long long gz_slot_stride, int use_wpart, float* wpart_back_dev, int exact, void* stream);
/* host only: the kernel launch_pw_bwd_weight gives a layer: 1 = pw_bwd_weight_kernel, 2 = pw_bwd_weight_wide_kernel (both counts >= 128) */
int jn_pw_bwd_weight_route(int cout, int cin);
/* Debug entries, context-free: ONE launch of a kernel that runs between the convolutions of a train-mode pass (csrc/kernels_conv.hip:
 * stem, SPP, upsample, shortcut sum, BatchNorm tables, embed_fpn linear; csrc/kernels_bwd.hip: their backward and the BatchNorm
 * sums) on caller tensors, then a wait for `stream`.  Maps are NHWC with a leading dimension that may exceed the channel count;
 * tables are f32 [3][C] (rows scale, shift, flag), per slot [S][3][C]; dtype 0 = f32, 1 = bf16 maps.  skip_flag_dev: NULL, or a device
 * int; nothing is done when *skip_flag_dev >= skip_when.  JN_EINVAL before any device call: a null pointer (but the optional ones),
 * a count below 1, n_slots outside 1..64, a leading dimension below its channel count or above 8192, max_wg < 0, and whatever the
 * launcher refuses: named per entry.
 *
 * jn_stem: out [N][P/2][P/2][out_ld] = the 6 x 6 stride-2 conv (Focus + 3 x 3, zero padding at the patch border) of the P x P patch
 * of image n at src + n * sample_stride (+ positions[pos_stride * n + {0, 1}] = (y, x) patch indices, if positions_dev is given),
 * channels chan_stride and rows row_stride elements apart; src_u8 != 0: bytes b read as b / 255.  w f32 [108][cout], k = 36 c + 6 dy
 * + dx.  out_dtype 0 / 1.  stats_dev: NULL, or f64 [nrep][2 cout] the launch ADDS (sum, sum of squares) per channel into, nrep 1..32.
 * max_wg: 0 = the launcher's rule, else a cap on the persistent workgroups along x.  Refused: odd P, cout % 16 != 0, out_ld % 4 != 0.
 * jn_stem_bwd_weight: gw [108][cout] += sum over slots and pixels of g_z * patch; g [S][N][P/2][P/2][g_ld] is g_z itself, or with
 * z_dev (same shape, z_ld) d loss / d activation, turned into g_z = k (g silu'(o_sc z + o_sh) - c1 - (z - mean) invstd c2) on the way:
 * otab [S][3][cout], save [S][cout][2], consts [S][cout][3].  Slot j reads positions + j * pos_slot_stride.  wpart_dev: the
 * f32 [32][16384] replica scratch, zero on entry and zero again afterwards.  Refused: as jn_stem, and cout > 144 (the scratch).
 * jn_spp: slices 1..3 of cat [N][H][W][ld] (h channels each) = max-pools 5 / 9 / 13 of the activation of slice 0 (tab [3][h]).
 * route: 0 = the launcher's rule, 1 = the quad kernel (f32, h % 16 == 0, ld % 4 == 0, H * W <= 510), 2 = the scalar kernel (h a
 * multiple of its 8 channels per workgroup, 4 where the map needs more than 48 KB of LDS with 8).  Refused: a route whose
 * preconditions the launch misses, LDS above what a workgroup can be granted, N > 65535.
 * jn_spp_bwd: slice 0 of gcat [S][N][H][W][ld] += the three pooled gradients of slices 1..3, each sent to the first maximum of
 * its window in row-major order; cat as in jn_spp per slot, tab [S][3][h].  Routes as jn_spp (quad: H * W <= 512; scalar: 4 channels
 * above 60 KB).
 * jn_spp_route: host only: the route (1 or 2) the rule gives (bwd != 0: the backward launcher's).
 * jn_upsample: out [N][2H][2W][out_ld] = nearest x2 copy of in [N][H][W][in_ld].  Refused: C or a leading dimension no multiple of 4.
 * jn_upsample_bwd: gsrc [S][N][H][W][src_ld] (=|+=) the sum of the 2 x 2 children in gdst [S][N][2H][2W][dst_ld]; f32.  Allocates
 * its workspace and frees it.
 * jn_addact: out [M][out_ld] = T_ztab(z) + T_rtab(res).  Refused: C or a leading dimension no multiple of 4, C > 2048.
 * jn_bn_finalize: train-mode BatchNorm of C channels from the f64 sums stats [32][rep_stride] ((sum, sum of squares) of channel c at
 * [2 c] of a replica) over `count` values: tab0 (and tab1, if given) [3][C] = (gamma invstd, beta - mean gamma invstd, 1); save [C][2]
 * = (mean, invstd) and the running statistics (unbiased variance) are optional.
 * jn_bn_finalize_all: the same for n_stat channels of many layers at once: channel i has hw[i] pixels per image (<= 0: skipped),
 * weight and bias at params[goff[i]] and params[boff[i]], table columns t0[i] and t1[i] (-1: none) of tab [3][tab_channels]; it sums
 * 8 replicas where N * hw <= defer_max_m, else all 32.  run_mean, run_var f32 [n_stat].  Allocates an address array and frees it.
 * jn_bn_bwd_sums: reduce != 0: red [S][32][2 C] += per channel (sum g silu'(y), sum g silu'(y) zhat) over the M pixels of g, z
 * [S][M][ld] with y = sc z + sh (tab [S][3][C], flag row not read), zhat = (z - mean) invstd from save [S][C][2]; refused: C % 4 != 0,
 * C > 1280, and above 1024 a C that is no multiple of 8 (two launches over halves of whole quads).  consts_dev given: consts
 * [S][C][3] = (sum1 / M, sum2 / M, gamma invstd) from the replicas' totals, g_beta += sum1,
 * g_gamma += sum2 over all slots; raw_moment != 0 (without reduce): the second sum is against y and is converted first.
 * jn_efpn_linear: part [N][KS][Co] = the K-slice partial sums of e [N][K] . wt [K][Co] (MFMA form where Co % 16 == 0 and K % 4 == 0,
 * else the scalar form).  Refused: the scalar form with Co > 256. */
int jn_stem(const void* src_dev, int src_u8, const int64_t* positions_dev, int pos_stride, long long sample_stride, long long chan_stride,
            int row_stride, int P, int N, int cout, const float* w_dev, void* out_dev, int out_ld, int out_dtype, double* stats_dev, int nrep,
            const int* skip_flag_dev, int skip_when, int max_wg, void* stream);
int jn_stem_bwd_weight(const void* src_dev, int src_u8, const int64_t* positions_dev, int pos_stride, long long pos_slot_stride,
                       long long sample_stride, long long chan_stride, int row_stride, int P, int N, int cout, const float* g_dev, int g_ld,
                       const float* z_dev, int z_ld, const float* otab_dev, const float* save_dev, const float* consts_dev, float* gw_dev,
                       float* wpart_dev, int n_slots, int max_wg, void* stream);
int jn_spp_route(int dtype, int ld, int h, int H, int W, int N, int bwd);
int jn_spp(void* cat_dev, int dtype, int ld, int h, int H, int W, int N, const float* tab_dev, const int* skip_flag_dev, int skip_when,
           int route, void* stream);
int jn_spp_bwd(const float* cat_dev, float* gcat_dev, int ld, int h, int H, int W, int N, const float* tab_dev, int n_slots, int route,
               void* stream);
int jn_upsample(const void* in_dev, int in_ld, void* out_dev, int out_ld, int dtype, int C, int H, int W, int N, const int* skip_flag_dev,
                int skip_when, void* stream);
int jn_upsample_bwd(const float* gdst_dev, int dst_ld, float* gsrc_dev, int src_ld, int C, int H, int W, int N, int accumulate, int n_slots,
                    void* stream);
int jn_addact(const void* z_dev, int z_ld, const float* ztab_dev, const void* res_dev, int res_ld, const float* rtab_dev, void* out_dev,
              int out_ld, int dtype, int C, long long M, const int* skip_flag_dev, int skip_when, void* stream);
int jn_bn_finalize(const double* stats_dev, long long rep_stride, double count, const float* gamma_dev, const float* beta_dev, float* run_mean_dev,
                   float* run_var_dev, float* save_dev, float* tab0_dev, float* tab1_dev, int C, float eps, float momentum,
                   const int* skip_flag_dev, int skip_when, void* stream);
int jn_bn_finalize_all(const double* stats_dev, long long rep_stride, int n_stat, int N, const float* hw_dev, const int* goff_dev,
                       const int* boff_dev, const float* params_dev, const int* t0_dev, const int* t1_dev, float* tab_dev, int tab_channels,
                       float* save_dev, float* run_mean_dev, float* run_var_dev, float eps, float momentum, const int* skip_flag_dev, int skip_when,
                       long long defer_max_m, void* stream);
int jn_bn_bwd_sums(const float* g_dev, int g_ld, const float* z_dev, int z_ld, const float* tab_dev, const float* save_dev, int C, long long M,
                   int n_slots, double* red_dev, const float* gamma_dev, const float* beta_dev, float* consts_dev, float* g_gamma_dev,
                   float* g_beta_dev, int reduce, int raw_moment, void* stream);
int jn_efpn_linear(const float* e_dev, const float* wt_dev, float* part_dev, int N, int K, int Co, int KS, const int* skip_flag_dev, int skip_when,
                   void* stream);
/* Debug entries, context-free: ONE launch of a decision-side training kernel (csrc/kernels_train.hip) on caller tensors, then a wait
 * for `stream`.  logits f32 [B][T][nA], actions / target int64 [B][T] inside [0, nA), masks uint8 [B][T], dlogits f32 [B][T][nA].
 * n_done_dev: NULL, or the rollout's int32 [T + 1] count of finished agents after each step; with it the executed steps are
 * S = the first t in 1..T with n_done[t] >= B (T if none) and the rows t >= S of dlogits are zero.  JN_EINVAL before any device
 * call: a null pointer (but the optional ones), B or T below 1, nA outside 1..256, B * T above 2^24.
 *
 * jn_reinforce_loss: the REINFORCE loss of jn_reinforce_step on given rollout tensors (returns, rewards f32 [B][T]): over the
 * tokens with t < S and logit_masks != 0, loss = mean(-logp[action] adv) + entropy_weight mean(-H), adv = (returns - ret_mean) /
 * (ret_std + 1e-8) with reward_norm, else the returns; dlogits = loss_scale d loss / d logits (zero rows elsewhere); metrics f32
 * [6] = action loss, entropy loss, loss, sum of the selected rewards / B, selected tokens / B, S.  No selected token: 0 / 0.
 * jn_logits_grad: dlogits = dlogprobs d logp[action] / d logits + dentropies d H / d logits for upstream gradients f32 [B][T]; either
 * may be NULL (zeros), not both.  A token whose upstream values are both 0 gets a zero row.
 * jn_ce_loss: the supervised loss of jn_supervised_step: cross-entropy with weight stop_weight on class 8 and 1 elsewhere, summed
 * over the tokens with masks != 0 and divided by their count n; dlogits its gradient (zero rows elsewhere); metrics f32 [3] = loss,
 * accuracy (the first maximum is the prediction), n / B.
 * jn_adamw: one clip_grad_value_ + AdamW update of jn_optimizer_step_group over n elements: g' = clamp(g grad_scale, +-clip_value)
 * (clip_value 0: no clamp), p -= lr weight_decay p, m = 0.9 m + 0.1 g', v = 0.999 v + 0.001 g'^2, p -= lr / (1 - 0.9^step) m /
 * (sqrt(v) / sqrt(1 - 0.999^step) + 1e-8); 0.1, 0.001, lr / (1 - 0.9^step) and sqrt(1 - 0.999^step) are formed in double and rounded
 * once, the per-element arithmetic is fp32.  JN_EINVAL: n or step below 1, a negative lr, weight_decay or clip_value. */
int jn_reinforce_loss(const float* logits_dev, const int64_t* actions_dev, const float* returns_dev, const float* rewards_dev,
                      const uint8_t* logit_masks_dev, const int32_t* n_done_dev, int B, int T, int nA, int reward_norm, float ret_mean,
                      float ret_std, float entropy_weight, float loss_scale, float* dlogits_dev, float* metrics_dev, void* stream);
int jn_logits_grad(const float* logits_dev, const int64_t* actions_dev, const float* dlogprobs_dev, const float* dentropies_dev,
                   const int32_t* n_done_dev, int B, int T, int nA, float* dlogits_dev, void* stream);
int jn_ce_loss(const float* logits_dev, const int64_t* target_dev, const uint8_t* masks_dev, int B, int T, int nA, float stop_weight,
               float* dlogits_dev, float* metrics_dev, void* stream);
int jn_adamw(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, long long n, float lr, float weight_decay, int step, float clip_value,
             float grad_scale, void* stream);
/* Arms the following rollouts of `ctx` with that teacher (the per-step `best_action` that test_model_on_env compares
 * each chosen action with, src/supervised.py:279-405): before the decision of step t, the set of the state that
 * decision sees (position and visited patches before the step) goes to sets_dev[b * T + t] (uint8 [B,T], T =
 * max_ep_len), on the rollout's stream and under the step's own early-stop flag; columns past the executed steps are
 * 0.  targets_dev: NULL = the env's own bbox masks, else a uint8 [B,Gh,Gw] grid on the env's canvas (cells outside a
 * ragged extent must be 0).  Both buffers are the caller's and must outlive the rollouts.  sets_dev = NULL disarms.
 * Independent of jn_set_rollout_positions. */
int jn_set_rollout_teacher(jn_ctx* ctx, const uint8_t* targets_dev, uint8_t* sets_dev);
/* Names the random stream of every agent of the following rollouts of `ctx`.  keys_host: uint64 [n][2] = (stream seed,
 * stream index) in HOST memory, read before the call returns (the context keeps its own copy and uploads it on the
 * stream of the next rollout that needs it).  While armed, the two sampled draws of agent b ignore the rollout's `seed`
 * argument and its index in the batch: the action of step t (JN_MODE_SAMPLE) is drawn from
 * Philox4x32-10(key = keys[b][0], counter = ((uint32) keys[b][1], t, 0x53414d50, 0)) and, without start_positions, the
 * reset position from Philox4x32-10(keys[b][0], ((uint32) keys[b][1], 0, 0x52455345, 0)) modulo the agent's own grid
 * extent — so keys (seed, b) reproduce the unarmed rollout of `seed`, and an agent keeps its walk wherever it sits in
 * whichever batch.  Greedy and forced actions, and the train-mode dropout masks (keyed by the batch index), are not
 * affected.  keys_host = NULL disarms (n is ignored); disarmed, every draw is what it was without this call.  Sticky
 * until set again.  While armed, jn_rollout, jn_reinforce_forward and jn_reinforce_step fail with JN_EINVAL before any
 * launch when the env's B != n.  Every check comes before any device call (the one such call: a new table waits for
 * the upload of the previous one).  JN_EINVAL: a null ctx, n < 1 with a table, a stream index >= 2^32
 * (the armed keys are then left as they were). */
int jn_set_rollout_keys(jn_ctx* ctx, const uint64_t* keys_host, int n);
/* Names the class behind the class token of every agent of the following rollouts of `ctx`: the free-running
 * evaluation of a class-conditioned (supervised) policy, where test_model_on_env feeds `classes=sample["class_id"]` at
 * every step and eval_envs hands each image's class down (src/supervised.py:284, 317-331, 663-687).  classes_host: int64
 * [n] in HOST memory, read before the call returns (the context keeps its own copy and uploads it on the stream of the
 * next rollout that needs it).  While armed, agent b's first token is row classes[b] of embed_class (gpt.py:476-478) on
 * both decision routes and under both token positions; a train-mode rollout (jn_reinforce_forward, jn_reinforce_step)
 * keeps the ids it ran with, and its backward — whenever it runs, whatever is armed by then — adds the class token's
 * gradient to those rows.  classes_host = NULL disarms (n is ignored); disarmed, every agent gets row 0 (the REINFORCE
 * loop's zeros, src/reinforce.py:128-129) and every result is what it was without this call.  Sticky until set again.
 * While armed, jn_rollout, jn_reinforce_forward and jn_reinforce_step fail with JN_EINVAL before any launch when the
 * env's B != n.  Every check comes before any device call (the one such call: a new table waits for the upload of the
 * previous one).  JN_EINVAL: a null ctx, n < 1 with a table, an id outside 0 .. 99 (nn.Embedding raises on it; the
 * message names the agent and the id; the armed table is then left as it was). */
int jn_set_rollout_classes(jn_ctx* ctx, const int64_t* classes_host, int n);
/* Invalid-action masking of the following rollouts of `ctx` (opt-in; not in the reference, whose env clamps a move that
 * leaves the grid).  Before the decision of step t every agent, finished ones included, gets an action set M, a uint16
 * whose bit a says that action a may be taken.  It is formed from the agent's position, its grid (its own extent in
 * ragged mode) and `visited` before this step's update (the current cell is marked); a move a < 8 is inside when its
 * target lies on the grid and fresh when it is inside and its target is unvisited:
 *   JN_MASK_NONE       no set is formed: every result is what it was without this call
 *   JN_MASK_GRID       M = the moves that are inside
 *   JN_MASK_UNVISITED  M = the fresh moves, or when there is none the moves that are inside
 * A set that is still empty (a 1 x 1 grid) becomes all of 0..7; with n_actions == 9 STOP is always a member, and in
 * JN_MODE_FORCED so is the forced action.  Under M the log-probability, the entropy, the greedy maximum (the first one)
 * and the sampled action (inverse CDF over the members in index order at the unmasked rollout's Philox uniform; the last
 * member when none passes) are those of the softmax over the members' logits; a logit outside M is never read.  The
 * outputs' logits stay the head's.  The set of step t goes to a buffer of the context and, with sets_out_dev (uint16
 * [B,T], the caller's, alive during the rollouts; columns past the executed steps are 0), to sets_out_dev[b * T + t].
 * jn_reinforce_step forms its loss, and jn_reinforce_backward its gradient, under the sets of the forward they
 * differentiate: d logp / d logits_j = [j == a] - p_j and d H / d logits_j = -p_j (logp_j + H) for j in M, exactly 0
 * elsewhere.  Arming between a jn_reinforce_forward and its backward makes that forward stale (JN_ESTATE from the
 * backward), as jn_set_activation_slots does; disarming does not.  Sticky until set again; policy 0 disarms.  Needs no
 * device.  JN_EINVAL: a null ctx, a policy outside 0..2 (what was armed stays). */
enum { JN_MASK_NONE = 0, JN_MASK_GRID = 1, JN_MASK_UNVISITED = 2 };
int jn_set_rollout_action_mask(jn_ctx* ctx, int policy, uint16_t* sets_out_dev);
/* The action sets of jn_set_rollout_action_mask for N given states, context-free, one launch on `stream`:
 * positions int64 [N][2] = (y, x), visited uint8 [N][Gh][Gw], extents int32 [N][2] = (gh, gw) or NULL (Gh, Gw), forced
 * int64 [N] or NULL, policy 1 or 2, nA 8 or 9; sets_dev uint16 [N].  JN_EINVAL before any device call: a null pointer
 * (but the optional ones), N, Gh or Gw below 1, another policy or nA.  Positions and extents are the caller's to keep on
 * the grid. */
int jn_action_sets(const int64_t* positions_dev, const uint8_t* visited_dev, const int32_t* extents_dev, const int64_t* forced_dev,
                   int N, int Gh, int Gw, int policy, int nA, uint16_t* sets_dev, void* stream);
/* jn_reinforce_loss and jn_logits_grad under action sets sets_dev uint16 [B][T] (debug entries like them; nA at most 16):
 * softmax, entropy and gradient over the members of each token's set, gradient exactly 0 elsewhere; the action of a
 * counted token must be a member and no counted token's set empty.  Sets that hold all nA bits give the bits of the
 * unmasked entries. */
int jn_reinforce_loss_masked(const float* logits_dev, const int64_t* actions_dev, const float* returns_dev, const float* rewards_dev,
                             const uint8_t* logit_masks_dev, const int32_t* n_done_dev, int B, int T, int nA, int reward_norm,
                             float ret_mean, float ret_std, float entropy_weight, float loss_scale, float* dlogits_dev,
                             float* metrics_dev, const uint16_t* sets_dev, void* stream);
int jn_logits_grad_masked(const float* logits_dev, const int64_t* actions_dev, const float* dlogprobs_dev, const float* dentropies_dev,
                          const int32_t* n_done_dev, int B, int T, int nA, float* dlogits_dev, const uint16_t* sets_dev, void* stream);
/* Number of steps S the last rollout executed (reference tensor width).  Synchronises
 * on `stream`. */
int jn_rollout_steps(jn_ctx* ctx, int* n_steps, void* stream);

/* Wall-clock helpers for bench.py: HIP-event time of the most recent jn_rollout on its
 * stream, split per kernel family.  what = 0 total ms, 1 backbone conv ms (forward, summed over the glimpse steps),
 * 2 conv-stack backward ms of the most recent jn_reinforce_step (embed_fpn + PAFPN backward).  Synchronises. */
int jn_last_timing(jn_ctx* ctx, int what, float* ms);
/* Enables HIP-event bracketing of the backbone conv section (costs two events/step). */
int jn_set_profiling(jn_ctx* ctx, int enabled);

#ifdef __cplusplus
}
#endif
#endif /* JNROLL_H */
