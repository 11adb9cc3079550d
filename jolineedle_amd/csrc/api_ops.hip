// C ABI of libjnroll.so, stateless product wrappers (patch gather, augmentation, box merge, postprocess, mAP, detection cells,
// teacher walks): argument checks around one launch each, no jn_ctx.  The kernel-level entries of the per-kernel tests are in
// api_kernels.hip.  Host code only (compiled by hipcc as C++); kernels live in kernels_*.hip.
#include "jn_internal.h"

using namespace jnr;

// jn_gather_patches* for fp32 and byte images; `indexed`: patch n reads image image_index[n] of n_images
template <typename T>
static int gather_patches(const char* who, bool indexed, const T* images_dev, const int64_t* image_index_dev,
                          const int64_t* positions_dev, float* out_dev, int N, int n_images, int C, int H, int W, int P, void* stream) {
  JN_CHECK(images_dev && (image_index_dev || !indexed) && positions_dev && out_dev, JN_EINVAL, "%s: null argument", who);
  JN_CHECK(N >= 0 && n_images >= 1 && C >= 1 && P >= 1 && H % P == 0 && W % P == 0, JN_EINVAL, "%s: bad shape", who);
  if (N == 0) return JN_OK;
  launch_gather(images_dev, positions_dev, out_dev, (long long)C * P * P, N, C, H, W, P, nullptr, 0, (hipStream_t)stream,
                image_index_dev);
  JN_HIP(hipGetLastError());
  return JN_OK;
}
extern "C" {

int jn_gather_patches(const float* images_dev, const int64_t* positions_dev, float* out_dev, int B, int C, int H, int W,
                      int P, void* stream) {
  return gather_patches("jn_gather_patches", false, images_dev, nullptr, positions_dev, out_dev, B, 1, C, H, W, P, stream);
}

int jn_gather_patches_u8(const uint8_t* images_dev, const int64_t* positions_dev, float* out_dev, int B, int C, int H,
                         int W, int P, void* stream) {
  return gather_patches("jn_gather_patches_u8", false, images_dev, nullptr, positions_dev, out_dev, B, 1, C, H, W, P, stream);
}

int jn_gather_patches_indexed(const float* images_dev, const int64_t* image_index_dev, const int64_t* positions_dev,
                              float* out_dev, int N, int n_images, int C, int H, int W, int P, void* stream) {
  return gather_patches("jn_gather_patches_indexed", true, images_dev, image_index_dev, positions_dev, out_dev, N, n_images, C, H,
                        W, P, stream);
}

int jn_gather_patches_indexed_u8(const uint8_t* images_dev, const int64_t* image_index_dev, const int64_t* positions_dev,
                                 float* out_dev, int N, int n_images, int C, int H, int W, int P, void* stream) {
  return gather_patches("jn_gather_patches_indexed_u8", true, images_dev, image_index_dev, positions_dev, out_dev, N, n_images, C,
                        H, W, P, stream);
}
int jn_augment_patches(const float* in_dev, float* out_dev, const float* params_dev, const float* noise_dev, uint64_t seed,
                       int N, int P, void* stream) {
  JN_CHECK(in_dev && out_dev && params_dev, JN_EINVAL, "jn_augment_patches: null argument");
  JN_CHECK(in_dev != out_dev, JN_EINVAL, "jn_augment_patches: in-place is not supported (tiles read their neighbours' halo)");
  JN_CHECK(N >= 0 && P >= 4, JN_EINVAL, "jn_augment_patches: bad shape");
  if (N == 0) return JN_OK;
  launch_augment(in_dev, out_dev, params_dev, noise_dev, (unsigned long long)seed, N, P, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// (the table was validated by whoever uploaded it; its element type selects the kernel, so the first entry is read back:
// one small copy and a stream sync per call, on a path that assembles samples and is not the rollout's)
int jn_gather_patches_views(const jn_image_view* views_dev, int n_views, const int64_t* image_index_dev,
                            const int64_t* positions_dev, void* out_dev, int out_u8, int N, int Hc, int Wc, int P, void* stream) {
  JN_CHECK(views_dev && image_index_dev && positions_dev && out_dev, JN_EINVAL, "jn_gather_patches_views: null argument");
  JN_CHECK(N >= 0 && n_views >= 1 && P >= 1 && Hc >= P && Wc >= P && Hc % P == 0 && Wc % P == 0, JN_EINVAL,
           "jn_gather_patches_views: bad shape");
  if (N == 0) return JN_OK;
  jn_image_view v0;
  JN_HIP(hipMemcpyAsync(&v0, views_dev, sizeof(v0), hipMemcpyDeviceToHost, (hipStream_t)stream));
  JN_HIP(hipStreamSynchronize((hipStream_t)stream));
  JN_CHECK((v0.src_u8 == 0 || v0.src_u8 == 1) && (v0.src_u8 || !out_u8), JN_EINVAL, "jn_gather_patches_views: a byte output needs byte sources");
  launch_view_gather(views_dev, v0.src_u8, image_index_dev, positions_dev, out_dev, out_u8, 3LL * P * P, N, P, nullptr, 0,
                     (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_rollout_boxes_to_image(const float* det_boxes_dev, const int32_t* det_counts_dev, const int64_t* positions_dev,
                              const uint8_t* masks_dev, int B, int T, int S, int K, int P, float* out_boxes_dev,
                              int32_t* out_totals_dev, void* stream) {
  JN_CHECK(det_boxes_dev && det_counts_dev && positions_dev && masks_dev && out_boxes_dev && out_totals_dev, JN_EINVAL,
           "jn_rollout_boxes_to_image: null argument");
  JN_CHECK(B >= 0 && T >= 0 && S >= 0 && S <= T && K >= 1 && P >= 1, JN_EINVAL, "jn_rollout_boxes_to_image: bad shape");
  // the kernel keeps four int32 per step in LDS (beside 2 KB of scan buffers); 48 KB of them is far beyond any block_size
  JN_CHECK((size_t)(S + 1) * 4 * sizeof(int32_t) <= (size_t)48 * 1024, JN_EINVAL,
           "jn_rollout_boxes_to_image: %d steps need more than 48 KB of LDS (at most 3071 steps)", S);
  if (B == 0) return JN_OK;
  launch_boxes_to_image(det_boxes_dev, det_counts_dev, positions_dev, masks_dev, B, T, S, K, P, out_boxes_dev, out_totals_dev,
                        (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_merge_boxes(const float* boxes_dev, const int32_t* counts_dev, int B, int Nmax, int W, int target, float threshold,
                   float* out_boxes_dev, int32_t* out_counts_dev, int32_t* rounds_dev, void* stream) {
  JN_CHECK(counts_dev && out_counts_dev && ((boxes_dev && out_boxes_dev) || Nmax == 0), JN_EINVAL, "jn_merge_boxes: null argument");
  JN_CHECK(B >= 0 && Nmax >= 0, JN_EINVAL, "jn_merge_boxes: bad shape");
  JN_CHECK(target ? W == 5 : (W == 6 || W == 7), JN_EINVAL,
           "jn_merge_boxes: %d columns; predictions have 6 or 7, targets 5", W);
  JN_CHECK(Nmax <= JN_EVAL_MAX_BOXES, JN_EINVAL, "jn_merge_boxes: %d boxes per image, the kernel holds at most %d in LDS", Nmax,
           JN_EVAL_MAX_BOXES);
  if (B == 0) return JN_OK;
  JN_CHECK(launch_merge_boxes(boxes_dev, counts_dev, B, Nmax, W, target, threshold, out_boxes_dev, out_counts_dev, rounds_dev,
                              (hipStream_t)stream) == 0,
           JN_EHIP, "jn_merge_boxes: %d bytes of LDS refused", 24 * Nmax);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_postprocess(const float* raw_dev, int N, int A, float conf_threshold, float nms_threshold, float clamp_max,
                   int max_out, float* boxes_dev, int32_t* counts_dev, int32_t* stats_dev, void* stream) {
  JN_CHECK(raw_dev && boxes_dev && counts_dev, JN_EINVAL, "jn_postprocess: null argument");
  JN_CHECK(N >= 1 && A >= 1, JN_EINVAL, "jn_postprocess: N=%d A=%d", N, A);
  JN_CHECK(max_out >= 1, JN_EINVAL, "jn_postprocess: max_out=%d", max_out);
  launch_postprocess(raw_dev, A, N, conf_threshold, nms_threshold, clamp_max, boxes_dev, counts_dev, max_out, stats_dev,
                     (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_postprocess_all(const float* raw_dev, int N, int A, float conf_threshold, float nms_threshold, float clamp_max,
                       int max_out, float* boxes_dev, int32_t* counts_dev, int32_t* stats_dev, void* stream) {
  JN_CHECK(raw_dev && boxes_dev && counts_dev, JN_EINVAL, "jn_postprocess_all: null argument");
  JN_CHECK(N >= 1 && A >= 1, JN_EINVAL, "jn_postprocess_all: N=%d A=%d", N, A);
  JN_CHECK(A <= POST_ALL_MAX_A, JN_EINVAL, "jn_postprocess_all: A=%d, the kernel holds at most %d candidates in LDS", A,
           POST_ALL_MAX_A);
  JN_CHECK(max_out >= 1, JN_EINVAL, "jn_postprocess_all: max_out=%d", max_out);
  launch_postprocess_all(raw_dev, A, N, conf_threshold, nms_threshold, clamp_max, boxes_dev, counts_dev, max_out, stats_dev,
                         (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_supervised_metrics(const float* logits_dev, const int64_t* current_actions_dev, const int64_t* next_actions_dev,
                          const uint8_t* masks_dev, int B, int T, int nA, float stop_weight, int on_self_trajectory,
                          float* token_loss_out_dev, uint8_t* predicted_out_dev, float* metrics_dev, void* stream) {
  JN_CHECK(logits_dev && next_actions_dev && masks_dev && metrics_dev, JN_EINVAL, "jn_supervised_metrics: null argument");
  JN_CHECK(!on_self_trajectory || current_actions_dev, JN_EINVAL, "jn_supervised_metrics: on-self-trajectory labels need current_actions");
  JN_CHECK(B >= 1 && T >= 1 && nA >= 1 && nA <= 256 && (long long)B * T <= (1LL << 24), JN_EINVAL,
           "jn_supervised_metrics: B=%d T=%d nA=%d", B, T, nA);
  launch_supervised_metrics(logits_dev, current_actions_dev, next_actions_dev, masks_dev, B, T, nA, stop_weight,
                            on_self_trajectory ? 1 : 0, token_loss_out_dev, predicted_out_dev, metrics_dev, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_match_detections(const float* preds_dev, const int32_t* pred_counts_dev, int B, int Nmax, int W,
                        const float* targets_dev, const int32_t* target_counts_dev, int Mmax, int max_det,
                        double* scores_dev, int32_t* hits_dev, int32_t* sel_dev, int32_t* n_pred_dev, int32_t* n_gt_dev,
                        void* stream) {
  JN_CHECK(pred_counts_dev && (preds_dev || Nmax == 0) && ((targets_dev && target_counts_dev) || Mmax == 0) && scores_dev &&
               hits_dev && sel_dev && n_pred_dev && n_gt_dev,
           JN_EINVAL, "jn_match_detections: null argument");
  JN_CHECK(B >= 0 && Nmax >= 0 && Mmax >= 0 && W >= 5 && max_det >= 1, JN_EINVAL, "jn_match_detections: bad shape");
  JN_CHECK(Nmax <= JN_EVAL_MAX_BOXES && Mmax <= JN_EVAL_MAX_BOXES, JN_EINVAL,
           "jn_match_detections: %d predictions / %d targets per image, at most %d of either", Nmax, Mmax, JN_EVAL_MAX_BOXES);
  if (B == 0) return JN_OK;
  launch_match_detections(preds_dev, pred_counts_dev, B, Nmax, W, targets_dev, target_counts_dev, Mmax, max_det, scores_dev,
                          hits_dev, sel_dev, n_pred_dev, n_gt_dev, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_average_precision(const double* scores_dev, const int32_t* hits_dev, const int32_t* n_pred_dev,
                         const int32_t* n_gt_dev, int B, int max_det, int pooled, const double* thresholds_dev,
                         int n_thresholds, double* out_dev, void* stream) {
  JN_CHECK(scores_dev && hits_dev && n_pred_dev && n_gt_dev && thresholds_dev && out_dev, JN_EINVAL,
           "jn_average_precision: null argument");
  JN_CHECK(B >= 1 && max_det >= 1, JN_EINVAL, "jn_average_precision: bad shape");
  JN_CHECK(n_thresholds >= 1 && n_thresholds <= JN_EVAL_MAX_THRESHOLDS, JN_EINVAL,
           "jn_average_precision: %d thresholds, at most %d", n_thresholds, JN_EVAL_MAX_THRESHOLDS);
  const long long slots = (long long)(pooled ? B : 1) * max_det;
  JN_CHECK(slots <= JN_EVAL_MAX_ENTRIES, JN_EINVAL, "jn_average_precision: a segment of %lld entries, at most %d", slots,
           JN_EVAL_MAX_ENTRIES);
  JN_CHECK(launch_average_precision(scores_dev, hits_dev, n_pred_dev, n_gt_dev, B, max_det, pooled, thresholds_dev, n_thresholds,
                                    out_dev, (hipStream_t)stream) == 0,
           JN_EHIP, "jn_average_precision: LDS for %lld entries refused", slots);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_average_precision_segments(const double* scores_dev, const int32_t* hits_dev, const int32_t* n_pred_dev,
                                  const int32_t* n_gt_dev, int U, int max_det, const int32_t* seg_offsets_dev, int NS,
                                  int max_units, const double* thresholds_dev, int n_thresholds, double* out_dev, void* stream) {
  JN_CHECK(scores_dev && hits_dev && n_pred_dev && n_gt_dev && seg_offsets_dev && thresholds_dev && out_dev, JN_EINVAL,
           "jn_average_precision_segments: null argument");
  JN_CHECK(U >= 1 && max_det >= 1 && NS >= 1 && max_units >= 1, JN_EINVAL, "jn_average_precision_segments: bad shape");
  JN_CHECK(n_thresholds >= 1 && n_thresholds <= JN_EVAL_MAX_THRESHOLDS, JN_EINVAL,
           "jn_average_precision_segments: %d thresholds, at most %d", n_thresholds, JN_EVAL_MAX_THRESHOLDS);
  const long long slots = (long long)max_units * max_det;
  JN_CHECK(slots <= JN_EVAL_MAX_ENTRIES, JN_EINVAL,
           "jn_average_precision_segments: a segment of %lld entries (%d units of %d), at most %d", slots, max_units, max_det,
           JN_EVAL_MAX_ENTRIES);
  JN_CHECK(launch_average_precision_segments(scores_dev, hits_dev, n_pred_dev, n_gt_dev, U, max_det, seg_offsets_dev, NS, max_units,
                                             thresholds_dev, n_thresholds, out_dev, (hipStream_t)stream) == 0,
           JN_EHIP, "jn_average_precision_segments: LDS for %lld entries refused", slots);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_pool_walk_detections(const float* det_boxes_dev, const int32_t* det_counts_dev, const int64_t* positions_dev,
                            const int32_t* walk_tokens_dev, const int32_t* walk_first_dev, const int32_t* walk_count_dev, int A,
                            int T, int S, int K_det, int NI, int max_walks, int Gh, int Gw, int max_per_cell,
                            float* cell_boxes_dev, int32_t* cell_counts_dev, int32_t* cell_stats_dev, uint8_t* visited_dev,
                            void* stream) {
  JN_CHECK(det_boxes_dev && det_counts_dev && positions_dev && walk_tokens_dev && walk_first_dev && walk_count_dev &&
               cell_boxes_dev && cell_counts_dev && visited_dev,
           JN_EINVAL, "jn_pool_walk_detections: null argument");
  JN_CHECK(NI >= 1 && max_per_cell >= 1, JN_EINVAL, "jn_pool_walk_detections: NI=%d max_per_cell=%d, both must be at least 1", NI,
           max_per_cell);
  JN_CHECK(A >= 1 && S >= 0 && S <= T && K_det >= 1 && max_walks >= 1 && Gh >= 1 && Gw >= 1 && NI <= 65535, JN_EINVAL,
           "jn_pool_walk_detections: bad shape");
  const long long pool = (long long)max_walks * (S + 1) * K_det;
  JN_CHECK(pool <= JN_EVAL_MAX_BOXES, JN_EINVAL,
           "jn_pool_walk_detections: a pool of up to %lld boxes per cell (%d walks x %d tokens x %d), the kernel holds at most %d "
           "in LDS", pool, max_walks, S + 1, K_det, JN_EVAL_MAX_BOXES);
  JN_CHECK(launch_pool_walk_detections(det_boxes_dev, det_counts_dev, positions_dev, walk_tokens_dev, walk_first_dev,
                                       walk_count_dev, A, T, S, K_det, NI, max_walks, Gh, Gw, max_per_cell, cell_boxes_dev,
                                       cell_counts_dev, cell_stats_dev, visited_dev, (hipStream_t)stream) == 0,
           JN_EHIP, "jn_pool_walk_detections: LDS for %lld boxes refused", pool);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// (the extents live on the device and an extent beyond the grid would index past the kernel's LDS lists, so they are
// read back and checked here: one small copy and a stream sync, in ragged mode only)
int jn_detection_cells(const int64_t* bboxes_dev, const int32_t* extents_dev, int B, int nb, int Gh, int Gw, int P,
                       int sample_neg, uint64_t seed, int capacity, int64_t* cells_dev, int64_t* targets_dev,
                       int32_t* offsets_dev, int32_t* n_pos_dev, void* stream) {
  JN_CHECK(offsets_dev && ((bboxes_dev && n_pos_dev) || B == 0) && ((cells_dev && targets_dev) || capacity == 0), JN_EINVAL,
           "jn_detection_cells: null argument");
  JN_CHECK(B >= 0 && capacity >= 0, JN_EINVAL, "jn_detection_cells: B=%d capacity=%d", B, capacity);
  JN_CHECK(nb >= 1 && P >= 1 && sample_neg >= 0, JN_EINVAL, "jn_detection_cells: nb=%d P=%d sample_neg=%d", nb, P, sample_neg);
  JN_CHECK(Gh >= 1 && Gw >= 1 && (long long)Gh * Gw <= JN_DETCELLS_MAX_CELLS, JN_EINVAL,
           "jn_detection_cells: a grid of %d x %d cells, the kernel holds at most %d per image in LDS", Gh, Gw,
           JN_DETCELLS_MAX_CELLS);
  JN_CHECK((long long)B * Gh * Gw <= INT32_MAX, JN_EINVAL, "jn_detection_cells: B * Gh * Gw beyond the int32 offsets");
  if (extents_dev && B > 0) {
    std::vector<int32_t> ext(2 * (size_t)B);
    JN_HIP(hipMemcpyAsync(ext.data(), extents_dev, ext.size() * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    JN_HIP(hipStreamSynchronize((hipStream_t)stream));
    for (int b = 0; b < B; ++b)
      JN_CHECK(ext[2 * b] >= 1 && ext[2 * b] <= Gh && ext[2 * b + 1] >= 1 && ext[2 * b + 1] <= Gw, JN_EINVAL,
               "jn_detection_cells: extent %d x %d of image %d outside 1..%d x 1..%d", ext[2 * b], ext[2 * b + 1], b, Gh, Gw);
  }
  launch_detection_cells(bboxes_dev, extents_dev, B, nb, Gh, Gw, P, sample_neg, seed, capacity, cells_dev, targets_dev,
                         offsets_dev, n_pos_dev, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_teacher_actions(const int64_t* positions_dev, const uint8_t* visited_dev, const uint8_t* targets_dev, int B, int Gh,
                       int Gw, uint8_t* sets_dev, void* stream) {
  JN_CHECK(positions_dev && visited_dev && targets_dev && sets_dev, JN_EINVAL, "jn_teacher_actions: null argument");
  JN_CHECK(B >= 1 && Gh >= 1 && Gw >= 1 && (long long)Gh * Gw <= INT32_MAX, JN_EINVAL, "jn_teacher_actions: B=%d grid %dx%d", B,
           Gh, Gw);
  launch_teacher_sets(positions_dev, visited_dev, targets_dev, sets_dev, 1, B, Gh, Gw, nullptr, 0, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_action_sets(const int64_t* positions_dev, const uint8_t* visited_dev, const int32_t* extents_dev, const int64_t* forced_dev,
                   int N, int Gh, int Gw, int policy, int nA, uint16_t* sets_dev, void* stream) {
  JN_CHECK(positions_dev && visited_dev && sets_dev, JN_EINVAL, "jn_action_sets: null argument");
  JN_CHECK(N >= 1 && Gh >= 1 && Gw >= 1 && (long long)Gh * Gw <= INT32_MAX, JN_EINVAL, "jn_action_sets: N=%d grid %dx%d", N, Gh, Gw);
  JN_CHECK((policy == JN_MASK_GRID || policy == JN_MASK_UNVISITED) && (nA == 8 || nA == 9), JN_EINVAL,
           "jn_action_sets: policy %d (1: grid, 2: unvisited), %d actions (8 or 9)", policy, nA);
  launch_action_sets(positions_dev, visited_dev, extents_dev, forced_dev, N, Gh, Gw, policy, nA, sets_dev, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_teacher_walks(const int64_t* bboxes_dev, const int64_t* start_positions_dev, int B, int nb, int Gh, int Gw, int P,
                     int T, int min_keypoints, int max_keypoints, int binomial_keypoints, uint64_t seed, int capacity,
                     int64_t* positions_dev, int64_t* current_actions_dev, int64_t* next_actions_dev, int64_t* labels_dev,
                     float* masks_dev, float* local_bboxes_dev, int32_t* n_steps_dev, uint8_t* targets_dev,
                     int64_t* cells_dev, float* bboxes_yolox_dev, int32_t* offsets_dev, void* stream) {
  JN_CHECK(B >= 0 && nb >= 0 && P >= 1 && capacity >= 0, JN_EINVAL, "jn_teacher_walks: B=%d nb=%d P=%d capacity=%d", B, nb, P,
           capacity);
  JN_CHECK(Gh >= 1 && Gw >= 1 && (long long)Gh * Gw <= JN_TWALK_MAX_CELLS, JN_EINVAL,
           "jn_teacher_walks: a grid of %d x %d cells, the kernel holds at most %d per image in LDS", Gh, Gw, JN_TWALK_MAX_CELLS);
  JN_CHECK(T >= 1 && T <= JN_TWALK_MAX_T, JN_EINVAL, "jn_teacher_walks: T=%d, the LDS ring holds 1..%d steps", T, JN_TWALK_MAX_T);
  JN_CHECK(min_keypoints >= 0 && max_keypoints >= min_keypoints && max_keypoints <= JN_TWALK_MAX_KEYPOINTS, JN_EINVAL,
           "jn_teacher_walks: min_keypoints=%d max_keypoints=%d, need 0 <= min <= max <= %d (the detour table)", min_keypoints,
           max_keypoints, JN_TWALK_MAX_KEYPOINTS);
  JN_CHECK((long long)B * Gh * Gw <= INT32_MAX, JN_EINVAL, "jn_teacher_walks: B * Gh * Gw beyond the int32 offsets");
  JN_CHECK(offsets_dev, JN_EINVAL, "jn_teacher_walks: null offsets");
  if (B == 0) {
    JN_HIP(hipMemsetAsync(offsets_dev, 0, sizeof(int32_t), (hipStream_t)stream));
    return JN_OK;
  }
  JN_CHECK(positions_dev && current_actions_dev && next_actions_dev && labels_dev && masks_dev && n_steps_dev && targets_dev,
           JN_EINVAL, "jn_teacher_walks: null output");
  JN_CHECK((bboxes_dev && local_bboxes_dev) || nb == 0, JN_EINVAL, "jn_teacher_walks: null boxes with nb=%d", nb);
  JN_CHECK((cells_dev && (bboxes_yolox_dev || nb == 0)) || capacity == 0, JN_EINVAL,
           "jn_teacher_walks: null detector rows with capacity=%d", capacity);
  TeacherWalkArgs a{bboxes_dev, start_positions_dev, B, nb, Gh, Gw, P, T, min_keypoints, max_keypoints,
                    binomial_keypoints != 0, seed, capacity, positions_dev, current_actions_dev, next_actions_dev, labels_dev,
                    masks_dev, local_bboxes_dev, n_steps_dev, targets_dev, cells_dev, bboxes_yolox_dev, offsets_dev};
  launch_teacher_walks(a, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

}  // extern "C"
