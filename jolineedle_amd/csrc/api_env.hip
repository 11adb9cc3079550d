// C ABI of libjnroll.so, environment unit: the env state, its patch sources (plain images, views, ragged extents) and the step calls.
// Host code only (compiled by hipcc as C++); kernels live in kernels_*.hip.
#include "jn_internal.h"

namespace jnr {

// ---- environment ---------------------------------------------------------------------
EnvPtrs env_ptrs(jn_ctx* ctx) {
  const EnvState& e = ctx->env;
  EnvPtrs p{e.positions, e.bbox_masks, e.visited, e.steps, e.has_stopped, e.n_bbox_tiles, ctx->found,
            e.B, e.Gh, e.Gw, e.T, e.stop, e.ragged ? e.extent : nullptr};
  return p;
}

// the env's images are read in place by the gathers and the stems; images_u8 selects the byte instantiations
void env_gather(const EnvState& e, float* out, long long out_sample_stride, int P, const int* skip_flag, int skip_when,
                hipStream_t s) {
  if (e.view_mode)
    launch_view_gather(e.views, e.images_u8, nullptr, e.positions, out, 0, out_sample_stride, e.B, P, skip_flag, skip_when, s);
  else if (e.images_u8)
    launch_gather((const uint8_t*)e.images, e.positions, out, out_sample_stride, e.B, 3, e.H, e.W, P, skip_flag, skip_when, s);
  else
    launch_gather((const float*)e.images, e.positions, out, out_sample_stride, e.B, 3, e.H, e.W, P, skip_flag, skip_when, s);
}

StemSrc env_stem_src(const EnvState& e, const int64_t* positions) {
  StemSrc ss{e.images, positions, 3LL * e.H * e.W, (long long)e.H * e.W, e.W};
  ss.src_u8 = e.images_u8;
  return ss;
}

// ---- view mode: the staging stack [cols][B][3][P][P] (element type of the sources) ----
static size_t stage_col_bytes(const EnvState& e, int P) { return (size_t)e.B * 3 * P * P * (e.images_u8 ? 1 : sizeof(float)); }
// cols = 1: every step overwrites the one column (stream order keeps its reader ahead of the next writer);
// cols = T + 1: column t holds the patches at positions[:, t] until the next rollout (the training backward and the
// detector's second stream read them later).  Sized for this env, not for max_batch: it is the one large view-mode buffer.
int ensure_stage(jn_ctx* ctx, int cols) {
  EnvState& e = ctx->env;
  // (whole 2 MiB granules, which is what the driver hands out for a buffer of this size anyway: the tail of the last
  // granule is then not shared with the context's small allocations, whose packing stays what it is in plain mode)
  const size_t granule = (size_t)2 << 20;
  const size_t need = ((size_t)cols * stage_col_bytes(e, ctx->cfg.patch_size) + granule - 1) / granule * granule;
  e.stage_cols = cols;
  if (e.stage && e.stage_bytes >= need) return JN_OK;
  if (e.stage) { JN_HIP(hipDeviceSynchronize()); JN_HIP(hipFree(e.stage)); e.stage = nullptr; e.stage_bytes = 0; }
  hipError_t er = hipMalloc(&e.stage, need);
  if (er != hipSuccess) { e.stage = nullptr; set_error("hipMalloc(%zu bytes) for the view staging stack failed: %s", need, hipGetErrorString(er)); return JN_ENOMEM; }
  e.stage_bytes = need;
  return JN_OK;
}
static void* stage_col(const EnvState& e, int P, int t) {
  return (char*)e.stage + (e.stage_cols == 1 ? 0 : (size_t)t) * stage_col_bytes(e, P);
}
void stage_fill(const EnvState& e, int P, int t, const int* skip_flag, int skip_when, hipStream_t s) {
  launch_view_gather(e.views, e.images_u8, nullptr, e.positions, stage_col(e, P, t), e.images_u8, 3LL * P * P, e.B, P, skip_flag,
                     skip_when, s);
}
// column t as the plain patch stack the supervised step already feeds the stems (positions = NULL)
StemSrc stage_stem_src(const EnvState& e, int P, int t) {
  StemSrc ss = patch_src(stage_col(e, P, t), P);
  ss.src_u8 = e.images_u8;
  return ss;
}

static int env_init_impl(jn_ctx* ctx, const void* images_dev, int images_u8, const int64_t* bboxes_dev, int B, int H, int W,
                         int nb, int max_ep_len, int stop_enabled, void* stream, const jn_image_view* views_host = nullptr,
                         const int32_t* extents_host = nullptr) {
  const int P = ctx->cfg.patch_size;
  JN_CHECK(B >= 1 && B <= ctx->cfg.max_batch, JN_EINVAL, "B=%d exceeds max_batch=%d", B, ctx->cfg.max_batch);
  // general_env.py:50-51
  JN_CHECK(H % P == 0 && W % P == 0, JN_EINVAL, "image %dx%d is not divisible by patch_size %d", H, W, P);
  JN_CHECK(H / P <= 256 && W / P <= 256, JN_EINVAL, "patch grid larger than 256");
  JN_CHECK(max_ep_len >= 1 && max_ep_len <= ctx->cfg.block_size, JN_EINVAL, "max_ep_len %d > block_size %d", max_ep_len,
           ctx->cfg.block_size);
  JN_HIP(hipSetDevice(ctx->cfg.device));
  EnvState& e = ctx->env;
  const int Gh = H / P, Gw = W / P;
  int rc;
  if (!e.positions) {
    const int MB = ctx->cfg.max_batch;
    if ((rc = dev_alloc(ctx, &e.positions, (size_t)MB * 2))) return rc;
    if ((rc = dev_alloc(ctx, &e.bbox_masks, (size_t)MB * 256 * 256))) return rc;
    if ((rc = dev_alloc(ctx, &e.visited, (size_t)MB * 256 * 256))) return rc;
    if ((rc = dev_alloc(ctx, &e.steps, (size_t)MB))) return rc;
    if ((rc = dev_alloc(ctx, &e.has_stopped, (size_t)MB))) return rc;
    if ((rc = dev_alloc(ctx, &e.n_bbox_tiles, (size_t)MB))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->found, (size_t)MB))) return rc;
    // the two small tables of view mode come with the env state (24 KB at the headline sizes), so that switching to
    // views later allocates nothing but the staging stack
    if ((rc = dev_alloc(ctx, &e.views, (size_t)MB))) return rc;
    if ((rc = dev_alloc(ctx, &e.stage_pos, (size_t)(ctx->cfg.block_size + 1) * MB * 2))) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  if (views_host) {
    // the previous table may still be read by work in flight; the new one is in place before anything launched below
    JN_HIP(hipStreamSynchronize(s));
    JN_HIP(hipMemcpy(e.views, views_host, (size_t)B * sizeof(jn_image_view), hipMemcpyHostToDevice));
    if (e.stage_pos_B != B) {
      std::vector<int64_t> sp((size_t)(ctx->cfg.block_size + 1) * B * 2, 0);
      for (int t = 0; t <= ctx->cfg.block_size; ++t)
        for (int b = 0; b < B; ++b) sp[((size_t)t * B + b) * 2] = 3LL * B * t;
      JN_HIP(hipMemcpy(e.stage_pos, sp.data(), sp.size() * sizeof(int64_t), hipMemcpyHostToDevice));
      e.stage_pos_B = B;
    }
    ctx->train_out_valid = false;     // the staged patches of an earlier rollout belong to the earlier views
  }
  if (extents_host) {
    if (!e.extent && (rc = dev_alloc(ctx, &e.extent, (size_t)ctx->cfg.max_batch * 2))) return rc;
    // (ragged mode comes with views: the stream was drained for their table above)
    JN_HIP(hipMemcpy(e.extent, extents_host, (size_t)B * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  e.ragged = extents_host != nullptr;
  e.view_mode = views_host != nullptr;
  e.images = images_dev; e.images_u8 = images_u8;
  e.B = B; e.H = H; e.W = W; e.nb = nb; e.Gh = Gh; e.Gw = Gw; e.T = max_ep_len;
  e.stop = stop_enabled ? 1 : 0;
  launch_bbox_masks(bboxes_dev, e.bbox_masks, e.n_bbox_tiles, B, nb, H, W, P, s, e.ragged ? e.extent : nullptr);
  launch_env_reset(env_ptrs(ctx), nullptr, 0, nullptr, s);   // zeroed state at (0,0)-independent start; reset() follows
  JN_HIP(hipGetLastError());
  e.ready = true;
  return JN_OK;
}

// the checks jn_env_init_views and jn_env_init_ragged share; extents_host = null: plain view mode
static int env_init_views_impl(jn_ctx* ctx, const jn_image_view* views_host, const int32_t* extents_host, const int64_t* bboxes_dev,
                               int B, int Hc, int Wc, int nb, int max_ep_len, int stop_enabled, void* stream) {
  JN_CHECK(B >= 1 && B <= ctx->cfg.max_batch, JN_EINVAL, "B=%d exceeds max_batch=%d", B, ctx->cfg.max_batch);
  const int P = ctx->cfg.patch_size;
  JN_CHECK(Hc >= P && Wc >= P && Hc % P == 0 && Wc % P == 0, JN_EINVAL, "canvas %dx%d is not a multiple of patch_size %d", Hc, Wc, P);
  for (int b = 0; b < B; ++b) {
    const jn_image_view& v = views_host[b];
    JN_CHECK(v.src, JN_EINVAL, "view %d: null source", b);
    JN_CHECK(v.rot == 0 || v.rot == 90 || v.rot == 180 || v.rot == 270, JN_EINVAL, "view %d: rot %d is not 0, 90, 180 or 270", b, v.rot);
    JN_CHECK(v.Hs >= 1 && v.Ws >= 1, JN_EINVAL, "view %d: stored size %dx%d", b, v.Hs, v.Ws);
    const bool turned = v.rot == 90 || v.rot == 270;
    JN_CHECK((turned ? v.Ws : v.Hs) <= Hc && (turned ? v.Hs : v.Ws) <= Wc, JN_EINVAL,
             "view %d: the rotated image %dx%d does not fit the canvas %dx%d", b, turned ? v.Ws : v.Hs, turned ? v.Hs : v.Ws, Hc, Wc);
    JN_CHECK((v.src_u8 == 0 || v.src_u8 == 1) && v.src_u8 == views_host[0].src_u8, JN_EINVAL,
             "view %d: mixed element types within one env", b);
    if (extents_host) {
      const int gh = extents_host[2 * b], gw = extents_host[2 * b + 1];
      JN_CHECK(gh >= 1 && gh <= Hc / P && gw >= 1 && gw <= Wc / P, JN_EINVAL,
               "view %d: extent %dx%d is outside the canvas grid %dx%d", b, gh, gw, Hc / P, Wc / P);
      JN_CHECK(v.ty == 0 && v.tx == 0, JN_EINVAL, "view %d: a ragged env takes no translation (ty %d, tx %d)", b, v.ty, v.tx);
      JN_CHECK((turned ? v.Ws : v.Hs) <= gh * P && (turned ? v.Hs : v.Ws) <= gw * P, JN_EINVAL,
               "view %d: the rotated image %dx%d does not fit its extent %dx%d patches", b, turned ? v.Ws : v.Hs,
               turned ? v.Hs : v.Ws, gh, gw);
    }
  }
  return env_init_impl(ctx, nullptr, views_host[0].src_u8, bboxes_dev, B, Hc, Wc, nb, max_ep_len, stop_enabled, stream, views_host,
                       extents_host);
}

}  // namespace jnr

using namespace jnr;

extern "C" {

int jn_env_init(jn_ctx* ctx, const float* images_dev, const int64_t* bboxes_dev, int B, int H, int W, int nb,
                int max_ep_len, int stop_enabled, void* stream) {
  JN_CHECK(ctx && images_dev && (bboxes_dev || nb == 0), JN_EINVAL, "jn_env_init: null argument");
  return env_init_impl(ctx, images_dev, 0, bboxes_dev, B, H, W, nb, max_ep_len, stop_enabled, stream);
}

int jn_env_init_u8(jn_ctx* ctx, const uint8_t* images_dev, const int64_t* bboxes_dev, int B, int H, int W, int nb,
                   int max_ep_len, int stop_enabled, void* stream) {
  JN_CHECK(ctx && images_dev && (bboxes_dev || nb == 0), JN_EINVAL, "jn_env_init_u8: null argument");
  return env_init_impl(ctx, images_dev, 1, bboxes_dev, B, H, W, nb, max_ep_len, stop_enabled, stream);
}

int jn_env_init_views(jn_ctx* ctx, const jn_image_view* views_host, const int64_t* bboxes_dev, int B, int Hc, int Wc, int nb,
                      int max_ep_len, int stop_enabled, void* stream) {
  JN_CHECK(ctx && views_host && (bboxes_dev || nb == 0), JN_EINVAL, "jn_env_init_views: null argument");
  return env_init_views_impl(ctx, views_host, nullptr, bboxes_dev, B, Hc, Wc, nb, max_ep_len, stop_enabled, stream);
}

int jn_env_init_ragged(jn_ctx* ctx, const jn_image_view* views_host, const int32_t* extents_host, const int64_t* bboxes_dev, int B,
                       int Hc, int Wc, int nb, int max_ep_len, int stop_enabled, void* stream) {
  JN_CHECK(ctx && views_host && extents_host && (bboxes_dev || nb == 0), JN_EINVAL, "jn_env_init_ragged: null argument");
  return env_init_views_impl(ctx, views_host, extents_host, bboxes_dev, B, Hc, Wc, nb, max_ep_len, stop_enabled, stream);
}

int jn_env_reset(jn_ctx* ctx, const int64_t* positions_dev, uint64_t seed, void* stream) {
  JN_CHECK(ctx && ctx->env.ready, JN_ESTATE, "jn_env_init has not been called");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  launch_env_reset(env_ptrs(ctx), positions_dev, seed, nullptr, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_env_step(jn_ctx* ctx, const int64_t* actions_dev, float* rewards_dev, uint8_t* terminated_dev,
                uint8_t* truncated_dev, void* stream) {
  JN_CHECK(ctx && ctx->env.ready, JN_ESTATE, "jn_env_init has not been called");
  JN_CHECK(actions_dev, JN_EINVAL, "jn_env_step: null actions");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  launch_env_step(env_ptrs(ctx), actions_dev, rewards_dev, terminated_dev, truncated_dev, (hipStream_t)stream);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_env_state(jn_ctx* ctx, int what, void** ptr_dev) {
  JN_CHECK(ctx && ptr_dev && ctx->env.ready, JN_ESTATE, "jn_env_init has not been called");
  switch (what) {
    case 0: *ptr_dev = ctx->env.positions; break;
    case 1: *ptr_dev = ctx->env.bbox_masks; break;
    case 2: *ptr_dev = ctx->env.visited; break;
    case 3: *ptr_dev = ctx->env.steps; break;
    case 4: *ptr_dev = ctx->env.has_stopped; break;
    case 5: *ptr_dev = ctx->env.ragged ? ctx->env.extent : nullptr; break;   // null outside ragged mode
    default: set_error("jn_env_state: unknown selector %d", what); return JN_EINVAL;
  }
  return JN_OK;
}

int jn_env_patches(jn_ctx* ctx, float* out_dev, void* stream) {
  JN_CHECK(ctx && ctx->env.ready && out_dev, JN_ESTATE, "jn_env_init has not been called");
  const EnvState& e = ctx->env;
  if (e.view_mode) {
    const int P = ctx->cfg.patch_size;
    env_gather(e, out_dev, 3LL * P * P, P, nullptr, 0, (hipStream_t)stream);
    JN_HIP(hipGetLastError());
    return JN_OK;
  }
  if (e.images_u8)
    return jn_gather_patches_u8((const uint8_t*)e.images, e.positions, out_dev, e.B, 3, e.H, e.W, ctx->cfg.patch_size, stream);
  return jn_gather_patches((const float*)e.images, e.positions, out_dev, e.B, 3, e.H, e.W, ctx->cfg.patch_size, stream);
}

}  // extern "C"
