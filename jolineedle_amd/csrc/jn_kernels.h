// Host-callable launchers of the HIP kernels (internal; not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/jnroll.h"

namespace jnr {

enum { ACT_NONE = 0, ACT_SILU = 1, ACT_RELU = 2, ACT_SIGMOID = 3 };
enum { JN_F32 = 0, JN_BF16 = 1 };   // storage type of an activation buffer (jn_types.h)

// Atomic accumulators (BN statistics, weight-gradient partials) are replicated JN_NREP times and a
// workgroup adds into replica (block id % JN_NREP): same-address contention drops 32x; the consumer
// (finalize / reduce kernels) sums the replicas.
constexpr int JN_NREP = 32;
constexpr int JN_WPART_MAX = 16384;   // floats per replica of the weight-gradient scratch
constexpr int JN_BN_BWD_MAX_C = 1280; // channels of one launch_bn_bwd_reduce call (above 1024: two halves; yolox-x's widest layer)
// What launch_bn_bwd_reduce takes: whole channel quads, and above 1024 channels two halves of whole quads (pure host code; the
// launcher returns -1 where this is false, check_can_train asks it for every BatchNorm layer before a training pass starts)
inline bool bn_bwd_reduce_admits(int C) { return C >= 4 && C % 4 == 0 && C <= JN_BN_BWD_MAX_C && (C <= 1024 || C % 8 == 0); }

// Every hot-loop kernel takes (skip_flag, skip_when): it returns at once when
// *skip_flag >= skip_when.  The rollout points skip_flag at n_done[t] with skip_when = B,
// which reproduces the reference's early `break` (src/reinforce.py:181-184) with no host sync.
// Per-channel "normalize on read" table of a buffer view: a = fl ? silu(z * sc + sh) : z.
struct ChanTab {
  float* sc; float* sh; float* fl;
  // Deferred entries (train-mode forward, DESIGN.md §4 "consumer-side BatchNorm tables"): a layer whose output has at
  // most JN_DEFER_MAX_M pixels in this launch gets NO bn_finalize launch; its consumers derive (scale, shift) of such a
  // channel from the producer's batch sums in their prologue (jn_tab.h), and ONE bn_finalize_all launch at the end of the
  // pass writes the table, the saved statistics and the running averages of all those layers.  All arrays below are
  // indexed like sc / sh / fl (per view channel); dsrc == nullptr: a plain table.
  const int* dsrc;         // index of the channel's (sum, sumsq) pair inside one replica of dstats, or -1 (never deferred)
  const float* dhw;        // H * W of the layer that produced the channel (the count is dN * dhw)
  const int* dgoff; const int* dboff;   // offsets of the channel's BatchNorm weight / bias in dparams
  const float* dparams;    // parameter arena
  const double* dstats;    // [JN_NREP_DEFER used][drep_stride] batch sums of the workspace slot
  long long drep_stride;
  int dN;                  // patches in this pass
  long long dmax;          // deferral limit in pixels (dN * dhw <= dmax: deferred), JN_DEFER_MAX_M
  // The same information as up to four channel runs in the kernel arguments (scalar registers, no memory round trip
  // before the sums can be requested): channels [c0, c1) of the view are BatchNorm channels stat0 + (c - c0) with affine
  // at g0 / b0 + (c - c0) and pixel count dN * hw — or, with stat0 < 0, plain table entries.  nseg == 0: use the arrays.
  // (four named members, not an array: an indexed array inside a by-value kernel argument sends the whole struct to
  // scratch memory — measured: 192 B / lane of scratch in every forward kernel and 30 - 50 % longer 28x28 layers)
  struct Run { int c0, c1, stat0, g0, b0; float hw; };
  int nseg;
  Run r0, r1, r2, r3;
};
constexpr long long JN_DEFER_MAX_M = 65536;   // output pixels (N * H * W) up to which a layer's table is deferred
constexpr int JN_NREP_DEFER = 8;              // statistics replicas such a layer accumulates into (its consumers sum them)

// Step batching of the backward: ONE launch covers `n` workspace slots (glimpse steps of a trajectory, each
// with its own batch-statistics tables); slot j adds j * stride to the per-slot pointers.  The default is the
// single-pass case.
struct SlotBatch {
  int n = 1;
  long long act = 0;      // activation elements between slots (z / x buffers)
  long long grad = 0;     // gradient floats between slots
  long long tab = 0;      // table floats between slots (the sc / sh / fl arrays each move by this)
  long long save = 0;     // saved (mean, invstd) floats between slots
  long long red = 0;      // doubles between slots of the reduction scratch
  long long consts = 0;   // floats between slots of the per-channel constants
  long long pos = 0;      // int64 elements between slots of the stem's patch positions
};

// Dynamic LDS above the 64 KB every kernel may use has to be granted per kernel (hipFuncAttributeMaxDynamicSharedMemorySize).
// Keeps, per kernel, the bytes granted so far and asks the runtime only when a launch needs more; false: refused.
template <auto Kernel>
bool allow_lds(size_t bytes) {
  static size_t granted = 64 * 1024;
  if (bytes <= granted) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return false;
  granted = bytes;
  return true;
}

// The most dynamic LDS a launcher asks to be granted: the 160 KB of a gfx950 CU less room for a kernel's static arrays
constexpr size_t JN_LDS_GRANT_MAX = 159 * 1024;

// Persistent grids are sized in resident rounds: workgroups one CU holds x the CUs of the chip.
constexpr int JN_NUM_CU = 256;
// Workgroups (256 threads, `smem` bytes of dynamic LDS) of the kernel that fit one CU: asked once per kernel, whose LDS
// size is a function of its template arguments; `fallback` when the runtime cannot say.  LDS above 64 KB: allow_lds first.
template <auto Kernel>
int resident_per_cu(size_t smem, int fallback) {
  static int per_cu = 0;
  if (!per_cu && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(Kernel), 256, smem) != hipSuccess || per_cu < 1))
    per_cu = fallback;
  return per_cu;
}

struct StemArgs {
  const void* src; const int64_t* positions; int pos_stride;    // positions[pos_stride * n + {0,1}] = (y, x)
  long long sample_stride, chan_stride; int row_stride;
  int P, N, cout;
  const float* w; void* out; int out_ld; int out_dtype;
  double* stats;                    // [JN_NREP][rep_stride]: [cout][2] sum / sumsq accumulators (train) or null
  long long stats_rep_stride;
  const int* skip_flag; int skip_when;
  int stats_nrep;                   // replicas in use (0 -> JN_NREP)
  int src_u8;                       // src holds uint8 (byte b = b / 255) instead of fp32; strides count elements
};

struct ConvArgs {
  const void* in; int in_ld; int in_dtype; ChanTab itab;
  const float* w; const float* bias;     // bias only for BN-free layers
  const void* w_bf16;                    // dense 3x3, bf16 mode: pre-rounded copy of w (or null)
  void* out; int out_ld; int out_dtype;
  int bf16_mfma;                         // 1x1 / dense 3x3: bf16 operands on v_mfma_f32_16x16x32_bf16
  int N, H, W, OH, OW, cin, cout, stride, act;
  int accumulate;                        // out += (gradient buffers)
  int w_transposed;                      // pw: w is [cin][cout] and read transposed (data-gradient)
  int in_identity;                       // the input needs no "normalize on read" (gradient views): kernels may skip the transform
  double* stats; long long stats_rep_stride;
  int stats_nrep;                        // replicas the workgroups spread their sums over (0 -> JN_NREP)
  const int* skip_flag; int skip_when;
  int n_slots;                           // pw: gridDim.z slots, pointers advance by the strides below (0 -> 1 slot)
  long long in_slot_stride, out_slot_stride, tab_slot_stride;
  const void* w_x3;                      // 1x1, fp32: the weights split into three bf16 planes (launch_w_split3), or null
  void* up_out; int up_ld;               // 1x1, fp32: also store the output nearest-x2 upsampled here (pixel stride up_ld floats), where
                                         // pw_fuses_upsample(pw_route(a), cin, cout); null: no
};

// eval-mode DWConv (depthwise 3x3 -> BN + SiLU -> pointwise 1x1) in one kernel; mtab = table of the depthwise output
struct DwPwArgs {
  const void* in; int in_ld; ChanTab itab; const float* w_dw; ChanTab mtab; const float* w_pw;
  void* out; int out_ld; int dtype; int C, cout, N, H, W, OH, OW, stride;
  const int* skip_flag; int skip_when;
  const void* res; int res_ld; ChanTab rtab;   // optional shortcut (eval): out = silu(bn(z)) + T(res), ptab = table of z
  ChanTab ptab;
};
bool dwpw_supported(int C, int cout, int stride);
int launch_dwpw(const DwPwArgs& a, hipStream_t s);
// (max_wg, here and in launch_stem_bwd_weight: debug entry, > 0 caps the persistent workgroups along x, so that one walks
// several tiles of a small batch.)  -1: an odd patch, output channels that are no whole blocks of 16, a null pointer
int launch_stem(const StemArgs& a, hipStream_t s, int max_wg = 0);
bool stem_args_ok(const StemArgs& a);
bool stem_rows_aligned(const StemArgs& a);        // the stem kernels may fetch the image tile with 4-element loads
// depthwise 3x3: the route of a launch (forced = 0: the launcher's rule; a forced route that does not admit the launch: -1)
enum { DW_ROUTE_LDS = 1, DW_ROUTE_STRIP = 2 };      // dw3x3_lds_kernel (C % 16 == 0, N <= 65535), dw3x3_kernel
int dw_route(const ConvArgs& a, int forced);
int launch_dw(const ConvArgs& a, hipStream_t s, int route = 0);
// ---- 1x1 convs: THE route of a launch (kernels_conv.hip) ------------------------------------------------------------
// Which kernel family runs a 1x1 conv is decided once, by pw_route, a pure function of the arguments (and of the test hook
// JN_PWN_MIN_M); launch_pw is a switch over it, and a launcher handed its route launches or fails (-1: no instantiation, or
// the LDS was refused).  The clauses, in order:
//   X1 / X3 / XS  at most JN_XS_MAX_M pixels, forward: the pixel-stationary kernels of kernels_pwxs.hip — bf16 inference
//                 mode, fp32 as three bf16 planes (a.w_x3 given and in fragment order), fp32 pipe
//   WIDE          K, N >= 64, forward and data gradient: pw_dir_kernel (kernels_pwres.hip)
//   NARROW        K <= 64, forward, at least JN_PW_BIG_M pixels: pw_narrow_kernel
//   MFMA          everything else: pw_mfma_kernel
// With a.up_out set only the routes and shapes of pw_fuses_upsample remain, anything else is NONE.
// Forced routes (the per-kernel tests, jn_pw in api_kernels.hip): pw_route(a, r) is r where that family's kernels admit the launch,
// else NONE; launch_pw(a, s, r) launches it.  max_wg > 0 caps the x extent of a persistent grid (MFMA has none: refused).
enum PwRoute { PW_NONE = 0, PW_X1, PW_X3, PW_XS, PW_WIDE, PW_NARROW, PW_MFMA };
PwRoute pw_route(const ConvArgs& a, int forced = 0);
int launch_pw(const ConvArgs& a, hipStream_t s, int route = 0, int max_wg = 0);
// THE tile variant pw_mfma_kernel<CT, KC, WT, WM, ..> gets: channel tiles per workgroup, K chunk, waves along the pixels (32 WM
// pixels per workgroup).  Pure host code, like pw_route; launch_pw's MFMA case is a switch over it.
struct PwMfmaVariant { int ct, kc, wm; };
PwMfmaVariant pw_mfma_variant(const ConvArgs& a);
// Pixels per launch (N * H * W; times the slots where said) at which the routes and tilings change:
// the pixel-stationary kernels up to here (the 56x56 / 28x28 / 14x14 maps of the headline batch: 10 - 30 % under the
// weight-stationary kernel on every one of them, profiles/r03_pwxsbench.txt)
constexpr long long JN_XS_MAX_M = 262144;
// from here on a persistent kernel has tiles to walk: pw_narrow_kernel's minimum (JN_PWN_MIN_M: test hook, read per launch so
// that a test can force the kernel onto small maps), and 64 -> 64 on pw_dir_kernel (below: pw_mfma_kernel, 14.3 against
// 14.6 us at 28x28)
constexpr long long JN_PW_BIG_M = 65536;
// pw_mfma_kernel, data gradients (all slots): 64-pixel workgroups up to here, 128-pixel ones above (JN_PW_WT_SMALL_M: test hook,
// read per launch - 0 forces the large-map variant onto the small parity shapes)
constexpr long long JN_PW_WT_SMALL_M = 65536;
// 14x14 maps at 64 patches: pw_mfma_kernel's 32-pixel workgroups (all slots), one pw_x3 workgroup per CU at 128 -> 128
constexpr long long JN_PW_TINY_M = 16384;
// fp32 buffers on the fp32 pipe, no bias / activation epilogue ...
inline bool pw_f32_bare(const ConvArgs& a) {
  return !a.bf16_mfma && a.in_dtype == JN_F32 && a.out_dtype == JN_F32 && !a.bias && a.act == ACT_NONE;
}
// ... of a plain forward layer: weight [N][K], output written, one slot
inline bool pw_f32_plain(const ConvArgs& a) { return pw_f32_bare(a) && !a.w_transposed && !a.accumulate && a.n_slots <= 1; }
bool pw_fuses_upsample(PwRoute r, int cin, int cout);  // kernels_pwxs.hip: the route's kernel for this shape can also write a.up_out
bool pw_res_supported(const ConvArgs& a);              // kernels_pwres.hip: shapes the resident-weight 1x1 kernels take (K, N >= 64)
int pw_dir_auto_ctw(int cin, int cout);                // launch_pw_dir's automatic slice (channel tiles), 0: none fits
// (max_wg, here and below: debug entry, > 0 caps the persistent workgroups along x, so that one walks several tiles of a small map)
int launch_pw_dir(const ConvArgs& a, int ctw, hipStream_t s, int max_wg = 0);
bool pw_xs_supported(const ConvArgs& a);               // kernels_pwxs.hip: pixel-stationary kernel for the small maps of a forward pass
int launch_pw_xs(const ConvArgs& a, int pt, hipStream_t s, int wg_per_cu = 0, int max_wg = 0);   // pt: pixel tiles per workgroup (0 = default)
// the same on the bf16 pipe (three-way split operands); needs a.w_x3.  frag: the order a.w_x3 is in (-1: the rule below; the
// other order of a shape is built for tools/pwxsbench.hip only)
int launch_pw_x3(const ConvArgs& a, int pt, hipStream_t s, int wg_per_cu = 0, int frag = -1, int max_wg = 0);
// THE layout rule of the split planes of a 1x1 conv (ConvArgs::w_x3): true = MFMA fragment order (kernels_pwxs.hip,
// w_split3_frag_kernel), false = the flat [row][k / 8][h | m | l] order of w_split3_kernel.  Asked by the splitter's table
// (api_net.hip) and by every reader: launch_pw_x3, its fused-upsample form and launch_pw_x1.  Shapes: what
// profiles/pwfrag_bench.txt decided, shape by shape — every shape pw_x3_kernel is built for gains more than the spread of
// the tool's repeats (K = 64, whose two k steps are fetched once per workgroup: 4 - 9 %; K >= 128: 9 - 41 %).
constexpr bool pw_x3_fragment_order(int cin, int cout) {
  return (cin == 64 && (cout == 64 || cout == 128)) || (cin == 128 && (cout == 64 || cout == 128 || cout == 256)) ||
         (cin == 256 && (cout == 128 || cout == 256)) || (cin == 512 && cout == 256);
}
struct X3FragConv { long long off; int cout, cin; };   // a conv of the splitter's table: arena offset of its weight (floats, % 8 == 0)
void launch_w_split3_frag(const float* params, void* params_x3, const X3FragConv* tab, int n_convs, int max_weights, hipStream_t s);
// the data gradient of a wide 1x1 layer on pw_x3_kernel (transposed split weight made on the way); -1: shape not taken
bool pw_x3_bwd_data_supported(int cout, int cin);
int launch_pw_x3_bwd_data(const ConvArgs& a, const float* w, void* w3t, hipStream_t s, int max_wg = 0);
bool pw_x1_supported(const ConvArgs& a);               // bf16 inference mode: single-plane form of the same kernel
int launch_pw_x1(const ConvArgs& a, hipStream_t s, int max_wg = 0);               // shapes on which the x3 kernel is the faster one
void launch_w_split3(const float* w, void* w3, long long n_floats, hipStream_t s);   // w3: 6 bytes per weight
// SPP: the route of a launch (forced = 0: the launchers' rule; a forced route that does not admit the launch: -1), pure host
// code; bwd = the backward pair of kernels.  The launchers return -1 where spp_route does, and for a null pointer.
enum { SPP_ROUTE_QUAD = 1, SPP_ROUTE_SCALAR = 2 };      // spp4_kernel / spp4_bwd_kernel; spp_kernel / spp_bwd_kernel
int spp_route(int dtype, int ld, int h, int H, int W, int N, int bwd, int forced);
int spp_scalar_channels(int H, int W, int bwd);         // channels per workgroup of the scalar kernels
int launch_spp(void* cat, int dtype, int ld, int h, int H, int W, int N, ChanTab it, const int* skip_flag,
               int skip_when, hipStream_t s, int route = 0);
int launch_upsample(const void* in, int in_ld, void* out, int out_ld, int dtype, int C, int H, int W, int N,
                    const int* skip_flag, int skip_when, hipStream_t s);
int launch_addact(const void* z, int z_ld, ChanTab zt, const void* res, int res_ld, ChanTab rt, void* out, int out_ld,
                  int dtype, int C, long long M, const int* skip_flag, int skip_when, hipStream_t s);
int launch_bn_finalize(const double* stats, long long rep_stride, double count, const float* gamma, const float* beta, float* run_mean,
                       float* run_var, float* save, ChanTab t0, ChanTab t1, int C, float eps, float momentum,
                       const int* skip_flag, int skip_when, hipStream_t s);
// deferred BatchNorm tables: one finalize launch per pass (kernels_conv.hip); arrays are per BatchNorm ("stat") channel
struct BnAllArgs {
  const double* stats; long long rep_stride; int n_stat; int N;
  const float* hw;                       // H * W of the channel's layer
  const int* goff; const int* boff;      // BatchNorm weight / bias offsets in params
  const float* params;
  const int* t0; const int* t1;          // table channel of the layer output, and of its upsampled alias (-1: none)
  float* tab; int tab_channels;          // the slot's table [3][tab_channels]
  float* save;                           // [n_stat][2] (mean, invstd)
  float* const* run_mean; float* const* run_var;   // per-channel addresses of the running statistics
  float eps, momentum;
  const int* skip_flag; int skip_when;
  long long defer_max_m;                 // layers with N * hw above it used all JN_NREP replicas
};
int launch_bn_finalize_all(const BnAllArgs& a, hipStream_t s);
int launch_nhwc_to_nchw(const void* in, int dtype, int in_ld, ChanTab it, float* out, int C, int HW, int N,
                        hipStream_t s);
int launch_efpn_linear(const float* e, const float* wt, float* part, int N, int K, int Co, int KS,
                       const int* skip_flag, int skip_when, hipStream_t s);

// ---- dense 3x3 conv (kernels_conv3.hip) ---------------------------------------------------------
// Every launcher takes a route: 0 = its own rule (what the networks pass), else that kernel family, for the per-kernel
// tests (jn_conv3* in api_kernels.hip).  The *_route functions are pure host code: the route a launch gets (forced = 0), or
// `forced` itself where the launch meets that route's preconditions; -1: refused.  The launchers return -1 likewise.
enum Conv3Route { C3_ROUTE_F32 = 1, C3_ROUTE_X3 = 2, C3_ROUTE_BF16 = 3 };      // conv3_mfma; conv3_x3 / conv3_x3s2 / conv3_x3_bwd_data_s2; conv3_bf16
enum Conv3WRoute { CW_ROUTE_TR = 1, CW_ROUTE_SPLIT = 2, CW_ROUTE_EXACT = 3 };  // conv3_bwd_weight_tr; conv3_bwd_weight<SP = true / false>
int conv3_route(const ConvArgs& a, int forced);
int launch_conv3(const ConvArgs& a, hipStream_t s, int route);     // w_transposed: data gradient of a stride-1 layer
int conv3_bwd_data_s2_route(int g_ld, int gin_ld, int OH, int OW, int Co, int Ci, int N, int n_slots, int forced);
int launch_conv3_bwd_data_s2(const float* gz, int g_ld, const float* w, float* gin, int gin_ld, int H, int W, int OH,
                             int OW, int Co, int Ci, int N, int accumulate, hipStream_t s, const SlotBatch& sb, int route);
int conv3_bwd_weight_route(int g_ld, int x_ld, int Co, int Ci, int forced);
// max_wg: 0 = the rule (2048 / (channel blocks x slots)), else the x extent of the persistent grid (1: one workgroup walks every pixel tile)
int launch_conv3_bwd_weight(const float* gz, int g_ld, const float* x, int x_ld, ChanTab it, float* gw, int H, int W, int OH,
                            int OW, int Co, int Ci, int N, int stride, hipStream_t s, const SlotBatch& sb, int route, int max_wg);
// ---- detector (kernels_det.hip) --------------------------------------------------------------
int launch_head_pred(const void* reg, int reg_ld, ChanTab rt, const void* cls, int cls_ld, ChanTab ct, int dtype,
                     const float* wp, const float* bp, float* raw, int hid, int Hl, int Wl, int stride, int A, int a0,
                     int N, hipStream_t s, int logits_only = 0);
int launch_det_scatter(const float* boxes, const int* counts, float* out_boxes, int* out_counts, int B, int cols, int col,
                       int K, const int* skip_flag, int skip_when, hipStream_t s);
// stats: nullable int [N][2] = (anchors with score >= conf before the 2048-candidate cap, NMS survivors before max_out)
int launch_postprocess(const float* raw, int A, int N, float conf, float nms_thr, float clamp_max, float* boxes,
                       int* counts, int max_out, int* stats, hipStream_t s);
// The same stage with EVERY passing anchor in the sort (no 2048-candidate cap): A <= POST_ALL_MAX_A, else nothing is
// launched and the return value is non-zero.  A <= 2048 goes to launch_postprocess (the two coincide there).
constexpr int POST_ALL_MAX_A = 8400;                    // 640 px at strides 8 / 16 / 32
int launch_postprocess_all(const float* raw, int A, int N, float conf, float nms_thr, float clamp_max, float* boxes,
                           int* counts, int max_out, int* stats, hipStream_t s);

// ---- detector training (kernels_detloss.hip) ------------------------------------------------------------
struct DetGeom { int A; int a0[3]; int H[3]; int W[3]; int stride[3]; };
// raw: [N][A][6] predictor outputs; labels [N][nb][5] = (class, cx, cy, w, h) floats, zero rows = padding;
// d_raw gets d loss / d raw before the 1 / max(num_fg, 1) factor, which `scale[0]` carries to the predictor backward;
// acc: [N][8] floats of scratch, one row of sums per patch (written, not accumulated: nothing to clear)
int launch_yolox_loss(const float* raw, const float* labels, int N, int nb, const DetGeom& geo, float* d_raw, float* acc,
                      int use_l1, float loss_scale, float* metrics, float* scale, hipStream_t s);
// The same loss over every box of a patch (yolox_loss_wide_kernel: no 8-box cap, no ng x nc matrix).  geo.A <=
// DETLOSS_WIDE_MAX_A and nb <= JN_DETLOSS_MAX_BOXES, else nothing is launched and the return value is non-zero.
constexpr int DETLOSS_WIDE_MAX_A = 8400;                // 640 px at strides 8 / 16 / 32
int launch_yolox_loss_wide(const float* raw, const float* labels, int N, int nb, const DetGeom& geo, float* d_raw, float* acc,
                           int use_l1, float loss_scale, float* metrics, float* scale, hipStream_t s);
int launch_head_pred_bwd(const float* d_raw, const float* scale, const void* reg, int reg_ld, ChanTab rt, const void* cls,
                         int cls_ld, ChanTab ct, int dtype, const float* wp, float* g_reg, float* g_cls, float* g_wp,
                         float* g_bp, int hid, int HW, int A, int a0, int N, hipStream_t s);

// ---- backward of the conv stack (kernels_bwd.hip, the 1x1 family in kernels_bwd_pw.hip) ----------------------------------------
// Activations (z, x, cat) are fp32: training refuses bf16 storage (run_net_backward).
int launch_bn_bwd_reduce(const float* g, int g_ld, const float* z, int z_ld, ChanTab t, const float* save, int C,
                         long long M, double* red_out, long long rep_stride, hipStream_t s,
                         const SlotBatch& sb = SlotBatch{});
// sums the replicas -> consts[c] = {sum_gy/n, sum_gy_zhat/n, gamma*invstd}; dgamma/dbeta += totals.  raw_moment: the second
// sum is sum gy * y (y = gamma * zhat + beta, formed by a consumer's fused kernel) and is converted here
int launch_bn_bwd_consts(const double* red, long long rep_stride, double count, const float* gamma, const float* beta,
                         const float* save, float* consts, float* g_gamma, float* g_beta, int C, hipStream_t s,
                         const SlotBatch& sb = SlotBatch{}, int raw_moment = 0);
int launch_bn_bwd_gz(float* g, int g_ld, const float* z, int z_ld, ChanTab t, const float* save, const float* consts, int C,
                     long long M, hipStream_t s, const SlotBatch& sb = SlotBatch{});
// weight-gradient kernels add into wpart (replicated scratch, zero on entry and on exit) when the
// tensor fits, else straight into gw; launch_wpart_reduce folds the replicas into gw.
// route (the wide kernel, N, K >= 128): 0 = the rule (split products unless JN_WW_EXACT is set), else as Conv3WRoute:
// CW_ROUTE_SPLIT / CW_ROUTE_EXACT = pw_bwd_weight_wide_kernel<true / false>; ignored by the narrower layers' fp32 kernel
// (the rule of launch_pw_bwd_weight, pure host code: the wide kernel takes layers of at least 128 x 128 channels in whole quads)
inline bool pw_bwd_weight_wide(int N, int K) { return N >= 128 && K >= 128 && N % 4 == 0 && K % 4 == 0; }
int launch_pw_bwd_weight(const float* gz, int g_ld, const float* x, int x_ld, ChanTab it, float* gw, float* wpart,
                         long long M, int N, int K, hipStream_t s, const SlotBatch& sb = SlotBatch{},
                         long long gz_slot_stride = -1, int route = 0);
int launch_wpart_reduce(float* gw, float* wpart, int n, hipStream_t s);
// bn_bwd_gz + data gradient + weight gradient of a pointwise layer in one pass (few-channel layers; fp32 buffers)
struct PwBwdFusedArgs {
  const float* g; int g_ld;              // d loss / d activation of the layer output
  const float* z; int z_ld; ChanTab ot;  // raw layer output and its table
  const float* save; const float* consts;
  const float* x; int x_ld; ChanTab it;  // raw layer input and its table
  const float* w;                        // [cout][cin]
  float* gx; int gx_ld; int accumulate;  // d loss / d activation of the layer input
  float* gw; float* wpart;
  long long M; int cout, cin;
  SlotBatch sb;
  // optional: accumulate the BN-backward sums of the layer(s) that produced the input (this op writes the FINAL gradient
  // of the view): channels [0, red_split) -> red_in, [red_split, cin) -> red_in2 (either may be null: that run is
  // skipped); red_split == 0: one run over all of cin into red_in
  double* red_in; long long red_rep_stride; double* red_in2; int red_split;
  // optional: a second gradient of the layer input, added while gx is written (the shortcut branch of a bottleneck:
  // g[input] = W^T g_z + g[sum]); same pixel indexing as gx
  const float* gadd; int gadd_ld;
  // optional ("RED2"): the run [0, red_split or cin) of the input is a materialised shortcut sum silu(bn(z2)) + res — the
  // sums formed for it belong to the BatchNorm of z2's conv (the bottleneck's last pointwise conv): z2 / its table replace
  // the raw input tile and the input table in that run's silu' and second moment
  const float* red2_z; int red2_ld; const float* red2_sc; const float* red2_sh;
  // optional: 6 bytes per weight of scratch (three bf16 planes; the fp32 form uses 4), 16-byte aligned, free during this
  // launch.  With it the (128, 128) and (64, 128) layers take pw_bwd_fused128_kernel, which streams the transposed weight
  // from there in fragment order
  float* w_frag;
  int route;                             // debug entry: 1 keeps the 64-pixel kernel
  int max_wg;                            // debug entry: > 0 caps the workgroups
};
struct DwBwdFusedArgs {                  // the depthwise counterpart (3x3, pad 1, stride 1 / 2)
  const float* g; int g_ld; const float* z; int z_ld; ChanTab ot; const float* save; const float* consts;
  const float* x; int x_ld; ChanTab it; const float* w;      // w: [9][C]
  float* gin; int gin_ld; int accumulate; float* gw; float* wpart;
  int C, H, W, OH, OW, N, stride;
  SlotBatch sb;
  double* red_in; long long red_rep_stride;      // as in PwBwdFusedArgs
  int max_wg;                            // debug entry: > 0 caps the persistent workgroups per channel block and slot
};
bool dw_bwd_fused_supported(int C, int H, int W, int OH, int OW, int stride);
int launch_dw_bwd_fused(const DwBwdFusedArgs& a, hipStream_t s);
// the [cout][cin] weight transposed and split into three bf16 planes, in the fragment order pw_x3_kernel<.., SLOTS> streams
int launch_w_split3_t(const float* w, void* w3t, int cout, int cin, hipStream_t s);
bool pw_bwd_fused_supported(int cout, int cin);
bool pw_bwd_fused_reduces_input(int cout, int cin);
int launch_pw_bwd_fused(const PwBwdFusedArgs& a, hipStream_t s);
int launch_dw_bwd_data(const float* gz, int g_ld, const float* w, float* gin, int gin_ld, int C, int H, int W, int OH,
                       int OW, int N, int stride, int accumulate, hipStream_t s, const SlotBatch& sb = SlotBatch{});
int launch_dw_bwd_weight(const float* gz, int g_ld, const float* x, int x_ld, ChanTab it, float* gw, float* wpart, int C,
                         int H, int W, int OH, int OW, int N, int stride, hipStream_t s, const SlotBatch& sb = SlotBatch{},
                         int max_wg = 0);      // debug entry: > 0 caps the workgroups per slot
// gz is d loss / d activation of the stem's output z: the BN + SiLU backward (g_z) is applied while staging
int launch_stem_bwd_weight(const StemArgs& a, const float* gz, int g_ld, float* gw, float* wpart, hipStream_t s,
                           const SlotBatch& sb, const float* z, int z_ld, ChanTab ot, const float* save, const float* consts,
                           int max_wg = 0);
int launch_spp_bwd(const float* cat, float* gcat, int ld, int h, int H, int W, int N, ChanTab it, hipStream_t s,
                   const SlotBatch& sb = SlotBatch{}, int route = 0);
int launch_upsample_bwd(const float* gdst, int dst_ld, float* gsrc, int src_ld, int C, int H, int W, int N,
                        int accumulate, hipStream_t s, const SlotBatch& sb = SlotBatch{});
int launch_grad_copy(const float* src, int src_ld, float* dst, int dst_ld, int C, long long M, int accumulate,
                     hipStream_t s, const SlotBatch& sb = SlotBatch{});
int launch_nchw_to_nhwc_grad(const float* in, float* out, int out_ld, int C, int HW, int N, int accumulate,
                             hipStream_t s);

// ---- env / rollout primitives (kernels_env.hip) -------------------------------------
// fused detection augmentation (kernels_aug.hip): params [N][AUG_NPARAM] = r_gain, b_gain, gray flag, gauss centre weight,
// gauss side weight, noise std, motion kernel [3][3] (row-major), 1 pad
#ifndef JN_DW_S2_PAD
#define JN_DW_S2_PAD 4      // LDS pixel-stride padding (floats) of the stride-2 depthwise tiles; 8 removes the bank
                            // conflicts the PMC shows (0.3-0.4 of the LDS-active cycles) but not a microsecond: 126.9 vs 127.3 ms
#endif
constexpr int AUG_NPARAM = 20;   // ... + shade intensity, shade quantity, roughness, stretch (plasma shadow), 1 pad
int launch_augment(const float* in, float* out, const float* params, const float* noise, unsigned long long seed, int N, int P,
                   hipStream_t s);
int launch_gather(const float* images, const int64_t* positions, float* out, long long out_sample_stride,
                  int B, int C, int H, int W, int P, const int* skip_flag, int skip_when, hipStream_t s,
                  const int64_t* image_index = nullptr);
int launch_gather(const uint8_t* images, const int64_t* positions, float* out, long long out_sample_stride,   // b -> b / 255
                  int B, int C, int H, int W, int P, const int* skip_flag, int skip_when, hipStream_t s,
                  const int64_t* image_index = nullptr);
int launch_bbox_masks(const int64_t* bboxes, uint8_t* masks, int32_t* n_tiles, int B, int nb, int H, int W, int P,
                      hipStream_t s, const int32_t* extent = nullptr);
// the detector's training batch (jnroll.h: jn_detection_cells): count, scan over B, select.  The select kernel keeps two
// uint16 lists of the image's cells in LDS, so Gh * Gw <= JN_DETCELLS_MAX_CELLS (16 KB); the caller checks it, and that
// every extent lies in 1..Gh x 1..Gw.
constexpr int JN_DETCELLS_MAX_CELLS = 4096;
int launch_detection_cells(const int64_t* bboxes, const int32_t* extents, int B, int nb, int Gh, int Gw, int P, int sample_neg,
                           uint64_t seed, int capacity, int64_t* cells, int64_t* targets, int32_t* offsets, int32_t* n_pos,
                           hipStream_t s);
// kernels_view.hip: the indexed gather through image views (jnroll.h: jn_image_view); all views of one element type.
// out is float, or uint8 when out_u8 (byte sources only); image_index = null: patch n reads view n
int launch_view_gather(const jn_image_view* views, int src_u8, const int64_t* image_index, const int64_t* positions,
                       void* out, int out_u8, long long out_sample_stride, int N, int P, const int* skip_flag,
                       int skip_when, hipStream_t s);

struct EnvPtrs {
  int64_t* positions; uint8_t* bbox_masks; uint8_t* visited; int32_t* steps; uint8_t* has_stopped;
  int32_t* n_bbox_tiles; int32_t* found;
  int B, Gh, Gw, T, stop;
  // ragged mode (jn_env_init_ragged): [B][2] = (gh, gw), the agent's own grid inside the [Gh, Gw] canvas grid it may not
  // leave; null = every agent walks the whole canvas.  The state arrays stay canvas-strided either way.
  const int32_t* extent;
};
int launch_env_reset(const EnvPtrs& e, const int64_t* start_positions, uint64_t seed, const uint64_t* keys, hipStream_t s);
int launch_env_step(const EnvPtrs& e, const int64_t* actions, float* rewards, uint8_t* terminated,
                    uint8_t* truncated, hipStream_t s);

struct RolloutBuffers {   // device, [B,T]-shaped unless noted; any may be null
  float* rewards; float* returns; float* logprobs; float* entropies;
  uint8_t* masks;        // [B,T+1]
  uint8_t* logit_masks;
  int64_t* positions;    // [B,T+1,2]
  int64_t* actions;
  float* logits;         // [B,T,nA]
  float* final_emb;      // [B,T+1,C]
};
int launch_rollout_begin(const EnvPtrs& e, const RolloutBuffers& r, int64_t* prev_action, int32_t* cache_len,
                         int32_t* n_done, hipStream_t s);
int launch_rollout_epilogue(const RolloutBuffers& r, const int32_t* n_done, int B, int T, int stop_early,
                            hipStream_t s);
// the teacher's action set of every agent's state (jnroll.h: jn_teacher_actions); sets[b * set_stride], one wave per agent
int launch_teacher_sets(const int64_t* positions, const uint8_t* visited, const uint8_t* targets, uint8_t* sets,
                        long long set_stride, int B, int Gh, int Gw, const int* skip_flag, int skip_when, hipStream_t s);
// the action sets of N states under a masking policy (jnroll.h: jn_action_sets), one thread per state
int launch_action_sets(const int64_t* positions, const uint8_t* visited, const int32_t* extents, const int64_t* forced, int N,
                       int Gh, int Gw, int policy, int nA, uint16_t* sets, hipStream_t s);
// the teacher's whole walks of a batch (jnroll.h: jn_teacher_walks): walk (one wave per image; target / todo bytes of the
// grid and a ring of T steps in LDS), the scan of launch_detection_cells, detector rows.  The caller checks every limit.
constexpr int JN_TWALK_MAX_CELLS = JN_DETCELLS_MAX_CELLS;   // 2 x 4 KB of cell bytes
constexpr int JN_TWALK_MAX_T = 4096;                        // a ring of 8-byte steps: 32 KB
constexpr int JN_TWALK_MAX_KEYPOINTS = 64;                  // the detour table: one lane per detour
struct TeacherWalkArgs {
  const int64_t* bboxes; const int64_t* starts;             // [B,nb,4]; [B,2] or null
  int B, nb, Gh, Gw, P, T, min_keypoints, max_keypoints, binomial;
  uint64_t seed;
  int capacity;
  int64_t* positions; int64_t* current_actions; int64_t* next_actions; int64_t* labels;
  float* masks; float* local_bboxes; int32_t* n_steps; uint8_t* targets;
  int64_t* cells; float* bboxes_yolox; int32_t* offsets;
};
int launch_teacher_walks(const TeacherWalkArgs& a, hipStream_t s);
// kernels_ragged.hip: patch_bboxes2full_image for a whole batch (jnroll.h: jn_rollout_boxes_to_image)
int launch_boxes_to_image(const float* det_boxes, const int32_t* det_counts, const int64_t* positions, const uint8_t* masks,
                          int B, int T, int S, int K, int P, float* out_boxes, int32_t* out_totals, hipStream_t s);
// kernels_eval.hip: detection evaluation, one workgroup per image / segment (jnroll.h: jn_merge_boxes,
// jn_match_detections, jn_average_precision).  Each returns nonzero when the LDS it needs cannot be had.
constexpr int JN_EVAL_MAX_BOXES = 4096;        // boxes (and targets) per image
constexpr int JN_EVAL_MAX_ENTRIES = 8192;      // (score, hit) slots per average-precision segment
constexpr int JN_EVAL_MAX_THRESHOLDS = 256;
int launch_merge_boxes(const float* boxes, const int32_t* counts, int B, int Nmax, int W, int target, float threshold,
                       float* out_boxes, int32_t* out_counts, int32_t* out_rounds, hipStream_t s);
int launch_match_detections(const float* preds, const int32_t* pred_counts, int B, int Nmax, int W, const float* targets,
                            const int32_t* target_counts, int Mmax, int max_det, double* scores, int32_t* hits, int32_t* sel,
                            int32_t* n_pred, int32_t* n_gt, hipStream_t s);
int launch_average_precision(const double* scores, const int32_t* hits, const int32_t* n_pred, const int32_t* n_gt, int B,
                             int max_det, int pooled, const double* thresholds, int n_thresholds, double* out, hipStream_t s);
int launch_average_precision_segments(const double* scores, const int32_t* hits, const int32_t* n_pred, const int32_t* n_gt,
                                      int U, int max_det, const int32_t* seg_offsets, int NS, int max_units,
                                      const double* thresholds, int n_thresholds, double* out, hipStream_t s);
// the multistart evaluation's per-cell pool + NMS (jnroll.h: jn_pool_walk_detections), one workgroup per (cell, image)
int launch_pool_walk_detections(const float* det_boxes, const int32_t* det_counts, const int64_t* positions,
                                const int32_t* walk_tokens, const int32_t* walk_first, const int32_t* walk_count, int A, int T,
                                int S, int K, int NI, int max_walks, int Gh, int Gw, int M, float* cell_boxes,
                                int32_t* cell_counts, int32_t* cell_stats, uint8_t* visited, hipStream_t s);

// ---- decision transformer step (kernels_gpt.hip) -------------------------------------
struct GptLayerPtrs {
  float *ln1_w, *ln1_b, *qkv_wt, *qkv_b, *proj_wt, *proj_b, *ln2_w, *ln2_b, *fc_wt, *fc_b, *fc2_wt, *fc2_b;
};

constexpr int JN_N_CLASS_ROWS = 100;   // rows of embed_class (src/models/gpt.py:227)
enum { GPT_SRC_ENV = 0, GPT_SRC_TEACH = 1, GPT_SRC_GIVEN = 2, GPT_SRC_CLASS = 3 };

struct GptStepArgs {
  int C, n_head, n_layer, nA, Tmax, B, T;
  int use_pos_emb, no_patch_emb, concat_emb, dec_pos_enc, n_parts;
  int pe2_ch;                       // channels per axis of the 2-D sinusoid table
  const float *wte, *wpe, *embed_class, *proj_wt, *proj_b, *pos1d, *pe2, *head_wt, *lnf_w, *lnf_b;
  const int64_t* classes;           // [B] class id of every agent's class token (gpt.py:476-478), or null = class 0
  const GptLayerPtrs* layers;       // device array [n_layer]
  int kv_lds;                       // set by launch_gpt_step: the K / V rows of a layer are staged in LDS
  const float* pf_base; long long pf_floats;   // the run of the arena that holds head, ln_f and every layer (0: unknown)
  const float* emb_part; int KS; const float* efpn_lin_b;   // patch-embedding split-K partials [B][KS][C]
  float *kcache, *vcache;           // [L][B][Tmax][C]
  int64_t* prev_action; int32_t* cache_len;
  int step;                         // t
  // token source: rollout state, teacher arrays, a given embedding row, or the class token
  int src_mode;
  int pos_index;                    // 1-D position of the token (0 in recurrent mode: gpt.py:431-449 quirk)
  const int64_t* t_actions; const int64_t* t_positions; int t_stride, t_index;
  const float* tok_emb; int tok_emb_stride, tok_emb_index;   // patch embeddings [B][stride][C]
  const float* given_emb; int given_stride, given_index;
  int embed_only;                   // stop after writing the token embedding
  int emb_stride;                   // tokens per agent in out.final_emb
  float* logits_rows; int logits_stride;   // teacher/given modes: logits of this token -> row b
  int mode; const int64_t* forced; uint64_t seed;
  const uint64_t* keys;             // [B][2] = (stream seed, stream index) of every agent's sampled draws, or null = (seed, b)
  EnvPtrs env;
  RolloutBuffers out;
  int32_t* n_done;                  // [T+1]
  float* tok_emb_out;               // [B][T][C] finished patch embedding of this step (training) or null
  float pdrop; uint64_t drop_seed;  // train-mode dropout (0 = off), see drop_scale in jn_device.h
  const int* skip_flag; int skip_when;
  // the wide route (kernels_gptwide.hip), all null / 0 on the per-agent route
  int wide;                         // 1: launch_gpt_step_routed goes to launch_gpt_step_wide
  const GptLayerPtrs* layers_host;  // HOST array [n_layer] of the pointers `layers` holds on the device
  float* wide_scratch;              // gpt_wide_scratch_floats(...) floats, allocated with the workspaces
  // jn_set_rollout_action_mask: 0 = gpt_decide_and_step; else gpt_decide_and_step_masked forms the agent's action set under
  // this policy, decides inside it and writes it to mask_sets[b * T + t] (the context's) and mask_sets_out (the caller's, or null)
  int mask_policy; uint16_t* mask_sets; uint16_t* mask_sets_out;
};
int launch_gpt_step(const GptStepArgs& a, hipStream_t s);

// ---- the wide decision route (kernels_gptwide.hip): one step as a chain of launches over all B agents ----------------
constexpr int GPT_WIDE_MAX_C = 1024;        // 64 * LN_CQ of the batched backward (kernels_gptbwd.hip)
constexpr int GPT_PER_AGENT_MAX_C = 256;    // where gpt_step_kernel's envelope ends
// what the wide route takes: the GEMM's 64-column tiles and 32-row K chunks want n_embd a multiple of 64
inline bool gpt_wide_admits(int C, int n_head, int block_size) {
  return C >= 64 && C <= GPT_WIDE_MAX_C && C % 64 == 0 && n_head > 0 && C % n_head == 0 && block_size >= 1 && block_size <= 255;
}
size_t gpt_wide_scratch_floats(int C, int n_parts, int max_batch);
int launch_gpt_step_wide(const GptStepArgs& a, hipStream_t s);
// the step of a context's route: per-agent (launch_gpt_step) or wide
int launch_gpt_step_routed(const GptStepArgs& a, hipStream_t s);

// ---- training of the decision side (kernels_train.hip) ------------------------------------
struct LossArgs {
  const float* logits; const int64_t* actions; const float* returns; const float* rewards;
  const uint8_t* logit_masks; const int32_t* n_done;
  float* dlogits;                   // [B][T][nA]
  float* metrics;                   // [8]: action_loss, entropy_loss, loss, returns, episode_length, S
  int B, T, nA, stop_early, reward_norm;
  float ret_mean, ret_std, entropy_weight, scale;
  const uint16_t* sets;             // [B][T] action sets of a masked rollout (jn_set_rollout_action_mask), or null = all actions
};
int launch_reinforce_loss(const LossArgs& a, hipStream_t s);
// autograd bridge: d loss / d logits [B][T][nA] from d loss / d logprobs and d loss / d entropies [B][T] (either may be null)
int launch_logits_grad(const float* logits, const int64_t* actions, const float* dlogprobs, const float* dentropies,
                       const int32_t* n_done, float* dlogits, int B, int T, int nA, int stop_early, hipStream_t s,
                       const uint16_t* sets = nullptr);      // sets: as LossArgs::sets
// one trainable tensor of the flat arena: packing kind (api_ctx.hip PackKind) and dimensions; `off` is its offset both in the
// packed arena and in a reference-layout buffer of the same size
struct ArenaSeg { long long off, numel; int kind, d0, d1, d2; };
int launch_arena_copy(const ArenaSeg* segs, int n_segs, float* arena, float* ref, long long total, int to_ref, int accumulate,
                      hipStream_t s);

struct GptBwdArgs {
  int C, n_head, n_layer, nA, B, T, stop_early;
  int use_pos_emb, no_patch_emb, concat_emb, dec_pos_enc, pe2_ch;
  const int32_t* n_done;
  const float* final_emb;           // [B][T+1][C]
  const float* dlogits;             // [B][T][nA]
  const int64_t* actions;           // [B][T] actions taken (rollout)
  const int64_t* tok_actions;       // [B][T] action token of every patch token (teacher-forced mode) or null
  const int64_t* positions;         // [B][pos_tokens][2]
  const int64_t* classes;           // [B] class ids of the forward being differentiated, or null = class 0
  int pos_tokens;                   // T + 1 (rollout history) or T
  int pos1d_by_token;               // 1: token t has 1-D position t (full-sequence forward)
  const float* tok_emb;             // [B][T][C] patch embeddings
  float* d_tok_emb;                 // out: row of (agent b, token t) at (b * dte_stride_b + t * dte_stride_t) * C
  long long dte_stride_b, dte_stride_t;
  const float *wte, *wpe, *proj_wt, *pos1d, *pe2, *head_wt, *lnf_w, *lnf_b;
  const GptLayerPtrs* layers;       // weights
  const GptLayerPtrs* g_layers;     // gradients (same layout, non-const use)
  float *g_wte, *g_wpe, *g_embed_class, *g_proj_wt, *g_proj_b, *g_head_wt, *g_lnf_w, *g_lnf_b;
  float* scratch; long long scratch_per_agent;
  float pdrop; uint64_t drop_seed; int Tmax;   // dropout of the forward being differentiated (Tmax = block_size + 1)
};
int launch_gpt_backward(const GptBwdArgs& a, hipStream_t s);
// the same backward batched over the agents (kernels_gptbwd.hip): W / G are HOST arrays of the per-layer weight and
// gradient pointers; returns 1 when the shape is outside what it takes (caller falls back to launch_gpt_backward)
// (tiled: with the attention in its tiled form, below; the scratch then holds one more buffer of a layer's ATT shape)
size_t gpt_backward_batched_scratch(int C, int n_head, int n_layer, int nA, int B, int T, bool tiled = false);
bool gpt_backward_batched_admits(int C, int n_head, int T);   // pure: the shapes the LDS form of the attention kernels takes
int launch_gpt_backward_batched(const GptBwdArgs& a, const GptLayerPtrs* W, const GptLayerPtrs* G, hipStream_t s, bool tiled = false);
// Which backward differentiates the decision transformer is decided once, by gpt_backward_route, a pure function of the shape
// and the context's decision route (and of the test hook JN_GPT_BWD_TILED, read per call); launch_gpt_bwd (api_train.hip) is
// a switch over it and check_can_train refuses NONE.  In order:
//   LDS        where gpt_backward_batched_admits says yes: the batched backward, attention tiles of a head in 64 KB of LDS;
//   NONE       on the wide route (decision_route 1): a wide context has no other backward;
//   PER_AGENT  T <= GPT_PER_AGENT_MAX_T: gpt_backward_kernel, one workgroup per agent, never launched above that length;
//   TILED      head size <= 256, T <= 255: the batched backward with the attention kernels whose LDS does not grow with T;
//   NONE       otherwise.
// The hook sends a decision_route 0 shape that would take LDS or PER_AGENT to TILED.
enum GptBwdRoute { GPT_BWD_NONE = 0, GPT_BWD_LDS = 1, GPT_BWD_PER_AGENT = 2, GPT_BWD_TILED = 3 };
constexpr int GPT_PER_AGENT_MAX_T = 62;     // gpt_backward_kernel keeps the LayerNorm statistics of T + 1 <= 64 rows
GptBwdRoute gpt_backward_route(int C, int n_head, int T, int decision_route);
// one layer's attention recompute + backward on caller tensors (form 0: LDS, 1: tiled with DS of ATT's shape); 1: refused
int launch_gpt_attention(int form, const float* QKV, const float* dY, int B, int nh, int C, int Lm, const int* Lp, float pdrop,
                         uint64_t seed, int layer, int Tmax, float* ATT, float* Y, float* DS, float* dQKV, hipStream_t s);
int launch_ce_loss(const float* logits, const int64_t* target, const uint8_t* masks, float stop_weight, float* dlogits,
                   float* metrics, int n, int nA, int T, hipStream_t s);
// validation: loss / accuracy / episode length / valid tokens of logits [B][T][nA] against labels formed in the kernel
// (next, or with on_self the on-self-trajectory labels from current / next / masks); token_loss, predicted optional
int launch_supervised_metrics(const float* logits, const int64_t* current, const int64_t* next, const uint8_t* masks, int B, int T,
                              int nA, float stop_weight, int on_self, float* token_loss, uint8_t* predicted, float* metrics,
                              hipStream_t s);
// de[m][k] = 0 where e[m][k] <= 0 (ReLU mask of embed_fpn.0);  gb[o] += sum_m dpe[m][o]
int launch_relu_mask(float* de, const float* e, long long n, hipStream_t s);
int launch_colsum_add(const float* dpe, long long M, int Co, float* gb, hipStream_t s);
// (the betas are doubles: the bias corrections are formed in double from them, the per-element arithmetic is fp32)
int launch_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, double beta1, double beta2,
                 float eps, float wd, int step, float clip, float grad_scale, hipStream_t s);

}  // namespace jnr
