// C ABI of libjnroll.so, kernel-level entries: one kernel family each on the caller's tensors, no jn_ctx, for the per-kernel tests.
// Host code only (compiled by hipcc as C++); kernels live in kernels_*.hip.  Every argument check of an entry runs before its first
// device call.  Sections: what the entries share, fused 1x1 backward, dense 3x3, depthwise, 1x1, glue, decision-side training kernels.
#include <cstring>

#include "jn_internal.h"

using namespace jnr;

// ---- what the entries share ----------------------------------------------------------------------------------------------------------
// channels c0.. of a dense [3][C] table (scale | shift | flag)
static ChanTab chan_tab(const float* tab, long long C, int c0 = 0) {
  float* p = const_cast<float*>(tab) + c0;
  ChanTab t{};
  t.sc = p; t.sh = p + C; t.fl = p + 2 * C;
  return t;
}

// The ranges that keep the kernels' index arithmetic in int.  What a family adds to them (a stride, even maps, whole quads where
// the kernel has no scalar tail) is said where the family or the entry checks it.
static bool map_ok(int N, int H, int W) { return N >= 1 && H >= 1 && W >= 1 && (long long)N * H * W <= (1 << 24); }
static bool pixels_ok(long long M) { return M >= 1 && M <= (1 << 24); }
static bool quad_chan_ok(int C) { return C >= 4 && C % 4 == 0 && C <= 4096; }
static bool ld_ok(int ld, int C) { return ld >= C && ld <= 8192; }      // any alignment: the glue kernels
static bool quad_ld_ok(int ld, int C) { return ld_ok(ld, C) && ld % 4 == 0; }
static bool slots_ok(int n_slots) { return n_slots >= 1 && n_slots <= 64; }
static bool dtype_ok(int dtype) { return dtype == JN_F32 || dtype == JN_BF16; }

// An entry's device scratch.  Leaving the entry, by whichever return, waits for the entry's stream (copies queued there may still
// read the scratch) and then frees it; an entry that took none waits for nothing here.
class Scratch {
 public:
  explicit Scratch(hipStream_t s) : s_(s) {}
  Scratch(const Scratch&) = delete;
  ~Scratch() {
    if (p_) { (void)hipStreamSynchronize(s_); (void)hipFree(p_); }
  }
  hipError_t take(size_t bytes) { return hipMalloc(&p_, bytes); }      // once per entry
  template <typename T>
  T* as() const { return static_cast<T*>(p_); }      // null where none was taken
 private:
  hipStream_t s_;
  void* p_ = nullptr;
};

// The kernels step every buffer of one workspace by ONE slot stride (the engine's activation and gradient slots); a caller's
// [S, ...] tensors are dense.  `in` lays S tensors of n floats into the field at `field` of slots `slot` floats apart, `back`
// copies such a field to the caller.
struct SlotLayout {
  int S;
  hipStream_t s;
  hipError_t in(float* field, size_t slot, const float* dense, size_t n) const {
    return hipMemcpy2DAsync(field, slot * sizeof(float), dense, n * sizeof(float), n * sizeof(float), S, hipMemcpyDeviceToDevice, s);
  }
  hipError_t back(float* dense, size_t n, const float* field, size_t slot) const {
    return hipMemcpy2DAsync(dense, n * sizeof(float), field, slot * sizeof(float), n * sizeof(float), S, hipMemcpyDeviceToDevice, s);
  }
};

// The tail of an entry.  `launch` runs its launcher or launchers and returns their code; `back` queues what is copied back to the
// caller; then the stream is waited for.  A HIP error comes first, then a launcher's refusal (non-zero: nothing was launched), which
// is the entry's: a launcher may have refused because the device did, its LDS for one.  HostRefusal: the launchers refuse by their
// arguments alone, before any device call, and so does the entry, whatever state the device is in.
static const auto nothing_back = [] { return hipSuccess; };
template <bool HostRefusal = false, typename L, typename B = decltype(nothing_back)>
static int run_entry(const char* who, hipStream_t s, L launch, const char* refusal = "the launcher refused the arguments", B back = nothing_back) {
  const int rc = launch();
  if (HostRefusal) JN_CHECK(rc == 0, JN_EINVAL, "%s: %s", who, refusal);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = back();
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  JN_CHECK(e == hipSuccess, JN_EHIP, "%s: the launch, the copy back or the wait for the stream failed: %s", who, hipGetErrorString(e));
  JN_CHECK(rc == 0, JN_EINVAL, "%s: %s", who, refusal);
  return JN_OK;
}

// ---- fused 1x1 backward on caller tensors (kernels_bwd_pw.hip) -----------------------------------------------------------------------
extern "C" {

// (the slots and the fragment-order scratch of the 128-input-channel kernel are allocated and freed here, so the call waits for the
// stream)
int jn_pw_bwd_fused(const float* g_dev, const float* z_dev, const float* x_dev, const float* tab_dev, const float* save_dev,
                    const float* consts_dev, const float* w_dev, const float* gadd_dev, int accumulate, float* gx_dev,
                    float* gw_dev, int S, long long M, int cout, int cin, int route, int max_wg, void* stream) {
  JN_CHECK(g_dev && z_dev && x_dev && tab_dev && save_dev && consts_dev && w_dev && gx_dev && gw_dev, JN_EINVAL,
           "jn_pw_bwd_fused: null argument");
  JN_CHECK(S >= 1 && M >= 1 && M <= (1LL << 40), JN_EINVAL, "jn_pw_bwd_fused: S=%d M=%lld", S, M);      // (its own, wider ranges)
  JN_CHECK(cout >= 16 && cin >= 16 && pw_bwd_fused_supported(cout, cin), JN_EINVAL, "jn_pw_bwd_fused: %d -> %d channels: no fused kernel",
           cin, cout);
  JN_CHECK((route == 0 || route == 1) && max_wg >= 0, JN_EINVAL, "jn_pw_bwd_fused: route=%d max_wg=%d", route, max_wg);
  // slots [z | x] of the activations and [g | gx | gadd] of the gradients, then w_frag (6 bytes per weight)
  hipStream_t s = (hipStream_t)stream;
  const long long C = cout + cin;
  const size_t zn = (size_t)M * cout, xn = (size_t)M * cin, act = zn + xn, grad = zn + 2 * xn;
  Scratch scratch(s);
  JN_HIP(scratch.take(((size_t)S * (act + grad) + (size_t)2 * cout * cin) * sizeof(float)));
  float* ws = scratch.as<float>();
  float *za = ws, *xa = za + zn, *ga = ws + (size_t)S * act, *gxa = ga + zn, *gadda = gxa + xn, *w_frag = ws + (size_t)S * (act + grad);
  const SlotLayout lay{S, s};
  JN_HIP(lay.in(za, act, z_dev, zn));
  JN_HIP(lay.in(xa, act, x_dev, xn));
  JN_HIP(lay.in(ga, grad, g_dev, zn));
  if (accumulate) JN_HIP(lay.in(gxa, grad, gx_dev, xn));
  if (gadd_dev) JN_HIP(lay.in(gadda, grad, gadd_dev, xn));
  PwBwdFusedArgs a{};
  a.g = ga; a.g_ld = cout; a.z = za; a.z_ld = cout;
  a.ot = chan_tab(tab_dev, C);      // one [3][cout + cin] table: the output's channels, then the input's
  a.save = save_dev; a.consts = consts_dev;
  a.x = xa; a.x_ld = cin;
  a.it = chan_tab(tab_dev, C, cout);
  a.w = w_dev; a.gx = gxa; a.gx_ld = cin; a.accumulate = accumulate ? 1 : 0; a.gw = gw_dev;
  a.M = M; a.cout = cout; a.cin = cin;
  a.sb.n = S; a.sb.act = (long long)act; a.sb.grad = (long long)grad; a.sb.tab = 3 * C; a.sb.save = 2LL * cout; a.sb.consts = 3LL * cout;
  if (gadd_dev) { a.gadd = gadda; a.gadd_ld = cin; }
  a.w_frag = w_frag; a.route = route; a.max_wg = max_wg;
  return run_entry("jn_pw_bwd_fused", s, [&] { return launch_pw_bwd_fused(a, s); }, "no fused kernel took the launch",
                   [&] { return lay.back(gx_dev, xn, gxa, grad); });
}

}  // extern "C"

// ---- dense 3x3 kernels on caller tensors (kernels_conv3.hip) -------------------------------------------------------------------------
// What the three entries and jn_conv3_route check of a shape before anything else: H x W is the layer's INPUT map, even at stride 2
static bool conv3_shape_ok(int N, int H, int W, int cin, int cout, int stride, int n_slots, int ld_a, int c_a, int ld_b, int c_b) {
  return map_ok(N, H, W) && quad_chan_ok(cin) && quad_chan_ok(cout) && (stride == 1 || (stride == 2 && H % 2 == 0 && W % 2 == 0)) &&
         slots_ok(n_slots) && quad_ld_ok(ld_a, c_a) && quad_ld_ok(ld_b, c_b);
}

// the launch of jn_conv3 / jn_conv3_route(kind 0, 1) without its pointers
static ConvArgs conv3_entry_args(int N, int H, int W, int cin, int cout, int stride, int transposed, int in_ld, int out_ld,
                                 int n_slots, int dtype) {
  ConvArgs a{};
  a.in_ld = in_ld; a.in_dtype = dtype; a.out_ld = out_ld; a.out_dtype = dtype; a.bf16_mfma = dtype == JN_BF16;
  a.N = N; a.H = H; a.W = W; a.OH = H / stride; a.OW = W / stride; a.cin = cin; a.cout = cout; a.stride = stride; a.act = ACT_NONE;
  a.w_transposed = transposed ? 1 : 0; a.n_slots = n_slots;
  return a;
}

extern "C" {

int jn_conv3_route(int kind, int N, int H, int W, int cin, int cout, int stride, int n_slots, int ld_a, int ld_b) {
  JN_CHECK(kind >= 0 && kind <= 3, JN_EINVAL, "jn_conv3_route: kind=%d", kind);
  const bool fwd_like = kind <= 1;      // (ld_a, ld_b) = (in_ld, out_ld) of jn_conv3, else (g_ld, gin_ld | x_ld)
  JN_CHECK(conv3_shape_ok(N, H, W, cin, cout, stride, n_slots, ld_a, fwd_like ? cin : cout, ld_b, fwd_like ? cout : cin) &&
               (kind != 1 || stride == 1) && (kind != 2 || stride == 2),
           JN_EINVAL, "jn_conv3_route: kind %d, %d x %d x %d, %d -> %d channels, stride %d, %d slots, leading dimensions %d and %d", kind, N,
           H, W, cin, cout, stride, n_slots, ld_a, ld_b);
  int r;
  if (fwd_like) {
    ConvArgs a = conv3_entry_args(N, H, W, cin, cout, stride, kind == 1, ld_a, ld_b, n_slots, JN_F32);
    r = conv3_route(a, 0);
  } else if (kind == 2) {
    r = conv3_bwd_data_s2_route(ld_a, ld_b, H / 2, W / 2, cout, cin, N, n_slots, 0);
  } else {
    r = conv3_bwd_weight_route(ld_a, ld_b, cout, cin, 0);
  }
  JN_CHECK(r > 0, JN_EINVAL, "jn_conv3_route: no dense 3x3 kernel takes this launch");
  return r;
}

int jn_conv3(const void* in_dev, int in_ld, const float* tab_dev, const float* w_dev, void* out_dev, int out_ld, int N, int H,
             int W, int cin, int cout, int stride, int transposed, int accumulate, double* stats_dev, const int* skip_flag_dev,
             int skip_when, int n_slots, long long in_slot_stride, long long out_slot_stride, int route, void* stream) {
  JN_CHECK(in_dev && tab_dev && w_dev && out_dev, JN_EINVAL, "jn_conv3: null argument");
  JN_CHECK(conv3_shape_ok(N, H, W, cin, cout, stride, n_slots, in_ld, cin, out_ld, cout) && (!transposed || stride == 1), JN_EINVAL,
           "jn_conv3: %d x %d x %d, %d -> %d channels, stride %d, transposed %d, %d slots, leading dimensions %d and %d", N, H, W, cin, cout,
           stride, transposed, n_slots, in_ld, out_ld);
  const int OH = H / stride, OW = W / stride;
  JN_CHECK(route >= 0 && route <= C3_ROUTE_BF16 && in_slot_stride >= 0 && out_slot_stride >= 0 &&
               (n_slots == 1 || (in_slot_stride >= (long long)N * H * W * in_ld && out_slot_stride >= (long long)N * OH * OW * out_ld &&
                                 in_slot_stride % 4 == 0 && out_slot_stride % 4 == 0)),
           JN_EINVAL, "jn_conv3: route=%d, slot strides %lld and %lld", route, in_slot_stride, out_slot_stride);
  const bool bf16 = route == C3_ROUTE_BF16;
  JN_CHECK(!bf16 || n_slots == 1, JN_EINVAL, "jn_conv3: the bf16 kernel takes one slot");
  ConvArgs a = conv3_entry_args(N, H, W, cin, cout, stride, transposed, in_ld, out_ld, n_slots, bf16 ? JN_BF16 : JN_F32);
  a.in = in_dev; a.itab = chan_tab(tab_dev, cin); a.w = w_dev; a.out = out_dev;
  a.accumulate = accumulate ? 1 : 0; a.stats = stats_dev; a.stats_rep_stride = 2LL * cout; a.skip_flag = skip_flag_dev; a.skip_when = skip_when;
  a.in_slot_stride = in_slot_stride; a.out_slot_stride = out_slot_stride;
  if (bf16) a.w_bf16 = w_dev;      // stands for the rounded copy made below while the route is checked
  JN_CHECK(conv3_route(a, route) > 0, JN_EINVAL, "jn_conv3: route %d does not take this launch", route);
  hipStream_t s = (hipStream_t)stream;
  Scratch wb(s);
  if (bf16) {      // round to nearest even, as the context does once per dense 3x3 layer in bf16 mode (api_ctx.hip)
    const size_t n = (size_t)9 * cout * cin;
    std::vector<float> hw(n);
    std::vector<uint16_t> hb(n);
    JN_HIP(hipMemcpy(hw.data(), w_dev, n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      uint32_t u;
      std::memcpy(&u, &hw[i], 4);
      u += 0x7FFFu + ((u >> 16) & 1u);
      hb[i] = (uint16_t)(u >> 16);
    }
    JN_HIP(wb.take(n * sizeof(uint16_t)));
    JN_HIP(hipMemcpy(wb.as<uint16_t>(), hb.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
    a.w_bf16 = wb.as<uint16_t>();
  }
  return run_entry("jn_conv3", s, [&] { return launch_conv3(a, s, route); }, "the kernel's LDS was refused");
}

// (the kernels step g_z and the input gradient by ONE slot stride, the engine's gradient workspace: the caller's dense tensors are
// laid into slots [g_z | g_in] and the input gradient copied back, so the call allocates, waits for the stream and frees)
int jn_conv3_bwd_data_s2(const float* gz_dev, int g_ld, const float* w_dev, float* gin_dev, int gin_ld, int N, int H, int W, int cout,
                         int cin, int accumulate, int n_slots, int route, void* stream) {
  JN_CHECK(gz_dev && w_dev && gin_dev, JN_EINVAL, "jn_conv3_bwd_data_s2: null argument");
  JN_CHECK(conv3_shape_ok(N, H, W, cin, cout, 2, n_slots, g_ld, cout, gin_ld, cin), JN_EINVAL,
           "jn_conv3_bwd_data_s2: %d x %d x %d, %d -> %d channels, %d slots, leading dimensions %d and %d", N, H, W, cin, cout, n_slots, g_ld,
           gin_ld);
  const int OH = H / 2, OW = W / 2;
  JN_CHECK(route >= 0 && route <= C3_ROUTE_X3 && conv3_bwd_data_s2_route(g_ld, gin_ld, OH, OW, cout, cin, N, n_slots, route) > 0, JN_EINVAL,
           "jn_conv3_bwd_data_s2: route %d does not take this launch", route);
  hipStream_t s = (hipStream_t)stream;
  const size_t gn = (size_t)N * OH * OW * g_ld, xn = (size_t)N * H * W * gin_ld, slot = gn + xn;
  Scratch scratch(s);
  JN_HIP(scratch.take((size_t)n_slots * slot * sizeof(float)));
  float *ga = scratch.as<float>(), *gina = ga + gn;
  const SlotLayout lay{n_slots, s};
  JN_HIP(lay.in(ga, slot, gz_dev, gn));
  JN_HIP(lay.in(gina, slot, gin_dev, xn));      // always: the channels past cin and, with accumulate, the previous gradient come back as they were
  SlotBatch sb;
  sb.n = n_slots; sb.grad = (long long)slot;
  auto launch = [&] { return launch_conv3_bwd_data_s2(ga, g_ld, w_dev, gina, gin_ld, H, W, OH, OW, cout, cin, N, accumulate ? 1 : 0, s, sb, route); };
  return run_entry("jn_conv3_bwd_data_s2", s, launch, "the kernel's LDS was refused", [&] { return lay.back(gin_dev, xn, gina, slot); });
}

int jn_conv3_bwd_weight(const float* gz_dev, int g_ld, const float* x_dev, int x_ld, const float* tab_dev, float* gw_dev, int N, int H,
                        int W, int cout, int cin, int stride, int n_slots, int route, int max_wg, void* stream) {
  JN_CHECK(gz_dev && x_dev && tab_dev && gw_dev, JN_EINVAL, "jn_conv3_bwd_weight: null argument");
  JN_CHECK(conv3_shape_ok(N, H, W, cin, cout, stride, n_slots, g_ld, cout, x_ld, cin), JN_EINVAL,
           "jn_conv3_bwd_weight: %d x %d x %d, %d -> %d channels, stride %d, %d slots, leading dimensions %d and %d", N, H, W, cin, cout,
           stride, n_slots, g_ld, x_ld);
  JN_CHECK(route >= 0 && route <= CW_ROUTE_EXACT && max_wg >= 0 && conv3_bwd_weight_route(g_ld, x_ld, cout, cin, route) > 0, JN_EINVAL,
           "jn_conv3_bwd_weight: route=%d max_wg=%d does not take this launch", route, max_wg);
  const int OH = H / stride, OW = W / stride;
  hipStream_t s = (hipStream_t)stream;
  const ChanTab it = chan_tab(tab_dev, cin);
  SlotBatch sb;      // the caller's [S, ...] tensors are slots already: g_z, x and the [3][cin] tables each by their own size
  sb.n = n_slots; sb.grad = (long long)N * OH * OW * g_ld; sb.act = (long long)N * H * W * x_ld; sb.tab = 3LL * cin;
  auto launch = [&] { return launch_conv3_bwd_weight(gz_dev, g_ld, x_dev, x_ld, it, gw_dev, H, W, OH, OW, cout, cin, N, stride, s, sb, route, max_wg); };
  return run_entry("jn_conv3_bwd_weight", s, launch, "the kernel's LDS was refused");
}

}  // extern "C"

// ---- depthwise 3x3 kernels on caller tensors (kernels_conv.hip, kernels_bwd.hip) -----------------------------------------------------
// What the entries check of a shape before anything else: H x W is the layer's INPUT map, odd sizes included at stride 2
static bool dw_shape_ok(int N, int H, int W, int C, int stride) { return map_ok(N, H, W) && quad_chan_ok(C) && (stride == 1 || stride == 2); }

extern "C" {

int jn_dw3x3_route(int N, int C, int stride, int dtype) {
  JN_CHECK(dw_shape_ok(N, 1, 1, C, stride) && dtype_ok(dtype), JN_EINVAL, "jn_dw3x3_route: N=%d C=%d stride=%d dtype=%d", N, C, stride, dtype);
  ConvArgs a{};
  a.N = N; a.cin = a.cout = C; a.stride = stride; a.in_dtype = a.out_dtype = dtype;
  return dw_route(a, 0);
}

int jn_dw3x3(const void* in_dev, int in_ld, const float* tab_dev, const float* w_dev, void* out_dev, int out_ld, int N, int H, int W,
             int C, int stride, int dtype, double* stats_dev, const int* skip_flag_dev, int skip_when, int nrep, int route, void* stream) {
  JN_CHECK(in_dev && tab_dev && w_dev && out_dev, JN_EINVAL, "jn_dw3x3: null argument");
  JN_CHECK(dw_shape_ok(N, H, W, C, stride) && quad_ld_ok(in_ld, C) && quad_ld_ok(out_ld, C) && dtype_ok(dtype), JN_EINVAL,
           "jn_dw3x3: %d x %d x %d, %d channels, stride %d, dtype %d, leading dimensions %d and %d", N, H, W, C, stride, dtype, in_ld, out_ld);
  JN_CHECK(nrep >= 1 && nrep <= JN_NREP && route >= 0 && route <= DW_ROUTE_STRIP, JN_EINVAL, "jn_dw3x3: nrep=%d route=%d", nrep, route);
  ConvArgs a{};
  a.in = in_dev; a.in_ld = in_ld; a.in_dtype = dtype; a.itab = chan_tab(tab_dev, C); a.w = w_dev;
  a.out = out_dev; a.out_ld = out_ld; a.out_dtype = dtype;
  a.N = N; a.H = H; a.W = W; a.OH = (H + stride - 1) / stride; a.OW = (W + stride - 1) / stride; a.cin = a.cout = C; a.stride = stride;
  a.act = ACT_NONE; a.stats = stats_dev; a.stats_rep_stride = 2LL * C; a.stats_nrep = nrep;
  a.skip_flag = skip_flag_dev; a.skip_when = skip_when;
  JN_CHECK(dw_route(a, route) > 0, JN_EINVAL, "jn_dw3x3: route %d does not take this launch", route);
  hipStream_t s = (hipStream_t)stream;
  return run_entry("jn_dw3x3", s, [&] { return launch_dw(a, s, route); }, "no kernel took the launch");
}

int jn_dwpw(const void* in_dev, int in_ld, const float* itab_dev, const float* w_dw_dev, const float* mtab_dev, const float* w_pw_dev,
            void* out_dev, int out_ld, const void* res_dev, int res_ld, const float* rtab_dev, const float* ptab_dev, int N, int H, int W,
            int C, int cout, int stride, int dtype, const int* skip_flag_dev, int skip_when, void* stream) {
  JN_CHECK(in_dev && itab_dev && w_dw_dev && mtab_dev && w_pw_dev && out_dev, JN_EINVAL, "jn_dwpw: null argument");
  // (cout: whole quads under out_ld, so up to 8192; dwpw_supported has the last word on it)
  JN_CHECK(dw_shape_ok(N, H, W, C, stride) && quad_ld_ok(in_ld, C) && cout >= 4 && cout % 4 == 0 && quad_ld_ok(out_ld, cout) && dtype_ok(dtype),
           JN_EINVAL, "jn_dwpw: %d x %d x %d, %d -> %d channels, stride %d, dtype %d, leading dimensions %d and %d", N, H, W, C, cout, stride,
           dtype, in_ld, out_ld);
  JN_CHECK(dwpw_supported(C, cout, stride), JN_EINVAL, "jn_dwpw: %d -> %d channels at stride %d: no fused kernel", C, cout, stride);
  JN_CHECK(!res_dev || (rtab_dev && ptab_dev && quad_ld_ok(res_ld, cout)), JN_EINVAL, "jn_dwpw: a shortcut needs both tables and res_ld=%d >= %d",
           res_ld, cout);
  DwPwArgs f{};
  f.in = in_dev; f.in_ld = in_ld; f.itab = chan_tab(itab_dev, C); f.w_dw = w_dw_dev; f.mtab = chan_tab(mtab_dev, C); f.w_pw = w_pw_dev;
  f.out = out_dev; f.out_ld = out_ld; f.dtype = dtype; f.C = C; f.cout = cout; f.N = N; f.H = H; f.W = W;
  f.OH = (H + stride - 1) / stride; f.OW = (W + stride - 1) / stride; f.stride = stride; f.skip_flag = skip_flag_dev; f.skip_when = skip_when;
  if (res_dev) { f.res = res_dev; f.res_ld = res_ld; f.rtab = chan_tab(rtab_dev, cout); f.ptab = chan_tab(ptab_dev, cout); }
  hipStream_t s = (hipStream_t)stream;
  return run_entry("jn_dwpw", s, [&] { return launch_dwpw(f, s); }, "no kernel took the launch");
}

// (the kernels step z and x by ONE slot stride and g and the input gradient by another, the engine's workspaces: the caller's dense
// tensors are laid into slots [z | x] and [g | g_in] as in jn_pw_bwd_fused, so the call allocates, waits for the stream and frees;
// the unfused route turns the copy of g into g_z in place, as the engine does with its gradient buffer)
int jn_dw_bwd(const float* g_dev, int g_ld, const float* z_dev, int z_ld, const float* x_dev, int x_ld, const float* otab_dev,
              const float* itab_dev, const float* save_dev, const float* consts_dev, const float* w_dev, float* gin_dev, int gin_ld,
              int accumulate, float* gw_dev, double* red_out_dev, int N, int H, int W, int C, int stride, int n_slots, int route,
              int use_wpart, float* wpart_back_dev, int max_wg, void* stream) {
  JN_CHECK(g_dev && z_dev && x_dev && otab_dev && itab_dev && save_dev && consts_dev && w_dev && gin_dev && gw_dev, JN_EINVAL,
           "jn_dw_bwd: null argument");
  JN_CHECK(dw_shape_ok(N, H, W, C, stride) && slots_ok(n_slots) && quad_ld_ok(g_ld, C) && quad_ld_ok(z_ld, C) && quad_ld_ok(x_ld, C) &&
               quad_ld_ok(gin_ld, C),
           JN_EINVAL, "jn_dw_bwd: %d x %d x %d, %d channels, stride %d, %d slots, leading dimensions %d, %d, %d and %d", N, H, W, C, stride,
           n_slots, g_ld, z_ld, x_ld, gin_ld);
  JN_CHECK(route >= 0 && route <= 2 && max_wg >= 0 && (!use_wpart || wpart_back_dev), JN_EINVAL, "jn_dw_bwd: route=%d max_wg=%d use_wpart=%d",
           route, max_wg, use_wpart);
  const int OH = (H + stride - 1) / stride, OW = (W + stride - 1) / stride;
  const bool fused_ok = dw_bwd_fused_supported(C, H, W, OH, OW, stride);
  if (route == 0) route = fused_ok ? 1 : 2;      // the backward plan's choice (plan.cpp)
  JN_CHECK(route == 2 || fused_ok, JN_EINVAL, "jn_dw_bwd: the fused kernel takes whole blocks of 16 channels, not %d", C);
  JN_CHECK(!red_out_dev || (route == 1 && !accumulate), JN_EINVAL,
           "jn_dw_bwd: the input layer's sums are formed by the fused kernel only, from a gradient it writes (route %d, accumulate %d)", route,
           accumulate);
  hipStream_t s = (hipStream_t)stream;
  const size_t zn = (size_t)N * OH * OW * z_ld, xn = (size_t)N * H * W * x_ld, gn = (size_t)N * OH * OW * g_ld, gin_n = (size_t)N * H * W * gin_ld;
  const size_t act = zn + xn, grad = gn + gin_n, wp = use_wpart ? (size_t)JN_NREP * JN_WPART_MAX : 0;
  Scratch scratch(s);
  JN_HIP(scratch.take(((size_t)n_slots * (act + grad) + wp) * sizeof(float)));
  float* ws = scratch.as<float>();
  float *za = ws, *xa = za + zn, *ga = ws + (size_t)n_slots * act, *gina = ga + gn, *wpart = use_wpart ? ws + (size_t)n_slots * (act + grad) : nullptr;
  const SlotLayout lay{n_slots, s};
  JN_HIP(lay.in(za, act, z_dev, zn));
  JN_HIP(lay.in(xa, act, x_dev, xn));
  JN_HIP(lay.in(ga, grad, g_dev, gn));
  JN_HIP(lay.in(gina, grad, gin_dev, gin_n));      // always: the channels past C and, with accumulate, the previous gradient
  if (wpart) JN_HIP(hipMemsetAsync(wpart, 0, wp * sizeof(float), s));
  SlotBatch sb;
  sb.n = n_slots; sb.act = (long long)act; sb.grad = (long long)grad; sb.tab = 3LL * C; sb.save = 2LL * C; sb.consts = 3LL * C;
  sb.red = (long long)JN_NREP * 2 * C;
  const ChanTab ot = chan_tab(otab_dev, C), it = chan_tab(itab_dev, C);
  auto launch = [&] {
    if (route == 1) {
      DwBwdFusedArgs fa{};
      fa.g = ga; fa.g_ld = g_ld; fa.z = za; fa.z_ld = z_ld; fa.ot = ot; fa.save = save_dev; fa.consts = consts_dev;
      fa.x = xa; fa.x_ld = x_ld; fa.it = it; fa.w = w_dev;
      fa.gin = gina; fa.gin_ld = gin_ld; fa.accumulate = accumulate ? 1 : 0; fa.gw = gw_dev; fa.wpart = wpart;
      fa.C = C; fa.H = H; fa.W = W; fa.OH = OH; fa.OW = OW; fa.N = N; fa.stride = stride; fa.sb = sb;
      fa.red_in = red_out_dev; fa.red_rep_stride = 2LL * C; fa.max_wg = max_wg;
      return launch_dw_bwd_fused(fa, s);
    }
    // BR_DW of the conv-stack backward (api_net.hip)
    const long long M = (long long)N * OH * OW;
    int rc = launch_bn_bwd_gz(ga, g_ld, za, z_ld, ot, save_dev, consts_dev, C, M, s, sb);
    if (rc == 0) rc = launch_dw_bwd_data(ga, g_ld, w_dev, gina, gin_ld, C, H, W, OH, OW, N, stride, accumulate ? 1 : 0, s, sb);
    if (rc == 0) rc = launch_dw_bwd_weight(ga, g_ld, xa, x_ld, it, gw_dev, wpart, C, H, W, OH, OW, N, stride, s, sb, max_wg);
    return rc;
  };
  auto back = [&] {
    hipError_t e = lay.back(gin_dev, gin_n, gina, grad);
    if (e == hipSuccess && wpart) e = hipMemcpyAsync(wpart_back_dev, wpart, wp * sizeof(float), hipMemcpyDeviceToDevice, s);
    return e;
  };
  return run_entry("jn_dw_bwd", s, launch, "no kernel took the launch", back);
}

}  // extern "C"

// ---- 1x1 (pointwise) kernels on caller tensors (kernels_conv.hip, kernels_pwres.hip, kernels_pwxs.hip, kernels_bwd_pw.hip) -------------
// What the entries check of a shape before anything else: M = N * H * W pixels; H and W matter to the fused upsample alone
static bool pw_shape_ok(int N, int H, int W, int cin, int cout, int in_ld, int out_ld, int n_slots) {
  return map_ok(N, H, W) && quad_chan_ok(cin) && quad_chan_ok(cout) && quad_ld_ok(in_ld, cin) && quad_ld_ok(out_ld, cout) && slots_ok(n_slots);
}
static bool pw_flags_ok(int dtype_in, int dtype_out, int act) { return dtype_ok(dtype_in) && dtype_ok(dtype_out) && act >= ACT_NONE && act <= ACT_SIGMOID; }

// the launch of jn_pw / jn_pw_route without its pointers; `some` stands for every optional pointer that is given, and for the split
// planes, which the entry makes whenever the route reads them (what the networks have unless JN_NO_PW_X3 is set)
static ConvArgs pw_entry_args(int N, int H, int W, int cin, int cout, int in_ld, int out_ld, int dtype_in, int dtype_out, int bf16_mfma,
                              int transposed, int in_identity, int accumulate, bool has_bias, int act, int n_slots, bool has_up, const void* some) {
  ConvArgs a{};
  a.in_ld = in_ld; a.in_dtype = dtype_in; a.out_ld = out_ld; a.out_dtype = dtype_out; a.bf16_mfma = bf16_mfma ? 1 : 0;
  a.N = N; a.H = a.OH = H; a.W = a.OW = W; a.cin = cin; a.cout = cout; a.stride = 1; a.act = act;
  a.accumulate = accumulate ? 1 : 0; a.w_transposed = transposed ? 1 : 0; a.in_identity = in_identity ? 1 : 0; a.n_slots = n_slots;
  a.bias = has_bias ? (const float*)some : nullptr; a.w_x3 = some; a.up_out = has_up ? const_cast<void*>(some) : nullptr;
  return a;
}

// the runs of a descriptor: ascending, disjoint, inside [0, cin); a deferred run's sums inside one replica
static bool pw_defer_ok(const jn_pw_defer* d, int cin) {
  if (!d->sums_dev || !d->params_dev || d->dN < 1 || d->dmax < 0 || d->n_runs < 1 || d->n_runs > 4 || d->rep_stride < 2) return false;
  int prev = 0;
  for (int i = 0; i < d->n_runs; ++i) {
    const jn_pw_run& r = d->run[i];
    if (r.c0 < prev || r.c1 <= r.c0 || r.c1 > cin || !(r.hw >= 1.0f)) return false;
    if (r.stat0 >= 0 && (r.g0 < 0 || r.b0 < 0 || 2LL * (r.stat0 + (r.c1 - r.c0)) > d->rep_stride)) return false;
    prev = r.c1;
  }
  return true;
}

// The split planes of jn_pw at `ws`, as the context makes them for the 1x1 weights of its arena: the flat planes, then the regions in
// fragment order, by the splitter's one-row table at ws + plane_bytes
static int pw_split_planes(const float* w_dev, char* ws, size_t plane_bytes, int cin, int cout, hipStream_t s) {
  const size_t nw = (size_t)cout * cin;
  launch_w_split3(w_dev, ws, (long long)nw, s);
  if (!pw_x3_fragment_order(cin, cout)) return JN_OK;
  const X3FragConv row{0, cout, cin};
  JN_HIP(hipMemcpyAsync(ws + plane_bytes, &row, sizeof(row), hipMemcpyHostToDevice, s));
  JN_HIP(hipStreamSynchronize(s));      // (`row` leaves scope)
  launch_w_split3_frag(w_dev, ws, (const X3FragConv*)(ws + plane_bytes), 1, (int)nw, s);
  return JN_OK;
}

// The deferred half of jn_pw's input table: the descriptor's runs in the kernel arguments, or, with `arr` (4 * cin words of
// scratch), as the per-channel arrays [dsrc | dhw | dgoff | dboff]
static int pw_defer_table(ChanTab& t, const jn_pw_defer* defer, int cin, char* arr, hipStream_t s) {
  t.dparams = defer->params_dev; t.dstats = defer->sums_dev; t.drep_stride = defer->rep_stride; t.dN = defer->dN; t.dmax = defer->dmax;
  if (arr) {
    std::vector<int32_t> h(4 * (size_t)cin, -1);      // channels outside every run: never deferred
    float* hw = reinterpret_cast<float*>(h.data() + cin);
    for (int c = 0; c < cin; ++c) { hw[c] = 0.0f; h[2 * cin + c] = h[3 * cin + c] = 0; }
    for (int i = 0; i < defer->n_runs; ++i) {
      const jn_pw_run& q = defer->run[i];
      for (int c = q.c0; c < q.c1; ++c) {      // (the limit is applied by the kernel here: dN * dhw <= dmax)
        h[c] = q.stat0 >= 0 ? q.stat0 + (c - q.c0) : -1; hw[c] = q.hw;
        h[2 * cin + c] = q.stat0 >= 0 ? q.g0 + (c - q.c0) : 0; h[3 * cin + c] = q.stat0 >= 0 ? q.b0 + (c - q.c0) : 0;
      }
    }
    JN_HIP(hipMemcpyAsync(arr, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
    JN_HIP(hipStreamSynchronize(s));      // (`h` leaves scope)
    t.dsrc = (const int*)arr; t.dhw = (const float*)(arr + 4 * (size_t)cin); t.dgoff = (const int*)(arr + 8 * (size_t)cin);
    t.dboff = (const int*)(arr + 12 * (size_t)cin);
    t.nseg = 0;
    return JN_OK;
  }
  t.dsrc = reinterpret_cast<const int*>(defer->sums_dev);      // (non-null marks the table as deferred; the runs form never reads it)
  t.nseg = defer->n_runs;
  ChanTab::Run* dst[4] = {&t.r0, &t.r1, &t.r2, &t.r3};
  for (int i = 0; i < defer->n_runs; ++i) {
    const jn_pw_run& q = defer->run[i];
    // a run whose layer is above the deferral limit reads the table in either form (defer_tab_runs, api_net.hip)
    const bool deferred = q.stat0 >= 0 && (double)defer->dN * q.hw <= (double)defer->dmax;
    *dst[i] = ChanTab::Run{q.c0, q.c1, deferred ? q.stat0 : -1, q.g0, q.b0, q.hw};
  }
  return JN_OK;
}

extern "C" {

int jn_pw_route(int N, int H, int W, int cin, int cout, int in_ld, int out_ld, int dtype_in, int dtype_out, int bf16_mfma, int transposed,
                int accumulate, int has_bias, int act, int n_slots, int has_up, int route, int32_t* variant_out) {
  JN_CHECK(pw_shape_ok(N, H, W, cin, cout, in_ld, out_ld, n_slots) && pw_flags_ok(dtype_in, dtype_out, act), JN_EINVAL,
           "jn_pw_route: %d x %d x %d, %d -> %d channels, leading dimensions %d and %d, dtypes %d -> %d, act %d, %d slots", N, H, W, cin, cout,
           in_ld, out_ld, dtype_in, dtype_out, act, n_slots);
  static const float some = 0.0f;
  const ConvArgs a = pw_entry_args(N, H, W, cin, cout, in_ld, out_ld, dtype_in, dtype_out, bf16_mfma, transposed, 0, accumulate, has_bias != 0,
                                   act, n_slots, has_up != 0, &some);
  JN_CHECK(route >= 0 && route <= PW_MFMA, JN_EINVAL, "jn_pw_route: route=%d", route);
  const PwRoute r = pw_route(a, route);
  JN_CHECK(r != PW_NONE, JN_EINVAL, route ? "jn_pw_route: route %d does not take this launch" : "jn_pw_route: no 1x1 kernel takes this launch", route);
  if (variant_out) {
    variant_out[0] = variant_out[1] = variant_out[2] = 0;
    if (r == PW_MFMA) {
      const PwMfmaVariant v = pw_mfma_variant(a);
      variant_out[0] = v.ct; variant_out[1] = v.kc; variant_out[2] = v.wm;
    }
  }
  return (int)r;
}

int jn_pw(const void* in_dev, int in_ld, int dtype_in, const float* tab_dev, const jn_pw_defer* defer, const float* w_dev,
          const float* bias_dev, void* out_dev, int out_ld, int dtype_out, int N, int H, int W, int cin, int cout, int bf16_mfma,
          int transposed, int in_identity, int accumulate, int act, double* stats_dev, int nrep, const int* skip_flag_dev, int skip_when,
          int n_slots, long long in_slot_stride, long long out_slot_stride, long long tab_slot_stride, float* up_out_dev, int up_ld,
          int route, int max_wg, void* stream) {
  JN_CHECK(in_dev && tab_dev && w_dev && out_dev, JN_EINVAL, "jn_pw: null argument");
  JN_CHECK(pw_shape_ok(N, H, W, cin, cout, in_ld, out_ld, n_slots) && pw_flags_ok(dtype_in, dtype_out, act), JN_EINVAL,
           "jn_pw: %d x %d x %d, %d -> %d channels, leading dimensions %d and %d, dtypes %d -> %d, act %d, %d slots", N, H, W, cin, cout, in_ld,
           out_ld, dtype_in, dtype_out, act, n_slots);
  const long long M = (long long)N * H * W;
  JN_CHECK(nrep >= 1 && nrep <= JN_NREP && route >= 0 && route <= PW_MFMA && max_wg >= 0, JN_EINVAL, "jn_pw: nrep=%d route=%d max_wg=%d", nrep,
           route, max_wg);
  JN_CHECK(in_slot_stride >= 0 && out_slot_stride >= 0 && tab_slot_stride >= 0 &&
               (n_slots == 1 || (in_slot_stride >= M * in_ld && out_slot_stride >= M * out_ld && in_slot_stride % 4 == 0 &&
                                 out_slot_stride % 4 == 0 && tab_slot_stride % 4 == 0)),
           JN_EINVAL, "jn_pw: slot strides %lld, %lld and %lld", in_slot_stride, out_slot_stride, tab_slot_stride);
  JN_CHECK(!up_out_dev || (quad_ld_ok(up_ld, cout) && dtype_out == JN_F32), JN_EINVAL, "jn_pw: the upsampled copy is fp32 with up_ld=%d >= %d",
           up_ld, cout);
  JN_CHECK(!defer || (n_slots == 1 && pw_defer_ok(defer, cin)), JN_EINVAL,
           "jn_pw: a deferred table takes one slot, 1..4 ascending runs inside the %d input channels, sums and parameters", cin);
  ConvArgs a = pw_entry_args(N, H, W, cin, cout, in_ld, out_ld, dtype_in, dtype_out, bf16_mfma, transposed, in_identity, accumulate,
                             bias_dev != nullptr, act, n_slots, up_out_dev != nullptr, w_dev);
  const PwRoute r = pw_route(a, route);
  JN_CHECK(r != PW_NONE, JN_EINVAL, "jn_pw: route %d does not take this launch", route);
  JN_CHECK(max_wg == 0 || r != PW_MFMA, JN_EINVAL, "jn_pw: pw_mfma_kernel has no persistent grid to cap (max_wg=%d)", max_wg);
  a.in = in_dev; a.itab = chan_tab(tab_dev, cin); a.w = w_dev; a.bias = bias_dev; a.out = out_dev;
  a.stats = stats_dev; a.stats_rep_stride = 2LL * cout; a.stats_nrep = nrep; a.skip_flag = skip_flag_dev; a.skip_when = skip_when;
  a.in_slot_stride = in_slot_stride; a.out_slot_stride = out_slot_stride; a.tab_slot_stride = tab_slot_stride;
  a.up_out = up_out_dev; a.up_ld = up_ld; a.w_x3 = nullptr;
  // scratch: the split planes (6 bytes per weight) and the splitter's one-row table; the per-channel arrays of a deferred table
  const bool planes = r == PW_X1 || r == PW_X3, arrays = defer && !defer->use_runs;
  const size_t plane_bytes = planes ? ((size_t)cout * cin * 6 + 63) / 64 * 64 : 0, arr_at = plane_bytes + (planes ? 64 : 0);
  const size_t bytes = arr_at + (arrays ? (size_t)4 * cin * 4 : 0);
  hipStream_t s = (hipStream_t)stream;
  Scratch scratch(s);
  if (bytes) JN_HIP(scratch.take(bytes));
  char* ws = scratch.as<char>();
  if (planes) {
    const int rc = pw_split_planes(w_dev, ws, plane_bytes, cin, cout, s);
    if (rc != JN_OK) return rc;
    a.w_x3 = ws;
  }
  if (defer) {
    const int rc = pw_defer_table(a.itab, defer, cin, arrays ? ws + arr_at : nullptr, s);
    if (rc != JN_OK) return rc;
  }
  return run_entry("jn_pw", s, [&] { return launch_pw(a, s, r, max_wg); }, "no kernel took the launch, or its LDS was refused");
}

int jn_pw_bwd_data_x3(const float* gz_dev, int g_ld, const float* w_dev, float* gx_dev, int gx_ld, long long M, int cout, int cin,
                      int n_slots, int max_wg, void* stream) {
  JN_CHECK(gz_dev && w_dev && gx_dev, JN_EINVAL, "jn_pw_bwd_data_x3: null argument");
  JN_CHECK(pixels_ok(M) && quad_chan_ok(cin) && quad_chan_ok(cout) && quad_ld_ok(g_ld, cout) && quad_ld_ok(gx_ld, cin) && slots_ok(n_slots) &&
               max_wg >= 0,
           JN_EINVAL, "jn_pw_bwd_data_x3: M=%lld, %d -> %d channels, leading dimensions %d and %d, %d slots, max_wg=%d", M, cin, cout, g_ld, gx_ld,
           n_slots, max_wg);
  JN_CHECK(pw_x3_bwd_data_supported(cout, cin), JN_EINVAL, "jn_pw_bwd_data_x3: %d -> %d channels: the split data gradient has no kernel", cin, cout);
  hipStream_t s = (hipStream_t)stream;
  // scratch: the transposed split planes, and the identity table a gradient view carries
  const size_t plane_bytes = ((size_t)cout * cin * 6 + 63) / 64 * 64;
  std::vector<float> ident(3 * (size_t)cout, 0.0f);
  for (int c = 0; c < cout; ++c) ident[c] = 1.0f;
  Scratch scratch(s);
  JN_HIP(scratch.take(plane_bytes + ident.size() * sizeof(float)));
  char* ws = scratch.as<char>();
  float* tab = reinterpret_cast<float*>(ws + plane_bytes);
  JN_HIP(hipMemcpyAsync(tab, ident.data(), ident.size() * sizeof(float), hipMemcpyHostToDevice, s));
  JN_HIP(hipStreamSynchronize(s));
  ConvArgs a{};      // the gradient conv as the conv-stack backward builds it: in = g_z over the layer's cout, out = g_x
  a.in = gz_dev; a.in_ld = g_ld; a.in_dtype = JN_F32; a.itab = chan_tab(tab, cout);
  a.w = w_dev; a.out = gx_dev; a.out_ld = gx_ld; a.out_dtype = JN_F32;
  a.N = 1; a.H = a.OH = 1; a.W = a.OW = (int)M; a.cin = cout; a.cout = cin; a.stride = 1; a.act = ACT_NONE; a.w_transposed = 1; a.in_identity = 1;
  a.n_slots = n_slots; a.in_slot_stride = M * g_ld; a.out_slot_stride = M * gx_ld;
  return run_entry("jn_pw_bwd_data_x3", s, [&] { return launch_pw_x3_bwd_data(a, w_dev, ws, s, max_wg); },
                   "no kernel took the launch, or its LDS was refused");
}

int jn_pw_bwd_weight_route(int cout, int cin) {
  JN_CHECK(quad_chan_ok(cin) && quad_chan_ok(cout), JN_EINVAL, "jn_pw_bwd_weight_route: %d -> %d channels", cin, cout);
  return pw_bwd_weight_wide(cout, cin) ? 2 : 1;
}

int jn_pw_bwd_weight(const float* gz_dev, int g_ld, const float* x_dev, int x_ld, const float* tab_dev, float* gw_dev, long long M, int cout,
                     int cin, int n_slots, long long gz_slot_stride, int use_wpart, float* wpart_back_dev, int exact, void* stream) {
  JN_CHECK(gz_dev && x_dev && tab_dev && gw_dev, JN_EINVAL, "jn_pw_bwd_weight: null argument");
  JN_CHECK(pixels_ok(M) && quad_chan_ok(cin) && quad_chan_ok(cout) && quad_ld_ok(g_ld, cout) && quad_ld_ok(x_ld, cin) && slots_ok(n_slots) &&
               gz_slot_stride >= M * g_ld && gz_slot_stride % 4 == 0,
           JN_EINVAL, "jn_pw_bwd_weight: M=%lld, %d -> %d channels, leading dimensions %d and %d, %d slots, g_z slots %lld apart", M, cin, cout,
           g_ld, x_ld, n_slots, gz_slot_stride);
  const bool wide = pw_bwd_weight_wide(cout, cin);
  JN_CHECK((exact == 0 || exact == 1) && (!exact || wide), JN_EINVAL, "jn_pw_bwd_weight: exact=%d; the exact form is the wide kernel's (both channel counts >= 128)", exact);
  JN_CHECK(!use_wpart || (wpart_back_dev && !wide && (long long)cout * cin <= JN_WPART_MAX), JN_EINVAL,
           "jn_pw_bwd_weight: the replica scratch takes at most %d weights of a layer below 128 x 128, and a buffer to copy it back to", JN_WPART_MAX);
  hipStream_t s = (hipStream_t)stream;
  const size_t wp = (size_t)JN_NREP * JN_WPART_MAX;
  Scratch scratch(s);
  if (use_wpart) JN_HIP(scratch.take(wp * sizeof(float)));
  float* wpart = scratch.as<float>();
  if (wpart) JN_HIP(hipMemsetAsync(wpart, 0, wp * sizeof(float), s));
  const ChanTab it = chan_tab(tab_dev, cin);
  SlotBatch sb;      // the caller's [S, ...] tensors are slots already: x and the [3][cin] tables by their own size, g_z as said
  sb.n = n_slots; sb.act = M * x_ld; sb.tab = 3LL * cin; sb.grad = gz_slot_stride;
  auto launch = [&] {
    return launch_pw_bwd_weight(gz_dev, g_ld, x_dev, x_ld, it, gw_dev, wpart, M, cout, cin, s, sb, gz_slot_stride,
                                wide ? (exact ? CW_ROUTE_EXACT : CW_ROUTE_SPLIT) : 0);
  };
  auto back = [&] { return wpart ? hipMemcpyAsync(wpart_back_dev, wpart, wp * sizeof(float), hipMemcpyDeviceToDevice, s) : hipSuccess; };
  return run_entry("jn_pw_bwd_weight", s, launch, "no kernel took the launch, or its LDS was refused", back);
}

}  // extern "C"

// ---- stem, SPP, upsample, shortcut sum, BatchNorm tables and sums, embed_fpn linear on caller tensors (kernels_conv.hip, kernels_bwd.hip) ----
// The launchers refuse what their kernels cannot take (-1, before anything is launched); the entries check what only they can know
// (ranges that keep the index arithmetic in int, table shapes) and pass the launchers' refusals on.  These kernels have scalar
// tails: any channel count from 1 and any leading dimension (ld_ok), where the launcher does not say otherwise.  An entry with
// no device call before its launch passes the refusal on whatever state the device is in (run_entry<true>).
static StemArgs stem_entry_args(const void* src_dev, int src_u8, const int64_t* positions_dev, int pos_stride, long long sample_stride,
                                long long chan_stride, int row_stride, int P, int N, int cout, const float* w_dev) {
  StemArgs a{};
  a.src = src_dev; a.src_u8 = src_u8 ? 1 : 0; a.positions = positions_dev; a.pos_stride = pos_stride; a.sample_stride = sample_stride;
  a.chan_stride = chan_stride; a.row_stride = row_stride; a.P = P; a.N = N; a.cout = cout; a.w = w_dev;
  return a;
}
static bool stem_entry_ok(int P, int N, int cout, long long sample_stride, long long chan_stride, int row_stride) {
  return P >= 1 && P <= 4096 && N >= 1 && N <= 65536 && cout >= 1 && cout <= 4096 && sample_stride >= 0 && chan_stride >= 1 && row_stride >= 1;
}

extern "C" {

int jn_stem(const void* src_dev, int src_u8, const int64_t* positions_dev, int pos_stride, long long sample_stride, long long chan_stride,
            int row_stride, int P, int N, int cout, const float* w_dev, void* out_dev, int out_ld, int out_dtype, double* stats_dev, int nrep,
            const int* skip_flag_dev, int skip_when, int max_wg, void* stream) {
  JN_CHECK(src_dev && w_dev && out_dev, JN_EINVAL, "jn_stem: null argument");
  JN_CHECK(stem_entry_ok(P, N, cout, sample_stride, chan_stride, row_stride) && ld_ok(out_ld, cout) && dtype_ok(out_dtype) && nrep >= 1 &&
               nrep <= JN_NREP && max_wg >= 0,
           JN_EINVAL, "jn_stem: P=%d N=%d cout=%d out_ld=%d out_dtype=%d nrep=%d max_wg=%d", P, N, cout, out_ld, out_dtype, nrep, max_wg);
  StemArgs a = stem_entry_args(src_dev, src_u8, positions_dev, pos_stride, sample_stride, chan_stride, row_stride, P, N, cout, w_dev);
  a.out = out_dev; a.out_ld = out_ld; a.out_dtype = out_dtype; a.stats = stats_dev; a.stats_rep_stride = 2LL * cout; a.stats_nrep = nrep;
  a.skip_flag = skip_flag_dev; a.skip_when = skip_when;
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_stem", s, [&] { return launch_stem(a, s, max_wg); });
}

int jn_stem_bwd_weight(const void* src_dev, int src_u8, const int64_t* positions_dev, int pos_stride, long long pos_slot_stride,
                       long long sample_stride, long long chan_stride, int row_stride, int P, int N, int cout, const float* g_dev, int g_ld,
                       const float* z_dev, int z_ld, const float* otab_dev, const float* save_dev, const float* consts_dev, float* gw_dev,
                       float* wpart_dev, int n_slots, int max_wg, void* stream) {
  JN_CHECK(src_dev && g_dev && gw_dev && wpart_dev, JN_EINVAL, "jn_stem_bwd_weight: null argument");
  JN_CHECK(stem_entry_ok(P, N, cout, sample_stride, chan_stride, row_stride) && ld_ok(g_ld, cout) && slots_ok(n_slots) && max_wg >= 0 &&
               pos_slot_stride >= 0,
           JN_EINVAL, "jn_stem_bwd_weight: P=%d N=%d cout=%d g_ld=%d slots=%d max_wg=%d", P, N, cout, g_ld, n_slots, max_wg);
  JN_CHECK(!z_dev || (otab_dev && save_dev && consts_dev && ld_ok(z_ld, cout)), JN_EINVAL,
           "jn_stem_bwd_weight: the fused g_z form needs the output table, save and consts, and z_ld=%d >= %d", z_ld, cout);
  const StemArgs a = stem_entry_args(src_dev, src_u8, positions_dev, pos_stride, sample_stride, chan_stride, row_stride, P, N, cout, gw_dev);
  // (StemArgs::w: the weight gradient does not read the weight; the field holds the [108][cout] array of the same shape, as the
  // check both stem launchers share wants it set)
  const long long px = (long long)N * (P / 2) * (P / 2);
  SlotBatch sb;
  sb.n = n_slots; sb.grad = px * g_ld; sb.act = px * z_ld; sb.tab = 3LL * cout; sb.save = 2LL * cout; sb.consts = 3LL * cout; sb.pos = pos_slot_stride;
  const ChanTab ot = z_dev ? chan_tab(otab_dev, cout) : ChanTab{};
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_stem_bwd_weight", s, [&] {
    return launch_stem_bwd_weight(a, g_dev, g_ld, gw_dev, wpart_dev, s, sb, z_dev, z_ld, ot, save_dev, consts_dev, max_wg);
  });
}

int jn_spp_route(int dtype, int ld, int h, int H, int W, int N, int bwd) {
  JN_CHECK(dtype_ok(dtype), JN_EINVAL, "jn_spp_route: dtype=%d", dtype);
  const int r = spp_route(dtype, ld, h, H, W, N, bwd ? 1 : 0, 0);
  JN_CHECK(r > 0, JN_EINVAL, "jn_spp_route: no kernel takes %d x %d x %d with %d channels of %d (bwd %d)", N, H, W, h, ld, bwd);
  return r;
}

int jn_spp(void* cat_dev, int dtype, int ld, int h, int H, int W, int N, const float* tab_dev, const int* skip_flag_dev, int skip_when,
           int route, void* stream) {
  JN_CHECK(cat_dev && tab_dev, JN_EINVAL, "jn_spp: null argument");
  JN_CHECK(map_ok(N, H, W) && h >= 1 && h <= 2048 && ld_ok(ld, 4 * h) && dtype_ok(dtype) && route >= 0 && route <= SPP_ROUTE_SCALAR, JN_EINVAL,
           "jn_spp: %d x %d x %d, %d channels of %d, dtype %d, route %d", N, H, W, h, ld, dtype, route);
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_spp", s, [&] { return launch_spp(cat_dev, dtype, ld, h, H, W, N, chan_tab(tab_dev, h), skip_flag_dev, skip_when, s, route); });
}

int jn_spp_bwd(const float* cat_dev, float* gcat_dev, int ld, int h, int H, int W, int N, const float* tab_dev, int n_slots, int route,
               void* stream) {
  JN_CHECK(cat_dev && gcat_dev && tab_dev, JN_EINVAL, "jn_spp_bwd: null argument");
  JN_CHECK(map_ok(N, H, W) && h >= 1 && h <= 2048 && ld_ok(ld, 4 * h) && slots_ok(n_slots) && route >= 0 && route <= SPP_ROUTE_SCALAR, JN_EINVAL,
           "jn_spp_bwd: %d x %d x %d, %d channels of %d, %d slots, route %d", N, H, W, h, ld, n_slots, route);
  SlotBatch sb;      // the caller's [S, ...] tensors are slots already
  sb.n = n_slots; sb.act = sb.grad = (long long)N * H * W * ld; sb.tab = 3LL * h;
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_spp_bwd", s, [&] { return launch_spp_bwd(cat_dev, gcat_dev, ld, h, H, W, N, chan_tab(tab_dev, h), s, sb, route); });
}

int jn_upsample(const void* in_dev, int in_ld, void* out_dev, int out_ld, int dtype, int C, int H, int W, int N, const int* skip_flag_dev,
                int skip_when, void* stream) {
  JN_CHECK(in_dev && out_dev, JN_EINVAL, "jn_upsample: null argument");
  JN_CHECK(map_ok(N, 2 * H, 2 * W) && H >= 1 && W >= 1 && C >= 1 && ld_ok(in_ld, C) && ld_ok(out_ld, C), JN_EINVAL,      // (the OUTPUT map in range)
           "jn_upsample: %d x %d x %d, %d channels, leading dimensions %d and %d", N, H, W, C, in_ld, out_ld);
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_upsample", s, [&] { return launch_upsample(in_dev, in_ld, out_dev, out_ld, dtype, C, H, W, N, skip_flag_dev, skip_when, s); });
}

// (the kernel steps both gradients by ONE slot stride, the engine's gradient workspace: the caller's dense tensors are laid into
// slots [g_dst | g_src] as in jn_dw_bwd, so the call allocates, waits for the stream and frees)
int jn_upsample_bwd(const float* gdst_dev, int dst_ld, float* gsrc_dev, int src_ld, int C, int H, int W, int N, int accumulate, int n_slots,
                    void* stream) {
  JN_CHECK(gdst_dev && gsrc_dev, JN_EINVAL, "jn_upsample_bwd: null argument");
  JN_CHECK(map_ok(N, 2 * H, 2 * W) && H >= 1 && W >= 1 && C >= 1 && ld_ok(dst_ld, C) && ld_ok(src_ld, C) && slots_ok(n_slots), JN_EINVAL,
           "jn_upsample_bwd: %d x %d x %d, %d channels, leading dimensions %d and %d, %d slots", N, H, W, C, dst_ld, src_ld, n_slots);
  // (the launcher's refusal, taken before the workspace is allocated: whole quads, of up to 8192 channels)
  JN_CHECK(C >= 4 && C % 4 == 0 && dst_ld % 4 == 0 && src_ld % 4 == 0, JN_EINVAL, "jn_upsample_bwd: %d channels, leading dimensions %d and %d: whole quads",
           C, dst_ld, src_ld);
  hipStream_t s = (hipStream_t)stream;
  const size_t dn = (size_t)N * 4 * H * W * dst_ld, sn = (size_t)N * H * W * src_ld, slot = dn + sn;
  Scratch scratch(s);
  JN_HIP(scratch.take((size_t)n_slots * slot * sizeof(float)));
  float *gda = scratch.as<float>(), *gsa = gda + dn;
  const SlotLayout lay{n_slots, s};
  JN_HIP(lay.in(gda, slot, gdst_dev, dn));
  JN_HIP(lay.in(gsa, slot, gsrc_dev, sn));      // always: the channels past C and, with accumulate, the previous gradient come back as they were
  SlotBatch sb;
  sb.n = n_slots; sb.grad = (long long)slot;
  return run_entry("jn_upsample_bwd", s, [&] { return launch_upsample_bwd(gda, dst_ld, gsa, src_ld, C, H, W, N, accumulate ? 1 : 0, s, sb); },
                   "the launcher refused the arguments", [&] { return lay.back(gsrc_dev, sn, gsa, slot); });
}

int jn_addact(const void* z_dev, int z_ld, const float* ztab_dev, const void* res_dev, int res_ld, const float* rtab_dev, void* out_dev,
              int out_ld, int dtype, int C, long long M, const int* skip_flag_dev, int skip_when, void* stream) {
  JN_CHECK(z_dev && ztab_dev && res_dev && rtab_dev && out_dev, JN_EINVAL, "jn_addact: null argument");
  JN_CHECK(pixels_ok(M) && C >= 1 && ld_ok(z_ld, C) && ld_ok(res_ld, C) && ld_ok(out_ld, C), JN_EINVAL,
           "jn_addact: M=%lld, %d channels, leading dimensions %d, %d and %d", M, C, z_ld, res_ld, out_ld);
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_addact", s, [&] {
    return launch_addact(z_dev, z_ld, chan_tab(ztab_dev, C), res_dev, res_ld, chan_tab(rtab_dev, C), out_dev, out_ld, dtype, C, M, skip_flag_dev, skip_when, s);
  });
}

int jn_bn_finalize(const double* stats_dev, long long rep_stride, double count, const float* gamma_dev, const float* beta_dev, float* run_mean_dev,
                   float* run_var_dev, float* save_dev, float* tab0_dev, float* tab1_dev, int C, float eps, float momentum,
                   const int* skip_flag_dev, int skip_when, void* stream) {
  JN_CHECK(stats_dev && gamma_dev && beta_dev && tab0_dev, JN_EINVAL, "jn_bn_finalize: null argument");
  JN_CHECK(C >= 1 && C <= 8192 && eps > 0.0f && momentum >= 0.0f && momentum <= 1.0f, JN_EINVAL, "jn_bn_finalize: C=%d eps=%g momentum=%g", C, eps,
           momentum);
  const ChanTab t0 = chan_tab(tab0_dev, C), t1 = tab1_dev ? chan_tab(tab1_dev, C) : ChanTab{};
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_bn_finalize", s, [&] {
    return launch_bn_finalize(stats_dev, rep_stride, count, gamma_dev, beta_dev, run_mean_dev, run_var_dev, save_dev, t0, t1, C, eps, momentum,
                              skip_flag_dev, skip_when, s);
  });
}

// (the kernel takes the running statistics as per-channel addresses, as the engine's parameter arena has them: built here from the
// two dense arrays, so the call allocates, waits for the stream and frees)
int jn_bn_finalize_all(const double* stats_dev, long long rep_stride, int n_stat, int N, const float* hw_dev, const int* goff_dev,
                       const int* boff_dev, const float* params_dev, const int* t0_dev, const int* t1_dev, float* tab_dev, int tab_channels,
                       float* save_dev, float* run_mean_dev, float* run_var_dev, float eps, float momentum, const int* skip_flag_dev, int skip_when,
                       long long defer_max_m, void* stream) {
  JN_CHECK(stats_dev && hw_dev && goff_dev && boff_dev && params_dev && t0_dev && t1_dev && tab_dev && save_dev && run_mean_dev && run_var_dev,
           JN_EINVAL, "jn_bn_finalize_all: null argument");
  JN_CHECK(n_stat >= 1 && n_stat <= (1 << 20) && N >= 1 && tab_channels >= 1 && rep_stride >= 2LL * n_stat && eps > 0.0f && momentum >= 0.0f &&
               momentum <= 1.0f && defer_max_m >= 0,
           JN_EINVAL, "jn_bn_finalize_all: %d channels, N=%d, table of %d, replicas %lld apart", n_stat, N, tab_channels, rep_stride);
  hipStream_t s = (hipStream_t)stream;
  std::vector<float*> addr(2 * (size_t)n_stat);      // (pageable memory the copy below reads until the stream is waited for: it outlives `scratch`)
  for (int i = 0; i < n_stat; ++i) { addr[i] = run_mean_dev + i; addr[n_stat + i] = run_var_dev + i; }
  Scratch scratch(s);
  JN_HIP(scratch.take(addr.size() * sizeof(float*)));
  float** addr_dev = scratch.as<float*>();
  JN_HIP(hipMemcpyAsync(addr_dev, addr.data(), addr.size() * sizeof(float*), hipMemcpyHostToDevice, s));
  BnAllArgs a{};
  a.stats = stats_dev; a.rep_stride = rep_stride; a.n_stat = n_stat; a.N = N; a.hw = hw_dev; a.goff = goff_dev; a.boff = boff_dev;
  a.params = params_dev; a.t0 = t0_dev; a.t1 = t1_dev; a.tab = tab_dev; a.tab_channels = tab_channels; a.save = save_dev;
  a.run_mean = addr_dev; a.run_var = addr_dev + n_stat; a.eps = eps; a.momentum = momentum; a.skip_flag = skip_flag_dev;
  a.skip_when = skip_when; a.defer_max_m = defer_max_m;
  return run_entry("jn_bn_finalize_all", s, [&] { return launch_bn_finalize_all(a, s); });
}

int jn_bn_bwd_sums(const float* g_dev, int g_ld, const float* z_dev, int z_ld, const float* tab_dev, const float* save_dev, int C, long long M,
                   int n_slots, double* red_dev, const float* gamma_dev, const float* beta_dev, float* consts_dev, float* g_gamma_dev,
                   float* g_beta_dev, int reduce, int raw_moment, void* stream) {
  JN_CHECK(save_dev && red_dev && (!reduce || (g_dev && z_dev && tab_dev)), JN_EINVAL, "jn_bn_bwd_sums: null argument");
  JN_CHECK(!consts_dev || (gamma_dev && beta_dev && g_gamma_dev && g_beta_dev), JN_EINVAL, "jn_bn_bwd_sums: consts need gamma, beta and their gradients");
  JN_CHECK((reduce || consts_dev) && !(reduce && raw_moment), JN_EINVAL,
           "jn_bn_bwd_sums: nothing to do, or a raw moment asked of the reduce kernel (it forms the moment against zhat)");
  JN_CHECK(pixels_ok(M) && C >= 1 && C <= 8192 && slots_ok(n_slots) && (!reduce || (ld_ok(g_ld, C) && ld_ok(z_ld, C))), JN_EINVAL,
           "jn_bn_bwd_sums: M=%lld, %d channels, leading dimensions %d and %d, %d slots", M, C, g_ld, z_ld, n_slots);
  SlotBatch sb;      // the caller's [S, ...] tensors are slots already
  sb.n = n_slots; sb.grad = M * g_ld; sb.act = M * z_ld; sb.tab = 3LL * C; sb.save = 2LL * C; sb.consts = 3LL * C; sb.red = (long long)JN_NREP * 2 * C;
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_bn_bwd_sums", s, [&] {
    int rc = reduce ? launch_bn_bwd_reduce(g_dev, g_ld, z_dev, z_ld, chan_tab(tab_dev, C), save_dev, C, M, red_dev, 2LL * C, s, sb) : 0;
    if (rc == 0 && consts_dev)
      rc = launch_bn_bwd_consts(red_dev, 2LL * C, (double)M, gamma_dev, beta_dev, save_dev, consts_dev, g_gamma_dev, g_beta_dev, C, s, sb, raw_moment ? 1 : 0);
    return rc;
  });
}

int jn_efpn_linear(const float* e_dev, const float* wt_dev, float* part_dev, int N, int K, int Co, int KS, const int* skip_flag_dev, int skip_when,
                   void* stream) {
  JN_CHECK(e_dev && wt_dev && part_dev, JN_EINVAL, "jn_efpn_linear: null argument");
  JN_CHECK(N >= 1 && N <= 65535 && K >= 1 && K <= (1 << 24) && Co >= 1 && Co <= 4096 && KS >= 1 && KS <= 4096, JN_EINVAL,
           "jn_efpn_linear: N=%d K=%d Co=%d KS=%d", N, K, Co, KS);
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_efpn_linear", s, [&] { return launch_efpn_linear(e_dev, wt_dev, part_dev, N, K, Co, KS, skip_flag_dev, skip_when, s); });
}

}  // extern "C"

// ---- decision-side training kernels on caller tensors (kernels_train.hip) ------------------------------------------------------------
// The three loss kernels and the optimiser update, one launch each.  The launchers refuse nothing, so every range is the entry's:
// B * T tokens and n_actions that keep the kernels' index arithmetic in int.  Actions and targets are the caller's to keep inside
// [0, nA) (the context's rollouts and teachers do); n_done is the rollout's int32 [T + 1] count of finished agents per step.
static bool tokens_ok(int B, int T, int nA) { return B >= 1 && T >= 1 && nA >= 1 && nA <= 256 && (long long)B * T <= (1LL << 24); }

extern "C" {

int jn_reinforce_loss(const float* logits_dev, const int64_t* actions_dev, const float* returns_dev, const float* rewards_dev,
                      const uint8_t* logit_masks_dev, const int32_t* n_done_dev, int B, int T, int nA, int reward_norm, float ret_mean,
                      float ret_std, float entropy_weight, float loss_scale, float* dlogits_dev, float* metrics_dev, void* stream) {
  JN_CHECK(logits_dev && actions_dev && returns_dev && rewards_dev && logit_masks_dev && dlogits_dev && metrics_dev, JN_EINVAL,
           "jn_reinforce_loss: null argument");
  JN_CHECK(tokens_ok(B, T, nA), JN_EINVAL, "jn_reinforce_loss: B=%d T=%d nA=%d", B, T, nA);
  LossArgs a{};
  a.logits = logits_dev; a.actions = actions_dev; a.returns = returns_dev; a.rewards = rewards_dev; a.logit_masks = logit_masks_dev;
  a.n_done = n_done_dev; a.dlogits = dlogits_dev; a.metrics = metrics_dev;
  a.B = B; a.T = T; a.nA = nA; a.stop_early = n_done_dev ? 1 : 0; a.reward_norm = reward_norm ? 1 : 0;
  a.ret_mean = ret_mean; a.ret_std = ret_std; a.entropy_weight = entropy_weight; a.scale = loss_scale;
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_reinforce_loss", s, [&] { return launch_reinforce_loss(a, s); });
}

int jn_logits_grad(const float* logits_dev, const int64_t* actions_dev, const float* dlogprobs_dev, const float* dentropies_dev,
                   const int32_t* n_done_dev, int B, int T, int nA, float* dlogits_dev, void* stream) {
  JN_CHECK(logits_dev && actions_dev && dlogits_dev && (dlogprobs_dev || dentropies_dev), JN_EINVAL, "jn_logits_grad: null argument");
  JN_CHECK(tokens_ok(B, T, nA), JN_EINVAL, "jn_logits_grad: B=%d T=%d nA=%d", B, T, nA);
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_logits_grad", s, [&] {
    return launch_logits_grad(logits_dev, actions_dev, dlogprobs_dev, dentropies_dev, n_done_dev, dlogits_dev, B, T, nA, n_done_dev ? 1 : 0, s);
  });
}

int jn_reinforce_loss_masked(const float* logits_dev, const int64_t* actions_dev, const float* returns_dev, const float* rewards_dev,
                             const uint8_t* logit_masks_dev, const int32_t* n_done_dev, int B, int T, int nA, int reward_norm,
                             float ret_mean, float ret_std, float entropy_weight, float loss_scale, float* dlogits_dev,
                             float* metrics_dev, const uint16_t* sets_dev, void* stream) {
  JN_CHECK(logits_dev && actions_dev && returns_dev && rewards_dev && logit_masks_dev && dlogits_dev && metrics_dev && sets_dev, JN_EINVAL,
           "jn_reinforce_loss_masked: null argument");
  JN_CHECK(tokens_ok(B, T, nA) && nA <= 16, JN_EINVAL, "jn_reinforce_loss_masked: B=%d T=%d nA=%d", B, T, nA);
  LossArgs a{};
  a.logits = logits_dev; a.actions = actions_dev; a.returns = returns_dev; a.rewards = rewards_dev; a.logit_masks = logit_masks_dev;
  a.n_done = n_done_dev; a.dlogits = dlogits_dev; a.metrics = metrics_dev; a.sets = sets_dev;
  a.B = B; a.T = T; a.nA = nA; a.stop_early = n_done_dev ? 1 : 0; a.reward_norm = reward_norm ? 1 : 0;
  a.ret_mean = ret_mean; a.ret_std = ret_std; a.entropy_weight = entropy_weight; a.scale = loss_scale;
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_reinforce_loss_masked", s, [&] { return launch_reinforce_loss(a, s); });
}

int jn_logits_grad_masked(const float* logits_dev, const int64_t* actions_dev, const float* dlogprobs_dev, const float* dentropies_dev,
                          const int32_t* n_done_dev, int B, int T, int nA, float* dlogits_dev, const uint16_t* sets_dev, void* stream) {
  JN_CHECK(logits_dev && actions_dev && dlogits_dev && sets_dev && (dlogprobs_dev || dentropies_dev), JN_EINVAL,
           "jn_logits_grad_masked: null argument");
  JN_CHECK(tokens_ok(B, T, nA) && nA <= 16, JN_EINVAL, "jn_logits_grad_masked: B=%d T=%d nA=%d", B, T, nA);
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_logits_grad_masked", s, [&] {
    return launch_logits_grad(logits_dev, actions_dev, dlogprobs_dev, dentropies_dev, n_done_dev, dlogits_dev, B, T, nA, n_done_dev ? 1 : 0, s,
                              sets_dev);
  });
}

int jn_ce_loss(const float* logits_dev, const int64_t* target_dev, const uint8_t* masks_dev, int B, int T, int nA, float stop_weight,
               float* dlogits_dev, float* metrics_dev, void* stream) {
  JN_CHECK(logits_dev && target_dev && masks_dev && dlogits_dev && metrics_dev, JN_EINVAL, "jn_ce_loss: null argument");
  JN_CHECK(tokens_ok(B, T, nA), JN_EINVAL, "jn_ce_loss: B=%d T=%d nA=%d", B, T, nA);
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_ce_loss", s, [&] { return launch_ce_loss(logits_dev, target_dev, masks_dev, stop_weight, dlogits_dev, metrics_dev, B * T, nA, T, s); });
}

// (the betas and eps are those of jn_optimizer_step_group: torch's defaults)
int jn_adamw(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, long long n, float lr, float weight_decay, int step, float clip_value,
             float grad_scale, void* stream) {
  JN_CHECK(p_dev && g_dev && m_dev && v_dev, JN_EINVAL, "jn_adamw: null argument");
  JN_CHECK(n >= 1 && n <= (1LL << 38) && step >= 1 && lr >= 0.0f && weight_decay >= 0.0f && clip_value >= 0.0f, JN_EINVAL,
           "jn_adamw: n=%lld step=%d lr=%g weight_decay=%g clip_value=%g", n, step, lr, weight_decay, clip_value);
  hipStream_t s = (hipStream_t)stream;
  return run_entry<true>("jn_adamw", s, [&] { return launch_adamw(p_dev, g_dev, m_dev, v_dev, n, lr, 0.9, 0.999, 1e-8f, weight_decay, step, clip_value, grad_scale, s); });
}

}  // extern "C"
