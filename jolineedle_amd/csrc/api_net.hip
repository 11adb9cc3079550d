// C ABI of libjnroll.so, conv-stack unit: workspace slots and tables, the forward and backward launch loops of a PAFPN, embed_fpn.
// Host code only (compiled by hipcc as C++); kernels live in kernels_*.hip.
#include <algorithm>
#include <cstring>

#include "jn_internal.h"

using namespace jnr;

// (scale, shift, flag) of BN channels from the running statistics (eval mode)
extern "C"
__global__ void bn_eval_table_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                     const float* __restrict__ rmean, const float* __restrict__ rvar, ChanTab t0,
                                     ChanTab t1, int C, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = gamma[c] / sqrtf(rvar[c] + eps);
  const float sh = beta[c] - rmean[c] * sc;
  t0.sc[c] = sc; t0.sh[c] = sh; t0.fl[c] = 1.0f;
  if (t1.sc) { t1.sc[c] = sc; t1.sh[c] = sh; t1.fl[c] = 1.0f; }
}

extern "C"
__global__ void fill_kernel(float* p, float v, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// *total += the number of 32-bit words in which a and b differ (grid-stride; a workgroup adds its count once)
extern "C"
__global__ __launch_bounds__(256) void word_diff_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, long long n,
                                                        unsigned long long* __restrict__ total) {
  __shared__ unsigned int wg_count;
  if (threadIdx.x == 0) wg_count = 0;
  __syncthreads();
  unsigned int c = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) c += a[i] != b[i] ? 1u : 0u;
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&wg_count, c);
  __syncthreads();
  if (threadIdx.x == 0 && wg_count) atomicAdd(total, (unsigned long long)wg_count);
}

// finishes the split-K sums: out[n][c] = bias[c] + sum_ks part[n][ks][c]
extern "C"
__global__ void emb_finish_kernel(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ out,
                                  long long out_stride, int N, int KS, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  float s = bias[c];
  for (int k = 0; k < KS; ++k) s += part[((long long)n * KS + k) * C + c];
  out[(long long)n * out_stride + c] = s;
}

namespace jnr {

// YOLOX BaseConv = bias-free conv + BatchNorm2d(eps=1e-3, momentum=0.03) + SiLU.
// Nothing is folded: convs write raw z and consumers apply (scale, shift) + SiLU on read.
constexpr float kBnEps = 1e-3f;
constexpr float kBnMomentum = 0.03f;

// Train-mode pass over N patches that defers: the channel runs of view v for the kernel arguments (ChanTab::r0..r3; at
// most four: a concat of a few producers; more: nseg = 0 and the kernels read the arrays).  False, t untouched: no
// channel of the view has its table deferred at this N.  Needs the host descriptors of ensure_defer_tables.
static bool defer_tab_runs(const Net& net, const View& v, int N, ChanTab& t) {
  const int off = net.tab_off[v.buf] + v.coff;
  auto deferred = [&](int c) { return net.h_td_hw[off + c] > 0.0f && (double)N * net.h_td_hw[off + c] <= (double)JN_DEFER_MAX_M; };
  bool any = false;
  for (int c = 0; c < v.C && !any; ++c) any = deferred(c);
  if (!any) return false;
  int ns = 0;
  bool fits = true;
  for (int c = 0; c < v.C && fits;) {
    const int tc = off + c;
    const bool d = deferred(c);
    int e = c + 1;
    if (d) {
      while (e < v.C && net.h_td_src[off + e] == net.h_td_src[tc] + (e - c) && net.h_td_goff[off + e] == net.h_td_goff[tc] + (e - c) &&
             net.h_td_boff[off + e] == net.h_td_boff[tc] + (e - c) && net.h_td_hw[off + e] == net.h_td_hw[tc])
        ++e;
    } else {
      while (e < v.C && !deferred(e)) ++e;
    }
    if (ns == 4) { fits = false; break; }
    const ChanTab::Run run{c, e, d ? net.h_td_src[tc] : -1, net.h_td_goff[tc], net.h_td_boff[tc], net.h_td_hw[tc]};
    (ns == 0 ? t.r0 : ns == 1 ? t.r1 : ns == 2 ? t.r2 : t.r3) = run;
    ++ns;
    c = e;
  }
  t.nseg = fits ? ns : 0;
  return true;
}

// N plain patches [n][3][P][P] (no positions), sample_stride elements apart (0: back to back)
StemSrc patch_src(const void* ptr, int P, long long sample_stride) {
  return StemSrc{ptr, nullptr, sample_stride ? sample_stride : 3LL * P * P, (long long)P * P, P};
}

// Allocates (or grows to) n_slots workspace slots of a net; tables start as identity
// (scale 1, shift 0, flag 0 = "already an activation").
// The activations get a_slots slots of their own (default: as many).  Either count only grows, and a call that grows
// neither allocates nothing.
int ensure_slots(jn_ctx* ctx, Net& net, int n_slots, int a_slots) {
  if (a_slots < 0) a_slots = n_slots;
  const bool grow_tab = net.n_slots < n_slots, grow_act = net.a_slots < a_slots;
  if (!grow_tab && !grow_act) return JN_OK;
  const int MB = ctx->cfg.max_batch;
  float *tab = net.tab, *save = net.save;
  double* stats = net.stats;
  char* act = net.act;
  int rc;
  if (grow_act && (rc = dev_alloc(ctx, &act, (size_t)a_slots * net.per_image_floats * MB * act_esz(net)))) return rc;
  if (grow_tab) {
    if ((rc = dev_alloc(ctx, &tab, (size_t)n_slots * 3 * net.tab_channels))) return rc;
    if ((rc = dev_alloc(ctx, &save, (size_t)n_slots * 2 * net.stat_channels))) return rc;
    if ((rc = dev_alloc(ctx, &stats, (size_t)n_slots * JN_NREP * 2 * net.stat_channels))) return rc;
  }
  // old (smaller) allocations stay owned by the context until jn_destroy; slots are grown once per config.  What the
  // old slots hold moves along (a detector pass may need its slot AFTER a train-mode rollout filled the encoder's, and
  // the rollout's backward still reads them: the reference's statement order, src/reinforce.py:326-341)
  const int n_old = net.n_slots, a_old = net.a_slots;
  if (n_old > 0 || a_old > 0) JN_HIP(hipDeviceSynchronize());
  if (grow_act && a_old > 0)
    JN_HIP(hipMemcpy(act, net.act, (size_t)a_old * net.per_image_floats * MB * act_esz(net), hipMemcpyDeviceToDevice));
  if (grow_tab && n_old > 0) {
    JN_HIP(hipMemcpy(tab, net.tab, (size_t)n_old * 3 * net.tab_channels * sizeof(float), hipMemcpyDeviceToDevice));
    JN_HIP(hipMemcpy(save, net.save, (size_t)n_old * 2 * net.stat_channels * sizeof(float), hipMemcpyDeviceToDevice));
    JN_HIP(hipMemcpy(stats, net.stats, (size_t)n_old * JN_NREP * 2 * net.stat_channels * sizeof(double), hipMemcpyDeviceToDevice));
  }
  net.act = act; net.a_slots = std::max(a_old, a_slots);
  if (!grow_tab) return JN_OK;
  net.tab = tab; net.save = save; net.stats = stats; net.n_slots = n_slots;
  for (int sl = n_old; sl < n_slots; ++sl) {
    float* t = tab + (size_t)sl * 3 * net.tab_channels;
    const long long n = net.tab_channels;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, t, 1.0f, n);
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, 0, t + n, 0.0f, 2 * n);
  }
  JN_HIP(hipGetLastError());
  JN_HIP(hipDeviceSynchronize());           // (the fills ran on the null stream; callers launch on theirs)
  if (n_old == 0) net.eval_tab_dirty = true;
  return JN_OK;
}

// Slot-0 table from the BN running statistics (after a weight load or a training step).
int refresh_eval_table(jn_ctx* ctx, Net& net, hipStream_t s) {
  if (!net.eval_tab_dirty) return JN_OK;
  for (const Op& op : net.ops) {
    if (op.wslot < 0) continue;
    const ConvW& cw = net.convs[op.wslot];
    if (!cw.has_bn) continue;
    ChanTab t1{nullptr, nullptr, nullptr};
    if (op.alias.buf >= 0) t1 = view_tab(net, 0, op.alias);
    hipLaunchKernelGGL(bn_eval_table_kernel, dim3((cw.cout + 63) / 64), dim3(64), 0, s, cw.gamma_dev, cw.beta_dev,
                       cw.rmean_dev, cw.rvar_dev, view_tab(net, 0, op.out), t1, cw.cout, kBnEps);
  }
  JN_HIP(hipGetLastError());
  net.eval_tab_dirty = false;
  return JN_OK;
}

// fp32 passes: the 1x1 weights of `net` as three bf16 planes for pw_x3_kernel (bf16 inference mode uses the h plane
// alone: pw_x1).  Split again only after something wrote the arena (mark_params_written): a rollout's T passes and
// every eval pass in between reuse the planes (for yolox-s / -m detectors the split is tens of MB per pass).
// Two launches per split: the whole range in flat order, then the convs of pw_x3_fragment_order rewritten in fragment
// order from one device table (built once per net, with the range, when the weights have their arena places).
static int refresh_x3_planes(jn_ctx* ctx, Net& net, hipStream_t s) {
  if (net.x3_hi == 0) {
    size_t lo = ctx->arena_size, hi = 0;
    std::vector<X3FragConv> frag;
    for (const Op& op : net.ops) {
      if (op.kind != OP_PW || op.wslot < 0) continue;
      const ConvW& cw = net.convs[op.wslot];
      if (!cw.w_dev) continue;
      const size_t o = (size_t)(cw.w_dev - ctx->params);
      lo = std::min(lo, o); hi = std::max(hi, o + (size_t)cw.cout * cw.cin);
      // (the shape and the alignment run_net hands the kernels: a.cin, a.cout, a.w_x3)
      if (o % 8 == 0 && op.in.C * op.out.C == cw.cin * cw.cout && pw_x3_fragment_order(op.in.C, op.out.C)) {
        bool seen = false;                                // (a conv two ops share is rewritten once)
        for (const X3FragConv& f : frag) seen = seen || f.off == (long long)o;
        if (!seen) frag.push_back(X3FragConv{(long long)o, op.out.C, op.in.C});
      }
    }
    if (!frag.empty() && !net.x3_frag) {
      int rc;
      if ((rc = dev_alloc(ctx, &net.x3_frag, frag.size()))) return rc;
      JN_HIP(hipMemcpy(net.x3_frag, frag.data(), frag.size() * sizeof(X3FragConv), hipMemcpyHostToDevice));
      net.x3_frag_n = (int)frag.size();
      for (const X3FragConv& f : frag) net.x3_frag_max = std::max(net.x3_frag_max, f.cout * f.cin);
    }
    net.x3_lo = lo / 8 * 8; net.x3_hi = hi > lo ? (hi + 7) / 8 * 8 : 0;
  }
  if (net.x3_hi > net.x3_lo && net.x3_dirty) {
    launch_w_split3(ctx->params + net.x3_lo, ctx->params_x3 + 3 * net.x3_lo, (long long)(net.x3_hi - net.x3_lo), s);
    launch_w_split3_frag(ctx->params, ctx->params_x3, net.x3_frag, net.x3_frag_n, net.x3_frag_max, s);
    net.x3_dirty = false;
  }
  return JN_OK;
}

// Something wrote the parameter arena (jn_load_weights, an optimiser step, jn_import_arena): BN affine and 1x1 weights
// may have moved, so the slot-0 tables and the split-bf16 planes of both nets are stale.
void mark_params_written(jn_ctx* ctx) {
  for (Net& net : ctx->nets) net.eval_tab_dirty = net.x3_dirty = true;
}

// ---- network execution ---------------------------------------------------------------
static View net_full_view(const Net& net, int buf) {
  View v; v.buf = buf; v.H = net.bufs[buf].H; v.W = net.bufs[buf].W; v.C = net.bufs[buf].C; v.coff = 0;
  return v;
}

// Descriptors of the deferred BatchNorm tables (ChanTab): which (sum, sumsq) pair, BatchNorm weight / bias and pixel
// count stand behind every table channel, and the reverse map for the one finalize launch per pass.  Only a net that
// is defer_eligible (plan.cpp) takes part.
static int ensure_defer_tables(jn_ctx* ctx, Net& net) {
  if (net.defer_built) return JN_OK;
  net.defer_built = true;
  if (!ctx->params || !defer_eligible(net)) return JN_OK;
  const int n_ops = net.n_backbone_ops < 0 ? (int)net.ops.size() : net.n_backbone_ops;
  const int TC = net.tab_channels, SC = net.stat_channels;
  std::vector<int> td_src(TC, -1), td_g(TC, 0), td_b(TC, 0), fd_g(SC, 0), fd_b(SC, 0), fd_t0(SC, 0), fd_t1(SC, -1);
  std::vector<float> td_hw(TC, 0.0f), fd_hw(SC, 0.0f);
  std::vector<float*> fd_rm(SC, nullptr), fd_rv(SC, nullptr);
  for (int oi = 0; oi < n_ops; ++oi) {
    const Op& op = net.ops[oi];
    if (op.wslot < 0) continue;
    const ConvW& cw = net.convs[op.wslot];
    const float hw = (float)(op.out.H * op.out.W);
    for (int j = 0; j < cw.cout; ++j) {
      const int i = cw.stat_off + j;
      const int g = (int)(cw.gamma_dev - ctx->params) + j, b = (int)(cw.beta_dev - ctx->params) + j;
      fd_hw[i] = hw; fd_g[i] = g; fd_b[i] = b; fd_rm[i] = cw.rmean_dev + j; fd_rv[i] = cw.rvar_dev + j;
      const View* vs[2] = {&op.out, op.alias.buf >= 0 ? &op.alias : nullptr};
      for (int k = 0; k < 2; ++k) {
        if (!vs[k]) continue;
        const int tc = net.tab_off[vs[k]->buf] + vs[k]->coff + j;
        (k == 0 ? fd_t0 : fd_t1)[i] = tc;
        td_src[tc] = i; td_hw[tc] = hw; td_g[tc] = g; td_b[tc] = b;
      }
    }
  }
  int rc;
  auto up = [&](auto** dst, const auto& host) -> int {
    using T = typename std::remove_reference<decltype(host[0])>::type;
    typename std::remove_const<T>::type* d = nullptr;
    if ((rc = dev_alloc(ctx, &d, host.size()))) return rc;
    JN_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = d;
    return JN_OK;
  };
  if ((rc = up(&net.td_src, td_src)) || (rc = up(&net.td_goff, td_g)) || (rc = up(&net.td_boff, td_b)) || (rc = up(&net.td_hw, td_hw)) ||
      (rc = up(&net.fd_hw, fd_hw)) || (rc = up(&net.fd_goff, fd_g)) || (rc = up(&net.fd_boff, fd_b)) || (rc = up(&net.fd_t0, fd_t0)) ||
      (rc = up(&net.fd_t1, fd_t1)) || (rc = up(&net.fd_rm, fd_rm)) || (rc = up(&net.fd_rv, fd_rv)))
    return rc;
  net.h_td_hw.assign(TC, 0.0f);
  for (int tc = 0; tc < TC; ++tc) if (td_src[tc] >= 0) net.h_td_hw[tc] = td_hw[tc];
  net.h_td_src = td_src; net.h_td_goff = td_g; net.h_td_boff = td_b;
  net.defer_ok = true;
  return JN_OK;
}

// JN_LAYER_PROFILE / JN_BWD_PROFILE: HIP events around every op of a pass and its table on stderr (a measuring aid, off
// by default).  Event i closes op i - 1 of a forward pass; the backward walks in reverse, so event i + 1 opens its op i.
namespace {
struct OpProfile {
  std::vector<hipEvent_t> ev;
  hipStream_t s;
  double tot_us = 0, tot_b = 0;
  OpProfile(bool on, int n_events, hipStream_t s_) : s(s_) {
    if (on) { ev.resize(n_events); for (auto& e : ev) (void)hipEventCreate(&e); }
  }
  ~OpProfile() { for (auto& e : ev) (void)hipEventDestroy(e); }
  explicit operator bool() const { return !ev.empty(); }
  void mark(int i) { if (!ev.empty()) (void)hipEventRecord(ev[i], s); }
  void row(const Op& op, int from, int to, double bytes, bool bwd) {
    static const char* kn[] = {"stem", "pw", "dw", "conv3", "spp", "upsample", "addact", "pred"};
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev[from], ev[to]);
    tot_us += ms * 1e3; tot_b += bytes;
    fprintf(stderr, "%-8s %-44s in %3dx%3dx%3d out %3dx%3dx%3d s%d", kn[op.kind], op.name.c_str(), op.in.H, op.in.W, op.in.C,
            op.out.H, op.out.W, op.out.C, op.stride);
    if (bwd) fprintf(stderr, " acc %d  %8.1f us  %8.1f MB  %6.0f GB/s\n", (int)op.acc_in, ms * 1e3, bytes / 1e6, bytes / (ms * 1e-3) / 1e9);
    else fprintf(stderr, "  %8.1f us  %7.1f MB  %7.0f GB/s\n", ms * 1e3, bytes / 1e6, bytes / (ms * 1e-3) / 1e9);
  }
  void total() { fprintf(stderr, "# total %.1f us, %.1f MB, %.0f GB/s\n", tot_us, tot_b / 1e6, tot_b / (tot_us * 1e-6) / 1e9); }
};
}  // namespace

// The autograd bridges differentiate LATER what a forward left in the workspace: a pass over the same slots in between
// makes that state stale (the backward entry points then fail with JN_ESTATE instead of computing garbage).  Slots: 0 =
// eval / supervised pass; 1 .. T = the glimpse steps of a train-mode rollout of the ENCODER net; from det_slot_base on =
// detector training passes.
static void invalidate_slot_state(jn_ctx* ctx, int ni, int slot) {
  if (ni == ctx->enc_net) {
    if (slot == 0) ctx->sup_valid = false;
    else if (ni != JN_NET_DETECTOR || slot < det_slot_base(ctx)) ctx->train_out_valid = false;
  }
  if (ni == JN_NET_DETECTOR && slot >= det_slot_base(ctx) && slot - det_slot_base(ctx) < (int)ctx->det_pass.size())
    ctx->det_pass[slot - det_slot_base(ctx)].valid = false;
}

static ChanTab tab_at(ChanTab t, int c0) { t.sc += c0; t.sh += c0; t.fl += c0; return t; }      // channels c0 .. of a table

// The stem conv cw over the N patches of ss: source and weight.  Output, statistics and skip fields are the caller's.
static StemArgs stem_args(const StemSrc& ss, const Net& net, int N, const ConvW& cw) {
  StemArgs a{};
  a.src = ss.src; a.positions = ss.positions; a.pos_stride = ss.pos_stride; a.sample_stride = ss.sample_stride;
  a.chan_stride = ss.chan_stride; a.row_stride = ss.row_stride; a.P = net.P; a.N = N; a.cout = cw.cout; a.w = cw.w_dev;
  a.src_u8 = ss.src_u8;
  return a;
}

// One pass of a PAFPN over N patches in workspace slot `slot`.  train != 0: batch-statistics
// BatchNorm (stats accumulated by every conv, finalised per layer, running stats updated).
// The routes come from plan_forward (plan.cpp); what depends on launch-time state stays here.
// The activations go to slot `slot`, tables / saved statistics / sums to table slot tab_slot (< 0: the same slot).
// mode RUN_REPLAY: the train-mode pass that filled table slot tab_slot once more, into activation slot `slot`, from what
// that slot kept: the same plan, kernels and instantiations; consumers of deferred tables read the kept sums, the others
// the kept table; the producers add their sums to a sink nobody reads (the accumulating instantiations, so that no
// element rounds differently); no finalize launch, no running-statistics update, no write to `save`.  Every conv has one
// writer per element, so the slot comes out bit for bit.  Of the validity flags only the eval workspace's (slot 0) moves.
int run_net(jn_ctx* ctx, int ni, int N, const StemSrc& ss, int slot, int train, const int* skip_flag, int skip_when,
            hipStream_t s, bool with_head, int first_op, int tab_slot, RunMode mode) {
  Net& net = ctx->nets[ni];
  const int MB = ctx->cfg.max_batch;
  const bool replay = mode == RUN_REPLAY;
  const int ts = tab_slot < 0 ? slot : tab_slot;
  int rc;
  JN_CHECK(slot >= 0 && slot < net.a_slots && ts >= 0 && ts < net.n_slots, JN_ESTATE, "pass over activation slot %d, table slot %d: not allocated", slot, ts);
  JN_CHECK(!replay || (train && !with_head && first_op == 0), JN_ESTATE, "a replay is a whole train-mode pass without the head");
  if (!replay) invalidate_slot_state(ctx, ni, slot);
  else if (slot == 0 && ni == ctx->enc_net) ctx->sup_valid = false;
  if (!train && (rc = refresh_eval_table(ctx, net, s))) return rc;
  const bool x3 = ctx->params_x3 && !std::getenv("JN_NO_PW_X3");   // read per pass: tests flip it
  if (x3 && (rc = refresh_x3_planes(ctx, net, s))) return rc;
  double* stats = train ? slot_stats(net, ts) : nullptr;    // what the consumers of deferred tables read
  float* save = train ? slot_save(net, ts) : nullptr;
  if (replay && !net.stats_sink) {
    if ((rc = dev_alloc(ctx, &net.stats_sink, (size_t)JN_NREP * 2 * net.stat_channels))) return rc;
    JN_HIP(hipMemsetAsync(net.stats_sink, 0, (size_t)JN_NREP * 2 * net.stat_channels * sizeof(double), s));
  }
  double* acc = replay ? net.stats_sink : stats;            // what the producers add to
  // (a train-mode rollout zeroes the statistics of all its slots with ONE memset up front)
  if (train && !replay && !ctx->stats_prezeroed) JN_HIP(hipMemsetAsync(stats, 0, (size_t)JN_NREP * 2 * net.stat_channels * sizeof(double), s));
  const long long rep_stride = 2LL * net.stat_channels;
  // deferred tables: the small-map layers of the depthwise fp32 encoder get no finalize launch of their own; their
  // consumers read the batch sums (ChanTab in jn_kernels.h), one finalize launch closes the pass
  if (train && !with_head && (rc = ensure_defer_tables(ctx, net))) return rc;
  const bool defer = train && !with_head && net.defer_ok;
  std::vector<FwdStep> plan;
  if ((rc = plan_forward(net, N, train != 0, with_head, first_op, defer, plan))) return rc;
  const int n_ops = first_op + (int)plan.size();
  auto ptr = [&](const View& v) { return view_ptr(net, slot, MB, v); };
  auto tab = [&](const View& v) {
    ChanTab t = view_tab(net, ts, v);
    if (defer && defer_tab_runs(net, v, N, t)) {     // the view holds a channel whose table is deferred in this pass
      const int off = net.tab_off[v.buf] + v.coff;
      t.dsrc = net.td_src + off; t.dhw = net.td_hw + off; t.dgoff = net.td_goff + off; t.dboff = net.td_boff + off;
      t.dparams = ctx->params; t.dstats = stats; t.drep_stride = rep_stride; t.dN = N; t.dmax = JN_DEFER_MAX_M;
    }
    return t;
  };
  auto ld = [&](const View& v) { return net.bufs[v.buf].C; };
  auto finalize = [&](const Op& op, const ConvW& cw, bool deferred) {
    if (!train || !cw.has_bn || deferred || replay) return 0;      // (a replay reads the table the pass left)
    ChanTab t1{nullptr, nullptr, nullptr};
    if (op.alias.buf >= 0) t1 = tab(op.alias);
    // with the end-of-pass finalize (defer): table only here, saved / running statistics there
    return launch_bn_finalize(stats + 2 * cw.stat_off, rep_stride, (double)N * op.out.H * op.out.W, cw.gamma_dev, cw.beta_dev,
                       defer ? nullptr : cw.rmean_dev, defer ? nullptr : cw.rvar_dev, defer ? nullptr : save + 2 * cw.stat_off,
                       tab(op.out), t1, cw.cout, kBnEps, kBnMomentum, skip_flag, skip_when, s);
  };
  static const bool layer_profile = std::getenv("JN_LAYER_PROFILE") != nullptr;
  OpProfile prof(layer_profile, n_ops + 1, s);
  prof.mark(first_op);
  std::vector<char> up_done(n_ops, 0);      // upsample ops whose copy the producing 1x1 kernel wrote
  for (int oi = first_op; oi < n_ops; ++oi) {
    const Op& op = net.ops[oi];
    const FwdStep& st = plan[oi - first_op];
    int lrc = 0;      // of the op's launchers: non-zero ends the pass
    switch (st.route) {
      case FR_STEM: {
        const ConvW& cw = net.convs[op.wslot];
        StemArgs a = stem_args(ss, net, N, cw);
        a.out = ptr(op.out); a.out_ld = ld(op.out); a.out_dtype = net.act_dtype; a.skip_flag = skip_flag; a.skip_when = skip_when;
        a.stats = train ? acc + 2 * cw.stat_off : nullptr; a.stats_rep_stride = rep_stride;
        a.stats_nrep = st.deferred ? JN_NREP_DEFER : JN_NREP;
        if (!(lrc = launch_stem(a, s))) lrc = finalize(op, cw, st.deferred);
        break;
      }
      case FR_DWPW:
      case FR_DWPW_ADD: {
        const Op& nx = net.ops[st.link];
        DwPwArgs f{};
        f.in = ptr(op.in); f.in_ld = ld(op.in); f.itab = tab(op.in); f.w_dw = net.convs[op.wslot].w_dev; f.mtab = tab(op.out);
        f.w_pw = net.convs[nx.wslot].w_dev; f.out = ptr(nx.out); f.out_ld = ld(nx.out); f.dtype = net.act_dtype;
        f.C = op.out.C; f.cout = nx.out.C; f.N = N; f.H = op.in.H; f.W = op.in.W; f.OH = op.out.H; f.OW = op.out.W;
        f.stride = op.stride; f.skip_flag = skip_flag; f.skip_when = skip_when;
        if (st.route == FR_DWPW_ADD) {
          const Op& ad = net.ops[st.add];
          f.res = ptr(ad.res); f.res_ld = ld(ad.res); f.rtab = tab(ad.res); f.ptab = tab(nx.out);
          f.out = ptr(ad.out); f.out_ld = ld(ad.out);
        }
        lrc = launch_dwpw(f, s);
        break;
      }
      case FR_CONV: {
        const ConvW& cw = net.convs[op.wslot];
        ConvArgs a{};
        a.in = ptr(op.in); a.in_ld = ld(op.in); a.in_dtype = net.act_dtype; a.itab = tab(op.in); a.w = cw.w_dev;
        a.w_bf16 = cw.w_bf16;
        if (x3 && op.kind == OP_PW && (cw.w_dev - ctx->params) % 8 == 0) a.w_x3 = ctx->params_x3 + 3 * (cw.w_dev - ctx->params);
        a.bias = cw.b_dev; a.out = ptr(op.out); a.out_ld = ld(op.out); a.out_dtype = net.act_dtype;
        a.bf16_mfma = net.act_dtype == JN_BF16;
        a.N = N; a.H = op.in.H; a.W = op.in.W; a.OH = op.out.H; a.OW = op.out.W;
        a.cin = op.in.C; a.cout = op.out.C; a.stride = op.stride; a.act = op.act;
        a.stats = (train && cw.has_bn) ? acc + 2 * cw.stat_off : nullptr;
        a.stats_rep_stride = rep_stride;
        a.stats_nrep = st.deferred ? JN_NREP_DEFER : JN_NREP;
        a.skip_flag = skip_flag; a.skip_when = skip_when;
        if (st.link >= 0 && pw_fuses_upsample(pw_route(a), a.cin, a.cout)) {      // the planned candidate, where this launch's route can
          const Op& up = net.ops[st.link];
          a.up_out = ptr(up.out); a.up_ld = ld(up.out); up_done[st.link] = 1;
        }
        lrc = op.kind == OP_PW ? launch_pw(a, s) : op.kind == OP_DW ? launch_dw(a, s) : launch_conv3(a, s, 0);
        if (!lrc) lrc = finalize(op, cw, st.deferred);
        break;
      }
      case FR_SPP:
        lrc = launch_spp(view_ptr(net, slot, MB, net_full_view(net, op.out.buf)), net.act_dtype, ld(op.out), op.in.C, op.in.H, op.in.W, N,
                   tab(op.in), skip_flag, skip_when, s);
        break;
      case FR_UPSAMPLE:
        if (!up_done[oi])
          lrc = launch_upsample(ptr(op.in), ld(op.in), ptr(op.out), ld(op.out), net.act_dtype, op.in.C, op.in.H, op.in.W, N, skip_flag,
                          skip_when, s);
        break;
      case FR_ADDACT:
        lrc = launch_addact(ptr(op.in), ld(op.in), tab(op.in), ptr(op.res), ld(op.res), tab(op.res), ptr(op.out), ld(op.out),
                      net.act_dtype, op.out.C, (long long)N * op.out.H * op.out.W, skip_flag, skip_when, s);
        break;
      case FR_PRED:
        lrc = launch_head_pred(ptr(op.in), ld(op.in), tab(op.in), ptr(op.res), ld(op.res), tab(op.res), net.act_dtype, net.pred_w[op.level],
                         net.pred_b[op.level], train ? ctx->det_logits : ctx->det_raw, net.head_hid, op.in.H, op.in.W, op.stride,
                         net.n_anchors, op.anchor0, N, s, train ? 1 : 0);
        break;
      case FR_ABSORBED: case FR_NONE: break;   // covered by the kernel of op st.link
    }
    JN_CHECK(lrc == 0, JN_ESTATE, "forward of %s: no kernel for this shape, or its LDS was refused", op.name.c_str());
    prof.mark(oi + 1);
  }
  if (prof) {
    (void)hipStreamSynchronize(s);
    const double esz = (double)act_esz(net);
    fprintf(stderr, "# layer profile: net %d, N=%d, train=%d, slot=%d\n", ni, N, train, slot);
    for (int oi = first_op; oi < n_ops; ++oi) {
      const Op& op = net.ops[oi];
      const double in_e = op.kind == OP_STEM ? 3.0 * net.P * net.P * 4.0 / esz : (double)op.in.H * op.in.W * op.in.C;
      const double out_e = (double)op.out.H * op.out.W * op.out.C;
      double elems = in_e + out_e;
      if (op.kind == OP_ADDACT) elems += out_e;
      if (op.kind == OP_SPP) elems = in_e * 4;
      prof.row(op, oi, oi + 1, elems * esz * N, false);
    }
    prof.total();
  }
  if (defer && !replay) {
    BnAllArgs fa{};
    fa.stats = stats; fa.rep_stride = rep_stride; fa.n_stat = net.stat_channels; fa.N = N; fa.hw = net.fd_hw;
    fa.goff = net.fd_goff; fa.boff = net.fd_boff; fa.params = ctx->params; fa.t0 = net.fd_t0; fa.t1 = net.fd_t1;
    fa.tab = net.tab + (size_t)ts * 3 * net.tab_channels; fa.tab_channels = net.tab_channels; fa.save = save;
    fa.run_mean = net.fd_rm; fa.run_var = net.fd_rv; fa.eps = kBnEps; fa.momentum = kBnMomentum;
    fa.skip_flag = skip_flag; fa.skip_when = skip_when; fa.defer_max_m = JN_DEFER_MAX_M;
    JN_CHECK(launch_bn_finalize_all(fa, s) == 0, JN_ESTATE, "forward: the end-of-pass BatchNorm finalize was not launched");
  }
  JN_HIP(hipGetLastError());
  if (train && !replay) net.eval_tab_dirty = true;     // running statistics moved
  return JN_OK;
}

// ---- training state --------------------------------------------------------------------
int ensure_train_state(jn_ctx* ctx, int g_slots) {
  int rc;
  if (!ctx->grads) {
    if ((rc = dev_alloc(ctx, &ctx->grads, ctx->arena_size))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->adam_m, ctx->arena_size))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->adam_v, ctx->arena_size))) return rc;
    JN_HIP(hipMemset(ctx->grads, 0, ctx->arena_size * sizeof(float)));
    JN_HIP(hipMemset(ctx->adam_m, 0, ctx->arena_size * sizeof(float)));
    JN_HIP(hipMemset(ctx->adam_v, 0, ctx->arena_size * sizeof(float)));
    std::vector<float> id(3 * 2048, 0.0f);
    for (int i = 0; i < 2048; ++i) id[i] = 1.0f;
    if ((rc = dev_upload(ctx, &ctx->ident, id))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->wpart, (size_t)JN_NREP * JN_WPART_MAX))) return rc;
    JN_HIP(hipMemset(ctx->wpart, 0, (size_t)JN_NREP * JN_WPART_MAX * sizeof(float)));
  }
  for (int ni = 0; ni < 2; ++ni) {
    if (!ctx->has_net[ni]) continue;
    Net& net = ctx->nets[ni];
    const int want = ni == ctx->enc_net ? g_slots : 1;
    if (net.g_slots >= want) continue;
    // (a smaller earlier allocation stays owned by the context until jn_destroy)
    if ((rc = dev_alloc(ctx, &net.gact, (size_t)want * net.per_image_floats * ctx->cfg.max_batch))) return rc;
    if ((rc = dev_alloc(ctx, &net.bred, (size_t)want * JN_NREP * 2 * net.stat_channels))) return rc;
    if ((rc = dev_alloc(ctx, &net.bconsts, (size_t)want * 3 * net.stat_channels))) return rc;
    net.g_slots = want;
  }
  return JN_OK;
}

// The context's second stream (non-blocking) with its fork / join events: independent kernel families run beside the
// caller's stream — weight-gradient GEMMs in the backward, the detector beside the next glimpse step in a rollout.
int ensure_aux_stream(jn_ctx* ctx) {
  if (ctx->aux_stream) return JN_OK;
  JN_HIP(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
  JN_HIP(hipEventCreateWithFlags(&ctx->aux_fork, hipEventDisableTiming));
  JN_HIP(hipEventCreateWithFlags(&ctx->aux_join, hipEventDisableTiming));
  return JN_OK;
}

// Backward of `nsl` train-mode PAFPN passes (workspace slots slot .. slot + nsl - 1, N patches each; gradient
// slots 0 .. nsl - 1): every kernel is launched ONCE for all the passes (SlotBatch), so a 20-step trajectory
// costs the launches of one pass.  g[fpn views] must hold the incoming gradients; parameter gradients are
// accumulated into ctx->grads.  ss.positions belongs to the first pass, pos_slot_stride int64s separate passes.
// fpn_zero: bit i set = NO gradient arrives in net.fpn[i] from outside the network (the REINFORCE / supervised backward
// only feeds fpn[2]).  The routes come from plan_backward (plan.cpp); what depends on launch-time state stays here.
int run_net_backward(jn_ctx* ctx, int ni, int N, const StemSrc& ss, int slot, hipStream_t s, int nsl, long long pos_slot_stride,
                     bool with_head, int fpn_zero, int tab_slot) {
  Net& net = ctx->nets[ni];
  const int ts = tab_slot < 0 ? slot : tab_slot;      // activations from slot `slot` on, tables / saved statistics from table slot ts on
  const int MB = ctx->cfg.max_batch;
  // THE refusal of the backward: every kernel below reads fp32 activations
  JN_CHECK(net.act_dtype == JN_F32, JN_ESTATE, "training needs act_dtype = fp32 (bf16 is the inference mode)");
  JN_CHECK(nsl >= 1 && nsl <= net.g_slots && slot >= 0 && slot + nsl <= net.a_slots && ts >= 0 && ts + nsl <= net.n_slots, JN_ESTATE,
           "backward over %d slots from %d (tables from %d): not allocated", nsl, slot, ts);
  std::vector<BwdStep> plan;
  int rc = plan_backward(net, with_head, fpn_zero, plan);
  if (rc) return rc;
  JN_HIP(hipMemsetAsync(net.bred, 0, (size_t)nsl * JN_NREP * 2 * net.stat_channels * sizeof(double), s));
  const long long rep_stride = 2LL * net.stat_channels;
  SlotBatch sb;
  sb.n = nsl;
  sb.act = (long long)net.per_image_floats * MB;
  sb.grad = (long long)net.per_image_floats * MB;
  sb.tab = 3LL * net.tab_channels;
  sb.save = 2LL * net.stat_channels;
  sb.red = (long long)JN_NREP * 2 * net.stat_channels;
  sb.consts = 3LL * net.stat_channels;
  sb.pos = pos_slot_stride;
  float* save = slot_save(net, ts);
  auto ptr = [&](const View& v) { return (const float*)view_ptr(net, slot, MB, v); };
  auto gptr = [&](const View& v) { return net.gact + net.buf_off[v.buf] * (size_t)MB + v.coff; };
  auto tab = [&](const View& v) { return view_tab(net, ts, v); };
  auto ld = [&](const View& v) { return net.bufs[v.buf].C; };
  auto sums = [&](int p, int half) {      // BN-backward sums of op p (half -1: the whole conv)
    const ConvW& pcw = net.convs[net.ops[p].wslot];
    return net.bred + 2 * (pcw.stat_off + (half > 0 ? pcw.cout / 2 : 0));
  };
  const ChanTab ident{ctx->ident, ctx->ident + 2048, ctx->ident + 4096};
  static const bool no_aux = std::getenv("JN_NO_AUX_STREAM") != nullptr;
  static const bool dbg_plan = std::getenv("JN_DBG_BWD_PLAN") != nullptr;
  bool aux_used = false;
  if (!no_aux) { int ra = ensure_aux_stream(ctx); if (ra) return ra; }
  // A weight-gradient GEMM with plain atomics on gw (no shared scratch) only feeds the optimiser: it runs on the second
  // stream, behind what `s` holds so far (g_z is complete), beside the data gradient of the same layer and whatever
  // follows; joined before this function returns.  ws: the stream to launch it on.
  auto fork_aux = [&](hipStream_t& ws) -> int {
    ws = s;
    if (no_aux) return JN_OK;
    JN_HIP(hipEventRecord(ctx->aux_fork, s));
    JN_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->aux_fork, 0));
    ws = ctx->aux_stream;
    aux_used = true;
    return JN_OK;
  };
  // a conv op: its gradient view (d loss / d activation; g_z once bn_gz ran), pixels, per-channel constants, weight gradient
  struct ConvB { const Op& op; const BwdStep& st; const ConvW& cw; float* g; int g_ld; long long M; float* consts; float* gw; };
  // BatchNorm sums and constants of the conv, whole or — a merged pair with a half reduced by its consumer — per half: a
  // part no consumer reduced gets its own pass, and consumer-made sums carry the moment against y (bn_bwd_consts)
  auto bn_sums_consts = [&](const ConvB& c) -> int {
    const ConvW& cw = c.cw;
    const int parts = c.st.red_by && !cw.prefix2.empty() ? 2 : 1, h = cw.cout / parts;
    double* red = net.bred + 2 * cw.stat_off;
    if (dbg_plan) {
      // elements per patch that a separate bn_bwd_reduce pass re-reads (g and z: 8 bytes each); merged pairs per half
      const int hm = c.st.red_by;
      const long long sep = parts == 2 ? (c.M / N) * h * (2 - ((hm & 1) + ((hm >> 1) & 1))) : hm ? 0 : (c.M / N) * cw.cout;
      std::fprintf(stderr, "[bwd-plan] %-34s kind %d cout %4d cin %4d M/patch %6lld stride %d acc_in %d separate-reduce elements/patch %8lld%s\n",
                   c.op.name.c_str(), (int)c.op.kind, cw.cout, cw.cin, c.M / N, c.op.stride, (int)c.op.acc_in, sep,
                   parts == 2 ? (hm == 3 ? " (both halves by their consumers)" : " (one half by its consumer)") : "");
    }
    for (int part = 0; part < parts; ++part) {
      const int c0 = part * h, by_consumer = (c.st.red_by >> part) & 1;
      float* sv = save + 2 * (cw.stat_off + c0);
      JN_CHECK(by_consumer || launch_bn_bwd_reduce(c.g + c0, c.g_ld, ptr(c.op.out) + c0, ld(c.op.out), tab_at(tab(c.op.out), c0), sv, h, c.M,
                                                   red + 2 * c0, rep_stride, s, sb) == 0,
               JN_ESTATE, "launch_bn_bwd_reduce: %s has %d channels (whole quads, at most %d)", c.op.name.c_str(), h, JN_BN_BWD_MAX_C);
      JN_CHECK(launch_bn_bwd_consts(red + 2 * c0, rep_stride, (double)c.M, cw.gamma_dev + c0, cw.beta_dev + c0, sv, c.consts + 3 * c0,
                                    grad_of(ctx, cw.gamma_dev) + c0, grad_of(ctx, cw.beta_dev) + c0, h, s, sb, by_consumer) == 0,
               JN_ESTATE, "launch_bn_bwd_consts: %s was refused", c.op.name.c_str());
    }
    return JN_OK;
  };
  // the data gradient of a stride-1 conv as its forward kernel over g_z with the transposed weight, all slots in one launch
  auto gz_conv_args = [&](const ConvB& c) {
    ConvArgs a{};
    a.in = c.g; a.in_ld = c.g_ld; a.in_dtype = JN_F32; a.itab = ident; a.w = c.cw.w_dev;
    a.out = gptr(c.op.in); a.out_ld = ld(c.op.in); a.out_dtype = JN_F32;
    a.N = N; a.H = c.op.out.H; a.W = c.op.out.W; a.OH = c.op.in.H; a.OW = c.op.in.W;
    a.cin = c.cw.cout; a.cout = c.cw.cin; a.stride = 1; a.act = ACT_NONE;
    a.accumulate = c.op.acc_in ? 1 : 0; a.w_transposed = 1; a.in_identity = 1;
    a.n_slots = nsl; a.in_slot_stride = sb.grad; a.out_slot_stride = sb.grad;
    return a;
  };
  auto bn_gz = [&](const ConvB& c) {      // g_a -> g_z in place (the unfused routes)
    launch_bn_bwd_gz(c.g, c.g_ld, ptr(c.op.out), ld(c.op.out), tab(c.op.out), save + 2 * c.cw.stat_off, c.consts, c.cw.cout, c.M,
                     s, sb);
  };
  const int n_ops_b = (int)plan.size();
  // JN_BWD_PROFILE=1: HIP events around the launches of every op, table on stderr (a measuring aid; use it together with
  // JN_NO_AUX_STREAM=1 so that the wide weight-gradient GEMMs are inside the brackets)
  static const bool bwd_profile = std::getenv("JN_BWD_PROFILE") != nullptr;
  OpProfile prof(bwd_profile, n_ops_b + 1, s);
  prof.mark(n_ops_b);
  for (int obi = n_ops_b - 1; obi >= 0; --obi) {
    const Op& op = net.ops[obi];
    const BwdStep& st = plan[obi];
    const long long M = (long long)N * op.out.H * op.out.W;
    if (op.wslot < 0) {
      switch (st.route) {
        case BR_ADDACT_COPY: case BR_ADDACT_FOLD:
          // (without acc_in the conv that feeds the add reads g[sum] in place, BwdStep::g; folded: that conv's kernel adds it)
          JN_CHECK(!op.acc_in || launch_grad_copy(gptr(op.out), ld(op.out), gptr(op.in), ld(op.in), op.out.C, M, 1, s, sb) == 0, JN_ESTATE,
                   "launch_grad_copy: %s was refused", op.name.c_str());
          JN_CHECK(st.route != BR_ADDACT_COPY ||
                       launch_grad_copy(gptr(op.out), ld(op.out), gptr(op.res), ld(op.res), op.out.C, M, op.acc_res ? 1 : 0, s, sb) == 0,
                   JN_ESTATE, "launch_grad_copy: %s was refused", op.name.c_str());
          break;
        case BR_SPP: {
          const View full = net_full_view(net, op.out.buf);
          JN_CHECK(launch_spp_bwd(ptr(full), gptr(full), ld(op.out), op.in.C, op.in.H, op.in.W, N, tab(op.in), s, sb) == 0, JN_ESTATE,
                   "launch_spp_bwd: %s was refused (channel block, alignment or LDS)", op.name.c_str());
          break;
        }
        case BR_UPSAMPLE:
          JN_CHECK(launch_upsample_bwd(gptr(op.out), ld(op.out), gptr(op.in), ld(op.in), op.in.C, op.in.H, op.in.W, N, op.acc_in ? 1 : 0, s, sb) == 0,
                   JN_ESTATE, "launch_upsample_bwd: %s was refused", op.name.c_str());
          break;
        default: break;      // nothing to differentiate here (the head's predictors: api_det.hip)
      }
      prof.mark(obi);
      continue;
    }
    const ConvW& cw = net.convs[op.wslot];
    const ConvB c{op, st, cw, gptr(st.g), ld(st.g), M, net.bconsts + 3 * cw.stat_off, grad_of(ctx, cw.w_dev)};
    hipStream_t ws = s;      // of a weight-gradient kernel that may run beside the rest (fork_aux)
    if ((rc = bn_sums_consts(c))) return rc;
    switch (st.route) {
      case BR_PW_FUSED: case BR_PW_FUSED_HALVES: {      // one launch, or one per half of the output channels
        const int parts = st.route == BR_PW_FUSED ? 1 : 2, pc = cw.cout / parts;
        for (int part = 0; part < parts; ++part) {
          const int c0 = part * pc;
          PwBwdFusedArgs fa{};
          fa.g = c.g + c0; fa.g_ld = c.g_ld; fa.z = ptr(op.out) + c0; fa.z_ld = ld(op.out); fa.ot = tab_at(tab(op.out), c0);
          fa.save = save + 2 * (cw.stat_off + c0); fa.consts = c.consts + 3 * c0;
          fa.x = ptr(op.in); fa.x_ld = ld(op.in); fa.it = tab(op.in); fa.w = cw.w_dev + (size_t)c0 * cw.cin;
          fa.gx = gptr(op.in); fa.gx_ld = ld(op.in); fa.accumulate = (op.acc_in || part > 0) ? 1 : 0;
          fa.gw = c.gw + (size_t)c0 * cw.cin; fa.wpart = ctx->wpart; fa.M = M; fa.cout = pc; fa.cin = cw.cin; fa.sb = sb;
          if (st.fold >= 0) {                   // the shortcut add's backward left its copy to this kernel
            const View& sum = net.ops[st.fold].out;
            fa.gadd = gptr(sum); fa.gadd_ld = ld(sum); fa.accumulate = 0;
          }
          if (st.red_in >= 0 || st.red_in2 >= 0) fa.red_rep_stride = rep_stride;
          if (st.red_in >= 0) fa.red_in = sums(st.red_in, st.red_half);
          if (st.red_in2 >= 0) fa.red_in2 = sums(st.red_in2, st.red_half2);
          fa.red_split = st.red_split;
          if (st.red2) {                        // the sums of the conv behind the shortcut sum: its raw output and table
            const Op& co = net.ops[st.red_in];
            const ChanTab zt = tab(co.out);
            fa.red2_z = ptr(co.out); fa.red2_ld = ld(co.out); fa.red2_sc = zt.sc; fa.red2_sh = zt.sh;
          }
          // 128 input channels: the transposed weight in fragment order goes into the layer's own stretch of the wide
          // route's scratch (6 bytes per weight, unused by a fused layer; 16-byte aligned under the same condition)
          if (ctx->params_x3t && cw.cin == 128 && (pc == 128 || pc == 64) && (fa.w - ctx->params) % 8 == 0)
            fa.w_frag = reinterpret_cast<float*>(ctx->params_x3t + 3 * (fa.w - ctx->params));
          JN_CHECK(launch_pw_bwd_fused(fa, s) == 0, JN_ESTATE, "launch_pw_bwd_fused: %s has no kernel, or its LDS was refused", op.name.c_str());
        }
        break;
      }
      case BR_DW_FUSED: {
        // stride 2 (round 4): the owner-staged variant of the kernel (every thread stages the 2 x 2 input block it
        // differentiates and keeps the raw values); round 3's variant re-read the input inside the gradient loop and lost
        // more than the separate pass costs
        DwBwdFusedArgs fa{};
        fa.g = c.g; fa.g_ld = c.g_ld; fa.z = ptr(op.out); fa.z_ld = ld(op.out); fa.ot = tab(op.out);
        fa.save = save + 2 * cw.stat_off; fa.consts = c.consts;
        fa.x = ptr(op.in); fa.x_ld = ld(op.in); fa.it = tab(op.in); fa.w = cw.w_dev;
        fa.gin = gptr(op.in); fa.gin_ld = ld(op.in); fa.accumulate = op.acc_in ? 1 : 0; fa.gw = c.gw; fa.wpart = ctx->wpart;
        fa.C = cw.cout; fa.H = op.in.H; fa.W = op.in.W; fa.OH = op.out.H; fa.OW = op.out.W; fa.N = N; fa.stride = op.stride;
        fa.sb = sb;
        if (st.red_in >= 0) {
          fa.red_in = sums(st.red_in, st.red_half); fa.red_rep_stride = rep_stride;
          fa.accumulate = 0;                      // sole reader: nothing but the (zero) outside seed was there before
        }
        JN_CHECK(launch_dw_bwd_fused(fa, s) == 0, JN_ESTATE, "launch_dw_bwd_fused: %s has no kernel", op.name.c_str());
        break;
      }
      case BR_STEM_FUSED:      // bn_bwd_gz inside: no pass over the largest map of the network
        JN_CHECK(launch_stem_bwd_weight(stem_args(ss, net, N, cw), c.g, c.g_ld, c.gw, ctx->wpart, s, sb, ptr(op.out), ld(op.out), tab(op.out),
                                        save + 2 * cw.stat_off, c.consts) == 0,
                 JN_ESTATE, "launch_stem_bwd_weight: %s was refused (patch size %d, %d output channels)", op.name.c_str(), net.P, cw.cout);
        break;
      case BR_PW: {
        bn_gz(c);
        const ConvArgs a = gz_conv_args(c);
        if (cw.cout >= 128 && cw.cin >= 128 && (rc = fork_aux(ws))) return rc;      // the wide weight-gradient kernel
        // wide layers: the data gradient on the bf16 pipe at fp32 accuracy (pw_x3_kernel over the slots, transposed weight
        // split on the way: kernels_pwxs.hip); JN_NO_PW_X3_BWD=1 keeps pw_dir_kernel<WT> on the fp32 pipe
        const bool x3 = !std::getenv("JN_NO_PW_X3_BWD") && !op.acc_in && ctx->params_x3t &&      // read per launch: a test flips it
                        pw_x3_bwd_data_supported(cw.cout, cw.cin) && (cw.w_dev - ctx->params) % 8 == 0;
        if (!x3 || launch_pw_x3_bwd_data(a, cw.w_dev, ctx->params_x3t + 3 * (cw.w_dev - ctx->params), s) != 0)
          JN_CHECK(launch_pw(a, s) == 0, JN_ESTATE, "data gradient of %s: no kernel for this shape, or its LDS was refused", op.name.c_str());
        JN_CHECK(launch_pw_bwd_weight(c.g, c.g_ld, ptr(op.in), ld(op.in), tab(op.in), c.gw, ctx->wpart, M, cw.cout, cw.cin, ws, sb) == 0,
                 JN_ESTATE, "launch_pw_bwd_weight: %s has no kernel, or its LDS was refused", op.name.c_str());
        break;
      }
      case BR_DW:
        bn_gz(c);
        launch_dw_bwd_data(c.g, c.g_ld, cw.w_dev, gptr(op.in), ld(op.in), cw.cout, op.in.H, op.in.W, op.out.H, op.out.W, N, op.stride,
                           op.acc_in ? 1 : 0, s, sb);
        launch_dw_bwd_weight(c.g, c.g_ld, ptr(op.in), ld(op.in), tab(op.in), c.gw, ctx->wpart, cw.cout, op.in.H, op.in.W, op.out.H,
                             op.out.W, N, op.stride, s, sb);
        break;
      case BR_CONV3_S1: case BR_CONV3_S2: {
        // dense 3x3 (non-depthwise patch encoders, e.g. yolox-s): stride 1 = the forward kernel over g_z with mirrored
        // taps and the transposed weight; stride 2 = one MFMA tile loop per input-pixel parity class
        bn_gz(c);
        if ((rc = fork_aux(ws))) return rc;      // the 9-tap weight gradient beside the data gradient
        const int rc3 = st.route == BR_CONV3_S1
                            ? launch_conv3(gz_conv_args(c), s, 0)
                            : launch_conv3_bwd_data_s2(c.g, c.g_ld, cw.w_dev, gptr(op.in), ld(op.in), op.in.H, op.in.W, op.out.H,
                                                       op.out.W, cw.cout, cw.cin, N, op.acc_in ? 1 : 0, s, sb, 0);
        JN_CHECK(rc3 == 0, JN_ESTATE, "backward of dense 3x3 conv %s: unsupported shape", op.name.c_str());
        JN_CHECK(launch_conv3_bwd_weight(c.g, c.g_ld, ptr(op.in), ld(op.in), tab(op.in), c.gw, op.in.H, op.in.W, op.out.H, op.out.W,
                                         cw.cout, cw.cin, N, op.stride, ws, sb, 0, 0) == 0,
                 JN_ESTATE, "launch_conv3_bwd_weight: the LDS of %s was refused", op.name.c_str());
        break;
      }
      default: JN_CHECK(false, JN_ESTATE, "backward plan: conv %s has route %d", op.name.c_str(), (int)st.route);
    }
    prof.mark(obi);
  }
  if (aux_used) {
    JN_HIP(hipEventRecord(ctx->aux_join, ctx->aux_stream));
    JN_HIP(hipStreamWaitEvent(s, ctx->aux_join, 0));
  }
  if (prof) {
    (void)hipStreamSynchronize(s);
    fprintf(stderr, "# backward profile: net %d, N=%d patches x %d steps; bytes = g_out + z_out + x read, g_in written (+ read when accumulated)\n", ni, N, nsl);
    for (int obi = n_ops_b - 1; obi >= 0; --obi) {
      const Op& op = net.ops[obi];
      const double in_e = op.kind == OP_STEM ? 0.0 : (double)op.in.H * op.in.W * op.in.C, out_e = (double)op.out.H * op.out.W * op.out.C;
      double elems;
      if (op.wslot >= 0) elems = 2.0 * out_e + (op.kind == OP_STEM ? 3.0 * net.P * net.P : 2.0 * in_e + (op.acc_in ? in_e : 0.0));
      else if (op.kind == OP_ADDACT) elems = 3.0 * out_e;                 // g read, two destinations
      else if (op.kind == OP_SPP) elems = 8.0 * in_e;
      else elems = in_e + out_e;
      prof.row(op, obi + 1, obi, elems * 4.0 * N * nsl, true);
    }
    prof.total();
  }
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// embed_fpn (src/models/gpt.py:294-306, 382) on the last FPN map of the encoder for N patches:
// 1x1 conv + ReLU, then the split-K partial sums of the Linear (finished by the consumer).
int run_embed_fpn(jn_ctx* ctx, int N, int slot, float* e_buf, const int* skip_flag, int skip_when, hipStream_t s, int tab_slot) {
  if (!e_buf) e_buf = ctx->efpn_act;
  const Net& net = ctx->nets[ctx->enc_net];
  jn_ctx& x = *ctx;
  const int C = ctx->cfg.n_embd, MB = ctx->cfg.max_batch;
  const View& f = net.fpn[2];
  ConvArgs a{};
  a.in = view_ptr(net, slot, MB, f); a.in_ld = net.bufs[f.buf].C; a.in_dtype = net.act_dtype; a.itab = view_tab(net, tab_slot < 0 ? slot : tab_slot, f);
  a.out_dtype = JN_F32; a.bf16_mfma = net.act_dtype == JN_BF16;
  a.w = ctx->gpt.efpn_w; a.bias = nullptr; a.out = e_buf; a.out_ld = C;
  a.N = N; a.H = f.H; a.W = f.W; a.OH = f.H; a.OW = f.W; a.cin = f.C; a.cout = C; a.stride = 1; a.act = ACT_RELU;
  a.skip_flag = skip_flag; a.skip_when = skip_when;
  JN_CHECK(launch_pw(a, s) == 0, JN_ESTATE, "embed_fpn.0: no kernel for this shape, or its LDS was refused");
  JN_CHECK(launch_efpn_linear(e_buf, ctx->gpt.efpn_lin_wt, x.emb_part, N, f.H * f.W * C, C, x.KS, skip_flag, skip_when, s) == 0, JN_ESTATE,
           "embed_fpn.3: no kernel for %d outputs", C);
  JN_HIP(hipGetLastError());
  return JN_OK;
}

// Words of activation slot slot_a that differ from slot_b, over the first N patches of every buffer of the net (a debug
// aid of the replay mode: waits for the stream).
int replay_slot_diff(jn_ctx* ctx, Net& net, int slot_a, int slot_b, int N, long long* n_diff, hipStream_t s) {
  const int MB = ctx->cfg.max_batch;
  JN_CHECK(slot_a >= 0 && slot_b >= 0 && slot_a < net.a_slots && slot_b < net.a_slots && N >= 1 && N <= MB, JN_ESTATE,
           "compare of activation slots %d and %d over %d patches: not allocated", slot_a, slot_b, N);
  JN_CHECK(net.act_dtype == JN_F32, JN_ESTATE, "the slot compare reads fp32 activations");
  unsigned long long* total = nullptr;
  JN_HIP(hipMalloc((void**)&total, sizeof(unsigned long long)));
  hipError_t e = hipMemsetAsync(total, 0, sizeof(unsigned long long), s);
  for (size_t b = 0; b < net.bufs.size() && e == hipSuccess; ++b) {
    View v; v.buf = (int)b; v.coff = 0;
    const long long n = (long long)N * (long long)net.bufs[b].per_image();
    if (n == 0) continue;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(word_diff_kernel, dim3(grid), dim3(256), 0, s, (const uint32_t*)view_ptr(net, slot_a, MB, v),
                       (const uint32_t*)view_ptr(net, slot_b, MB, v), n, total);
  }
  unsigned long long host = 0;
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&host, total, sizeof(host), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(total);
  JN_HIP(e);
  *n_diff = (long long)host;
  return JN_OK;
}

// Patches to token embeddings in the eval / supervised workspace (slot 0): the encoder over the N patches of ss, embed_fpn
// (e_buf: where embed_fpn.0's activations go, null = ctx->efpn_act), then the split-K sums finished into
// out[n * out_stride + c].
int embed_tokens(jn_ctx* ctx, const StemSrc& ss, int N, int train, float* e_buf, float* out, long long out_stride,
                 hipStream_t s) {
  int rc;
  if ((rc = run_net(ctx, ctx->enc_net, N, ss, 0, train, nullptr, 0, s))) return rc;
  if ((rc = run_embed_fpn(ctx, N, 0, e_buf, nullptr, 0, s))) return rc;
  const int C = ctx->cfg.n_embd;
  hipLaunchKernelGGL(emb_finish_kernel, dim3((N * C + 255) / 256), dim3(256), 0, s, ctx->emb_part, ctx->gpt.efpn_lin_b, out,
                     out_stride, N, ctx->KS, C);
  return JN_OK;
}

// the argument checks of the entry points that run one pass of `net` over N caller-given patches
static int check_net_batch(const jn_ctx* ctx, int net, int N) {
  JN_CHECK(net >= 0 && net < 2 && ctx->has_net[net], JN_EINVAL, "network %d is not part of this context", net);
  JN_CHECK(ctx->weights_loaded, JN_ESTATE, "jn_load_weights has not been called");
  JN_CHECK(N >= 1 && N <= ctx->cfg.max_batch, JN_EINVAL, "N=%d exceeds max_batch=%d", N, ctx->cfg.max_batch);
  return JN_OK;
}

}  // namespace jnr

extern "C" {

// The forward plan of one pass as run_net would form it (plan.cpp: plan_forward; needs no device): (route, link,
// deferred) of each op from first_op on, at most `cap` triples.  Returns the number of ops of the pass, or an error.
int jn_debug_forward_plan(const jn_ctx* ctx, int net, int N, int train, int with_head, int first_op, int32_t* out, int cap) {
  JN_CHECK(ctx && net >= 0 && net < 2 && ctx->has_net[net] && (out || cap <= 0), JN_EINVAL, "jn_debug_forward_plan: bad argument");
  const Net& n = ctx->nets[net];
  std::vector<FwdStep> plan;
  const int rc = plan_forward(n, N, train != 0, with_head != 0, first_op, train && !with_head && defer_eligible(n), plan);
  if (rc) return rc;
  for (int i = 0; i < (int)plan.size() && i < cap; ++i) {
    out[3 * i] = plan[i].route; out[3 * i + 1] = plan[i].link; out[3 * i + 2] = plan[i].deferred;
  }
  return (int)plan.size();
}

int jn_backbone_forward(jn_ctx* ctx, int net, const float* patches_dev, int N, int train, float* fpn0_dev,
                        float* fpn1_dev, float* fpn2_dev, void* stream) {
  JN_CHECK(ctx && patches_dev, JN_EINVAL, "jn_backbone_forward: null argument");
  int rc = check_net_batch(ctx, net, N);
  if (rc) return rc;
  JN_HIP(hipSetDevice(ctx->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  if ((rc = run_net(ctx, net, N, patch_src(patches_dev, ctx->cfg.patch_size), 0, train ? 1 : 0, nullptr, 0, s))) return rc;
  float* outs[3] = {fpn0_dev, fpn1_dev, fpn2_dev};
  const Net& n = ctx->nets[net];
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    const View& f = n.fpn[i];
    launch_nhwc_to_nchw(view_ptr(n, 0, ctx->cfg.max_batch, f), n.act_dtype, n.bufs[f.buf].C, view_tab(n, 0, f), outs[i], f.C,
                        f.H * f.W, N, s);
  }
  JN_HIP(hipGetLastError());
  return JN_OK;
}

int jn_backbone_backward(jn_ctx* ctx, int net, const float* patches_dev, int N, const float* g0_dev,
                         const float* g1_dev, const float* g2_dev, void* stream) {
  JN_CHECK(ctx && patches_dev, JN_EINVAL, "jn_backbone_backward: null argument");
  int rc = check_net_batch(ctx, net, N);
  if (rc) return rc;
  Net& n = ctx->nets[net];
  // (run_net_backward's refusal, repeated before the gradient seeds below are launched)
  JN_CHECK(n.act_dtype == JN_F32, JN_ESTATE, "training needs act_dtype = fp32 (bf16 is the inference mode)");
  JN_HIP(hipSetDevice(ctx->cfg.device));
  if ((rc = ensure_train_state(ctx))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int MB = ctx->cfg.max_batch;
  const float* gs[3] = {g0_dev, g1_dev, g2_dev};
  int fpn_zero = 0;                 // bit i: no gradient arrives in fpn[i] from outside (the training backward's routes)
  for (int i = 0; i < 3; ++i) {
    const View& f = n.fpn[i];
    float* gp = n.gact + n.buf_off[f.buf] * (size_t)MB + f.coff;
    if (gs[i]) {
      launch_nchw_to_nhwc_grad(gs[i], gp, n.bufs[f.buf].C, f.C, f.H * f.W, N, 0, s);
    } else {
      JN_CHECK(n.bufs[f.buf].C == f.C, JN_ESTATE, "fpn output is a slice");
      JN_HIP(hipMemsetAsync(gp, 0, (size_t)N * f.H * f.W * f.C * sizeof(float), s));
      fpn_zero |= 1 << i;
    }
  }
  return run_net_backward(ctx, net, N, patch_src(patches_dev, ctx->cfg.patch_size), 0, s, 1, 0, false, fpn_zero);
}

int jn_embed_patches(jn_ctx* ctx, const float* patches_dev, int N, float* out_dev, void* stream) {
  JN_CHECK(ctx && patches_dev && out_dev, JN_EINVAL, "jn_embed_patches: null argument");
  JN_CHECK(!ctx->cfg.no_patch_emb, JN_ESTATE, "context was created with no_patch_emb");
  int rc = check_net_batch(ctx, ctx->enc_net, N);
  if (rc) return rc;
  JN_HIP(hipSetDevice(ctx->cfg.device));
  if ((rc = embed_tokens(ctx, patch_src(patches_dev, ctx->cfg.patch_size), N, 0, nullptr, out_dev, ctx->cfg.n_embd, (hipStream_t)stream)))
    return rc;
  JN_HIP(hipGetLastError());
  return JN_OK;
}

}  // extern "C"
