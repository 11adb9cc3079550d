// Layer plans: turns (depth, width, depthwise, P) into a flat list of conv ops over
// NHWC buffers, plus the state-dict table the weights are loaded by.
//
// Topology restated from the published YOLOX CSPDarknet / YOLOPAFPN / YOLOXHead
// (the package the reference imports at src/models/gpt.py:24, src/models/yolox.py:7-10;
// SURVEY.md §2.1).  Concats are free: producers write into channel slices of the
// consumer's buffer; nearest-x2 upsampling is a copy into a slice.
#include <cmath>
#include <cstring>

#include "jn_internal.h"

namespace jnr {

void add_param(std::vector<ParamEntry>& params, const std::string& name, std::initializer_list<int64_t> shape, int dtype,
               bool buffer, bool used) {
  ParamEntry e; std::memset(&e, 0, sizeof(e));
  std::snprintf(e.info.name, sizeof(e.info.name), "%s", name.c_str());
  e.info.dtype = dtype; e.info.ndim = (int)shape.size();
  int i = 0; for (auto s : shape) e.info.shape[i++] = s;
  e.info.is_buffer = buffer; e.info.used = used;
  params.push_back(e);
}

namespace {

struct Builder {
  Net& net;
  std::vector<ParamEntry>& params;
  std::string mod_prefix;         // state-dict prefix of the part being built ("gpt_backbone.", "yolox.head.")

  int new_buf(int H, int W, int C) {
    Buf b; b.H = H; b.W = W; b.C = C;
    net.bufs.push_back(b);
    return (int)net.bufs.size() - 1;
  }
  View full(int buf) const {
    const Buf& b = net.bufs[buf];
    View v; v.buf = buf; v.H = b.H; v.W = b.W; v.C = b.C; v.coff = 0;
    return v;
  }
  static View slice(View v, int coff, int C) { v.coff += coff; v.C = C; return v; }
  View fresh(int H, int W, int C) { return full(new_buf(H, W, C)); }

  void add_param(const std::string& name, std::initializer_list<int64_t> shape, int dtype, bool buffer, bool used) {
    jnr::add_param(params, name, shape, dtype, buffer, used);
  }

  int add_conv(const std::string& name, int cin, int cout, int k, int groups, bool bn, bool bias) {
    ConvW w; w.prefix = mod_prefix + name; w.cin = cin; w.cout = cout; w.k = k; w.groups = groups;
    w.has_bn = bn; w.has_bias = bias;
    net.convs.push_back(w);
    if (bn) {
      add_param(w.prefix + ".conv.weight", {cout, cin / groups, k, k}, 0, false, true);
      add_param(w.prefix + ".bn.weight", {cout}, 0, false, true);
      add_param(w.prefix + ".bn.bias", {cout}, 0, false, true);
      add_param(w.prefix + ".bn.running_mean", {cout}, 0, true, true);
      add_param(w.prefix + ".bn.running_var", {cout}, 0, true, true);
      add_param(w.prefix + ".bn.num_batches_tracked", {}, 1, true, false);
    } else {
      add_param(w.prefix + ".weight", {cout, cin / groups, k, k}, 0, false, true);
      if (bias) add_param(w.prefix + ".bias", {cout}, 0, false, true);
    }
    return (int)net.convs.size() - 1;
  }

  // conv `a` (first rows) and conv `b` as one 1x1 conv of 2h output channels over the same input
  int add_conv_pair(const std::string& a, const std::string& b, int cin, int h) {
    ConvW w; w.prefix = mod_prefix + a; w.prefix2 = mod_prefix + b; w.cin = cin; w.cout = 2 * h; w.cout_first = h;
    w.k = 1; w.groups = 1; w.has_bn = true; w.has_bias = false;
    net.convs.push_back(w);
    for (const std::string& pre : {w.prefix, w.prefix2}) {
      add_param(pre + ".conv.weight", {h, cin, 1, 1}, 0, false, true);
      add_param(pre + ".bn.weight", {h}, 0, false, true);
      add_param(pre + ".bn.bias", {h}, 0, false, true);
      add_param(pre + ".bn.running_mean", {h}, 0, true, true);
      add_param(pre + ".bn.running_var", {h}, 0, true, true);
      add_param(pre + ".bn.num_batches_tracked", {}, 1, true, false);
    }
    return (int)net.convs.size() - 1;
  }

  static int out_dim(int x, int s) { return (x + 2 - 3) / s + 1; }   // 3x3, pad 1

  // BaseConv(cin, cout, k, s, groups): conv + BN + SiLU.
  View base_conv(const std::string& name, View in, int cout, int k, int s, bool dw,
                 const View* dst = nullptr, const View* res = nullptr) {
    int OH = (k == 1) ? in.H : out_dim(in.H, s), OW = (k == 1) ? in.W : out_dim(in.W, s);
    // with a shortcut the conv writes raw z to a scratch buffer and OP_ADDACT materialises z + res
    View out = (dst && !res) ? *dst : fresh(OH, OW, cout);
    Op op;
    op.kind = (k == 1) ? OP_PW : (dw ? OP_DW : OP_CONV3);
    op.in = in; op.out = out; op.stride = s; op.act = ACT_NONE; op.name = name;
    op.wslot = add_conv(name, in.C, cout, k, dw ? in.C : 1, true, false);
    net.ops.push_back(op);
    if (!res) return out;
    Op add; add.kind = OP_ADDACT; add.in = out; add.res = *res; add.act = ACT_NONE; add.name = name + "+shortcut";
    add.out = dst ? *dst : fresh(OH, OW, cout);
    net.ops.push_back(add);
    return add.out;
  }
  // DWConv = depthwise k x k (stride s) + pointwise 1x1.
  View dw_conv(const std::string& name, View in, int cout, int k, int s,
               const View* dst = nullptr, const View* res = nullptr) {
    View d = base_conv(name + ".dconv", in, in.C, k, s, true);
    return base_conv(name + ".pconv", d, cout, 1, 1, false, dst, res);
  }
  View conv(const std::string& name, View in, int cout, int k, int s,
            const View* dst = nullptr, const View* res = nullptr) {
    if (net.depthwise) return dw_conv(name, in, cout, k, s, dst, res);
    return base_conv(name, in, cout, k, s, false, dst, res);
  }
  // Bottleneck(c, c, shortcut, expansion=1.0)
  View bottleneck(const std::string& name, View in, bool shortcut, const View* dst) {
    View u = base_conv(name + ".conv1", in, in.C, 1, 1, false);
    return conv(name + ".conv2", u, in.C, 3, 1, dst, shortcut ? &in : nullptr);
  }
  // CSPLayer: conv1 and conv2 read the same input, so they run as ONE 1x1 conv of 2h channels writing the slices
  // [conv2 | conv1] of a 3h-channel buffer [m(conv1) | conv2 | conv1]; conv3 reads the first 2h channels
  // (= cat(m(conv1), conv2), the reference's order).  Halves the input reads and the launches of the pair, in
  // eval and train mode alike (BN statistics are per channel).
  View csp(const std::string& name, View in, int cout, int n, bool shortcut, const View* dst = nullptr) {
    int h = cout / 2;
    if (n == 0) {
      View cat = fresh(in.H, in.W, 2 * h);
      View s0 = slice(cat, 0, h), s1 = slice(cat, h, h);
      base_conv(name + ".conv1", in, h, 1, 1, false, &s0);
      base_conv(name + ".conv2", in, h, 1, 1, false, &s1);
      return base_conv(name + ".conv3", cat, cout, 1, 1, false, dst);
    }
    View buf3 = fresh(in.H, in.W, 3 * h);
    View s0 = slice(buf3, 0, h), pair = slice(buf3, h, 2 * h), t = slice(buf3, 2 * h, h);
    Op op;
    op.kind = OP_PW; op.in = in; op.out = pair; op.stride = 1; op.act = ACT_NONE; op.name = name + ".conv2|conv1";
    op.wslot = add_conv_pair(name + ".conv2", name + ".conv1", in.C, h);
    net.ops.push_back(op);
    for (int i = 0; i < n; ++i)
      t = bottleneck(name + ".m." + std::to_string(i), t, shortcut, i == n - 1 ? &s0 : nullptr);
    return base_conv(name + ".conv3", slice(buf3, 0, 2 * h), cout, 1, 1, false, dst);
  }
  View spp(const std::string& name, View in, int cout) {
    int h = in.C / 2;
    View cat = fresh(in.H, in.W, 4 * h);
    View s0 = slice(cat, 0, h);
    base_conv(name + ".conv1", in, h, 1, 1, false, &s0);
    Op op; op.kind = OP_SPP; op.in = s0; op.out = cat; op.name = name + ".m"; op.act = ACT_NONE;
    net.ops.push_back(op);
    return base_conv(name + ".conv2", cat, cout, 1, 1, false);
  }
  void upsample(View in, View dst) {
    // the upsampled copy holds raw z of the producing conv: it shares that layer's (scale, shift)
    for (auto it = net.ops.rbegin(); it != net.ops.rend(); ++it)
      if (it->wslot >= 0 && it->out.buf == in.buf && it->out.coff == in.coff) { it->alias = dst; break; }
    Op op; op.kind = OP_UPSAMPLE; op.in = in; op.out = dst; op.name = "upsample"; op.act = ACT_NONE;
    net.ops.push_back(op);
  }
};

// per-image buffer offsets (every buffer 256-B aligned), table channels and BatchNorm statistics channels of the net
void layout_offsets(Net& net) {
  net.buf_off.resize(net.bufs.size());
  net.tab_off.resize(net.bufs.size());
  size_t off = 0;
  int toff = 0, soff = 0;
  for (size_t i = 0; i < net.bufs.size(); ++i) {
    net.buf_off[i] = off; off += (net.bufs[i].per_image() + 63) / 64 * 64;
    net.tab_off[i] = toff; toff += net.bufs[i].C;
  }
  for (auto& cw : net.convs) { cw.stat_off = soff; soff += cw.cout; }
  net.per_image_floats = off; net.tab_channels = (toff + 3) / 4 * 4; net.stat_channels = soff;
}

}  // namespace

int build_pafpn(Net& net, std::vector<ParamEntry>& params, const std::string& prefix,
                float depth, float width, bool depthwise, int P) {
  JN_CHECK(P % 32 == 0 && P >= 32, JN_EINVAL, "patch_size %d must be a multiple of 32", P);
  net.prefix = prefix; net.depthwise = depthwise; net.depth = depth; net.width = width; net.P = P;
  Builder b{net, params, prefix};
  const int bc = (int)(width * 64);
  const int bd = std::max((int)std::lround(depth * 3), 1);
  const int c0 = (int)(256 * width), c1 = (int)(512 * width), c2 = (int)(1024 * width);
  const int n = (int)std::lround(3 * depth);
  JN_CHECK(bc % 16 == 0, JN_EINVAL, "width %.3f gives %d stem channels; channel counts must be multiples of 16", width, bc);
  JN_CHECK(c0 == bc * 4 && c1 == bc * 8 && c2 == bc * 16, JN_EINVAL, "unsupported width %.3f", width);
  const int H2 = P / 2, H4 = P / 4, H8 = P / 8, H16 = P / 16, H32 = P / 32;

  // concat buffers of the PAFPN, allocated first so producers can target their slices
  View cat_p4 = b.fresh(H16, H16, 2 * c1);
  View cat_p3 = b.fresh(H8, H8, 2 * c0);
  View cat_n3 = b.fresh(H16, H16, 2 * c0);
  View cat_n4 = b.fresh(H32, H32, 2 * c1);

  // ---- CSPDarknet ("backbone.backbone.*") ----
  View stem = b.fresh(H2, H2, bc);
  {
    Op op; op.kind = OP_STEM; op.out = stem; op.act = ACT_NONE; op.name = "backbone.stem.conv";
    op.in.buf = -1; op.in.H = P; op.in.W = P; op.in.C = 3;
    op.wslot = b.add_conv("backbone.stem.conv", 12, bc, 3, 1, true, false);
    net.ops.push_back(op);
  }
  View x = b.conv("backbone.dark2.0", stem, bc * 2, 3, 2);
  x = b.csp("backbone.dark2.1", x, bc * 2, bd, true);
  x = b.conv("backbone.dark3.0", x, bc * 4, 3, 2);
  View x2_dst = Builder::slice(cat_p3, c0, c0);
  View x2 = b.csp("backbone.dark3.1", x, bc * 4, bd * 3, true, &x2_dst);
  x = b.conv("backbone.dark4.0", x2, bc * 8, 3, 2);
  View x1_dst = Builder::slice(cat_p4, c1, c1);
  View x1 = b.csp("backbone.dark4.1", x, bc * 8, bd * 3, true, &x1_dst);
  x = b.conv("backbone.dark5.0", x1, bc * 16, 3, 2);
  x = b.spp("backbone.dark5.1", x, bc * 16);
  View x0 = b.csp("backbone.dark5.2", x, bc * 16, bd, false);
  (void)H4;

  // ---- PAFPN ----
  View fpn_out0_dst = Builder::slice(cat_n4, c1, c1);
  View fpn_out0 = b.base_conv("lateral_conv0", x0, c1, 1, 1, false, &fpn_out0_dst);
  b.upsample(fpn_out0, Builder::slice(cat_p4, 0, c1));
  View f_out0 = b.csp("C3_p4", cat_p4, c1, n, false);
  View fpn_out1_dst = Builder::slice(cat_n3, c0, c0);
  View fpn_out1 = b.base_conv("reduce_conv1", f_out0, c0, 1, 1, false, &fpn_out1_dst);
  b.upsample(fpn_out1, Builder::slice(cat_p3, 0, c0));
  View pan_out2 = b.csp("C3_p3", cat_p3, c0, n, false);
  View bu2_dst = Builder::slice(cat_n3, 0, c0);
  b.conv("bu_conv2", pan_out2, c0, 3, 2, &bu2_dst);
  View pan_out1 = b.csp("C3_n3", cat_n3, c1, n, false);
  View bu1_dst = Builder::slice(cat_n4, 0, c1);
  b.conv("bu_conv1", pan_out1, c1, 3, 2, &bu1_dst);
  View pan_out0 = b.csp("C3_n4", cat_n4, c2, n, false);
  net.fpn[0] = pan_out2; net.fpn[1] = pan_out1; net.fpn[2] = pan_out0;

  layout_offsets(net);

  // Backward bookkeeping: walking the ops in reverse, the first contributor to a gradient view
  // writes it, later ones accumulate.  The three FPN outputs are seeded from outside first.
  std::vector<std::vector<char>> written(net.bufs.size());
  for (size_t i = 0; i < net.bufs.size(); ++i) written[i].assign(net.bufs[i].C, 0);
  auto mark = [&](const View& v, bool& acc, const char* what, const std::string& name) -> int {
    int n_w = 0;
    for (int c = 0; c < v.C; ++c) n_w += written[v.buf][v.coff + c];
    JN_CHECK(n_w == 0 || n_w == v.C, JN_EINVAL, "backward plan: partially written gradient view (%s of %s)", what,
             name.c_str());
    acc = n_w == v.C;
    for (int c = 0; c < v.C; ++c) written[v.buf][v.coff + c] = 1;
    return JN_OK;
  };
  for (int i = 0; i < 3; ++i) { bool dummy; int rc = mark(net.fpn[i], dummy, "fpn", "seed"); if (rc) return rc; }
  for (auto it = net.ops.rbegin(); it != net.ops.rend(); ++it) {
    Op& op = *it;
    int rc = JN_OK;
    switch (op.kind) {
      case OP_STEM: case OP_PRED: break;
      case OP_SPP: op.acc_in = true; break;                       // adds into slice 0, written by the cat consumer
      case OP_ADDACT:
        if ((rc = mark(op.in, op.acc_in, "in", op.name))) return rc;
        if ((rc = mark(op.res, op.acc_res, "res", op.name))) return rc;
        break;
      default:
        if ((rc = mark(op.in, op.acc_in, "in", op.name))) return rc;
    }
  }
  return JN_OK;
}

// YOLOXHead (inference branch) appended to the detector's op list: per level stem 1x1, two 3x3
// convs per branch, and one OP_PRED (the three predictor convs + decode).  State-dict names
// follow upstream ("yolox.head.stems.0.conv.weight", "yolox.head.cls_preds.0.bias", ...).
int build_head(Net& net, std::vector<ParamEntry>& params, const std::string& prefix, float width, bool depthwise,
               int num_classes) {
  JN_CHECK(num_classes == 1, JN_EINVAL, "the needle detector has one class");
  Builder b{net, params, prefix};
  net.n_backbone_ops = (int)net.ops.size();
  const int hid = (int)(256 * width);
  const int strides[3] = {8, 16, 32};
  int a0 = 0;
  for (int k = 0; k < 3; ++k) {
    const std::string s = std::to_string(k);
    View x = b.base_conv("stems." + s, net.fpn[k], hid, 1, 1, false);
    View c = b.conv("cls_convs." + s + ".0", x, hid, 3, 1);
    c = b.conv("cls_convs." + s + ".1", c, hid, 3, 1);
    View r = b.conv("reg_convs." + s + ".0", x, hid, 3, 1);
    r = b.conv("reg_convs." + s + ".1", r, hid, 3, 1);
    Op op; op.kind = OP_PRED; op.in = r; op.res = c; op.act = ACT_NONE; op.name = "preds." + s;
    op.stride = strides[k]; op.level = k; op.anchor0 = a0;
    b.add_param(prefix + "cls_preds." + s + ".weight", {num_classes, hid, 1, 1}, 0, false, true);
    b.add_param(prefix + "cls_preds." + s + ".bias", {num_classes}, 0, false, true);
    b.add_param(prefix + "reg_preds." + s + ".weight", {4, hid, 1, 1}, 0, false, true);
    b.add_param(prefix + "reg_preds." + s + ".bias", {4}, 0, false, true);
    b.add_param(prefix + "obj_preds." + s + ".weight", {1, hid, 1, 1}, 0, false, true);
    b.add_param(prefix + "obj_preds." + s + ".bias", {1}, 0, false, true);
    net.ops.push_back(op);
    a0 += r.H * r.W;
  }
  net.n_anchors = a0;
  net.head_hid = hid;
  // backward bookkeeping of the head ops (detector training): the head is differentiated before the PAFPN, its stems
  // are the first writers of the three FPN gradient views (which the PAFPN plan treats as seeded from outside)
  {
    std::vector<std::vector<char>> written(net.bufs.size());
    for (size_t i = 0; i < net.bufs.size(); ++i) written[i].assign(net.bufs[i].C, 0);
    for (int oi = (int)net.ops.size() - 1; oi >= net.n_backbone_ops; --oi) {
      Op& op = net.ops[oi];
      if (op.kind == OP_PRED) {       // the predictor backward writes g[reg_feat] and g[cls_feat] in full
        for (int c = 0; c < op.in.C; ++c) written[op.in.buf][op.in.coff + c] = 1;
        for (int c = 0; c < op.res.C; ++c) written[op.res.buf][op.res.coff + c] = 1;
        continue;
      }
      int n_w = 0;
      for (int c = 0; c < op.in.C; ++c) n_w += written[op.in.buf][op.in.coff + c];
      JN_CHECK(n_w == 0 || n_w == op.in.C, JN_EINVAL, "backward plan: partially written gradient view (head op %s)", op.name.c_str());
      op.acc_in = n_w == op.in.C;
      for (int c = 0; c < op.in.C; ++c) written[op.in.buf][op.in.coff + c] = 1;
    }
  }
  layout_offsets(net);         // buffer / table / stats offsets grew with the head
  return JN_OK;
}

// ---- backward plan ---------------------------------------------------------------------------------------------------
namespace {

bool views_overlap(const View& a, const View& b) {
  return a.buf >= 0 && a.buf == b.buf && a.coff < b.coff + b.C && b.coff < a.coff + a.C;
}

// The one op that writes segment `seg` (as output or upsampled alias), provided it comes before op `before` and every
// op that reads the segment passes may_read(op, as_residual); -1 otherwise, and also when an SPP works on the buffer
// (it reads and writes the whole concat) or when seg is an FPN output that gets a gradient from outside the network
// (fpn_zero bit clear).  All ops are scanned, the head's too when it is not differentiated: a view it reads is not a
// single-consumer output.
template <class MayRead>
int sole_writer(const Net& net, const View& seg, int before, int fpn_zero, MayRead may_read) {
  for (int i = 0; i < 3; ++i)
    if (!((fpn_zero >> i) & 1) && views_overlap(seg, net.fpn[i])) return -1;
  int w = -1;
  for (int j = 0; j < (int)net.ops.size(); ++j) {
    const Op& o = net.ops[j];
    if ((views_overlap(o.in, seg) && !may_read(j, false)) || (views_overlap(o.res, seg) && !may_read(j, true))) return -1;
    if (o.kind == OP_SPP && o.out.buf == seg.buf) return -1;
    if (views_overlap(o.out, seg) || views_overlap(o.alias, seg)) {
      if (w >= 0 || j >= before) return -1;
      w = j;
    }
  }
  return w;
}

// The conv whose whole output is the `in` operand of shortcut add `add`, read by that add alone; -1 otherwise.
int shortcut_conv(const Net& net, int add, int fpn_zero) {
  const View& z = net.ops[add].in;
  const int w = sole_writer(net, z, add, fpn_zero, [&](int j, bool res) { return j == add && !res; });
  if (w < 0) return -1;
  const Op& o = net.ops[w];
  return o.wslot >= 0 && o.out.buf == z.buf && o.out.coff == z.coff && o.out.C == z.C ? w : -1;
}

// The BatchNorm conv that alone writes segment `seg` of op `reader`'s input: its whole output (*half = -1) or one half
// of a merged conv2|conv1 pair (*half = 0: conv2 rows, 1: conv1 rows), read by nothing but the reader and, as residual,
// `also` (the shortcut add whose copy the reader's kernel absorbs).  The reader then holds the FINAL gradient of the
// segment and can form that layer's BN-backward sums in its epilogue.  -1 otherwise.
int bn_producer(const Net& net, const View& seg, int reader, int also, int fpn_zero, int* half) {
  *half = -1;
  const int p = sole_writer(net, seg, reader, fpn_zero, [&](int j, bool res) { return j == reader || (res && j == also); });
  if (p < 0) return -1;
  const Op& po = net.ops[p];
  if (po.wslot < 0 || po.out.buf != seg.buf || views_overlap(po.alias, seg)) return -1;
  const ConvW& pw = net.convs[po.wslot];
  if (!pw.has_bn) return -1;
  if (pw.prefix2.empty()) return po.out.coff == seg.coff && po.out.C == seg.C && pw.cout == seg.C ? p : -1;
  if (pw.cout != 2 * seg.C || 2 * pw.cout_first != pw.cout || po.out.C != 2 * seg.C) return -1;
  *half = seg.coff == po.out.coff ? 0 : seg.coff == po.out.coff + seg.C ? 1 : -1;
  return *half >= 0 ? p : -1;
}

// RED2: segment `seg` of op `reader`'s input is a materialised shortcut sum (an OP_ADDACT's whole output) read by
// nothing but the reader and, as residual, `also`: the reader writes the FINAL gradient of the sum, which is also the
// gradient of the activation of the add's `in` operand.  Returns the conv behind that operand — the bottleneck's last
// 1x1 conv, BatchNorm, a single conv — or -1.
int shortcut_sum_conv(const Net& net, const View& seg, int reader, int also, int fpn_zero) {
  const int add = sole_writer(net, seg, reader, fpn_zero, [&](int j, bool res) { return j == reader || (res && j == also); });
  if (add < 0 || net.ops[add].kind != OP_ADDACT) return -1;
  const Op& ao = net.ops[add];
  if (ao.out.coff != seg.coff || ao.out.C != seg.C || ao.in.C != seg.C) return -1;
  const int conv = shortcut_conv(net, add, fpn_zero);
  if (conv < 0) return -1;
  const Op& co = net.ops[conv];
  const ConvW& cw = net.convs[co.wslot];
  return co.kind == OP_PW && !views_overlap(co.alias, ao.in) && cw.has_bn && cw.prefix2.empty() && cw.cout == seg.C ? conv : -1;
}

}  // namespace

// The backward of `net` as a pure function of its topology, the head (with_head) and the FPN outputs that get no
// outside gradient (fpn_zero bit i: none arrives in fpn[i], the training backward's case): one record per op of the
// backward range, filled walking it in reverse like the launcher (run_net_backward, api_net.hip).  fp32 activations
// only: the backward kernels read nothing else.
int plan_backward(const Net& net, bool with_head, int fpn_zero, std::vector<BwdStep>& plan) {
  JN_CHECK(net.act_dtype == JN_F32, JN_ESTATE, "training needs act_dtype = fp32 (bf16 is the inference mode)");
  const int n = (with_head || net.n_backbone_ops < 0) ? (int)net.ops.size() : net.n_backbone_ops;
  plan.assign(n, BwdStep{});
  auto fused_whole = [&](int j) {       // a 1x1 conv that takes pw_bwd_fused_kernel in one piece
    const Op& o = net.ops[j];
    const ConvW& cw = net.convs[o.wslot];
    return o.kind == OP_PW && cw.prefix2.empty() && pw_bwd_fused_supported(cw.cout, cw.cin);
  };
  for (int i = n - 1; i >= 0; --i) {
    const Op& op = net.ops[i];
    BwdStep& st = plan[i];
    if (op.wslot >= 0) {
      const ConvW& cw = net.convs[op.wslot];
      JN_CHECK(cw.has_bn, JN_ESTATE, "backward of BN-free conv %s inside a PAFPN", op.name.c_str());
      if (st.g.buf < 0) st.g = op.out;
      // a merged pair too wide for the fused kernel is differentiated as its two halves (independent output rows)
      const bool whole = pw_bwd_fused_supported(cw.cout, cw.cin);
      const bool halves = !whole && !cw.prefix2.empty() && 2 * cw.cout_first == cw.cout && pw_bwd_fused_supported(cw.cout_first, cw.cin);
      if (op.kind == OP_PW && (whole || halves)) {
        st.route = whole ? BR_PW_FUSED : BR_PW_FUSED_HALVES;
        // BN-backward sums of the input's producer(s) in the kernel's epilogue: it must write the FINAL gradient of the
        // view (sole reader, or the shortcut folded in) — one run, or the two halves of a CSP conv3's input
        if (!whole || (op.acc_in && st.fold < 0) || !pw_bwd_fused_reduces_input(cw.cout, cw.cin)) continue;
        auto seg = [&](int c0, int C) { View v = op.in; v.coff += c0; v.C = C; return v; };
        int r2 = -1;
        st.red_in = bn_producer(net, op.in, i, st.fold, fpn_zero, &st.red_half);
        if (st.red_in < 0 && (r2 = shortcut_sum_conv(net, op.in, i, st.fold, fpn_zero)) >= 0) {
          st.red_in = r2; st.red2 = true; st.red_split = op.in.C;
        } else if (st.red_in < 0 && op.in.C % 32 == 0 && st.fold < 0) {
          const int hC = op.in.C / 2;
          st.red_in = bn_producer(net, seg(0, hC), i, -1, fpn_zero, &st.red_half);
          st.red_in2 = bn_producer(net, seg(hC, hC), i, -1, fpn_zero, &st.red_half2);
          if (st.red_in < 0 && (r2 = shortcut_sum_conv(net, seg(0, hC), i, -1, fpn_zero)) >= 0) {
            st.red_in = r2; st.red2 = true;       // [shortcut sum | conv2 half]: the input of a CSP's conv3
          }
          if (st.red_in >= 0 || st.red_in2 >= 0) st.red_split = hC;   // (a lone second run still needs the split)
        }
      } else if (op.kind == OP_DW && dw_bwd_fused_supported(cw.cout, op.in.H, op.in.W, op.out.H, op.out.W, op.stride)) {
        st.route = BR_DW_FUSED;
        // A view that only the network's outside could also write (an FPN output) and that gets no outside gradient in
        // this backward (fpn_zero) is an ordinary single-consumer output: the kernel then WRITES its gradient (the
        // buffer holds zeros) and forms the producer's sums like for any other.
        bool ext_zero = false;
        for (int k = 0; k < 3; ++k) ext_zero = ext_zero || (((fpn_zero >> k) & 1) && views_overlap(op.in, net.fpn[k]));
        if (!op.acc_in || ext_zero) st.red_in = bn_producer(net, op.in, i, -1, fpn_zero, &st.red_half);
      } else if (op.kind == OP_STEM) {
        st.route = BR_STEM_FUSED;
      } else if (op.kind == OP_PW) {
        st.route = BR_PW;
      } else if (op.kind == OP_DW) {
        st.route = BR_DW;
      } else {
        JN_CHECK(op.kind == OP_CONV3, JN_ESTATE, "backward of op %s is not implemented", op.name.c_str());
        st.route = op.stride == 1 ? BR_CONV3_S1 : BR_CONV3_S2;
      }
      continue;
    }
    if (op.kind == OP_ADDACT) {
      // the gradient of the conv that feeds the add IS the gradient of the sum: as the sum's sole consumer it reads it
      // in place (no copy)
      const int z = shortcut_conv(net, i, fpn_zero);
      JN_CHECK(op.acc_in || z >= 0, JN_ESTATE, "backward plan: shortcut %s has no single conv behind its input", op.name.c_str());
      if (!op.acc_in) plan[z].g = op.out;
      // The shortcut branch, g[res] += g[sum]: when the only other reader of `res` is the bottleneck's first 1x1 conv
      // and that layer takes the fused kernel, the kernel adds g[sum] while it writes its data gradient (one read of
      // g[sum] instead of a copy pass over the largest 16 / 32-channel maps).  g[sum] must still hold the gradient
      // then: fine when the conv that feeds the add is a fused 1x1 too, not for the unfused paths, whose bn_bwd_gz
      // turns it into g_z IN PLACE (dense 3x3 bottlenecks of the non-depthwise encoders).
      int conv1 = -1;
      const bool one_reader = sole_writer(net, op.res, i, fpn_zero, [&](int j, bool res) {
        if (j == i) return res;
        const Op& o = net.ops[j];
        if (conv1 >= 0 || res || j > i || o.kind != OP_PW || o.in.buf != op.res.buf || o.in.coff != op.res.coff || o.in.C != op.res.C)
          return false;
        conv1 = j;
        return true;
      }) >= 0;
      const bool fold = !op.acc_res && one_reader && conv1 >= 0 && net.ops[conv1].acc_in && fused_whole(conv1) &&
                        z >= 0 && fused_whole(z);
      if (fold) plan[conv1].fold = i;
      st.route = fold ? BR_ADDACT_FOLD : BR_ADDACT_COPY;
    } else if (op.kind == OP_SPP) {
      st.route = BR_SPP;
    } else if (op.kind == OP_UPSAMPLE) {
      st.route = BR_UPSAMPLE;
    }
  }
  // every BN conv gets its sums formed exactly once: by one consumer that runs before it in the backward (per half for
  // merged pairs), else by its own reduce; every folded shortcut goes to a whole-route fused 1x1 conv
  for (int c = n - 1; c >= 0; --c) {
    const BwdStep& st = plan[c];
    const int runs[2][2] = {{st.red_in, st.red_half}, {st.red_in2, st.red_half2}};
    for (const auto& r : runs) {
      if (r[0] < 0) continue;
      const Op& po = net.ops[r[0]];
      const int bit = r[1] < 0 ? 1 : 1 << r[1];
      JN_CHECK((st.route == BR_PW_FUSED || st.route == BR_DW_FUSED) && r[0] < c && po.wslot >= 0 &&
               (r[1] >= 0) == !net.convs[po.wslot].prefix2.empty() && !(plan[r[0]].red_by & bit),
               JN_ESTATE, "backward plan: %s cannot form the BatchNorm sums of %s", net.ops[c].name.c_str(), po.name.c_str());
      plan[r[0]].red_by |= bit;
    }
    JN_CHECK(st.fold < 0 || st.route == BR_PW_FUSED, JN_ESTATE, "backward plan: shortcut %s folded into %s, not a fused 1x1 conv",
             st.fold < 0 ? "" : net.ops[st.fold].name.c_str(), net.ops[c].name.c_str());
  }
  return JN_OK;
}

// ---- forward plan ----------------------------------------------------------------------------------------------------
// Deferred BatchNorm tables (ChanTab in jn_kernels.h) need every consumer to read its table through jn_tab.h: only the
// depthwise fp32 PAFPN (the nano patch encoder) qualifies.
bool defer_eligible(const Net& net) {
  if (!net.depthwise || net.act_dtype != JN_F32) return false;
  const int n = net.n_backbone_ops < 0 ? (int)net.ops.size() : net.n_backbone_ops;
  for (int i = 0; i < n; ++i) {
    const Op& op = net.ops[i];
    if (op.kind == OP_CONV3 || op.kind == OP_PRED || (op.kind == OP_DW && op.in.C % 16 != 0)) return false;
    if (op.wslot >= 0 && !net.convs[op.wslot].has_bn) return false;
  }
  return true;
}

// One forward pass of `net` over N patches as a pure function of its topology, activation dtype and the pass (train,
// with_head, the first op, whether it defers): one record per op of [first_op, n_ops), in launch order.  What depends
// on launch-time state (pw_route for the fused upsample, JN_NO_PW_X3, the stream) stays with the launcher (run_net, api_net.hip).
int plan_forward(const Net& net, int N, bool train, bool with_head, int first_op, bool defer, std::vector<FwdStep>& plan) {
  const int n = (with_head || net.n_backbone_ops < 0) ? (int)net.ops.size() : net.n_backbone_ops;
  const bool f32 = net.act_dtype == JN_F32;
  JN_CHECK(first_op >= 0 && first_op <= n && N >= 1, JN_EINVAL, "forward plan: first op %d of %d, N = %d", first_op, n, N);
  JN_CHECK(!defer || (train && !with_head), JN_ESTATE, "forward plan: only a train-mode pass without the head defers");
  plan.assign(n - first_op, FwdStep{});
  auto at = [&](int i) -> FwdStep& { return plan[i - first_op]; };
  auto same = [](const View& a, const View& b) { return a.buf == b.buf && a.coff == b.coff && a.C == b.C; };
  for (int i = first_op; i < n; ++i) {
    const Op& op = net.ops[i];
    FwdStep& st = at(i);
    if (st.route == FR_ABSORBED) continue;
    static const FwdRoute by_kind[] = {FR_STEM, FR_CONV, FR_CONV, FR_CONV, FR_SPP, FR_UPSAMPLE, FR_ADDACT, FR_PRED};   // OpKind order
    st.route = by_kind[op.kind];
    if (!train && f32 && op.kind == OP_DW && i + 1 < n) {
      // eval: DWConv = depthwise + pointwise in one kernel, the depthwise output stays on chip
      const Op& nx = net.ops[i + 1];
      if (nx.kind == OP_PW && same(nx.in, op.out) && dwpw_supported(op.out.C, nx.out.C, op.stride)) {
        st.route = FR_DWPW; st.link = i + 1;
        at(i + 1).route = FR_ABSORBED; at(i + 1).link = i;
        // bottleneck shortcut: the add + activation goes into the epilogue, the pconv's raw z is never stored
        if (i + 2 < n && net.ops[i + 2].kind == OP_ADDACT && net.ops[i + 2].in.buf == nx.out.buf && net.ops[i + 2].in.coff == nx.out.coff) {
          st.route = FR_DWPW_ADD; st.add = i + 2;
          at(i + 2).route = FR_ABSORBED; at(i + 2).link = i;
        }
      }
    }
    // the source of a nearest x2 upsample: the producing fp32 1x1 kernel writes the upsampled copy where its route can
    for (int u = i + 1; st.route == FR_CONV && op.kind == OP_PW && f32 && u < n; ++u)
      if (net.ops[u].kind == OP_UPSAMPLE && same(net.ops[u].in, op.out)) { st.link = u; break; }
    st.deferred = defer && op.wslot >= 0 && (long long)N * op.out.H * op.out.W <= JN_DEFER_MAX_M;
  }
  // every op is launched or absorbed by exactly one launched fusion that precedes it and matches its kind and views; an
  // upsample is the candidate of at most one conv; fusions are eval fp32 only; a deferred layer has BatchNorm
  std::vector<char> covered(n, 0), cand(n, 0);
  for (int i = first_op; i < n; ++i) {
    const Op& op = net.ops[i];
    const FwdStep& st = at(i);
    const char* name = op.name.c_str();
    JN_CHECK(st.route != FR_NONE, JN_ESTATE, "forward plan: op %s has no route", name);
    if (st.route == FR_ABSORBED) {
      JN_CHECK(covered[i] == 1, JN_ESTATE, "forward plan: op %s is covered by %d kernels", name, (int)covered[i]);
      continue;
    }
    JN_CHECK(covered[i] == 0, JN_ESTATE, "forward plan: op %s is launched and absorbed", name);
    if (st.route == FR_DWPW || st.route == FR_DWPW_ADD) {
      const bool add = st.route == FR_DWPW_ADD;
      JN_CHECK(!train && f32 && op.kind == OP_DW && st.link == i + 1 && st.link < n && st.add == (add ? i + 2 : -1) && st.add < n,
               JN_ESTATE, "forward plan: %s cannot run as a fused DWConv", name);
      const Op& pw = net.ops[st.link];
      JN_CHECK(pw.kind == OP_PW && same(pw.in, op.out) && at(st.link).route == FR_ABSORBED && at(st.link).link == i, JN_ESTATE,
               "forward plan: %s does not absorb the 1x1 conv %s", name, pw.name.c_str());
      ++covered[st.link];
      if (add) {
        const Op& ad = net.ops[st.add];
        JN_CHECK(ad.kind == OP_ADDACT && same(ad.in, pw.out) && at(st.add).route == FR_ABSORBED && at(st.add).link == i, JN_ESTATE,
                 "forward plan: %s does not absorb the shortcut %s", name, ad.name.c_str());
        ++covered[st.add];
      }
    } else if (st.link >= 0) {
      JN_CHECK(st.route == FR_CONV && op.kind == OP_PW && f32 && st.link > i && st.link < n && net.ops[st.link].kind == OP_UPSAMPLE &&
               same(net.ops[st.link].in, op.out) && !cand[st.link]++, JN_ESTATE, "forward plan: %s cannot write upsample %d", name, st.link);
    }
    JN_CHECK(!st.deferred || (defer && op.wslot >= 0 && net.convs[op.wslot].has_bn), JN_ESTATE,
             "forward plan: %s defers a BatchNorm table it does not have", name);
  }
  return JN_OK;
}

}  // namespace jnr
