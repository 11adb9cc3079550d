#!/usr/bin/env python3
"""Device time of one conv-stack pass of every YOLOX size the engine runs (nano, s, m, l, x; yolox-tiny is refused), on one GPU, in one process, over
16 patches of 448 px.  Gates nothing and no default depends on it: nobody had measured the sizes beside nano and s.

Per size, through the public entries of one model that holds the size as patch encoder and as detector:
  eval    one eval-mode forward pass of the encoder (GPT.backbone_features: jn_backbone_forward, the three FPN maps copied out NCHW);
  train   one train-mode forward pass and its backward (backbone_features(train=True) + backbone_backward: every conv and BatchNorm
          gradient of the stack; x included);
  detect  one jn_detect of the detector (PAFPN, head, decode, threshold and NMS).
A sample is one pass between two HIP events; after one warm-up of every (size, pass) the sizes are interleaved, `--repeats` samples
each, in alternating order; the figure is the median with (max - min).  Every GPU step runs under a hard time limit.

Beside each figure the pass's algorithmic bytes: every conv reads its input map and writes its output map once in fp32, plus its
weights (eval: sum over the convs of (in + out) x 4 B x N + 4 B x weights; the backward reads g_out, z_out and x and writes g_in:
(2 in + 2 out) x 4 B x N + 8 B x weights more), counted off the oracle's modules; concat copies, SPP and upsample are not counted.
`gbps` = those bytes over the measured time, for reading against the 8 TB/s of the HBM: what a pass is short of, it spends in the
matrix pipe or in launches.  Prints ONE JSON line and writes it to `--out`.

    python tools/zoo_ab.py [--patches 16] [--repeats 7] [--sizes yolox-nano,...] [--out profiles/zoo_ab.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from infer_ab import Limit  # noqa: E402

SIZES = ("yolox-nano", "yolox-s", "yolox-m", "yolox-l", "yolox-x")


def algorithmic_bytes(size, P, N, with_head):
    """(forward, backward) bytes of the size's convs over N patches of P px, from the oracle's modules at 64 px scaled by area."""
    from oracle import yolox_ref
    net = yolox_ref.build_yolox(size, 2).eval()
    elems, weights = [0], [0]

    def hook(m, inp, out):
        elems[0] += inp[0][0].numel() + out[0].numel()
        weights[0] += m.weight.numel()
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.register_forward_hook(hook)
    with torch.no_grad():
        feats = net.backbone(torch.rand(1, 3, 64, 64))
        if with_head:
            net.head.raw_maps(feats)
    area = (P / 64) ** 2
    fwd = elems[0] * area * 4 * N + 4 * weights[0]
    return fwd, 2 * elems[0] * area * 4 * N + 8 * weights[0]


PW_ROUTES = {1: "X1", 2: "X3", 3: "XS", 4: "WIDE", 5: "NARROW", 6: "MFMA"}
C3_ROUTES = {1: "F32", 2: "X3", 3: "BF16"}
CW_ROUTES = {1: "TR", 2: "SPLIT", 3: "EXACT"}


def route_table(sizes, P, N):
    """Needs no GPU: per size, every distinct conv launch (kind, cin -> cout, stride, input map) of the oracle's backbone, PAFPN and
    head at N patches of P px, with the route the route entries name: forward fp32 / forward bf16 / data gradient / weight gradient."""
    from jolineedle_amd import _lib
    from oracle import yolox_ref
    lib = _lib.load_library()
    lines = []
    for size in sizes:
        net = yolox_ref.build_yolox(size, 2).eval()
        rec = set()
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d) and m.bias is None and m.in_channels != 12:
                m.register_forward_hook(lambda m, i, o: rec.add((m.kernel_size[0], m.groups > 1, m.in_channels, m.out_channels, m.stride[0],
                                                                i[0].shape[2] * P // 64)))
        with torch.no_grad():
            net.head.raw_maps(net.backbone(torch.rand(1, 3, 64, 64)))
        stem = net.backbone.backbone.stem.conv.conv.out_channels
        lines.append(f"{size}: stem 12 -> {stem} ({P // 2} px map): " + ("stem_mfma_kernel / stem_bwd_weight_kernel" if stem % 16 == 0 else
                     "REFUSED by jn_create (no multiple of 16); the routes below are what the entries name for the layers behind it"))
        for k, dw, cin, cout, stride, hw in sorted(rec):
            if k == 1:
                f32 = lib.jn_pw_route(N, hw, hw, cin, cout, cin, cout, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, None)
                b16 = lib.jn_pw_route(N, hw, hw, cin, cout, cin, cout, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, None)
                dat = lib.jn_pw_route(N, hw, hw, cout, cin, cout, cin, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, None)
                wgt = {1: "narrow", 2: "wide"}[lib.jn_pw_bwd_weight_route(cout, cin)]
                lines.append(f"  1x1 {cin:5d} -> {cout:5d}       map {hw:4d}: fwd {PW_ROUTES[f32]:6s} bf16 {PW_ROUTES[b16]:6s} data {PW_ROUTES[dat]:6s} weight {wgt}")
            elif dw:
                r = lib.jn_dw3x3_route(N, cin, stride, 0)
                lines.append(f"  dw3 {cin:5d}          s{stride}   map {hw:4d}: fwd route {r}")
            else:
                f32 = lib.jn_conv3_route(0, N, hw, hw, cin, cout, stride, 1, cin, cout)
                dat = lib.jn_conv3_route(1 if stride == 1 else 2, N, hw, hw, cin, cout, stride, 1, cout if stride == 2 else cin,
                                         cin if stride == 2 else cout)
                wgt = lib.jn_conv3_route(3, N, hw, hw, cin, cout, stride, 1, cout, cin)
                lines.append(f"  3x3 {cin:5d} -> {cout:5d} s{stride}   map {hw:4d}: fwd {C3_ROUTES[f32]:6s} bf16 BF16   data {C3_ROUTES[dat]:6s} weight {CW_ROUTES[wgt]}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--routes", metavar="FILE", help="write the route table of every size (host code only, no GPU) to FILE and exit")
    ap.add_argument("--patches", type=int, default=16)
    ap.add_argument("--patch-size", type=int, default=448)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "zoo_ab.json"))
    args = ap.parse_args()
    if args.routes:
        Path(args.routes).write_text(route_table([s for s in args.sizes.split(",") if s], args.patch_size, args.patches))
        return

    from jolineedle_amd import _lib
    from jolineedle_amd._lib import check, ptr
    from tests.helpers import make_pair

    assert torch.cuda.is_available(), "zoo_ab needs the GPU"
    dev = torch.device("cuda:0")
    N, P, lim = args.patches, args.patch_size, args.step_timeout
    sizes = [s for s in args.sizes.split(",") if s]
    x = torch.rand((N, 3, P, P), generator=torch.Generator().manual_seed(1)).to(dev)

    models, grads, det_bufs = {}, {}, {}
    for size in sizes:
        product, _ = make_pair(3, patch_size=P, block_size=4, gpt_backbone=size, image_processor=size, max_batch=N)
        models[size] = product
        with Limit(lim):
            outs = product.backbone_features(x)
            torch.cuda.synchronize()
        grads[size] = [torch.randn(o.shape, device=dev) for o in outs]
        eng = product.engine()
        A = sum((P // s) ** 2 for s in (8, 16, 32))
        det_bufs[size] = (torch.empty((N, A, 6), device=dev), torch.zeros((N, eng.cfg.max_det_per_patch, 7), device=dev),
                          torch.zeros(N, device=dev, dtype=torch.int32))

    def run(size, what):
        product = models[size]
        if what == "eval":
            product.backbone_features(x)
        elif what == "train":
            product.backbone_features(x, train=True)
            product.backbone_backward(x, grads[size])
        else:
            eng = product.engine()
            raw, boxes, counts = det_bufs[size]
            check(eng.lib.jn_detect(eng.handle, ptr(x), N, ptr(boxes), ptr(counts), ptr(raw), _lib.current_stream(dev)), "jn_detect")

    def sample(size, what):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        run(size, what)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    passes = ("eval", "train", "detect")
    pairs = [(s, w) for s in sizes for w in passes]
    ms = {p: [] for p in pairs}
    for p in pairs:                                   # warm-up: LDS grants, the aux stream, the allocator
        with Limit(lim):
            sample(*p)
            models[p[0]].engine_zero_grad()
    for r in range(args.repeats):
        for p in (pairs if r % 2 == 0 else pairs[::-1]):
            with Limit(lim):
                ms[p].append(sample(*p))
        for s in sizes:
            models[s].engine_zero_grad()

    out = {"tool": "zoo_ab", "patches": N, "patch_size": P, "repeats": args.repeats,
           "note": "ms per pass under HIP events, median and (max - min), sizes interleaved; bytes = algorithmic conv traffic "
                   "(see tools/zoo_ab.py); gbps = bytes / ms"}
    for size in sizes:
        f_enc, b_enc = algorithmic_bytes(size, P, N, False)
        f_det, _ = algorithmic_bytes(size, P, N, True)
        row = {}
        for what, nbytes in (("eval", f_enc), ("train", f_enc + b_enc), ("detect", f_det)):
            v = ms[(size, what)]
            med = statistics.median(v)
            row[what] = {"ms": round(med, 3), "ms_spread": round(max(v) - min(v), 3), "mbytes": round(nbytes / 1e6, 1),
                         "gbps": round(nbytes / med / 1e6, 1)}
        out[size] = row
        print(f"{size}: " + ", ".join(f"{w} {row[w]['ms']} ms ({row[w]['mbytes']} MB, {row[w]['gbps']} GB/s)" for w in passes), file=sys.stderr, flush=True)

    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
