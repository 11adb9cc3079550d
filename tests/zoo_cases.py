"""Kernel cases at the channel counts of the YOLOX sizes that are no powers of two (yolox-m 48 ... 1536, yolox-x 80 ... 2560, and the
24 ... 768 of yolox-tiny's layers behind the stem), for the kernels a dense pass launches.  No new inputs, references or bars: every
case is a Case of tests/glue_cases.py, tests/pw_cases.py or tests/conv3_cases.py, whose inputs(), reference() and over_bars() take
any shape.

Shared by tests/test_zoo_cases_cpu.py (the cases are admitted by the route entries and the bars hold for plain fp32 on them) and
tests/test_gpu_zoo_kernels.py (every kernel against fp64).

1x1 convs: forward 48 -> 48, 24 -> 24, 96 -> 48, 80 -> 40 and 1280 -> 640 with statistics, the data gradient of the same layers
(transposed, read through the identity table) and their weight gradient; M = 5 and 69 pixels (69: a second, partial tile of every
pixel tile of 16, 32 or 64), the weight gradient at 5, 200 and, on the wide kernel (1280 -> 640), 300.

Dense 3x3 convs on maps of 3 x 5, 7 x 7 and 24 x 24 output pixels (the last: a full and a partial 16 x 16 / 8 x 16 tile each way):
forward stride 2 24 -> 48, stride 1 24 -> 24, 48 -> 48, 80 -> 80, the stride-1 data gradient of those, the stride-2 data gradient
48 -> 24, and the weight gradient at Co = 24, 40 (no multiple of 16: the SPLIT form) and 48 (TR).

BatchNorm backward sums at C = 24, 40, 48, 80, 96, 1032 and 1280 (above 1024 channels launch_bn_bwd_reduce goes in two halves of whole
quads: 516 or 640 channels at 32 rows a workgroup each), M one row below and above a workgroup's rows and past 32 workgroups.

Shortcut sum, upsample (forward and backward) and SPP (forward and backward) at C = 24, 96 and 192.

The stem kernels are not here: they own 16 output channels a workgroup, every size but yolox-tiny has a stem width that is a multiple
of 16 (48, 64, 80 are covered by the 16 / 32 / 48 of glue_cases.py: one, two and three groups), and yolox-tiny's 24 stays refused."""
from tests import conv3_cases as cc
from tests import glue_cases as gc
from tests import pw_cases as pc

# ---- 1x1 -------------------------------------------------------------------------------------------------------------------------
PW_LAYERS = ((48, 48), (24, 24), (96, 48), (80, 40), (1280, 640))      # (cin, cout) of the forward layer
PW_M = (5, 69)


def pw_forward_cases():
    return [pc._case("pw", 0, M, cin, cout, stats=1) for cin, cout in PW_LAYERS for M in PW_M]


def pw_data_gradient_cases():
    """The entry's (cin, cout) = the layer's (cout, cin): g_z in, the transposed weight, no input transform."""
    return [pc._case("pw", 0, M, cout, cin, transposed=1, identity=1) for cin, cout in PW_LAYERS for M in PW_M]


def pw_weight_gradient_cases():
    cases = []
    for cin, cout in PW_LAYERS:
        wide = cin >= 128 and cout >= 128
        for M in ((300,) if wide else (5, 200)):
            for slots in (1, 3):
                cases.append(pc._case("bw", 0, M, cin, cout, slots=slots, use_wpart=int(not wide and cin * cout <= pc.WPART_MAX)))
    return cases


# ---- dense 3x3 -------------------------------------------------------------------------------------------------------------------
C3_MAPS = ((3, 5), (7, 7), (24, 24))      # OUTPUT maps
C3_S1 = ((24, 24), (48, 48), (80, 80))
C3_S2 = ((24, 48),)
C3_DW = ((1, (24, 24)), (1, (40, 40)), (1, (48, 48)), (2, (24, 48)))      # (stride, (cin, cout)): Co = 24, 40 SPLIT, 48 TR


def _in_map(hw, stride):
    return (hw[0] * stride, hw[1] * stride)


def conv3_cases():
    cases = []
    for hw in C3_MAPS:
        for p in C3_S1:
            cases.append(cc._case("fwd", 0, 1, hw, p, stats=1))
            cases.append(cc._case("wt", 0, 1, hw, p[::-1]))
        for p in C3_S2:
            cases.append(cc._case("fwd", 0, 2, _in_map(hw, 2), p, stats=1))
            cases.append(cc._case("ds2", 0, 2, _in_map(hw, 2), p))
        for stride, p in C3_DW:
            cases.append(cc._case("dw", 0, stride, _in_map(hw, stride), p))
    cases.append(cc._case("dw", 0, 1, (24, 24), (40, 40), slots=3))
    cases.append(cc._case("ds2", 0, 2, (48, 48), (24, 48), slots=3, accumulate=1))
    return cases


def conv3_weight_route(c):
    """What conv3_bwd_weight_route names: TR needs Co % 16 == 0 (and Ci % 4 == 0), else SPLIT.  A restatement: both test files hold
    it to jn_conv3_route on every case."""
    return 1 if c.cout % 16 == 0 else 2


# ---- BatchNorm backward sums -------------------------------------------------------------------------------------------------------
BNB_CHANNELS = (24, 40, 48, 80, 96, 1032, 1280)      # 1032 = two halves of 129 quads: the smallest count above 1024 that is admitted


def bnb_rows_per_block(C):
    """Rows a workgroup of launch_bn_bwd_reduce takes: 256 / (quads of a launch) rows at a time, 32 times; above 1024 channels a launch
    holds half of them."""
    per_launch = C // 2 if C > 1024 else C
    return (256 // (per_launch // 4)) * 32


def bnb_cases():
    cases = []
    for C in BNB_CHANNELS:
        rows = bnb_rows_per_block(C)
        cases += [gc._case("bnb", C=C, M=M, consts=1) for M in (rows - 1, rows + 1, 33 * rows + 3)]
    cases += [gc._case("bnb", C=C, M=bnb_rows_per_block(C) + 1, slots=3, consts=1) for C in (24, 1280)]
    return cases


# ---- shortcut sum, upsample, SPP ---------------------------------------------------------------------------------------------------
GLUE_CHANNELS = (24, 96, 192)


def glue_cases():
    cases = []
    for C in GLUE_CHANNELS:
        for dt in (0, 1):
            cases += [gc._case("add", C=C, dtype=dt, M=gc.N * 7 * 7), gc._case("up", H=3, W=5, C=C, dtype=dt, M=gc.N * 15),
                      gc._case("spp", H=7, W=7, C=C, dtype=dt), gc._case("spp", H=3, W=5, C=C, dtype=dt)]
        cases += [gc._case("upb", H=7, W=7, C=C, M=gc.N * 49), gc._case("upb", H=3, W=5, C=C, M=gc.N * 15, slots=3, accumulate=1, ints=1),
                  gc._case("sppb", H=7, W=7, C=C), gc._case("sppb", H=3, W=5, C=C, slots=3)]
    return cases
