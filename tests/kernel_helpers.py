"""What the per-kernel test modules (test_gpu_{pw,dw,conv3,glue}_kernels.py) and their case modules ({pw,dw,conv3,glue}_cases.py)
share: tensor placement, the bit-for-bit comparison, bf16 rounding, layout permutes and SiLU's derivative."""
import torch

DEV = "cuda:0"


def _dev(t):
    return t.to(DEV).contiguous()


def _pattern(*shape):
    """What the fp64 accumulators hold before the launch adds to them: not zero."""
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=torch.float64, device=DEV) % 7).reshape(shape)


def _bits(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                       b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _dsilu(y):
    s = torch.sigmoid(y)
    return s * (1 + y * (1 - s))
