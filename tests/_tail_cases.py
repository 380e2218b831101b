"""Inputs, float64 references, error bounds and CPU emulations of the classifier-tail operator
tests: fc_mfma and gap (fc.hip), head_dense = gap_dense1_kernel + dense2_kernel (pool_head.hip).

Every input is rounded to its storage type first (activations and MFMA weights to bf16 or fp16;
the head's weights are fp32) and every reference is computed in float64 from the rounded values.
The bounds are per element and derived from the number formats and the lengths of the fp32 sums;
nothing in them is measured. tests/test_tail_ops_cpu.py shows that fp32 emulations of correct
kernels fit them and that the known-bad variants do not; tests/test_tail_ops_gpu.py holds the
kernels to them."""
import functools

import torch

from _mbconv_cases import TINY, U16, U32, ratio  # noqa: F401  (re-exported)
from _vit_cases import GUARD, SENTINEL16, guarded, guards_intact, within  # noqa: F401  (re-exported)

DTYPES = (torch.bfloat16, torch.float16)
U_OUT = (2.0 ** -8, 2.0 ** -11)
FLOOR = (TINY, 2.0 ** -25)


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _seq_sum(t: torch.Tensor, dim: int) -> torch.Tensor:
    """float32 sum along dim, one term after the other."""
    assert t.dtype == torch.float32
    if t.shape[dim] == 0:
        return torch.zeros(t.sum(dim).shape)
    return torch.cumsum(t, dim, dtype=torch.float32).select(dim, -1)


# ---------------------------------------------------------------------------------------------
# fc_mfma

FC_B = [1, 15, 16, 17, 64, 65, 80]
FC_SMALL = [(32, 1), (96, 10)]                   # KT = 1, 3: the four-way K split leaves waves with nothing
FC_LARGE = [(768, 1000), (2560, 1008)]           # the ViT and EfficientNet-B7 heads (N = 1008: a full last fragment)


def fc_launches():
    """(B, F, N, relu, dt, nan_rows): the cross product at F <= 96; every B, both relu and both
    types on the large heads. Rows B .. round_up(B, 16) of xb are NaN in half of the launches."""
    out, n = [], 0
    for F, N in FC_SMALL:
        for B in FC_B:
            for relu in (0, 1):
                for dt in (0, 1):
                    out.append((B, F, N, relu, dt, n % 2 == 0))
                    n += 1
    for (F, N), Bs in zip(FC_LARGE, ([1, 17, 64, 65], [15, 16, 65, 80])):
        for k, B in enumerate(Bs):
            out.append((B, F, N, k % 2, (k // 2) % 2, k % 2 == 1))
    return out


@functools.lru_cache(maxsize=8)
def fc_inputs(B: int, F: int, N: int, dt: int):
    """x [B][F], w [N][F] rounded to dt (as float32), bias [N] float32."""
    gen = torch.Generator().manual_seed(100000 * dt + 1000 * B + 10 * F + N)
    x = torch.randn(B, F, generator=gen).to(DTYPES[dt]).float()
    w = (torch.randn(N, F, generator=gen) / F ** 0.5).to(DTYPES[dt]).float()
    bias = torch.randn(N, generator=gen) * 0.3
    return x, w, bias.float()


def fc_reference(x, w, bias, relu: int):
    """float64 (ref, bound) [B][N]: F products and four partial sums in fp32, the bias add."""
    F = x.shape[1]
    pre = x.double() @ w.double().t() + bias.double()
    A = x.double().abs() @ w.double().abs().t() + bias.double().abs()
    return (torch.relu(pre) if relu else pre), (F + 4) * U32 * A


def fc_emulate(x, w, bias, relu: int, variant: str = "") -> torch.Tensor:
    """fc_mfma_kernel in float32: wave v sums k-steps [v KT / 4, (v + 1) KT / 4) in order, the four
    partial sums and the bias are added in order. 'drop_slice': every wave takes KT / 4 steps
    rounded down, so the last KT % 4 steps are lost."""
    B, F = x.shape
    KT = F // 32
    prod = (x.double()[:, None, :] * w.double()[None, :, :]).float()          # exact products
    parts = []
    for v in range(4):
        k0, k1 = v * KT // 4, (v + 1) * KT // 4
        if variant == "drop_slice":
            k0, k1 = v * (KT // 4), (v + 1) * (KT // 4)
        parts.append(_seq_sum(prod[:, :, 32 * k0:32 * k1], 2))
    out = parts[0] + parts[1] + parts[2] + parts[3] + bias
    return torch.relu(out) if relu else out


# ---------------------------------------------------------------------------------------------
# gap

GAP_HW = [1, 7, 8, 9, 31, 32, 33]                # GAP_PARTS = 8, the loop is unrolled four deep
GAP_F = [8, 264]


@functools.lru_cache(maxsize=8)
def gap_inputs(B: int, HW: int, F: int, ldx: int, dt: int):
    """x [B][HW][ldx] in dt, NaN from column F on; the mean of order one."""
    gen = torch.Generator().manual_seed(10000 * dt + 1000 * HW + F + B)
    x = torch.randn(B, HW, ldx, generator=gen) + 0.5
    x[:, :, F:] = float("nan")
    return x.to(DTYPES[dt])


def gap_reference(x, F: int, dt: int):
    """float64 (mean [B][F], bound of the fp32 output, bound of the dt copy): at most HW sums, the
    reciprocal and the product round once each."""
    xd = x[:, :, :F].double()
    HW = xd.shape[1]
    ref = xd.mean(1)
    d = (HW + 2) * U32 * xd.abs().mean(1)
    return ref, d, d + U_OUT[dt] * (ref.abs() + d) + FLOOR[dt]


# ---------------------------------------------------------------------------------------------
# head_dense

HEAD_CASES = [   # (kind, B, HW, F, H1, NC, ldx - F)
    ("benign", 1, 1, 64, 1, 1, 0),
    ("benign", 8, 3, 128, 100, 10, 8),
    ("benign", 9, 4, 2048, 128, 16, 0),
    ("benign", 33, 5, 64, 100, 17, 8),
    ("cancel", 9, 100, 2048, 100, 10, 8),
    ("benign", 1, 100, 128, 128, 17, 0),
    ("cancel", 8, 5, 64, 1, 16, 8),
    ("cancel", 33, 1, 128, 128, 10, 0),
    ("cancel", 1, 3, 64, 100, 17, 8),
]
HEAD_LISTS = dict(B=[1, 8, 9, 33], HW=[1, 3, 4, 5, 100], F=[64, 128, 2048], H1=[1, 100, 128], NC=[1, 10, 16, 17])


@functools.lru_cache(maxsize=4)
def head_inputs(kind: str, B: int, HW: int, F: int, H1: int, NC: int, pad: int):
    """x [B][HW][F + pad] bf16 (NaN in the pad columns), w1t [H1][F], b1 [H1], w2 [H1][NC], b2 [NC] fp32.
    'cancel': the images are small perturbations of one image and b1 = -(w1 f) of their mean plus a
    little noise, so the hidden pre-activations sit near 0 on both sides of the ReLU."""
    gen = torch.Generator().manual_seed(100000 * B + 1000 * HW + 10 * F + H1 + NC + 7 * pad)
    x = torch.randn(B, HW, F + pad, generator=gen)
    if kind == "cancel":
        x = x[:1] + 0.02 * torch.randn(B, HW, F + pad, generator=gen)
    x[:, :, F:] = float("nan")
    x = x.to(torch.bfloat16)
    w1t = (torch.randn(H1, F, generator=gen) / F ** 0.5 * HW ** 0.5).float()
    b1 = (torch.randn(H1, generator=gen) * 0.1).float()
    if kind == "cancel":
        f0 = x[:, :, :F].double().mean((0, 1))
        b1 = (-(w1t.double() @ f0) + 0.003 * torch.randn(H1, generator=gen).double()).float()
    w2 = (torch.randn(H1, NC, generator=gen) / H1 ** 0.5).float()
    b2 = (torch.randn(NC, generator=gen) * 0.1).float()
    return x, w1t.contiguous(), b1, w2.contiguous(), b2


def head_reference(x, w1t, b1, w2, b2):
    """float64 (out [B][NC], bound, hidden pre-activations). The bound, stage by stage, in the style
    of _mbconv_cases.pool_reference:
    f = mean: HW - 1 sums, the reciprocal and the product: (HW + 1) 2^-24 mean|x|;
    pre = w1 f + b1: that error through sum |w1| |f|, and F products, F / 64 partial sums and the
    bias add in fp32; ReLU has slope at most 1;
    out = w2 h + b2: the hidden error through sum |w2| |h|, and H1 products, the 16-lane tree and the
    bias add in fp32."""
    H1, F = w1t.shape
    xd = x[:, :, :F].double()
    HW = xd.shape[1]
    w1d, w2d = w1t.double(), w2.double()
    f, fa = xd.mean(1), xd.abs().mean(1)
    df = (HW + 1) * U32 * fa
    pre = f @ w1d.t() + b1.double()
    dpre = df @ w1d.abs().t() + (F + F // 64 + 2) * U32 * (fa @ w1d.abs().t() + b1.double().abs())
    h = torch.relu(pre)
    out = h @ w2d + b2.double()
    dout = dpre @ w2d.abs() + (H1 + 6) * U32 * ((h + dpre) @ w2d.abs() + b2.double().abs())
    return out, dout, pre


def head_emulate(x, w1t, b1, w2, b2, variant: str = "") -> torch.Tensor:
    """The two kernels in float32 with their summation orders: four pixel groups (pixels pg, pg + 4,
    ...) added in order and scaled by 1 / HW; one partial sum per 64 features; the partial sums in
    two halves (even and odd blocks), b1 + even + odd, ReLU; 16 slices of the hidden units per
    logit, folded by the xor tree; + b2. Variants: 'no_hw' forgets the 1 / HW; 'group_twice' has a
    pixel group beyond HW read pixel pg % HW again; 'relu_first' applies the ReLU before b1."""
    H1, F = w1t.shape
    B, HW, _ = x.shape
    xf = x[:, :, :F].float()
    groups = []
    for pg in range(4):
        px = xf[:, pg::4]
        if variant == "group_twice" and pg >= HW:
            px = xf[:, pg % HW:pg % HW + 1]
        groups.append(_seq_sum(px, 1))
    inv = torch.tensor(1.0 if variant == "no_hw" else 1.0 / HW, dtype=torch.float32)
    f = (((groups[0] + groups[1]) + groups[2]) + groups[3]) * inv
    halves = [torch.zeros(B, H1), torch.zeros(B, H1)]
    for kb in range(F // 64):
        prod = (f[:, None, 64 * kb:64 * kb + 64].double() * w1t[None, :, 64 * kb:64 * kb + 64].double()).float()
        halves[kb % 2] = halves[kb % 2] + _seq_sum(prod, 2)
    if variant == "relu_first":
        h = torch.relu(halves[0] + halves[1]) + b1
    else:
        h = torch.relu(b1 + halves[0] + halves[1])
    prod = (h[:, :, None].double() * w2[None, :, :].double()).float()          # [B][H1][NC]
    sl = [_seq_sum(prod[:, s::16], 1) for s in range(16)]
    for step in (1, 2, 4, 8):
        sl = [sl[s] + sl[s ^ step] for s in range(16)]
    return sl[0] + b2
