"""Inputs, float64 references, error bounds, CPU emulations and the launch matrix of the stem
operator tests (stem_kernel and stem_rows_kernel of stem.hip, every instance stem_conv dispatches).

Weights are rounded to the storage type (bf16 or fp16) first and the reference is computed in
float64 from exactly the operands the MFMA sees: the rounded weights and the *rounded* A operand,
which for a normalise-on-load ('generic') instance is round_dt(fp32(raw * scale + shift)) and 0,
not shift, at a padded tap. stem_rows_kernel computes raw * scale + shift with fmaf; stem_kernel
writes it as a product and a sum, which the compiler may contract or not. There are only 768
(pixel value, channel) pairs: operand_table() computes both orders for all of them, the reference
uses the fused one, and an output of stem_kernel that touches a pair whose two orders round to
different values gains |w_k| * |difference| (one unit in the last place of a_k) in its bound.

The bound is per element and derived from the number formats; nothing in it is measured:
    d     = (K_terms + 2) * 2^-24 * A [+ the term above],  A = sum |a_k| |w_k| + |bias|
    SiLU:   d <- 1.1 d + 8 * 2^-24 |y| + 2^-24 |pre| |y|    (as _mbconv_cases.dw_bound)
    bound = d + U_out * (|y| + d) + the smallest step of the output format near zero
with K_terms the padded K of the instance, U_out = 2^-8 (bf16) or 2^-11 (fp16).
tests/test_stem_ops_cpu.py shows that an fp32 emulation of a correct kernel fits it on every
launch of the matrix and that the known-bad variants do not; tests/test_stem_ops_gpu.py holds
the kernels to it."""
import functools
from typing import NamedTuple

import numpy as np
import torch

from _mbconv_cases import TINY, U32, _silu32, ratio, share_over  # noqa: F401  (re-exported)
from _vit_cases import GUARD, SENTINEL16, guarded, guards_intact, within  # noqa: F401  (re-exported)

MEAN = (0.485, 0.456, 0.406)                    # torchvision, as the ResNet / EfficientNet engines
STD = (0.229, 0.224, 0.225)
SCALE = tuple(float(np.float32(1.0 / (255.0 * s))) for s in STD)        # what the launcher receives
SHIFT = tuple(float(np.float32(-m / s)) for m, s in zip(MEAN, STD))
DTYPES = (torch.bfloat16, torch.float16)
U_OUT = (2.0 ** -8, 2.0 ** -11)
FLOOR = (TINY, 2.0 ** -25)                      # a flush to zero; half an fp16 subnormal step
KINDS = ["benign", "cancel", "edge"]


class Instance(NamedTuple):
    kernel: str       # 'stem' (k = (ky*KW + kx)*3 + c) or 'rows' (k = ky*RP + kx*3 + c)
    in_kind: int      # 0 uint8, 1 fp32
    KW: int
    cout: int
    generic: bool     # normalise on load, bounds checks
    dt: int           # 0 bf16, 1 fp16


class Problem(NamedTuple):
    B: int
    H: int
    W: int
    stride: int
    pad: int


class Launch(NamedTuple):
    inst: Instance
    prob: Problem
    kind: str
    act: int          # 0 none, 1 ReLU, 2 SiLU
    ldy_extra: int    # ldy = cout + ldy_extra
    off: int          # bytes the image pointer is moved into its buffer (uint8 only)


def out_size(n: int, K: int, S: int, pad: int) -> int:
    return (n + 2 * pad - K) // S + 1


def rp_of(KW: int) -> int:
    return 32 if KW == 7 else 16


def kt_of(inst: Instance) -> int:
    K = inst.KW * rp_of(inst.KW) if inst.kernel == "rows" else inst.KW * inst.KW * 3
    return (K + 31) >> 5


def round_dt(f: torch.Tensor, dt: int) -> torch.Tensor:
    assert f.dtype == torch.float32
    return f.to(DTYPES[dt]).float()


def truncate_dt(f: torch.Tensor, dt: int) -> torch.Tensor:
    """float32 -> bf16 / fp16 towards zero (the broken conversion), as float32."""
    if dt == 0:
        return (f.contiguous().view(torch.int32) & -65536).view(torch.float32)
    h = f.to(torch.float16)
    over = h.float().abs() > f.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h).float()


# ---------------------------------------------------------------------------------------------
# the A operand of the normalise-on-load instances

@functools.lru_cache(maxsize=None)
def operand_table(dt: int):
    """(fused, separate) float32 [256][3]: round_dt(fmaf(v, scale_c, shift_c)) and
    round_dt(fp32(v * scale_c) + shift_c) for every pixel value and channel."""
    v = torch.arange(256, dtype=torch.float32)[:, None]
    sc, sh = torch.tensor(SCALE, dtype=torch.float32), torch.tensor(SHIFT, dtype=torch.float32)
    fused = (v.double() * sc.double() + sh.double()).float()        # exact in float64: one rounding
    sep = (v * sc) + sh
    return round_dt(fused, dt), round_dt(sep, dt)


def operand(raw: torch.Tensor, dt: int, variant: str = "") -> torch.Tensor:
    """float32 A operand [..][3] of pixel values raw (integers 0..255 in any dtype).
    'separate' takes the other order; 'channel' the scale / shift of the next channel; 'truncate'
    the truncating conversion."""
    idx = raw.long()
    c = torch.arange(3).expand_as(idx)
    if variant == "channel":
        c = (c + 1) % 3
    if variant == "truncate":
        sc, sh = torch.tensor(SCALE, dtype=torch.float32), torch.tensor(SHIFT, dtype=torch.float32)
        f = (idx.double() * sc.double()[c] + sh.double()[c]).float()
        return truncate_dt(f, dt)
    fused, sep = operand_table(dt)
    return (sep if variant == "separate" else fused)[idx, c]


# ---------------------------------------------------------------------------------------------
# inputs

def _seed(*key) -> int:
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=64)
def inputs(kind: str, prob: Problem, KW: int, cout: int, generic: bool, dt: int, in_kind: int):
    """(image, w [cout][KW][KW][3] float32 rounded to dt, bias [cout] float32).
    image: uint8 [B][H][W][3]; for in_kind 1 float32, pixel values as floats for a generic instance
    and already-normalised floats (x / 127.5 - 1) for the non-generic one."""
    B, H, W, _, _ = prob
    gen = torch.Generator().manual_seed(_seed(KINDS.index(kind), *prob, KW, cout, generic, dt, in_kind))
    w = torch.randn(cout, KW, KW, 3, generator=gen) * (0.6 / KW)
    bias = torch.randn(cout, generator=gen) * 0.1
    if kind == "benign":
        img = torch.randint(0, 256, (B, H, W, 3), generator=gen, dtype=torch.uint8)
    elif kind == "cancel":     # every channel's taps sum to zero, input channel by input channel
        img = (180 + torch.randint(0, 3, (B, H, W, 3), generator=gen)).to(torch.uint8)
        w = torch.round(w * 32) / 32
        w[:, -1, -1, :] = 0
        w[:, -1, -1, :] = -w.sum((1, 2))
        assert bool((w.double().sum((1, 2)) == 0).all())
        bias = bias * 0.01
    else:                      # 'edge': 0 inside, 255 on the outermost ring, or the reverse
        ring = torch.ones(H, W, dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        hi, lo = (255, 0) if (H + W + B) % 2 else (0, 255)
        img = torch.where(ring[None, :, :, None], hi, lo).expand(B, H, W, 3).to(torch.uint8).contiguous()
    wr = round_dt(w.float(), dt)
    if kind == "cancel":
        assert torch.equal(wr, w.float())            # multiples of 1/32 below 8: exact in both formats
    if in_kind == 1:
        img = img.float() if generic else (img.float() / 127.5 - 1.0)
    return img, wr.contiguous(), bias.float().contiguous()


def a_operand(img: torch.Tensor, generic: bool, dt: int, variant: str = "") -> torch.Tensor:
    """float32 [B][H][W][3]: what the MFMA multiplies for every pixel that is read."""
    if generic:
        return operand(img, dt, variant)
    f = img.float()
    return truncate_dt(f, dt) if variant == "truncate" else round_dt(f, dt)


# ---------------------------------------------------------------------------------------------
# reference and bound

def conv_reference(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, stride: int, pad: int):
    """float64 (pre, A) [B][OH][OW][cout]: tap by tap over the zero-padded operand."""
    B, H, W, _ = a.shape
    cout, KH, KW, _ = w.shape
    OH, OW = out_size(H, KH, stride, pad), out_size(W, KW, stride, pad)
    ad, wd, bd = a.double(), w.double(), bias.double()
    ap = torch.zeros(B, H + 2 * pad, W + 2 * pad, 3, dtype=torch.float64)
    ap[:, pad:pad + H, pad:pad + W] = ad
    pre = torch.zeros(B, OH, OW, cout, dtype=torch.float64)
    A = torch.zeros_like(pre)
    for ky in range(KH):
        for kx in range(KW):
            v = ap[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride]
            pre += v @ wd[:, ky, kx].t()
            A += v.abs() @ wd[:, ky, kx].abs().t()
    return pre + bd, A + bd.abs()


def act_of(pre: torch.Tensor, act: int) -> torch.Tensor:
    return torch.relu(pre) if act == 1 else pre * torch.sigmoid(pre) if act == 2 else pre


def bound_of(pre, A, extra, k_terms: int, act: int, dt: int):
    y = act_of(pre, act)
    d = (k_terms + 2) * U32 * A + extra
    if act == 2:
        d = 1.1 * d + 8 * U32 * y.abs() + U32 * pre.abs() * y.abs()
    return d + U_OUT[dt] * (y.abs() + d) + FLOOR[dt]


class Case:
    """The float64 reference of one launch; read-only once built."""

    def __init__(self, L: Launch):
        i, p = L.inst, L.prob
        self.L = L
        self.KH = self.KW = i.KW
        self.OH, self.OW = out_size(p.H, i.KW, p.stride, p.pad), out_size(p.W, i.KW, p.stride, p.pad)
        self.M = p.B * self.OH * self.OW
        self.img, self.w, self.bias = inputs(L.kind, p, i.KW, i.cout, i.generic, i.dt, i.in_kind)
        a = a_operand(self.img, i.generic, i.dt)
        self.pre, self.A = conv_reference(a, self.w, self.bias, p.stride, p.pad)
        self.extra = torch.zeros_like(self.pre)
        if i.generic and i.kernel == "stem":     # the compiler may or may not contract raw * s + sh
            diff = (a_operand(self.img, True, i.dt, "separate").double() - a.double()).abs()
            if bool((diff > 0).any()):
                _, self.extra = conv_reference(diff, self.w, torch.zeros_like(self.bias), p.stride, p.pad)
        self.ref = act_of(self.pre, L.act).reshape(self.M, i.cout)
        self.bound = bound_of(self.pre, self.A, self.extra, kt_of(i) * 32, L.act, i.dt).reshape(self.M, i.cout)
        assert bool(torch.isfinite(self.ref).all()) and self.M > 0

    def err(self, y: torch.Tensor) -> torch.Tensor:
        return (y.double().reshape(self.M, -1) - self.ref).abs()


@functools.lru_cache(maxsize=8)
def case(L: Launch) -> Case:
    return Case(L)


def describe_instance(i: Instance) -> str:
    return (f"{'stem_rows_kernel' if i.kernel == 'rows' else 'stem_kernel'}<in {i.in_kind}, {i.KW}x{i.KW}, cout {i.cout}, "
            f"{'generic' if i.generic else 'folded'}, {'fp16' if i.dt else 'bf16'}>")


def describe(L: Launch) -> str:
    p = L.prob
    return (f"{describe_instance(L.inst)} B {p.B} {p.H}x{p.W} s{p.stride} pad {p.pad} {L.kind} act {L.act} "
            f"ldy +{L.ldy_extra} off {L.off}")


# ---------------------------------------------------------------------------------------------
# the launch matrix

FIVE = [(32, False, 0), (32, True, 0), (64, False, 0), (64, True, 0), (64, True, 1)]     # (cout, generic, dt)
V3 = [Problem(1, 3, 3, 2, 0),        # M = 1
      Problem(1, 4, 5, 2, 0),        # an even side: the last row is unused
      Problem(2, 9, 7, 2, 0),        # M = 24: the image boundary falls inside a fragment
      Problem(3, 33, 21, 2, 0),      # M = 480: 3.75 blocks
      Problem(1, 17, 33, 2, 0),      # M = 128 exactly
      Problem(1, 7, 87, 2, 0)]       # M = 129
P3 = [Problem(1, 1, 1, 2, 1), Problem(1, 2, 5, 2, 1), Problem(1, 6, 5, 2, 1), Problem(3, 12, 9, 2, 1)]
S1 = [Problem(1, 5, 4, 1, 1)]        # stride is an argument the launcher accepts
P7 = [Problem(1, 2, 2, 2, 3),        # smaller than the padding; 12 bytes: byte-wise reads at both ends
      Problem(1, 7, 8, 2, 3),
      Problem(2, 13, 9, 2, 3),
      Problem(3, 30, 23, 2, 3),      # M = 540
      Problem(1, 1, 40, 2, 3)]       # a single row, long enough for the aligned path
V7 = [Problem(1, 7, 8, 2, 0), Problem(2, 13, 9, 2, 0), Problem(3, 30, 23, 2, 0)]
UNALIGNED = {3: Problem(2, 9, 7, 2, 0), 7: Problem(2, 13, 9, 2, 3)}


def instances():
    out = [Instance("stem", in_kind, KW, *f) for in_kind in (0, 1) for KW in (3, 7) for f in FIVE]
    return out + [Instance("rows", 0, KW, *f) for KW in (3, 7) for f in FIVE]


def problems(inst: Instance):
    if not inst.generic:               # pad 0 is what makes an instance non-generic
        return V3 if inst.KW == 3 else V7
    return V3 + P3 + S1 if inst.KW == 3 else P7 + V7[1:2]


@functools.lru_cache(maxsize=None)
def launches(kernel: str, KW: int):
    """Every instance of (kernel, KW) on every problem it can run. Kind, activation and the output
    stride rotate with the instance and the problem: each instance meets every kind, ldy = cout and
    cout + 8, and the cout-64 generic ones SiLU and no activation as well as ReLU."""
    out = []
    for i, inst in enumerate(x for x in instances() if x.kernel == kernel and x.KW == KW):
        for n, prob in enumerate(problems(inst)):
            act = [1, 2, 0][(i + n) % 3] if inst.cout == 64 and inst.generic else 1
            out.append(Launch(inst, prob, KINDS[(i + 2 * n) % 3], act, 8 * ((i + n) % 2), 0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def unaligned_launches():
    """stem_rows_kernel with the image 1, 2 and 3 bytes into its buffer (the engine hands it image k
    of a batch of 299 x 299 x 3 bytes): (aligned launch, [the three moved ones])."""
    out = []
    for i, inst in enumerate(x for x in instances() if x.kernel == "rows"):
        prob = UNALIGNED[inst.KW]
        if prob.pad and not inst.generic:
            continue
        base = Launch(inst, prob, KINDS[i % 3], 1, 8 * (i % 2), 0)
        out.append((base, [base._replace(off=o) for o in (1, 2, 3)]))
    return tuple(out)


def all_launches():
    return [L for k in ("stem", "rows") for KW in (3, 7) for L in launches(k, KW)]


# ---------------------------------------------------------------------------------------------
# CPU emulation: the kernels' addressing and rounding points in float32

def gather(L: Launch, variant: str = ""):
    """(idx, valid, ow, OW): idx int64 and valid bool [M][KH][KW][3], the flat element each k slot
    reads and whether the kernel keeps it; ow [M] the output column of each pixel. Variants: 'swap_hw' strides the rows by H; 'no_boundary' takes the image of a
    16-row fragment's first pixel for all of its rows."""
    i, p = L.inst, L.prob
    K = i.KW
    OH, OW = out_size(p.H, K, p.stride, p.pad), out_size(p.W, K, p.stride, p.pad)
    M = p.B * OH * OW
    m = np.arange(M)
    b = (m // 16 * 16 if variant == "no_boundary" else m) // (OH * OW)
    rem = m - b * OH * OW
    oh, ow = rem // OW, rem % OW
    ih = (oh * p.stride - p.pad)[:, None, None, None] + np.arange(K)[None, :, None, None]
    iw = (ow * p.stride - p.pad)[:, None, None, None] + np.arange(K)[None, None, :, None]
    c = np.arange(3)[None, None, None, :]
    valid = np.broadcast_to((ih >= 0) & (ih < p.H) & (iw >= 0) & (iw < p.W), (M, K, K, 3))
    rowlen = p.H if variant == "swap_hw" else p.W
    idx = ((b[:, None, None, None] * p.H * p.W + ih * rowlen + iw) * 3 + c)
    if not i.generic:
        valid = np.ones_like(valid)
    total = p.B * p.H * p.W * 3
    return torch.from_numpy(np.mod(idx, total)), torch.from_numpy(valid.copy()), ow, OW


def emulate(L: Launch, variant: str = "") -> torch.Tensor:
    """[M][cout] in the output type. The operand conversion, the K order of the layout (fp32
    products summed one after the other over the padded K), the bias, the activation and the
    output rounding of a correct kernel; or one of the known-bad variants:
    'lost_tap'    tap (KH/2, KW-1) is missing in the last output column;
    'pad_shift'   a padded tap holds a raw 0 pixel, i.e. shift, instead of 0;
    'channel'     scale / shift of the wrong channel;
    'swap_hw'     H and W swapped in the address;
    'truncate'    a truncating conversion of the A operand;
    'no_boundary' the image boundary ignored inside a fragment;
    'separate'    raw * scale + shift without contraction (a correct kernel too)."""
    i, p = L.inst, L.prob
    img, w, bias = inputs(L.kind, p, i.KW, i.cout, i.generic, i.dt, i.in_kind)
    a = a_operand(img, i.generic, i.dt, variant if variant in ("channel", "truncate", "separate") else "")
    idx, valid, ow, OW = gather(L, variant if variant in ("swap_hw", "no_boundary") else "")
    cols = a.reshape(-1)[idx]
    fill = torch.zeros(3)
    if variant == "pad_shift" and i.generic:
        fill = round_dt(torch.tensor(SHIFT, dtype=torch.float32), i.dt)
    cols = torch.where(valid, cols, fill.expand_as(cols))
    if variant == "lost_tap":
        cols[torch.from_numpy(ow == OW - 1), i.KW // 2, i.KW - 1, :] = 0
    M = cols.shape[0]
    if i.kernel == "rows":
        RP = rp_of(i.KW)
        ck = torch.zeros(M, i.KW, RP)
        ck[:, :, :i.KW * 3] = cols.reshape(M, i.KW, i.KW * 3)
        wk = torch.zeros(i.cout, i.KW, RP)
        wk[:, :, :i.KW * 3] = w.reshape(i.cout, i.KW, i.KW * 3)
    else:
        ck, wk = cols, w
    ck, wk = ck.reshape(M, -1), wk.reshape(i.cout, -1)
    prod = (ck.double()[:, None, :] * wk.double()[None, :, :]).float()        # exact: 8 or 11 bit factors
    acc = torch.cumsum(prod, 2, dtype=torch.float32)[:, :, -1]
    f = acc + bias
    f = torch.relu(f) if L.act == 1 else _silu32(f) if L.act == 2 else f
    assert f.dtype == torch.float32
    return f.to(DTYPES[i.dt])


def rows_windows(L: Launch):
    """stem_rows_kernel's window addressing, lane by lane, over a byte buffer that holds the image
    L.off bytes in: rq, ky, the aligned 12-byte load + alignbyte or the byte-wise path, the rv / iw
    masks. Returns (raw [M][KT*32] uint8 as the kernel would convert it, keep [M][KT*32] bool,
    lowest and highest byte read relative to x, aligned windows, byte-wise windows before x,
    byte-wise windows past the end)."""
    i, p = L.inst, L.prob
    assert i.kernel == "rows" and i.in_kind == 0
    img = inputs(L.kind, p, i.KW, i.cout, i.generic, i.dt, 0)[0]
    KH = KW = i.KW
    RP, RUN = rp_of(KW), KW * 3
    OH, OW = out_size(p.H, KH, p.stride, p.pad), out_size(p.W, KW, p.stride, p.pad)
    M, KT = p.B * OH * OW, (KH * RP + 31) >> 5
    total = p.B * p.H * p.W * 3
    pre_pad = 64
    buf = np.full(pre_pad + L.off + total + 64, 0xA5, dtype=np.uint8)
    x0 = pre_pad + L.off                                   # buf[x0] is x[0]
    buf[x0:x0 + total] = img.reshape(-1).numpy()
    m = np.arange(M)
    b = m // (OH * OW)
    rem = m - b * OH * OW
    oh, ow = rem // OW, rem % OW
    ih0, iw0 = oh * p.stride - p.pad, ow * p.stride - p.pad
    rbase = (b * p.H * p.W + iw0) * 3
    raw = np.zeros((M, KT * 32), dtype=np.uint8)
    keep = np.zeros((M, KT * 32), dtype=bool)
    lo, hi, n_al, n_before, n_past = total, -1, 0, 0, 0
    j = np.arange(8)
    for ks in range(KT):
        for q in range(4):
            ky, rq = (ks * 32 + 8 * q) // RP, (8 * q) % RP
            ih = ih0 + ky
            row_ok = (ky < KH) & (ih >= 0) & (ih < p.H) & (rq < RUN)
            p0 = rbase + ih * p.W * 3 + rq
            al = p0 & ~3
            aligned = row_ok & (al >= 0) & (al + 12 <= total)
            bytewise = row_ok & ~aligned
            win = np.zeros((M, 8), dtype=np.uint8)
            if aligned.any():
                a_ = al[aligned]
                lo, hi = min(lo, int(a_.min())), max(hi, int(a_.max()) + 11)
                d = buf[x0 + a_[:, None] + np.arange(12)[None, :]]          # d0, d1, d2
                sh = (p0[aligned] - a_)[:, None]
                win[aligned] = np.take_along_axis(d, sh + j[None, :], 1)    # alignbyte(d1, d0, sh), (d2, d1, sh)
                n_al += int(aligned.sum())
            if bytewise.any():
                pj = p0[bytewise][:, None] + j[None, :]
                inside = (pj >= 0) & (pj < total)
                if inside.any():
                    lo, hi = min(lo, int(pj[inside].min())), max(hi, int(pj[inside].max()))
                win[bytewise] = np.where(inside, buf[x0 + np.clip(pj, 0, total - 1)], 0)
                n_before += int((al[bytewise] < 0).sum())
                n_past += int((al[bytewise] + 12 > total).sum())
            r = rq + j
            ok = row_ok[:, None] & (r < RUN)[None, :]
            if i.generic:
                iw = iw0[:, None] + (r // 3)[None, :]
                ok = ok & (iw >= 0) & (iw < p.W)
            k = ks * 32 + 8 * q
            raw[:, k:k + 8] = np.where(ok, win, 0)
            keep[:, k:k + 8] = ok
    return raw, keep, lo, hi, n_al, n_before, n_past


def rows_gather_reference(L: Launch):
    """(raw, keep) [M][KT*32] straight from the image: slot ky*RP + kx*3 + c holds pixel
    (b, oh*s - pad + ky, ow*s - pad + kx, c) where that is inside the image."""
    i, p = L.inst, L.prob
    img = inputs(L.kind, p, i.KW, i.cout, i.generic, i.dt, 0)[0].numpy()
    K, RP = i.KW, rp_of(i.KW)
    OH, OW = out_size(p.H, K, p.stride, p.pad), out_size(p.W, K, p.stride, p.pad)
    M, KT = p.B * OH * OW, (K * RP + 31) >> 5
    raw = np.zeros((M, KT * 32), dtype=np.uint8)
    keep = np.zeros((M, KT * 32), dtype=bool)
    for m in range(M):
        b, rem = divmod(m, OH * OW)
        oh, ow = divmod(rem, OW)
        for ky in range(K):
            ih = oh * p.stride - p.pad + ky
            if not 0 <= ih < p.H:
                continue
            for kx in range(K):
                iw = ow * p.stride - p.pad + kx
                if 0 <= iw < p.W:
                    k = ky * RP + kx * 3
                    raw[m, k:k + 3] = img[b, ih, iw]
                    keep[m, k:k + 3] = True
    return raw, keep
