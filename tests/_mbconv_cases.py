"""Inputs, float64 references, error bounds, CPU emulations and the launch matrix of the MBConv
operator tests (dwk_kernel, dwv_kernel, se_kernel, chscale_kernel of dwconv_k.hip).

Every input is rounded to its storage format first (x to bf16; weights and biases are fp32) and
every reference is computed in float64 from the rounded values, so a bound only has to cover what
a kernel itself does. The bounds are derived from the number formats, per element; nothing in
them is measured. tests/test_mbconv_ops_cpu.py shows that an fp32 emulation of a correct kernel
fits them and that the known-bad variants do not; tests/test_mbconv_ops_gpu.py holds the kernels
to them."""
import functools

import torch
import torch.nn.functional as F

from _vit_cases import GUARD, SENTINEL16, guarded, guards_intact, within  # noqa: F401  (re-exported)

U32 = 2.0 ** -24          # fp32: half a unit in the last place, relative
U16 = 2.0 ** -8           # bf16 round-to-nearest, the same
TINY = 2.0 ** -126        # smallest normal fp32 / bf16: what a flush to zero may cost


def ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max of err / bound for messages: nan if any err is NaN, 0 / 0 counts as 0, x / 0 as inf."""
    if bool(torch.isnan(err).any()) or bool(torch.isnan(bound).any()):
        return float("nan")
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")),
                                                         torch.zeros_like(err)))
    return float(r.max())


def share_over(err: torch.Tensor, bound: torch.Tensor) -> float:
    return float((~(err <= bound)).double().mean())


def out_size(n: int, K: int, S: int) -> int:
    pad = (K - 1) // 2
    return (n + 2 * pad - K) // S + 1


# ---------------------------------------------------------------------------------------------
# depthwise: inputs

KINDS = ["benign", "neg", "big", "cancel"]
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
MAPS = [(1, 1), (2, 9), (7, 10), (12, 11)]     # every tap but the centre padding; H < K; even W at stride 2; ragged
CS_ROT = [1, 3, 20, 260]                       # squeeze widths: one unit .. more than the 256 threads


def dw_inputs(kind: str, B: int, H: int, W: int, C: int, K: int, S: int, Cs: int):
    """x [B][H][W][C] bf16, w [K*K][C], bias [C], w1 [Cs][C] fp32."""
    gen = torch.Generator().manual_seed(7919 * H + 613 * W + 31 * C + 5 * K + S + 1009 * B + 17 * KINDS.index(kind))
    x = torch.randn(B, H, W, C, generator=gen)
    w = torch.randn(K * K, C, generator=gen) / K
    bias = torch.randn(C, generator=gen) * 0.1
    if kind == "neg":          # __expf(-v) overflows, rcp gives 0: the output is -0 or far below 1
        bias = bias - torch.where(torch.arange(C) % 2 == 0, 60.0, 100.0)
    elif kind == "big":        # pre-activations up to +-200
        x = x * 40
    elif kind == "cancel":     # every channel's taps sum to zero exactly: A >> |pre| away from the border
        x = 3 + 0.01 * x
        w = torch.round(w * 1024) / 1024
        w[-1] = -w[:-1].sum(0)
        assert bool((w.double().sum(0) == 0).all())
    w1 = torch.randn(Cs, C, generator=gen) / C ** 0.5
    return x.to(torch.bfloat16), w.float().contiguous(), bias.float().contiguous(), w1.float().contiguous()


def _taps(x: torch.Tensor, K: int, S: int, shift: int = 0):
    """(dy, dx, strided view of the padded x that tap (dy, dx) multiplies) for every tap, in the
    kernels' accumulation order. shift > 0 moves the padding towards the top / left (a broken variant)."""
    B, H, W, C = x.shape
    pad = (K - 1) // 2
    OH, OW = out_size(H, K, S), out_size(W, K, S)
    far = pad + S + K
    xp = F.pad(x, (0, 0, pad + shift, far, pad + shift, far))
    for dy in range(K):
        for dx in range(K):
            yield dy, dx, xp[:, dy:dy + S * (OH - 1) + 1:S, dx:dx + S * (OW - 1) + 1:S]


def dw_reference(x, w, bias, K: int, S: int):
    """float64 (pre, A): pre = conv(x, w) + bias, A = conv(|x|, |w|) + |bias|."""
    xd, wd, bd = x.double(), w.double(), bias.double()
    pre, A = None, None
    for (dy, dx, v), (_, _, va) in zip(_taps(xd, K, S), _taps(xd.abs(), K, S)):
        t = dy * K + dx
        pre = v * wd[t] if pre is None else pre + v * wd[t]
        A = va * wd[t].abs() if A is None else A + va * wd[t].abs()
    return pre + bd, A + bd.abs()


def dw_act(pre: torch.Tensor, act: int) -> torch.Tensor:
    return pre * torch.sigmoid(pre) if act == 2 else pre


def dw_bound(pre, A, K: int, act: int):
    """K*K fused multiply-adds and the bias add in fp32 (d); with SiLU, |silu'| <= 1.1, the exp,
    rcp and mul roundings, and the rounding of the scaled exp argument; then the bf16 rounding of
    a value that may be d away from y; 2^-126 for a result flushed to zero."""
    y = dw_act(pre, act)
    d = (K * K + 2) * U32 * A
    if act == 2:
        d = 1.1 * d + 8 * U32 * y.abs() + U32 * pre.abs() * y.abs()
    return d + U16 * (y.abs() + d) + TINY


def _fma32(a, b, c):
    """float32 fma: the product of two floats is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _silu32(v: torch.Tensor) -> torch.Tensor:
    """fast_silu in float32: v * rcp(1 + exp(-v)); exp overflows to inf and the quotient to 0."""
    return v * (1.0 / (1.0 + torch.exp(-v)))


def truncate_bf16(f: torch.Tensor) -> torch.Tensor:
    """float32 -> bf16 by dropping the low 16 bits (the broken conversion)."""
    return (f.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def dw_emulate(x, w, bias, K: int, S: int, act: int, variant: str = "", rounded: bool = True):
    """The kernels' arithmetic in float32: one fma per tap in (dy, dx) order, the bias add, the
    fast SiLU, round-to-nearest bf16. Variants, each a bug a kernel could have:
    'lost_tap'  tap (K/2, 0) is missing in the last output column only;
    'pad_shift' the padding sits one pixel further towards the top / left;
    'truncate'  the bf16 conversion truncates.
    rounded=False returns the float32 values before the conversion."""
    xf = x.float()
    acc = None
    for dy, dx, v in _taps(xf, K, S, shift=1 if variant == "pad_shift" else 0):
        wt = w[dy * K + dx]
        if variant == "lost_tap" and dy == K // 2 and dx == 0:
            v = v.clone()
            v[:, :, -1] = 0
        acc = _fma32(v, wt, torch.zeros_like(v) if acc is None else acc)
    f = acc + bias
    if act == 2:
        f = _silu32(f)
    assert f.dtype == torch.float32
    if not rounded:
        return f
    return truncate_bf16(f) if variant == "truncate" else f.to(torch.bfloat16)


class DwCase:
    """One depthwise problem with its float64 reference; read-only once built."""

    def __init__(self, kind, B, H, W, C, K, S, Cs):
        self.key = (kind, B, H, W, C, K, S, Cs)
        self.kind, self.B, self.H, self.W, self.C, self.K, self.S, self.Cs = self.key
        self.pad = (K - 1) // 2
        self.OH, self.OW = out_size(H, K, S), out_size(W, K, S)
        self.x, self.w, self.bias, self.w1 = dw_inputs(kind, B, H, W, C, K, S, Cs)
        self.pre, self.A = dw_reference(self.x, self.w, self.bias, K, S)
        assert bool(torch.isfinite(self.pre).all()) and bool(torch.isfinite(dw_act(self.pre, 2)).all())

    def ref(self, act: int):
        return dw_act(self.pre, act)

    def bound(self, act: int):
        return dw_bound(self.pre, self.A, self.K, act)

    def geom(self) -> dict:
        return dict(B=self.B, H=self.H, W=self.W, C=self.C, OH=self.OH, OW=self.OW, K=self.K, S=self.S,
                    pad=self.pad, Cs=self.Cs)


@functools.lru_cache(maxsize=24)
def dw_case(kind, B, H, W, C, K, S, Cs) -> DwCase:
    return DwCase(kind, B, H, W, C, K, S, Cs)


# ---------------------------------------------------------------------------------------------
# depthwise: the fused pool

def pool_reference(y_stored: torch.Tensor, w1: torch.Tensor, nparts: int):
    """float64 (ref [B][Cs], bound): sum_c w1[j][c] * sum_pixels y_stored, from the bf16 output
    as stored; fp32 sums over the pixels, the channels and (were the parts summed in fp32) the parts."""
    B, OH, OW, C = y_stored.shape
    yd = y_stored.double()
    w1d = w1.double()
    ref = yd.sum((1, 2)) @ w1d.t()
    bound = (OH * OW + C + nparts) * U32 * (yd.abs().sum((1, 2)) @ w1d.abs().t())
    return ref, bound


def pool_emulate(y: torch.Tensor, w1: torch.Tensor, rows_per_part: int) -> torch.Tensor:
    """pool [B][nparts][Cs] in float32 with sequential sums: a part is a band of output rows;
    y is what the kernel summed (the stored bf16 values; fp32 in the broken variant)."""
    B, OH, OW, C = y.shape
    parts = []
    for h0 in range(0, OH, rows_per_part):
        px = y[:, h0:h0 + rows_per_part].float().reshape(B, -1, C)
        cs = torch.cumsum(px, 1, dtype=torch.float32)[:, -1]                    # [B][C], in order
        h = torch.zeros(B, w1.shape[0])
        for c in range(C):
            h = _fma32(cs[:, c:c + 1], w1[None, :, c], h)
        parts.append(h)
    return torch.stack(parts, 1)


# ---------------------------------------------------------------------------------------------
# depthwise: the launch matrix (what tests/test_mbconv_ops_gpu.py runs, and what
# tests/test_mbconv_ops_cpu.py proves the bounds on)

DWV_CB = [8, 16, 32, 64, 24, 36, 40, 48]
DWV_SEG = [2, 4]
DWV_PD = [1, 3]
DWV_RB = [1, 5, 64, 0]            # one row; divides none of 12, 7, 6; >= OH; the plan's own
DWT_SEG = [3, 4, 5, 7, 8]
DWT_CG = [1, 2, 4, 8]
DWT_RB = [1, 5, 3, 12]
DWT_TW = [4, 16]                  # ragged last tile at OW 5, 6, 10, 11; >= OW
ACTS = [2, 0]


def _rot_cases(K, S, unit: int, i: int, one_block: bool = True):
    """The five problems of chunk width ``unit`` channels: the four maps with one channel block
    (two where one block is no multiple of 32 channels) and the ragged map with two. Kind, batch
    and squeeze width rotate with the map and the width index i, so that every instance meets
    every kind and both batch sizes."""
    out = []
    for m, (H, W) in enumerate(MAPS + [MAPS[-1]]):
        C = unit if (m < len(MAPS) and one_block) else 2 * unit
        out.append(dw_key(KINDS[(i + m) % 4], 1 + 2 * ((i + m) % 2), H, W, C, K, S, CS_ROT[(i + m + 1) % 4]))
    return out


def dw_key(kind, B, H, W, C, K, S, Cs):
    return (kind, B, H, W, C, K, S, Cs)


def dwv_launches(K: int, S: int):
    """Direct kernel: every SEG x CB x PD x act instance of (K, S) on five problems each, then
    the wide maps whose segments outnumber the 32 segment lanes of CB 8 / SEG 2 (nsb > 1).
    Yields (case key, overrides, act)."""
    for i, CB in enumerate(DWV_CB):
        cases = _rot_cases(K, S, 4 * CB, i, one_block=(4 * CB) % 32 == 0)
        inst = 0
        for seg in DWV_SEG:
            for pd in DWV_PD:
                for act in ACTS:
                    for m, key in enumerate(cases):
                        yield key, dict(algo=2, cg=CB, seg=seg, pd=pd, rb=DWV_RB[(inst + m) % 4]), act
                    inst += 1
    H, W = (4, 70) if S == 1 else (3, 140)
    n = 0
    for pd in DWV_PD:
        for act in ACTS:
            key = dw_key(KINDS[n % 4], 1 + 2 * (n % 2), H, W, 32, K, S, CS_ROT[n % 4])
            yield key, dict(algo=2, cg=8, seg=2, pd=pd, rb=DWV_RB[(n + 1) % 4]), act
            n += 1


def dwt_launches(K: int, S: int):
    """Tiled kernel: every SEG x CG x act instance of (K, S) on five problems each, with ragged
    and oversized row bands and column tiles; at K 5 / S 1 one patch of more than 2048 staged
    vectors and 256 items. Yields (case key, overrides, act)."""
    for i, CG in enumerate(DWT_CG):
        cases = _rot_cases(K, S, 8 * CG, i)
        for si, seg in enumerate(DWT_SEG):
            for ai, act in enumerate(ACTS):
                inst = si * 2 + ai
                for m, key in enumerate(cases):
                    yield key, dict(algo=1, cg=CG, seg=seg, rb=DWT_RB[(inst + m) % 4],
                                    tw=DWT_TW[(si + ai + m) % 2]), act
    if (K, S) == (5, 1):
        for seg, act in ((3, 2), (4, 0)):      # 12 x 23 x 8 = 2208 vectors; 8 x 8 x ceil(19 / seg) >= 320 items
            yield dw_key("benign", 1, 24, 23, 64, K, S, 20), dict(algo=1, cg=8, rb=8, tw=19, seg=seg), act


def dwt_fallback_launches(K: int, S: int):
    """The tiled kernel's own tile choice: no overrides, with and without an LDS budget."""
    for n, (H, W, C) in enumerate([(12, 11, 64), (24, 23, 72)]):
        for li, lds in enumerate((0, 8)):
            key = dw_key(KINDS[(2 * n + li) % 4], 3 - 2 * n, H, W, C, K, S, CS_ROT[(n + 1) % 4])
            yield key, dict(algo=1, lds_kb=lds), 2


def instance_key(K, S, over: dict, act: int):
    """(K, S, algo, seg, CB or CG, pd, act) of a launch with explicit overrides."""
    return (K, S, over["algo"], over["seg"], over["cg"], over.get("pd", 0), act)


@functools.lru_cache(maxsize=None)
def matrix_keys() -> frozenset:
    keys = set()
    for K, S in KS:
        for gen in (dwv_launches, dwt_launches):
            keys.update(instance_key(K, S, over, act) for _, over, act in gen(K, S))
    return frozenset(keys)


def all_case_keys(K: int, S: int):
    """Every distinct problem of (K, S), in launch order (neighbours share a problem)."""
    seen, out = set(), []
    for gen in (dwv_launches, dwt_launches, dwt_fallback_launches):
        for key, _, _ in gen(K, S):
            if key not in seen:
                seen.add(key)
                out.append(key)
    return out


# ---------------------------------------------------------------------------------------------
# squeeze-excite tail

SE_CS = [1, 20, 160, 256, 257, 300]            # the last two take se_kernel's Cs > 256 branch
SE_C = [8, 264, 520]                           # the last 256-channel slice is ragged
SE_B = [1, 3]


def se_ntiles(Cs: int):
    """1; one fewer than the G = 256 / Cs thread groups; no multiple of G; several hundred.
    (Not thousands: the worst case of an fp32 sum of n terms is n^2 u32 times their mean size,
    which from n = 1000 on is a tenth of one term, and a lost part would begin to fit the bound.)"""
    G = 256 // Cs if Cs <= 256 else 1
    return sorted({1, max(1, G - 1), G + max(1, G // 2), 333})


def se_inputs(B: int, ntiles: int, C: int, Cs: int, HW: int = 132, logit: float = 0.0):
    """pool [B][ntiles][Cs], b1 [Cs], w2t [Cs][C], b2 [C] fp32. The pooled mean is of order one,
    so a part lost or counted twice moves it by about 1 / sqrt(ntiles). logit: b2 = -+logit by channel."""
    gen = torch.Generator().manual_seed(1000 * Cs + 10 * C + ntiles + B)
    pool = torch.randn(B, ntiles, Cs, generator=gen) * (HW / ntiles ** 0.5) + 0.25 * HW / ntiles
    b1 = torch.randn(Cs, generator=gen) * 0.1
    w2t = torch.randn(Cs, C, generator=gen) / Cs ** 0.5
    b2 = torch.randn(C, generator=gen) * 0.1
    if logit:
        w2t = w2t * 0.01
        b2 = b2 + torch.where(torch.arange(C) % 2 == 0, -logit, logit)
    return pool.float(), b1.float(), w2t.float().contiguous(), b2.float()


def se_reference(pool, b1, w2t, b2, HW: int):
    """float64 (scale [B][C], bound). The bound, stage by stage:
    h = sum of ntiles fp32 terms: every term passes through at most ntiles roundings;
    a = h / HW + b1: the reciprocal, the product and the sum round once each;
    hid = silu(a): |silu'| <= 1.1, the exp, rcp and mul roundings, the scaled exp argument;
    s = b2 + sum of Cs fp32 products; scale = sigmoid(s): |sigmoid'| <= 1/4, the same three
    kinds of rounding, and 2^-126 for a quotient flushed to zero."""
    B, nt, Cs = pool.shape
    pd = pool.double()
    h, ha = pd.sum(1), pd.abs().sum(1)
    a = h / HW + b1.double()
    da = (nt + 3) * U32 * ha / HW + U32 * a.abs()
    hid = a * torch.sigmoid(a)
    dh = 1.1 * da + 8 * U32 * hid.abs() + U32 * a.abs() * hid.abs()
    w2d, b2d = w2t.double(), b2.double()
    s = hid @ w2d + b2d
    ds = dh @ w2d.abs() + (Cs + 1) * U32 * (hid.abs() @ w2d.abs() + b2d.abs())
    ref = torch.sigmoid(s)
    return ref, 0.25 * ds + 8 * U32 * ref + U32 * s.abs() * ref + TINY


def se_emulate(pool, b1, w2t, b2, HW: int, variant: str = "") -> torch.Tensor:
    """se_kernel in float32 with sequential sums. Variants: 'drop' loses the last part, 'twice'
    counts it twice, 'no_hw' forgets the 1 / HW."""
    p = pool
    if variant == "drop":
        p = pool[:, :-1] if pool.shape[1] > 1 else pool * 0
    elif variant == "twice":
        p = torch.cat([pool, pool[:, -1:]], 1)
    h = torch.cumsum(p, 1, dtype=torch.float32)[:, -1]
    inv = torch.tensor(1.0 if variant == "no_hw" else 1.0 / HW, dtype=torch.float32)
    hid = _silu32(h * inv + b1)
    s = b2[None, :].expand(pool.shape[0], -1)
    for j in range(pool.shape[2]):
        s = _fma32(w2t[j][None, :], hid[:, j:j + 1], s)
    return 1.0 / (1.0 + torch.exp(-s))


# ---------------------------------------------------------------------------------------------
# channel scale

CHS_SHAPES = [(hw, 8) for hw in (255, 256, 257, 767, 768, 769)] + [(7, 264), (31, 264), (97, 520)]   # (HW, C)


def chscale_inputs(B: int, HW: int, C: int):
    """y [B][HW][C] bf16 and scale [B][C] fp32 with 0, 1, -1 and negative values; every product is
    zero or a normal number."""
    gen = torch.Generator().manual_seed(HW * 1000 + C + B)
    y = (torch.randn(B, HW, C, generator=gen) * 3).to(torch.bfloat16)
    scale = torch.randn(B, C, generator=gen)
    scale[:, 0], scale[:, 1], scale[:, 2], scale[:, 3] = 0.0, 1.0, -1.0, -0.37
    return y, scale.float()


def chscale_expected(y, scale) -> torch.Tensor:
    """One fp32 multiply, one round-to-nearest-even conversion: exact."""
    return (y.float() * scale[:, None, :]).to(torch.bfloat16)
