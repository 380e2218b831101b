"""Inputs, float64 references, error bounds and CPU emulations for the ViT operator tests
(attention, LayerNorm, patchify, token embedding, GELU / SiLU epilogue).

Every generator rounds its values to bf16 first; every reference is computed in float64 from
the rounded values, so a bound only has to cover what the kernel itself does. The emulations
repeat a kernel's rounding points (or its exact summation order) in float32 on the CPU:
tests/test_vit_ops_cpu.py uses them to show that a correct kernel fits the bounds and that the
known-bad variants do not."""
import functools
import math

import numpy as np
import torch

DH = 64
LOG2E = 1.4426950408889634
U8 = 2.0 ** -8            # bf16: half a unit in the last place, relative
U8P = U8 * (1 + 2.0 ** -6)
GUARD = 4                 # guard rows before and after every buffer a kernel touches


def bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16)


def within(err: torch.Tensor, bound: torch.Tensor) -> bool:
    """err <= bound everywhere; a NaN on either side is a miss."""
    return bool((err <= bound).all())


def worst(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max of err / bound (nan if any err is NaN), for messages."""
    r = err / bound
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


SENTINEL16 = 0x5A5A        # as bf16: 1.5e16, nothing a kernel under test would write
SENTINEL8 = 0x5A


def guarded(rows: int, ld: int, dtype, fill, device="cpu"):
    """[GUARD + rows + GUARD][ld] filled with ``fill``; returns (whole buffer, the middle rows)."""
    buf = torch.full((rows + 2 * GUARD, ld), fill, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf: torch.Tensor, used_cols: int, fill) -> bool:
    """The guard rows of a ``guarded`` buffer, and the columns from ``used_cols`` on of its
    middle rows, still hold ``fill`` bit for bit."""
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all()
                and (buf[GUARD:-GUARD, used_cols:] == fill).all())


# ---------------------------------------------------------------------------------------------
# attention

ATTN_LAYOUTS = [(1, 1), (2, 3)]                      # (B, H); H != 12 moves the q / k / v offsets
ATTN_T = {1: [1, 15, 16, 17, 63, 64, 65, 128, 129, 197, 255, 256],      # whole-head kernel
          2: [1, 17, 64, 65, 197, 256, 257, 320, 321],                  # query-tiled kernel
          0: [197, 300]}                                                # the launcher's own choice
ATTN_KINDS = ["benign", "peaked", "offset", "negative"]
ATTN_F8_T = [65, 197, 257]
ATTN_F8_KINDS = ["benign", "peaked"]
ATTN_INV_SCALE = (16.0, 200.0)                       # nothing saturates / most of the output does
SCALE = 1.0 / math.sqrt(DH)


def attn_qkv(kind: str, B: int, T: int, H: int) -> torch.Tensor:
    """qkv [B*T][3*H*64] bf16. V = randn + 3 in every kind, so softmax mass that is lost or
    leaks to a padded key moves the output. The scores of 'offset' and 'negative' are -+128 with
    a standard deviation of 5.7, so the extreme of a few hundred thousand of them comes within
    a unit or two of the ranges those kinds promise: a draw that misses its range is drawn again
    (at most 7 times), and the range is asserted on what is returned."""
    for redraw in range(8):
        gen = torch.Generator().manual_seed(1000 * T + 10 * H + B + 7 * ATTN_KINDS.index(kind) + 1000003 * redraw)
        q, k, v = (torch.randn(B * T, H * DH, generator=gen) for _ in range(3))
        if kind == "peaked":
            q = q * 8
        elif kind == "offset":
            q, k = q + 4, k + 4
        elif kind == "negative":
            q, k = q + 4, k - 4
        qkv = bf16(torch.cat([q, k, v + 3], 1))
        s = attn_scores(qkv, B, T, H)
        lo, hi = float(s.min()), float(s.max())
        if (kind != "offset" or lo * LOG2E > 128) and (kind != "negative" or hi < -100):
            break
    if kind == "offset":       # exp2 of these overflows fp32 unless the row maximum is subtracted
        assert lo * LOG2E > 128, lo
    if kind == "negative":     # a zero-padded key (score 0) that escapes the mask takes all the weight
        assert hi < -100, hi
    return qkv


def _split(qkv: torch.Tensor, B: int, T: int, H: int, dtype):
    q, k, v = qkv.to(dtype).view(B, T, 3, H, DH).permute(2, 0, 3, 1, 4)     # each [B][H][T][DH]
    return q, k, v


def _merge(o: torch.Tensor, B: int, T: int, H: int) -> torch.Tensor:
    return o.transpose(1, 2).reshape(B * T, H * DH)


def attn_scores(qkv, B, T, H) -> torch.Tensor:
    q, k, _ = _split(qkv, B, T, H, torch.float64)
    return q @ k.transpose(-1, -2) * SCALE


def attn_reference(qkv, B, T, H, leak_key: bool = False):
    """(ref, A) float64 [B*T][H*64]: ref = softmax(s) V, A = softmax(s) |V|.
    leak_key: the broken variant whose mask is off by one, so that the first zero-padded key
    (score 0, V = 0) takes part in the softmax."""
    q, k, v = _split(qkv, B, T, H, torch.float64)
    if leak_key:
        z = torch.zeros(B, H, 1, DH, dtype=torch.float64)
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
    p = torch.softmax(q @ k.transpose(-1, -2) * SCALE, -1)
    return _merge(p @ v, B, T, H), _merge(p @ v.abs(), B, T, H)


@functools.lru_cache(maxsize=None)
def attn_case(kind: str, B: int, T: int, H: int):
    """(qkv, ref, A) of one case, computed once for all the tests that use it; treat as read-only."""
    qkv = attn_qkv(kind, B, T, H)
    return (qkv, *attn_reference(qkv, B, T, H))


def attn_bound(ref, A):
    """bf16 output rounding (2^-8 |ref|), P rounded to bf16 before the PV product (2^-8 A),
    fp32 score error below 1e-5."""
    return U8 * (ref.abs() + A) + 1e-6


def attn_emulate(qkv, B, T, H, subtract_max: bool = True) -> torch.Tensor:
    """The kernels' rounding points in float32: scores and the online softmax over 64-key tiles
    in fp32, every p rounded to bf16 for the PV product while l sums the unrounded p, the
    output rounded to bf16. subtract_max=False is the broken variant p = exp2(s) with m = 0."""
    q, k, v = _split(qkv, B, T, H, torch.float32)
    sl2 = np.float32(SCALE) * np.float32(LOG2E)
    m = torch.full((B, H, T, 1), -math.inf)
    l = torch.zeros(B, H, T, 1)
    o = torch.zeros(B, H, T, DH)
    for k0 in range(0, T, 64):
        s = (q @ k[:, :, k0:k0 + 64].transpose(-1, -2)) * sl2
        mn = torch.maximum(m, s.amax(-1, keepdim=True)) if subtract_max else torch.zeros_like(m)
        alpha = torch.exp2(m - mn) if subtract_max else torch.ones_like(m)
        p = torch.exp2(s - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + bf16(p).float() @ v[:, :, k0:k0 + 64]
        m = mn
    return bf16(_merge(o / l, B, T, H))


def f8_bound(z, extra):
    """e4m3 half-step for normals (2^-4 |z|) and subnormals (2^-10), plus ``extra``."""
    return 2.0 ** -4 * z.abs() + 2.0 ** -10 + extra


def f8_check(byte: torch.Tensor, ref: torch.Tensor, inv_scale: float, extra: torch.Tensor, saturating: bool, tag=""):
    """byte: uint8 e4m3 output on the CPU, ref: float64. The bound, the saturation bytes and
    the absence of NaN bytes."""
    from kdl.ops.f8 import from_e4m3
    t = ref * inv_scale
    if saturating:
        assert float((t.abs() > 480).double().mean()) >= 0.01, (tag, "inputs do not saturate")
    else:
        assert float(t.abs().max()) < 448, (tag, "inputs saturate")
    assert not bool(((byte & 0x7F) == 0x7F).any()), (tag, "NaN byte in the e4m3 output")
    z = t.clamp(-448, 448)
    d = from_e4m3(byte.contiguous()).double()
    bound = f8_bound(z, extra)
    assert within((d - z).abs(), bound), (tag, worst((d - z).abs(), bound))
    sat = t.abs() > 480
    want = torch.where(t > 0, 0x7E, 0xFE).to(torch.uint8)
    assert bool((byte[sat] == want[sat]).all()), (tag, "a saturated value is not +-448")


# ---------------------------------------------------------------------------------------------
# LayerNorm

LN_D = [8, 200, 256, 264, 768, 1024, 1032, 2048]     # 1024: last D of layernorm2_kernel, 1032: first of layernorm_kernel
LN_ROWS = [1, 7, 8, 9, 64]
LN_EPS = 1e-6
LN_KINDS = [(0.5, 2), (64, 0.5), (100, 0.5), (300, 1), (-250, 1), (1000, 4), (20, 0.05), (3, 0.01), "const", "zeros"]
LN_F8_D = [200, 768, 1032]
LN_F8_KINDS = [(0.5, 2), (300, 1)]
LN_INV_SCALE = (48.0, 480.0)                         # nothing saturates / a good part of the output does
LN_GAIN_TOL = 2.0 ** -9
LN_GAIN_MIN_D = 200


def ln_strides(D: int):
    return [(ldx, ldy) for ldx in (D, D + 8, 3 * D) for ldy in (D, D + 8)]


def ln_row(kind, D: int, gen) -> torch.Tensor:
    if kind == "const":
        return torch.full((D,), 37.5)
    if kind == "zeros":
        return torch.zeros(D)
    mean, std = kind
    return torch.randn(D, generator=gen) * std + mean


def ln_inputs(D: int, rows: int, kinds=None, first: int | None = None):
    """x [rows][D] bf16 (row i is of kind kinds[(first + i) % len]), gamma, beta fp32, and the
    kind of every row. ``first`` defaults to ``rows``, so the short cases start on different kinds."""
    kinds = LN_KINDS if kinds is None else kinds
    first = rows if first is None else first
    gen = torch.Generator().manual_seed(100 * D + rows)
    rk = [kinds[(first + i) % len(kinds)] for i in range(rows)]
    x = bf16(torch.stack([ln_row(k, D, gen) for k in rk]))
    gamma = torch.rand(D, generator=gen) + 0.5
    beta = torch.randn(D, generator=gen) * 0.1
    return x, gamma, beta, rk


def ln_reference(x, gamma, beta):
    """float64: n (normalised), ref = n gamma + beta, R [rows][1] = max over the row of |n gamma| + |beta|."""
    x, g, b = x.double(), gamma.double(), beta.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    n = (x - mean) / torch.sqrt(var + LN_EPS)
    ref = n * g + b
    R = ((n * g).abs() + b.abs()).amax(1, keepdim=True)
    return n, ref, R


def ln_bound(ref, R):
    """bf16 output rounding, plus fp32 arithmetic at the scale of the row."""
    return U8P * ref.abs() + 2.0 ** -14 * R


def ln_gain(y, n, gamma, beta):
    """Per row, the least-squares gain of (y - beta) against n gamma (nan for a constant row):
    a wrong rstd scales the whole row, which the output rounding alone could hide."""
    t = n * gamma.double()
    den = (t * t).sum(1)
    g = ((y.double() - beta.double()) * t).sum(1) / den
    return torch.where(den > 0, g, torch.full_like(g, math.nan))


def ln_check(y, x, gamma, beta, tag=""):
    """The per-element bound on every row and, from D = 200 on, the gain of every non-constant row."""
    n, ref, R = ln_reference(x, gamma, beta)
    err, bound = (y.double() - ref).abs(), ln_bound(ref, R)
    assert within(err, bound), (tag, "err / bound", worst(err, bound))
    if x.shape[1] >= LN_GAIN_MIN_D:
        g = ln_gain(y, n, gamma, beta)
        g = g[~torch.isnan(g)]
        if g.numel():
            assert float((g - 1).abs().max()) <= LN_GAIN_TOL, (tag, "gain - 1", float((g - 1).abs().max()))


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _fma(a, b, c):
    """float32 fma(a, b, c): the product of two floats is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _ln_lane_sums(t: np.ndarray, lanes: int):
    """Per-lane running sums of t and t^2 in the kernels' order (lane hl owns the 8-element chunks
    hl, hl + lanes, ...; absent chunks add zeros), then the xor butterfly. t: [rows][D] float32."""
    rows, D = t.shape
    nch = -(-D // (8 * lanes))
    pad = np.zeros((rows, nch * lanes * 8), np.float32)
    pad[:, :D] = t
    c = pad.reshape(rows, nch, lanes, 8)
    s = np.zeros((rows, lanes), np.float32)
    ss = np.zeros((rows, lanes), np.float32)
    for j in range(nch):
        for d in range(8):
            v = c[:, j, :, d]
            s = s + v
            ss = _fma(v, v, ss)
    off = lanes // 2
    idx = np.arange(lanes)
    while off:
        s = s + s[:, idx ^ off]
        ss = ss + ss[:, idx ^ off]
        off >>= 1
    return s[:, :1], ss[:, :1]


def ln_emulate(x, gamma, beta, variant: str) -> torch.Tensor:
    """LayerNorm in float32 in a kernel's own summation order, output rounded to bf16.
    'twopass': the sum, then the squared deviations from the mean, as both kernels do (32 lanes
               per row up to D = 1024, layernorm2_kernel; 64 beyond, layernorm_kernel);
    'onepass': var = E[x^2] - mean^2 from one pass (32 lanes; layernorm2_kernel as it was);
    'pivot':   those one-pass sums of t = x - x[0], var = E[t^2] - E[t]^2: the other exact
               form, which no kernel uses (it measured slower than the second pass)."""
    xf = x.float().numpy()
    D = xf.shape[1]
    g, b = _f32(gamma.numpy()), _f32(beta.numpy())
    eps = np.float32(LN_EPS)
    if variant == "twopass":
        lanes = 32 if D <= 1024 else 64
        s, _ = _ln_lane_sums(xf, lanes)
        t = xf - s / np.float32(D)
        _, q = _ln_lane_sums(t, lanes)
        rstd = np.float32(1) / np.sqrt(q / np.float32(D) + eps)
    else:
        t = xf - xf[:, :1] if variant == "pivot" else xf
        s, ss = _ln_lane_sums(t, 32)
        inv_d = np.float32(1) / np.float32(D)
        mean = s * inv_d
        var = np.maximum(ss * inv_d - mean * mean, np.float32(0))
        rstd = np.float32(1) / np.sqrt(var + eps)
        t = t - mean
    assert t.dtype == np.float32 and rstd.dtype == np.float32
    return bf16(torch.from_numpy(t * rstd * g + b))


# ---------------------------------------------------------------------------------------------
# patchify, token embedding

PATCH_SHAPES = [(2, 32, 48, 16), (1, 64, 32, 8), (3, 64, 64, 32), (2, 224, 224, 16)]     # (B, H, W, P)
EMBED_SHAPES = [(3, 2, 8), (2, 5, 200), (2, 197, 768)]                                   # (B, T, D)


def imagenet_scale_shift():
    """The per-channel scale / shift the ViT engine hands to patchify (three distinct pairs)."""
    from kdl.models import vit as V
    return [1.0 / (255.0 * s) for s in V.STD], [-m / s for m, s in zip(V.MEAN, V.STD)]


def patchify_reference(img: torch.Tensor, P: int, scale, shift) -> torch.Tensor:
    """img [B][H][W][3] uint8 -> float64 [B * np][3 P P], the float32 scale / shift the kernel
    gets applied in float64, k = c P^2 + ky P + kx."""
    B, H, W, _ = img.shape
    sc = torch.tensor(scale, dtype=torch.float32).double()
    sh = torch.tensor(shift, dtype=torch.float32).double()
    x = img.double() * sc + sh                                             # [B][H][W][c]
    x = x.view(B, H // P, P, W // P, P, 3).permute(0, 1, 3, 5, 2, 4)       # b, py, px, c, ky, kx
    return x.reshape(B * (H // P) * (W // P), 3 * P * P)


def elementwise_bound(ref):
    return U8P * ref.abs() + 1e-6


def embed_inputs(B: int, T: int, D: int):
    """x [B*T][D] bf16 with NaN in row 0 of every image, cls [D], pos [T][D] fp32."""
    gen = torch.Generator().manual_seed(31 * T + D)
    x = bf16(torch.randn(B, T, D, generator=gen))
    x[:, 0] = math.nan
    cls = torch.randn(D, generator=gen)
    pos = torch.randn(T, D, generator=gen) * 0.5
    return x.view(B * T, D), cls, pos


def embed_reference(x, cls, pos, B: int, T: int) -> torch.Tensor:
    D = x.shape[1]
    ref = x.double().view(B, T, D) + pos.double()
    ref[:, 0] = cls.double() + pos[0].double()
    return ref.view(B * T, D)


# ---------------------------------------------------------------------------------------------
# GELU / SiLU epilogue

def act_grid() -> torch.Tensor:
    """bf16-representable inputs: +-0, +-2^-10 .. +-8 in quarter-octave steps, +-12, 30, 88, 100."""
    mag = [2.0 ** (e / 4) for e in range(-40, 13)] + [12.0, 30.0, 88.0, 100.0]
    v = bf16(torch.tensor([0.0] + mag)).float()
    return torch.cat([v, -v])


def act_input(M: int, C: int = 64) -> torch.Tensor:
    """[M][C] bf16 that walks the grid, so every value meets many rows and columns."""
    g = act_grid()
    idx = torch.arange(M * C) % g.numel()
    return bf16(g[idx].view(M, C))


def act_reference(x: torch.Tensor, mode: int) -> torch.Tensor:
    x = x.double()
    if mode == 3:
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))
    return x / (1 + torch.exp(-x))


def act_bound(ref, x):
    """bf16 output rounding, plus fast_erf's 1.5e-7 absolute error times |x| / 2 and one-ulp
    rcp / exp2."""
    return U8P * ref.abs() + 2.0 ** -20 * x.double().abs().clamp_min(1.0)
