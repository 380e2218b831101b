"""Host-side weight preparation: BN folding and MFMA fragment packing.

SURVEY.md §2.5 K8: BatchNorm is folded at load time (W' = W*gamma/sqrt(var+eps),
b' = beta - mean*gamma/sqrt(var+eps), Keras eps = 1e-3). The folded pointwise /
conv weights are then re-laid out into the exact order the MFMA B-operand
fragments are consumed by ``conv_gemm.hip``: ``[n_frag][k_step][lane][8]`` with
lane l holding W[16*n_frag + (l & 15)][32*k_step + 8*(l >> 4) + j].
"""
from __future__ import annotations

import torch

from ..models.layers import KERAS_BN_EPS


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def bn_scale_shift(p: dict, bn: str, eps: float = KERAS_BN_EPS):
    if f"{bn}/gamma" not in p:          # BN already folded into the kernel (kdl.ingest.fold)
        b = p[f"{bn}/beta"].double()
        return torch.ones_like(b), b
    g, b = p[f"{bn}/gamma"].double(), p[f"{bn}/beta"].double()
    m, v = p[f"{bn}/moving_mean"].double(), p[f"{bn}/moving_variance"].double()
    s = g / torch.sqrt(v + eps)
    return s, b - m * s


def pack_fragments(w_nk: torch.Tensor, nf: int, kt: int, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """W[N][K] (any float dtype) -> ``dtype`` (bf16 or fp16) [nf][kt][64][8] zero padded."""
    n, k = w_nk.shape
    assert n <= nf * 16 and k <= kt * 32, (w_nk.shape, nf, kt)
    full = torch.zeros(nf * 16, kt * 32, dtype=torch.float32)
    full[:n, :k] = w_nk.float()
    # [nf, 16(r), kt, 4(q), 8(j)] -> [nf, kt, q, r, j] ; lane = q*16 + r
    t = full.view(nf, 16, kt, 4, 8).permute(0, 2, 3, 1, 4).contiguous()
    return t.view(nf, kt, 64, 8).to(dtype)


def unpack_fragments(packed: torch.Tensor, n: int, k: int) -> torch.Tensor:
    nf, kt = packed.shape[0], packed.shape[1]
    t = packed.float().view(nf, kt, 4, 16, 8).permute(0, 3, 1, 2, 4).contiguous()
    return t.view(nf * 16, kt * 32)[:n, :k]


def grouped_slab_weights(w_nk: torch.Tensor, cg: int) -> torch.Tensor:
    """Grouped 3x3 weights W[C][9*cg] (k = tap*cg + c, row o in group o // cg) -> the per-slab
    dense tiles [C][KS*32] that grouped_conv.hip multiplies: row o's k-step t holds, for
    cg <= 16 (KS = 5), taps 2t and 2t + 1 over the 16 input channels of o's own 16-channel slab
    (k = 32t + 16*(tap & 1) + slab channel; zero outside o's group and for the tenth tap), and
    for cg = 32 (KS = 9) tap t over the group's 32 channels."""
    C, k = w_nk.shape
    assert cg in (4, 8, 16, 32) and k == 9 * cg and C % max(cg, 16) == 0, (w_nk.shape, cg)
    w = w_nk.reshape(C, 9, cg)
    if cg == 32:
        return w.reshape(C, 9 * 32)
    out = torch.zeros(C, 10, 16, dtype=w_nk.dtype)
    first = (torch.arange(C) % 16) // cg * cg          # o's group starts here inside its slab
    for c in range(cg):
        out[torch.arange(C), :9, first + c] = w[:, :, c]
    return out.reshape(C, 5 * 32)


def pack_grouped_fragments(w_nk: torch.Tensor, cg: int, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Grouped 3x3 weights W[C][9*cg] -> ``dtype`` [C/16][KS][64][8] in MFMA fragment order
    (GroupedConvArgs.wp): ``pack_fragments`` of the slab tiles, one 16-row fragment per slab."""
    t = grouped_slab_weights(w_nk, cg)
    return pack_fragments(t, t.shape[0] // 16, t.shape[1] // 32, dtype)


def grouped_dense_weights(w_nk: torch.Tensor, cg: int) -> torch.Tensor:
    """Grouped 3x3 weights W[C][9*cg] -> the block-diagonal dense W[C][9*C] (k = tap*C + c) of the
    same convolution: the MODE_CONV lowering, G times the MACs and weight bytes."""
    C = w_nk.shape[0]
    w = w_nk.reshape(C, 9, cg)
    out = torch.zeros(C, 9, C, dtype=w_nk.dtype)
    first = torch.arange(C) // cg * cg
    for c in range(cg):
        out[torch.arange(C), :, first + c] = w[:, :, c]
    return out.reshape(C, 9 * C)


def fold_layer_scale(w: torch.Tensor, b: torch.Tensor, scale: torch.Tensor):
    """ConvNeXt's ``layer_scale`` [C, 1, 1] folded into the block's last linear W [C][4C], b [C]:
    scale * (W h + b) = (scale W) h + scale b, in float64 (the GEMM's epilogue then adds the
    block input as its residual)."""
    s = scale.double().reshape(-1)
    return w.double() * s[:, None], b.double() * s


def s2d_weights(w_oihw: torch.Tensor) -> torch.Tensor:
    """A 2x2 / stride-2 conv weight [O][C][2][2] -> W[O][4C] with k = (ky*2 + kx)*C + c: the column
    order ``ln_s2d`` writes, so the conv is one pointwise GEMM over its space-to-depth rows."""
    o, c, kh, kw = w_oihw.shape
    assert (kh, kw) == (2, 2), w_oihw.shape
    return w_oihw.double().permute(0, 2, 3, 1).reshape(o, 4 * c)


def pad_vec(v: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=torch.float32)
    out[: v.numel()] = v.float()
    return out


def rowrun_weights(w_nk: torch.Tensor, kh: int, run: int, rp: int) -> torch.Tensor:
    """Stem weights W[N][kh*run] (k = ky*run + kx*3 + c) -> W[N][kh*rp]: every kernel row's
    run of kx*3 + c slots zero-padded to rp (the K layout of stem_rows_kernel, stem.hip)."""
    n = w_nk.shape[0]
    out = torch.zeros(n, kh, rp, dtype=w_nk.dtype)
    out[:, :, :run] = w_nk.reshape(n, kh, run)
    return out.reshape(n, kh * rp)
