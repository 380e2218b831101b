"""The ViT kernels called directly, against float64 references at their edges: both attention
kernels (AttnArgs.algo) at every T around a 16-query / 64-key boundary with peaked, offset and
strongly negative scores; both LayerNorm kernels on rows whose mean dwarfs their spread; the
e4m3 outputs of both; patchify and embed_tokens away from 224 x 224; and the GELU / SiLU
epilogue over a grid from 2^-10 to 100. Inputs, references and bounds are in _vit_cases.py;
test_vit_ops_cpu.py shows what the bounds let through and what they catch.

Every input sits between NaN guard rows and every output between guard rows of a fixed bit
pattern: a row read past the end poisons the result, a byte written outside is seen."""
import pytest
import torch

import _vit_cases as VC
from kdl.ops import _lib
from kdl.ops.conv import MODE_PW, ConvGemmLayer, Geometry

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
S16, S8 = VC.SENTINEL16, VC.SENTINEL8


def _sync():
    torch.cuda.synchronize()


def _in_guarded(x: torch.Tensor, ld: int | None = None):
    """x [rows][D] bf16 on the GPU inside a NaN buffer [GUARD + rows + GUARD][ld]; returns (buffer, rows view)."""
    rows, D = x.shape
    buf, mid = VC.guarded(rows, ld or D, torch.bfloat16, NAN, DEV)
    mid[:, :D] = x.to(DEV)
    return buf, mid


# ---------------------------------------------------------------------------------------------
# attention

def _attention(qkv, B, T, H, algo, inv_scale=None, dh=VC.DH):
    """One launch between guards; returns bf16 out [B*T][H*64] (or the e4m3 bytes) on the CPU."""
    qbuf, qmid = _in_guarded(qkv)
    f8 = inv_scale is not None
    obuf, omid = VC.guarded(B * T, H * VC.DH, torch.uint8 if f8 else torch.int16, S8 if f8 else S16, DEV)
    out = dict(out8=omid.data_ptr(), inv_scale=inv_scale) if f8 else dict(out=omid.data_ptr())
    _lib.lib().attention(dict(qkv=qmid.data_ptr(), B=B, T=T, H=H, dh=dh, scale=VC.SCALE, algo=algo, **out),
                         _lib.stream_ptr())
    _sync()
    assert VC.guards_intact(obuf, H * VC.DH, S8 if f8 else S16), "attention wrote outside its output rows"
    return omid.cpu() if f8 else omid.view(torch.bfloat16).cpu()


@pytest.mark.parametrize("algo,T", [(a, T) for a in (1, 2, 0) for T in VC.ATTN_T[a]])
def test_attention_bf16(algo, T):
    for B, H in VC.ATTN_LAYOUTS:
        for kind in VC.ATTN_KINDS:
            qkv, ref, A = VC.attn_case(kind, B, T, H)
            out = _attention(qkv, B, T, H, algo).double()
            err, bound = (out - ref).abs(), VC.attn_bound(ref, A)
            print(f"attention algo {algo} T {T} B {B} H {H} {kind}: err / bound {VC.worst(err, bound):.3f}")
            assert VC.within(err, bound), (algo, T, B, H, kind, VC.worst(err, bound))


@pytest.mark.parametrize("algo,T", [(a, T) for a in (1, 2) for T in VC.ATTN_F8_T if a == 2 or T <= 256])
def test_attention_e4m3(algo, T):
    """(The whole-head kernel refuses 257 tokens, test_attention_refuses.)"""
    for B, H in VC.ATTN_LAYOUTS:
        for kind in VC.ATTN_F8_KINDS:
            qkv, ref, A = VC.attn_case(kind, B, T, H)
            for inv, sat in zip(VC.ATTN_INV_SCALE, (False, True)):
                byte = _attention(qkv, B, T, H, algo, inv_scale=inv)
                VC.f8_check(byte, ref, inv, VC.U8 * A * inv, sat, (algo, T, B, H, kind, inv))


@pytest.mark.parametrize("bad", [dict(algo=1, T=257), dict(dh=32), dict(T=0), dict(algo=3)])
def test_attention_refuses(bad):
    B, H, T = 1, 1, 257
    qbuf, qmid = _in_guarded(torch.zeros(B * T, 3 * H * VC.DH, dtype=torch.bfloat16))
    obuf, omid = VC.guarded(B * T, H * VC.DH, torch.int16, S16, DEV)
    args = dict(qkv=qmid.data_ptr(), out=omid.data_ptr(), B=B, T=T, H=H, dh=VC.DH, scale=VC.SCALE)
    args.update(bad)
    with pytest.raises(RuntimeError):
        _lib.lib().attention(args, _lib.stream_ptr())
    _sync()
    assert bool((obuf == S16).all())


# ---------------------------------------------------------------------------------------------
# LayerNorm

def _layernorm(x, gamma, beta, ldx, ldy, inv_scale=None):
    """One launch between guards; returns y [rows][D] bf16 (or the e4m3 bytes) on the CPU."""
    rows, D = x.shape
    xbuf, xmid = _in_guarded(x, ldx)
    f8 = inv_scale is not None
    ybuf, ymid = VC.guarded(rows, ldy, torch.uint8 if f8 else torch.int16, S8 if f8 else S16, DEV)
    g, b = gamma.to(DEV), beta.to(DEV)
    out = dict(y8=ymid.data_ptr(), inv_scale=inv_scale) if f8 else dict(y=ymid.data_ptr())
    _lib.lib().layernorm(dict(x=xmid.data_ptr(), gamma=g.data_ptr(), beta=b.data_ptr(), rows=rows, D=D, ldx=ldx,
                              ldy=ldy, eps=VC.LN_EPS, **out), _lib.stream_ptr())
    _sync()
    assert VC.guards_intact(ybuf, D, S8 if f8 else S16), "layernorm wrote outside its output"
    return ymid[:, :D].cpu() if f8 else ymid[:, :D].contiguous().view(torch.bfloat16).cpu()


@pytest.mark.parametrize("rows", VC.LN_ROWS)
@pytest.mark.parametrize("D", VC.LN_D)
def test_layernorm_bf16(D, rows):
    """Row i is of kind LN_KINDS[(rows + i) % 10]: the 64-row cases hold every kind at least six
    times, the short ones start on different kinds. (The one-pass E[x^2] - mean^2 variance that
    layernorm2_kernel used to have missed this at D = 200, 264, 768 and 1024, by up to 3.0 times
    the per-element bound: profiles/layernorm_var.txt.)"""
    x, gamma, beta, kinds = VC.ln_inputs(D, rows)
    for ldx, ldy in VC.ln_strides(D):
        y = _layernorm(x, gamma, beta, ldx, ldy)
        VC.ln_check(y.float(), x, gamma, beta, (D, rows, ldx, ldy, kinds))


@pytest.mark.parametrize("D", VC.LN_F8_D)
def test_layernorm_e4m3(D):
    x, gamma, beta, _ = VC.ln_inputs(D, 9, kinds=VC.LN_F8_KINDS)
    _, ref, R = VC.ln_reference(x, gamma, beta)
    for ldy in (D, D + 8):
        for inv, sat in zip(VC.LN_INV_SCALE, (False, True)):
            byte = _layernorm(x, gamma, beta, D, ldy, inv_scale=inv)
            VC.f8_check(byte, ref, inv, 2.0 ** -14 * R * inv, sat, (D, ldy, inv))


@pytest.mark.parametrize("D,rows", [(772, 4), (2056, 4), (768, 0)])
def test_layernorm_refuses(D, rows):
    ld = (D + 15) // 8 * 8                      # a multiple of 8 that holds the row
    xbuf, xmid = _in_guarded(torch.zeros(4, D, dtype=torch.bfloat16), ld)
    ybuf, ymid = VC.guarded(4, ld, torch.int16, S16, DEV)
    g = torch.ones(ld, device=DEV)
    with pytest.raises(RuntimeError):
        _lib.lib().layernorm(dict(x=xmid.data_ptr(), y=ymid.data_ptr(), gamma=g.data_ptr(), beta=g.data_ptr(),
                                  rows=rows, D=D, ldx=ld, ldy=ld, eps=VC.LN_EPS), _lib.stream_ptr())
    _sync()
    assert bool((ybuf == S16).all())


# ---------------------------------------------------------------------------------------------
# patchify, token embedding

def _patchify_args(img, y, B, H, W, P, ldy):
    sc, sh = VC.imagenet_scale_shift()
    return dict(x=img.data_ptr(), y=y.data_ptr(), B=B, H=H, W=W, P=P, ldy=ldy, scale0=sc[0], scale1=sc[1],
                scale2=sc[2], shift0=sh[0], shift1=sh[1], shift2=sh[2])


@pytest.mark.parametrize("B,H,W,P", VC.PATCH_SHAPES)
def test_patchify(B, H, W, P):
    gen = torch.Generator().manual_seed(H + W + P)
    img = torch.randint(0, 256, (B, H, W, 3), generator=gen, dtype=torch.uint8)
    ref = VC.patchify_reference(img, P, *VC.imagenet_scale_shift())
    rows, K = ref.shape
    imgd = img.to(DEV)
    for ldy in (K, K + 8):
        ybuf, ymid = VC.guarded(rows, ldy, torch.int16, S16, DEV)
        _lib.lib().patchify(_patchify_args(imgd, ymid, B, H, W, P, ldy), _lib.stream_ptr())
        _sync()
        assert VC.guards_intact(ybuf, K, S16)
        y = ymid[:, :K].contiguous().view(torch.bfloat16).cpu().double()
        err, bound = (y - ref).abs(), VC.elementwise_bound(ref)
        assert VC.within(err, bound), (ldy, VC.worst(err, bound))


@pytest.mark.parametrize("H,W,P", [(48, 48, 12), (40, 32, 16), (32, 40, 16)])
def test_patchify_refuses(H, W, P):
    img = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    ybuf, ymid = VC.guarded(16, 3 * P * P + 8, torch.int16, S16, DEV)
    with pytest.raises(RuntimeError):
        _lib.lib().patchify(_patchify_args(img, ymid, 1, H, W, P, 3 * P * P + 8), _lib.stream_ptr())
    _sync()
    assert bool((ybuf == S16).all())


@pytest.mark.parametrize("B,T,D", VC.EMBED_SHAPES)
def test_embed_tokens(B, T, D):
    x, cls, pos = VC.embed_inputs(B, T, D)
    ref = VC.embed_reference(x, cls, pos, B, T)
    xbuf, xmid = VC.guarded(B * T, D, torch.int16, S16, DEV)
    xmid.copy_(x.view(torch.int16).to(DEV))
    c, p = cls.to(DEV), pos.to(DEV)
    _lib.lib().embed_tokens(dict(x=xmid.data_ptr(), cls=c.data_ptr(), pos=p.data_ptr(), B=B, T=T, D=D),
                            _lib.stream_ptr())
    _sync()
    assert VC.guards_intact(xbuf, D, S16)
    y = xmid.view(torch.bfloat16).cpu().double()
    err, bound = (y - ref).abs(), VC.elementwise_bound(ref)
    assert VC.within(err, bound), VC.worst(err, bound)      # a NaN read from row 0 is a miss


def test_embed_tokens_refuses():
    B, T, D = 2, 3, 100
    xbuf, xmid = VC.guarded(B * T, 104, torch.int16, S16, DEV)
    f = torch.zeros(T * 104, device=DEV)
    with pytest.raises(RuntimeError):
        _lib.lib().embed_tokens(dict(x=xmid.data_ptr(), cls=f.data_ptr(), pos=f.data_ptr(), B=B, T=T, D=D),
                                _lib.stream_ptr())
    _sync()
    assert bool((xbuf == S16).all())


# ---------------------------------------------------------------------------------------------
# GELU / SiLU epilogue

@pytest.mark.parametrize("mode", [3, 4])
def test_activation_epilogue_sweep(mode):
    """A 64 -> 64 pointwise layer with identity weights and no bias: the pre-activation is the
    input itself, so the epilogue's fast_erf / fast_silu see the whole grid exactly, tails and
    +-0 included, on every GEMM config that can run the layer."""
    M, C = 70, 64                               # two 64-row tiles, the second ragged
    x = VC.act_input(M, C)
    ref = VC.act_reference(x, mode)
    bound = VC.act_bound(ref, x)
    lay = ConvGemmLayer("act", MODE_PW, torch.eye(C, dtype=torch.float64), torch.zeros(C), cin_pad=C, n=C,
                        relu_out=mode, device=DEV)
    xd = x.to(DEV).contiguous()
    variants = lay.variants(None)
    assert variants
    for split, cfg in variants:
        y = torch.full((M * lay.ldy,), NAN, dtype=torch.bfloat16, device=DEV)
        lay.launch(xd, y, Geometry(1, 1, M, 1, M), cfg=cfg, split=split)
        _sync()
        y = y.view(M, lay.ldy).cpu().float()
        assert bool(torch.isfinite(y).all()), cfg
        err = (y.double() - ref).abs()
        assert VC.within(err, bound), (cfg, VC.worst(err, bound))
        xf = x.float()                          # act(-100) is +-0, act(100) is 100, with either activation
        assert bool((y[xf == -100] == 0).all()) and bool((y[xf == 100] == 100).all()), cfg
