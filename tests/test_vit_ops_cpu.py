"""The ViT operator tests' own references and bounds, checked on the CPU: float32 emulations
of what a correct kernel does fit every bound of tests/_vit_cases.py, and the known-bad
variants (a mask off by one key, a softmax without its maximum subtracted, a one-pass
E[x^2] - mean^2 variance) do not. So tests/test_vit_ops_gpu.py can fail for those reasons."""
import math

import pytest
import torch
import torch.nn.functional as F

import _vit_cases as VC

ALL_T = sorted({T for ts in VC.ATTN_T.values() for T in ts})


@pytest.mark.parametrize("T", ALL_T)
def test_attention_emulation_fits_the_bound(T):
    for B, H in VC.ATTN_LAYOUTS:
        for kind in VC.ATTN_KINDS:
            qkv = VC.attn_qkv(kind, B, T, H)
            ref, A = VC.attn_reference(qkv, B, T, H)
            err, bound = (VC.attn_emulate(qkv, B, T, H).double() - ref).abs(), VC.attn_bound(ref, A)
            assert VC.within(err, bound), (T, B, H, kind, VC.worst(err, bound))


def test_attention_reference_matches_torch():
    B, T, H = 2, 65, 3
    qkv = VC.attn_qkv("benign", B, T, H)
    q, k, v = (t.reshape(B, T, H, 64).transpose(1, 2) for t in qkv.double().split(H * 64, 1))
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * T, H * 64)
    assert torch.allclose(VC.attn_reference(qkv, B, T, H)[0], want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("T", [1, 63, 65, 197, 257, 321])       # T = 64k has no padded key in its last tile
def test_a_mask_off_by_one_key_misses_the_bound(T):
    B, H = 2, 3
    qkv = VC.attn_qkv("negative", B, T, H)
    ref, A = VC.attn_reference(qkv, B, T, H)
    bad, _ = VC.attn_reference(qkv, B, T, H, leak_key=True)
    err, bound = (bad - ref).abs(), VC.attn_bound(ref, A)
    assert float((err > bound).double().mean()) > 0.99      # the zero key takes all the weight


@pytest.mark.parametrize("T", [1, 65, 197, 300])
def test_a_softmax_without_max_subtraction_misses_the_bound(T):
    B, H = 2, 3
    qkv = VC.attn_qkv("offset", B, T, H)
    ref, A = VC.attn_reference(qkv, B, T, H)
    bad = VC.attn_emulate(qkv, B, T, H, subtract_max=False).double()
    assert not VC.within((bad - ref).abs(), VC.attn_bound(ref, A))
    assert not bool(torch.isfinite(bad).any())              # exp2 overflowed in every row


def test_attention_fp8_scales_saturate_as_the_gpu_test_assumes():
    """inv_scale 16 saturates nothing, 200 saturates over 1 % of the values, and exact e4m3
    rounding of the emulated output passes f8_check with both."""
    from kdl.ops.f8 import to_e4m3
    B, H = 2, 3
    for T in VC.ATTN_F8_T:
        for kind in VC.ATTN_F8_KINDS:
            qkv = VC.attn_qkv(kind, B, T, H)
            ref, A = VC.attn_reference(qkv, B, T, H)
            for inv, sat in zip(VC.ATTN_INV_SCALE, (False, True)):
                byte = to_e4m3(VC.attn_emulate(qkv, B, T, H).float() * inv)
                VC.f8_check(byte, ref, inv, VC.U8 * A * inv, sat, (T, kind, inv))


def test_f8_check_catches_scale_byte_order_and_nan_bytes():
    from kdl.ops.f8 import to_e4m3
    B, T, H = 2, 65, 3
    qkv = VC.attn_qkv("peaked", B, T, H)
    ref, A = VC.attn_reference(qkv, B, T, H)
    inv = VC.ATTN_INV_SCALE[0]
    good = to_e4m3(ref.float() * inv)
    VC.f8_check(good, ref, inv, VC.U8 * A * inv, False)
    swapped = good.view(-1, 4)[:, [1, 0, 2, 3]].reshape(good.shape)           # two bytes of a packed word
    with pytest.raises(AssertionError):
        VC.f8_check(swapped, ref, inv, VC.U8 * A * inv, False)
    with pytest.raises(AssertionError):                                      # scale in place of inv_scale
        VC.f8_check(to_e4m3(ref.float() / inv), ref, inv, VC.U8 * A * inv, False)
    nan = to_e4m3(ref.float() * VC.ATTN_INV_SCALE[1])
    VC.f8_check(nan, ref, VC.ATTN_INV_SCALE[1], VC.U8 * A * VC.ATTN_INV_SCALE[1], True)
    nan[3, 5] = 0x7F
    with pytest.raises(AssertionError):
        VC.f8_check(nan, ref, VC.ATTN_INV_SCALE[1], VC.U8 * A * VC.ATTN_INV_SCALE[1], True)


# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", VC.LN_D)
def test_layernorm_pivot_and_two_pass_fit_bound_and_gain(D):
    """The two-pass variance of both kernels, in the kernels' summation order, and the one-pass
    sums about a pivot element (the alternative that was measured against it), on 64 rows
    (every row kind at least six times) and on the short cases."""
    for rows in VC.LN_ROWS:
        x, g, b, _ = VC.ln_inputs(D, rows)
        for variant in ("pivot", "twopass"):
            VC.ln_check(VC.ln_emulate(x, g, b, variant).float(), x, g, b, (D, rows, variant))


def test_layernorm_constant_rows_give_beta():
    for D in VC.LN_D:
        x, g, b, _ = VC.ln_inputs(D, 4, kinds=["const", "zeros"])
        for variant in ("pivot", "twopass"):
            y = VC.ln_emulate(x, g, b, variant)
            assert torch.equal(y, VC.bf16(b).expand_as(y)), (D, variant)


@pytest.mark.parametrize("D", [200, 768, 1024])
@pytest.mark.parametrize("kind", [(300, 1), (20, 0.05)])
def test_layernorm_one_pass_variance_misses_the_gain_check(D, kind):
    """var = E[x^2] - mean^2 in fp32, summed as layernorm2_kernel summed it: the gain of a row
    with |mean| / std of 300-400 is off by more than the 2^-9 the GPU test allows, which the
    per-element bound then misses too. The two-pass kernel order passes on the same rows."""
    x, g, b, _ = VC.ln_inputs(D, 64, kinds=[kind])
    n, ref, R = VC.ln_reference(x, g, b)
    bad = VC.ln_emulate(x, g, b, "onepass").float()
    gain = VC.ln_gain(bad, n, g, b)
    assert float((gain - 1).abs().max()) > VC.LN_GAIN_TOL, float((gain - 1).abs().max())
    assert not VC.within((bad.double() - ref).abs(), VC.ln_bound(ref, R))
    with pytest.raises(AssertionError):
        VC.ln_check(bad, x, g, b)
    VC.ln_check(VC.ln_emulate(x, g, b, "twopass").float(), x, g, b)


def test_layernorm_reference_matches_torch():
    x, g, b, _ = VC.ln_inputs(264, 9)
    want = F.layer_norm(x.double(), (264,), g.double(), b.double(), VC.LN_EPS)
    assert torch.allclose(VC.ln_reference(x, g, b)[1], want, rtol=1e-9, atol=1e-9)


def test_layernorm_fp8_scales_saturate_as_the_gpu_test_assumes():
    from kdl.ops.f8 import to_e4m3
    for D in VC.LN_F8_D:
        x, g, b, _ = VC.ln_inputs(D, 9, kinds=VC.LN_F8_KINDS)
        _, ref, R = VC.ln_reference(x, g, b)
        for inv, sat in zip(VC.LN_INV_SCALE, (False, True)):
            for variant in ("pivot", "twopass"):
                y = VC.ln_emulate(x, g, b, variant).float()
                VC.f8_check(to_e4m3(y * inv), ref, inv, 2.0 ** -14 * R * inv, sat, (D, inv, variant))


# ---------------------------------------------------------------------------------------------

def test_patchify_reference_matches_unfold():
    gen = torch.Generator().manual_seed(0)
    sc, sh = VC.imagenet_scale_shift()
    assert len(set(sc)) == 3 and len(set(sh)) == 3
    for B, H, W, P in VC.PATCH_SHAPES[:3]:
        img = torch.randint(0, 256, (B, H, W, 3), generator=gen, dtype=torch.uint8)
        x = img.double() * torch.tensor(sc, dtype=torch.float32).double() + torch.tensor(sh, dtype=torch.float32).double()
        want = F.unfold(x.permute(0, 3, 1, 2), P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P)
        assert torch.equal(VC.patchify_reference(img, P, sc, sh), want)


def test_embed_reference_matches_the_model():
    from kdl.models import vit as V
    B = 2
    p = V.init_params(seed=1)
    x, _, _ = VC.embed_inputs(B, V.TOKENS, V.DIM)
    cls, pos = p["class_token"].reshape(-1).float(), p["encoder.pos_embedding"].reshape(V.TOKENS, V.DIM).float()
    ref = VC.embed_reference(x, cls, pos, B, V.TOKENS).view(B, V.TOKENS, V.DIM)
    tok = x.double().view(B, V.TOKENS, V.DIM)[:, 1:]
    want = torch.cat([cls.double().expand(B, 1, -1), tok], 1) + pos.double()
    assert torch.equal(ref, want) and not bool(torch.isnan(ref).any())


def test_activation_grid_and_references():
    g = VC.act_grid()
    assert torch.equal(VC.bf16(g).float(), g)                          # representable
    assert g.numel() == len(set(g.tolist())) + 1                       # distinct but for +-0
    assert {0.0, 2.0 ** -10, 8.0, 12.0, 30.0, 88.0, 100.0} <= set(g.abs().tolist())
    assert bool(torch.signbit(g[g == 0]).any()) and not bool(torch.signbit(g[g == 0]).all())
    x = VC.act_input(70)
    assert set(x.float().unique().tolist()) == set(g.unique().tolist())
    xd = x.double()
    assert torch.allclose(VC.act_reference(x, 3), F.gelu(xd), rtol=1e-12, atol=1e-300)
    assert torch.allclose(VC.act_reference(x, 4), F.silu(xd), rtol=1e-12, atol=1e-300)
    for mode in (3, 4):                                                # exact fp32 evaluation fits the bound
        ref = VC.act_reference(x, mode)
        y = VC.bf16((F.gelu if mode == 3 else F.silu)(x.float()))
        assert VC.within((y.double() - ref).abs(), VC.act_bound(ref, x)), mode
    # a tanh-approximated GELU, the classic substitute, does not
    ref = VC.act_reference(x, 3)
    y = VC.bf16(F.gelu(x.float(), approximate="tanh"))
    assert not VC.within((y.double() - ref).abs(), VC.act_bound(ref, x))
    assert math.isclose(float(VC.act_reference(torch.tensor([100.0]), 3)), 100.0)
