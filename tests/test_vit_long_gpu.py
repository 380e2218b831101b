"""ViT above 256 tokens (kernels/vit_long.hip): attn_ahat + rollout_chain and the vit_b16_384 engine. The
reference is float64 torch on the CPU from the same bf16 values, by test_rollout_gpu.py's definition (QKV of
standard deviation 1.7). The rollout
figure is max |got - ref| over the reference row's maximum; fp32 chains read ~1e-6 and bf16-rounded
operands 6e-3, and the ceiling of 1e-4 is there for the second (profiles/vit_384.txt has the measured)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_rollout_gpu as RG
from kdl.ops import _lib

pytestmark = pytest.mark.gpu
DEV, NAN = "cuda", float("nan")
CHAIN_T = [17, 257, 273, 577, 1024]      # the 3- / 5- / 8-fragment instances of attn_ahat, 1..4 column passes


def _ahat(qkv, B, T, H, ldr, Tq=None):
    out = RG.r_buffer(B, T, ldr)
    _lib.lib().attn_ahat(dict(qkv=qkv.data_ptr(), out=out.data_ptr(), B=B, T=T, Tq=Tq or T, H=H, dh=64, scale=0.125,
                              ldr=ldr), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out


def _chain(bufs, top, B, T, ldr, ldo):
    table = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=DEV)
    out = torch.full((B + 1, ldo), NAN, dtype=torch.float32, device=DEV)
    _lib.lib().rollout_chain(dict(ahat=table.data_ptr(), top=top.data_ptr(), out=out.data_ptr(), B=B, T=T,
                                  L=len(bufs), ldr=ldr, ldo=ldo), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("T", CHAIN_T)
def test_ahat_and_chain_against_float64(T):
    L, ld0 = RG.LAYERS, (T + 3) // 4 * 4
    for H in (1, 12):
        qkvs = RG.make_qkv(L, 3, T, H, 1000 * T + H)
        ahat = [RG.layer_ahat(qkvs[l], H) for l in range(L)]          # float64 [3, T, T], shared by B = 1 and 3
        v = ahat[L - 1][:, :1]
        for l in range(L - 2, -1, -1):
            v = v @ ahat[l]
        ref = v[:, 0, 1:] / v[:, 0, 1:].amax(dim=1, keepdim=True)     # its maximum is 1
        for B, ldr in [(B, ldr) for B in (1, 3) for ldr in (ld0, ld0 + 8)]:
            dev = qkvs[:, :B].contiguous().to(DEV)
            full = [_ahat(dev[l], B, T, H, ldr) for l in range(L)]
            for l in range(L):
                assert torch.isnan(full[l][:B, :, T:]).all() and torch.isnan(full[l][B]).all(), "padding or image B"
                body = full[l][:B, :, :T].double().cpu()
                assert ((body.sum(-1) - 1).abs() <= RG.ROWSUM_TOL).all() and (body - ahat[l][:B]).abs().max() <= RG.CEILING
            assert torch.equal(_bits(_ahat(dev[0], B, T, H, ldr)[:B, :, :T]), _bits(full[0][:B, :, :T]))
            one = _ahat(dev[L - 1], B, T, H, ldr, Tq=1)
            assert torch.equal(_bits(one[:B, 0, :T]), _bits(full[L - 1][:B, 0, :T]))
            assert torch.isnan(one[:B, 1:]).all() and torch.isnan(one[:B, 0, T:]).all() and torch.isnan(one[B]).all()
            top, ldo = RG.make_top(B), T + 1 + 3
            out = _chain(full[:L - 1] + [one], top, B, T, ldr, ldo)
            assert torch.equal(_bits(out[:B]), _bits(_chain(full[:L - 1] + [one], top, B, T, ldr, ldo)[:B]))
            assert torch.isnan(out[:B, T + 1:]).all() and torch.isnan(out[B]).all()
            assert torch.equal(_bits(out[:B, :2]), _bits(top))
            err = (out[:B, 2:T + 1].double().cpu() - ref[:B]).abs().max().item()
            print(f"rollout_chain T {T:4d} H {H:2d} B {B} ldr {ldr:4d}: error / row max {err:.3e}")
            assert err <= RG.CEILING, (T, H, B, ldr, err)


@pytest.fixture(scope="module")
def images():
    return torch.randint(0, 256, (2, 384, 384, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)


def test_engine_384_matches_the_oracle(images):
    from kdl.engine import registry
    from kdl.models import vit as V
    info = registry.get("vit_b16_384")
    p = info.init_params(0)
    eng = info.engine(p, 2, DEV)
    assert (eng.size, eng.T) == (384, 577) and any(s.kind == "attn" for s in eng.steps)
    out, ref = eng.forward(images.to(DEV)).cpu(), V.vit_forward(p, images, size=384)
    rel = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"vit_b16_384: cosine {F.cosine_similarity(out, ref, dim=1).min():.5f}, relative error {rel:.4f}")
    assert F.cosine_similarity(out, ref, dim=1).min() > 0.99 and rel < 0.1


def test_engine_384_rollout_matches_the_oracle(images):
    from kdl.engine import registry
    from kdl.engine.base import unpack_explain
    from kdl.models import vit as V
    info = registry.get("vit_b16_384")
    p = RG.peaked_params(info.init_params(0))
    cls_o, score_o, heat_o = V.vit_rollout(p, images, size=384)
    rows = info.engine(p, 2, DEV, rollout=True).forward(images.to(DEV)).cpu().numpy()
    assert rows.shape == (2, 2 + 24 * 24)
    c, s, heat = unpack_explain(rows, 24, 24)
    err = float(np.abs(heat - heat_o.numpy()).max())
    flat = float((heat_o.amin(dim=(1, 2)) / heat_o.amax(dim=(1, 2))).max())
    print(f"vit_b16_384 rollout: oracle min/max {flat:.3f}, max |heat - oracle| {err:.6f}")
    assert heat.max(axis=(1, 2)).tolist() == [1.0, 1.0] and err <= RG.ORACLE_GATE[False], err


def test_size_224_is_the_default_bit_for_bit():
    from kdl.engine.vit import ViTEngine
    from kdl.models import vit as V
    p = V.init_params(seed=0)
    x = torch.randint(0, 256, (2, 224, 224, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).to(DEV)
    a = ViTEngine(p, max_batch=2, device=DEV).forward(x).clone()
    assert torch.equal(a, ViTEngine(p, max_batch=2, device=DEV, size=224).forward(x))
