"""grouped_conv (kernels/grouped_conv.hip) at the smallest shapes that reach each of its indices,
against a float64 reference over the stored fp16 / bf16 values, and the ResNeXt-50 engine built
on it against the fp32 oracle and against its own dense lowering (run on MI355X).

Per-element bound (the form of tests/_conv_cases.py): products of two half-precision values are
exact in fp32, so fp32 accumulation of the 9*cg products in any order plus the bias add is within
(9*cg + 16) * 2^-24 * (sum |x*w| + |bias|) of the exact sum; the store adds half an ulp of the
output type at the exact value widened by that amount.
"""
import itertools

import numpy as np
import pytest
import torch

from _conv_cases import guarded, guards_intact, half_ulp, to_f64
from kdl.ops import _lib
from kdl.ops.pack import pack_grouped_fragments

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = ((7, 7), (6, 18))     # odd / even extents; one ragged 16-pixel tile, and two with the second ragged
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def make(cg, stride, dtype, H, W, seed, isolate=None):
    """Stored operands of one case: x [B][H+2][W+2][C] with an exactly zero border, w [C][9*cg], bias.
    ``isolate``: that group's weights are scaled by 64 and every other group's x by 256."""
    gen = torch.Generator().manual_seed(seed)
    B, C = 2, 64 if cg == 32 else 32
    x = torch.zeros(B, H + 2, W + 2, C)
    x[:, 1:-1, 1:-1] = torch.randn(B, H, W, C, generator=gen)
    w = torch.randn(C, 9 * cg, generator=gen) / (9 * cg) ** 0.5
    if isolate is not None:
        own = torch.arange(C) // cg == isolate
        x[..., ~own] *= 256
        w[own] *= 64
    bias = torch.randn(C, generator=gen) * 0.1
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    return dict(cg=cg, G=C // cg, C=C, B=B, H=H, W=W, OH=OH, OW=OW, stride=stride, dt=int(dtype == torch.float16),
                x=x.to(dtype), w=w.to(dtype), bias=bias)


def reference(c):
    """-> (exact [B][OH][OW][C] before ReLU, bound) in float64."""
    x, w = to_f64(c["x"]), to_f64(c["w"]).reshape(c["G"], c["cg"], 9, c["cg"])      # w[g][o][tap][c]
    s, OH, OW = c["stride"], c["OH"], c["OW"]
    v = np.zeros((c["B"], OH, OW, c["G"], c["cg"]))
    mag = np.zeros_like(v)
    for ky, kx in itertools.product(range(3), range(3)):
        xt = x[:, ky:ky + (OH - 1) * s + 1:s, kx:kx + (OW - 1) * s + 1:s].reshape(c["B"], OH, OW, c["G"], c["cg"])
        wt = w[:, :, ky * 3 + kx]
        v += np.einsum("bhwgc,goc->bhwgo", xt, wt)
        mag += np.einsum("bhwgc,goc->bhwgo", np.abs(xt), np.abs(wt))
    bias = to_f64(c["bias"])
    v = v.reshape(c["B"], OH, OW, c["C"]) + bias
    g = (9 * c["cg"] + 16) * 2.0 ** -24 * (mag.reshape(v.shape) + np.abs(bias))
    return v, g + half_ulp(np.abs(v) + g, c["dt"])


def launch(c, xd, wp, bd, ybody, ldy, relu, **over):
    args = dict(x=xd.data_ptr(), wp=wp.data_ptr(), bias=bd.data_ptr(), y=ybody.data_ptr(), ldx=c["C"], ldy=ldy,
                relu=relu, **{k: c[k] for k in ("B", "H", "W", "OH", "OW", "C", "G", "cg", "stride", "dt")})
    args.update(over)
    _lib.lib().grouped_conv(args, _lib.stream_ptr())
    torch.cuda.synchronize()


def run_and_check(c, relu, pad, ref, rows=0):
    """One launch into a guarded, pre-filled output with row stride C + pad; every element against
    its bound, pad columns and guards untouched. ``rows``: output rows per band (0: the launcher's,
    2 at these sizes). -> largest error / bound."""
    dtype = c["x"].dtype
    xd, bd = c["x"].to(DEV).contiguous(), c["bias"].to(DEV)
    wp = pack_grouped_fragments(c["w"].double(), c["cg"], dtype).to(DEV).contiguous()
    ldy, n = c["C"] + pad, c["B"] * c["OH"] * c["OW"]
    whole, body = guarded(n * ldy, 64 * ldy, dtype, 7.0, DEV)
    launch(c, xd, wp, bd, body, ldy, relu, rows=rows)
    y = to_f64(body).reshape(n, ldy)
    v, bnd = (a.reshape(n, c["C"]) for a in ref)
    err = np.abs(y[:, :c["C"]] - (np.maximum(v, 0) if relu else v))
    ratio = float(np.nanmax(np.where(np.isnan(err), np.inf, err) / bnd))
    print(f"RATIO cg={c['cg']} s={c['stride']} dt={c['dt']} {c['H']}x{c['W']} relu={relu} pad={pad} rows={rows}: {ratio:.3f}")
    assert ratio <= 1.0
    assert (y[:, c["C"]:] == 7.0).all(), "pad columns written"
    assert guards_intact(whole, n * ldy)
    return ratio


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cg", [4, 8, 16, 32])
def test_grouped_conv_within_bound(cg, stride, dtype):
    """Bands of two rows (prologue and one ring step) and one band of the whole map (3 to 7 rows:
    every ring slot is overwritten while its neighbours are still read)."""
    for (H, W) in SHAPES:
        c = make(cg, stride, DTYPES[dtype], H, W, seed=1000 * cg + 10 * stride + H)
        ref = reference(c)
        for relu, pad, rows in itertools.product((1, 0), (0, 16), (0, c["OH"])):
            run_and_check(c, relu, pad, ref, rows)


@pytest.mark.parametrize("cg", [4, 8, 16, 32])
def test_grouped_conv_reads_no_other_group(cg):
    """One group's weights are 64 times larger while every other group's x is 256 times larger: a
    read across a group boundary is off by orders of magnitude of the bound."""
    c = make(cg, 1, torch.float16, 6, 18, seed=cg, isolate=1)
    run_and_check(c, 0, 0, reference(c))


REFUSED = {"cg": dict(cg=12, G=4, C=48, ldx=48, ldy=48), "channels": dict(C=24, G=3), "stride": dict(stride=3, OH=3, OW=3),
           "x_align": {}, "ldy": dict(ldy=24)}


@pytest.mark.parametrize("bad", list(REFUSED))
def test_grouped_conv_refuses(bad):
    """cg = 12, C = 24, stride 3, x two bytes off a 16-byte boundary, ldy < C: the call raises and writes nothing."""
    c = make(8, 1, torch.float16, 7, 7, seed=3)
    xd = torch.zeros(c["x"].numel() * 2 + 8, dtype=torch.float16, device=DEV)
    wp, bd = torch.zeros(4 * 9 * 512, dtype=torch.float16, device=DEV), torch.zeros(64, device=DEV)
    n = c["B"] * c["OH"] * c["OW"] * 64
    whole, body = guarded(n, 4096, torch.float16, 7.0, DEV)
    over = dict(REFUSED[bad])
    with pytest.raises(RuntimeError):
        launch(c, xd[1:] if bad == "x_align" else xd, wp, bd, body, over.pop("ldy", c["C"]), 1, **over)
    torch.cuda.synchronize()
    assert bool((body == 7.0).all()) and guards_intact(whole, n)


# ------------------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def xparams():
    from kdl.models import resnet as R
    return R.init_params(seed=0, **R.RESNEXT50_32X4D)


def _rel(a, b):
    return ((a.float() - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("family", ["resnext50_32x4d", "resnext50_32x4d_bf16"])
def test_resnext_engine_matches_oracle_and_dense_lowering(xparams, family, monkeypatch):
    """test_resnet_gpu.py's gates on its three images (buckets 2 and 4); the grouped engine's largest
    relative logit error is at most 1.25 times the dense lowering's (the same products summed in
    fp32; the margin is summation order); captured replays are bit-equal to the eager forward."""
    from kdl.engine import registry
    info = registry.get(family)
    x = torch.randint(0, 256, (3, 224, 224, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    ref = info.oracle(xparams, x)
    eng = info.engine(xparams, 4, DEV, buckets=[2, 4])
    assert sum(s.kind == "gconv" for s in eng.steps) == 16
    eager = eng.forward(x.to(DEV), capture=False).cpu()
    for _ in range(3):
        assert torch.equal(eng.forward(x.to(DEV), capture=True).cpu(), eager)
    monkeypatch.setenv("KDL_GROUPED_CONV", "0")
    dense_eng = info.engine(xparams, 4, DEV, buckets=[4])
    assert not any(s.kind == "gconv" for s in dense_eng.steps)
    dense = dense_eng.forward(x.to(DEV), capture=False).cpu()
    cos = torch.nn.functional.cosine_similarity(eager, ref, dim=1).min().item()
    e_g, e_d = _rel(eager, ref), _rel(dense, ref)
    top = [(o.argmax(1) == ref.argmax(1)).tolist() for o in (eager, dense)]
    print(f"RESNEXT {family}: cos {cos:.5f} rel grouped {e_g:.5f} dense {e_d:.5f} top1 grouped {top[0]} dense {top[1]}")
    assert cos > 0.98 and e_g < 0.2
    assert sum(top[0]) / 3 >= 2 / 3
    assert e_g <= 1.25 * e_d


def test_resnext_embed_and_explain_forward(xparams):
    from kdl.engine import registry
    from kdl.engine.base import unpack_explain
    info = registry.get("resnext50_32x4d")
    x = torch.randint(0, 256, (2, 224, 224, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    rows = info.engine(xparams, 2, DEV, embed="l2").forward(x.to(DEV)).cpu()
    want = torch.nn.functional.normalize(info.feature_oracle(xparams, x), dim=1)
    assert rows.shape == want.shape == (2, 2048)
    assert torch.nn.functional.cosine_similarity(rows.float(), want, dim=1).min() > 0.98
    eng = info.engine(xparams, 2, DEV, explain=True)
    cls, score, heat = unpack_explain(eng.forward(x.to(DEV)), *info.map_size)
    assert cls.tolist() == eng.last_logits(0)[:2].argmax(1).tolist()
    assert heat.shape == (2, 7, 7) and heat.min() >= 0 and heat.max(axis=(1, 2)).tolist() == [1.0, 1.0]
