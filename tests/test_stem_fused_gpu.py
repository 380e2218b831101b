"""Fused Xception block1_conv1 + block1_conv2 (stem_conv3x3.hip): bit for bit against the
stem_rows_kernel -> conv3x3_2dw pair it replaces, at the smallest shapes where its tiling
(8 x 16 output tiles, 10 x 18 stem patches built by producer waves, ring over a workgroup's
tile run) can go wrong; once against the fp32 oracle; and the engine's lowering on CPU."""
import pytest
import torch

from kdl.ops.conv import MODE_CONV, ConvGemmLayer, Geometry
from kdl.ops.pack import pack_fragments, rowrun_weights, unpack_fragments

DEV = "cuda"
C3W_CFG = 215          # block1_conv2's tuned conv3x3_2dw config (same 8 x 16 tile)
FUSED_CFGS = range(4)  # KDL_SC3_CONFIGS: 4 / 2 producer waves, 2- / 3-deep ring


def _weights(seed):
    gen = torch.Generator().manual_seed(seed)
    w1 = torch.randn(32, 27, generator=gen, dtype=torch.float64) * 0.2 / 127.5     # k = (ky*3+kx)*3 + c
    b1 = torch.randn(32, generator=gen, dtype=torch.float64) * 0.1
    w2 = torch.zeros(64, 9 * 32, dtype=torch.float64)
    w2[:] = torch.randn(64, 288, generator=gen, dtype=torch.float64) / 288 ** 0.5
    b2 = torch.randn(64, generator=gen) * 0.1
    wp1 = pack_fragments(rowrun_weights(w1, 3, 9, 16), 2, 2).to(DEV).contiguous()
    lay = ConvGemmLayer("c2", MODE_CONV, w2, b2, cin_pad=32, n=64, relu_out=True, device=DEV)
    return gen, wp1, b1.float().to(DEV), lay


def _pair(img, wp1, b1, lay):
    """Today's two launches: stem_rows_kernel into a stem1 tensor, conv3x3_2dw from it."""
    from kdl.ops import _lib
    B, S = img.shape[0], img.shape[1]
    h1 = (S - 3) // 2 + 1
    stem1 = torch.zeros(B * h1 * h1 * 32, dtype=torch.bfloat16, device=DEV)
    _lib.lib().stem_conv(dict(x=_lib.ptr(img), wp=_lib.ptr(wp1), bias=_lib.ptr(b1), y=_lib.ptr(stem1), B=B, H=S, W=S,
                              OH=h1, OW=h1, ldy=32, in_kind=0, rows=1), _lib.stream_ptr())
    g = Geometry(B, h1, h1, h1 - 2, h1 - 2)
    y = torch.zeros(g.M * lay.ldy, dtype=torch.bfloat16, device=DEV)
    lay.launch(stem1, y, g, cfg=C3W_CFG)
    torch.cuda.synchronize()
    return stem1, y


def _fused(img, wp1, b1, lay, cfg, grid=0):
    from kdl.ops import _lib
    B, S = img.shape[0], img.shape[1]
    h1 = (S - 3) // 2 + 1
    y = torch.full((B * (h1 - 2) * (h1 - 2) * lay.ldy,), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.lib().stem_conv3x3(cfg, dict(x=_lib.ptr(img), wp1=_lib.ptr(wp1), b1=_lib.ptr(b1), wp2=_lib.ptr(lay.wp),
                                      b2=_lib.ptr(lay.bias), y=_lib.ptr(y), B=B, H=S, W=S, H1=h1, W1=h1,
                                      OH=h1 - 2, OW=h1 - 2, ldy=lay.ldy, NF=lay.nf_max, nstore=lay.ldy,
                                      relu_out=1, grid=grid), _lib.stream_ptr())
    torch.cuda.synchronize()
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,grids", [
    (3, 43, (0,)),      # 21^2 -> 19^2: ragged tiles in both directions, image boundaries inside a tile run
    (2, 37, (0,)),      # 18^2 -> 16^2: tiles divide exactly
    (1, 44, (0,)),      # even input size: last image row and column unused
    (3, 43, (2, 1)),    # 9 / 18 tiles per workgroup: the ring wraps more than twice
])
def test_fused_equals_two_launches(B, S, grids):
    gen, wp1, b1, lay = _weights(7)
    img = torch.randint(0, 256, (B, S, S, 3), generator=gen, dtype=torch.uint8).to(DEV)
    _, ref = _pair(img, wp1, b1, lay)
    assert torch.isfinite(ref.float()).all() and ref.float().abs().max() > 0
    for cfg in FUSED_CFGS:
        for grid in grids:
            y = _fused(img, wp1, b1, lay, cfg, grid)
            assert torch.equal(y, ref), f"cfg {cfg} grid {grid}: {(y.float() - ref.float()).abs().max().item()}"


@pytest.mark.gpu
@pytest.mark.parametrize("off", [1, 2, 3])
def test_image_pointer_at_any_byte(off):
    """A lane of a batch split starts at image k of the batch: 299 * 299 * 3 * k bytes in, not a
    multiple of 4 (here: a view ``off`` bytes into a buffer, so no byte behind the batch is readable
    by accident of alignment either)."""
    gen, wp1, b1, lay = _weights(10)
    B, S = 2, 43
    flat = torch.randint(0, 256, (B * S * S * 3 + off,), generator=gen, dtype=torch.uint8).to(DEV)
    img = flat[off:].view(B, S, S, 3)
    _, ref = _pair(img.clone(), wp1, b1, lay)
    for cfg in (0, 1):
        assert torch.equal(_fused(img, wp1, b1, lay, cfg), ref), f"cfg {cfg}"


@pytest.mark.gpu
def test_fused_against_fp32_oracle():
    from kdl.ops.reference import conv_gemm_ref
    gen, wp1, b1, lay = _weights(8)
    B, S = 2, 43
    h1 = (S - 3) // 2 + 1
    img = torch.randint(0, 256, (B, S, S, 3), generator=gen, dtype=torch.uint8).to(DEV)
    # stem in fp32 from the bf16-rounded weights the kernel multiplies with, rounded to bf16 like
    # every activation between two kernels; then the oracle of the second conv
    w1 = unpack_fragments(wp1.cpu(), 32, 48).view(32, 3, 16)[:, :, :9].reshape(32, 3, 3, 3).to(DEV)   # [n][ky][kx][c]
    s1 = torch.nn.functional.conv2d(img.float().permute(0, 3, 1, 2), w1.permute(0, 3, 1, 2), stride=2)
    s1 = torch.relu(s1 + b1[None, :, None, None]).permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    g = Geometry(B, h1, h1, h1 - 2, h1 - 2)
    ref = conv_gemm_ref(lay, s1, g)
    for cfg in FUSED_CFGS:
        y = _fused(img, wp1, b1, lay, cfg)
        err = (y.float().view(ref.shape) - ref).abs().max().item()
        scale = ref.abs().max().item() + 1e-6
        assert err <= 2e-2 * scale, f"cfg {cfg}: max err {err} vs scale {scale}"


@pytest.mark.gpu
def test_launcher_rejects_other_geometry():
    from kdl.ops import _lib
    gen, wp1, b1, lay = _weights(9)
    img = torch.zeros(1, 43, 43, 3, dtype=torch.uint8, device=DEV)
    y = torch.zeros(19 * 19 * 64, dtype=torch.bfloat16, device=DEV)
    ok = dict(x=_lib.ptr(img), wp1=_lib.ptr(wp1), b1=_lib.ptr(b1), wp2=_lib.ptr(lay.wp), b2=_lib.ptr(lay.bias),
              y=_lib.ptr(y), B=1, H=43, W=43, H1=21, W1=21, OH=19, OW=19, ldy=64, NF=4, nstore=64, relu_out=1)
    for bad in (dict(H1=20), dict(OH=21), dict(NF=2), dict(x=None), dict(grid=-1), dict(nstore=96)):
        with pytest.raises(RuntimeError):
            _lib.lib().stem_conv3x3(0, {**ok, **bad}, _lib.stream_ptr())
    with pytest.raises(RuntimeError):
        _lib.lib().stem_conv3x3(99, ok, _lib.stream_ptr())


def _engine(monkeypatch, fused):
    from kdl.engine import xception as XE
    from kdl.models import xception as X

    class Fake(XE.XceptionEngine):
        def __init__(self, p):
            self.device = torch.device("cpu")
            self.max_batch, self.buckets, self.steps, self.in_kind = 1, [1], [], "u8"
            self.head, self.size, self.shapes, self._remap = X.DEFAULT_HEAD, X.INPUT_SIZE, {}, {}
            self.fused_blocks = {}

    monkeypatch.delenv("KDL_STEM_FUSED_CFG", raising=False)
    monkeypatch.delenv("KDL_STEM_ROWS", raising=False)
    if fused is None:
        monkeypatch.delenv("KDL_STEM_FUSED", raising=False)
    else:
        monkeypatch.setenv("KDL_STEM_FUSED", fused)
    p = X.init_params(seed=0)
    e = Fake(p)
    e._build(p)
    return e


def test_lowering_switch(monkeypatch):
    """Switch on (the default): one step from the input to stem2, no stem1 buffer, one launch
    fewer. Switch off: the two-launch lowering, unchanged."""
    off = _engine(monkeypatch, "0")
    assert [(s.kind, s.name, s.src, s.dst) for s in off.steps[:2]] == [
        ("stem", "block1_conv1", "input", "stem1"), ("conv", "block1_conv2", "stem1", "stem2")]
    assert off.shapes["stem1"] == (149, 149, 32) and off.shapes["stem2"] == (147, 147, 64)
    for on in (_engine(monkeypatch, None), _engine(monkeypatch, "1")):
        st = on.steps[0]
        assert (st.kind, st.src, st.dst, st.geom) == ("stemconv", "input", "stem2", (299, 299, 147, 147))
        assert "stem1" not in on.shapes and on.shapes["stem2"] == (147, 147, 64)
        assert not any("stem1" in (s.src, s.dst, s.res) for s in on.steps)
        assert len(on.steps) == len(off.steps) - 1
        assert [s.name for s in on.steps[1:]] == [s.name for s in off.steps[2:]]
        assert {k: v for k, v in on.shapes.items()} == {k: v for k, v in off.shapes.items() if k != "stem1"}
    # the tuning table's entry for the fused step is optional; block1_conv2's may stay
    on.programs = {}
    on.apply_tuning({"block1_conv2": [0, 215]})
    assert on.stem_fused_cfg == 0
    on.apply_tuning({"block1_stem_conv": 2})
    assert on.stem_fused_cfg == 2
