"""Block-3 entry kernel with both depthwise convs on the matrix cores in the two-phase step
(entry_block.hip config 23: config 21's schedule, the depthwise as block-diagonal MFMAs) against the fp32
Keras-semantics oracle of the block with the bound of tests/test_entry_block_gpu.py.

No bit comparison with config 21: v_dot2c adds tap pairs in sequence in fp32, the MFMA sums its 32
products its own way, and a depthwise output may round to the neighbouring bf16. What must hold bit
for bit is the kernel against itself: an element's arithmetic does not depend on the plan (every grid
of a shape gives the same output) nor on the launch.

The kernel takes H and W at run time, so the maps are small even ones (leading pool pad 0) with block
3's channels (128 -> 256). Inputs and weights are random with negative values, so the leading ReLU and
the -inf pool borders matter; every output buffer is filled with NaN before the launch."""
import pytest
import torch

from kdl.models import xception as X
from kdl.models.layers import maxpool_same

pytestmark = pytest.mark.gpu
DEV = "cuda"
VALU = 21                 # the same schedule with the depthwise on the VALU: its error is printed beside
NEW = 23


def _block_oracle(p, x_nhwc, blk):
    """fp32 forward of entry block ``blk`` of X.SPEC on an NHWC input."""
    x = x_nhwc.float().permute(0, 3, 1, 2)
    b = X.SPEC[blk - 1]
    res = X._bn(X._conv(x, p, b.res_conv), p, b.res_conv.bn, False)
    y = x
    for op in b.main:
        y = X._bn(X._sep(torch.relu(y) if op.relu_in else y, p, op), p, op.bn, False)
        if op.relu_out:
            y = torch.relu(y)
    return (maxpool_same(y, 3, 2) + res).permute(0, 2, 3, 1)


_LAYERS = {}
_INPUTS = {}
_OUTS = {}


def _block3_layers(xparams):
    if "l" not in _LAYERS:
        from kdl.engine.xception import XceptionEngine as XE
        b = X.SPEC[2]
        _LAYERS["l"] = (XE._sep(xparams, b.main[0], DEV), XE._sep(xparams, b.main[1], DEV),
                        XE._pw(xparams, b.res_conv, DEV))
    return _LAYERS["l"]


def _input_and_oracle(xparams, B, H, W):
    """One seeded input with negative values (block 2's output is a sum) and its oracle per shape, shared."""
    key = (B, H, W)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(100 * H + W + B)
        x = torch.randn(B, H, W, 128, generator=gen).to(torch.bfloat16)
        _INPUTS[key] = (x.to(DEV), _block_oracle(xparams, x.float(), 3))
    return _INPUTS[key]


def _run(xparams, cfg, x, B, H, W, grid):
    from kdl.ops.entry_block import EntryBlock
    s1, s2, r = _block3_layers(xparams)
    eb = EntryBlock("block3", s1, s2, r, device=DEV, grid=grid, cfg=cfg)
    y = torch.full((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 256), float("nan"), dtype=torch.bfloat16, device=DEV)
    eb.emit(None, x.data_ptr(), y.data_ptr(), B, H, W)
    torch.cuda.synchronize()
    return y


def _out(xparams, cfg, H, W, B, grid):
    """The output of one (config, shape, grid), computed once and left unchanged."""
    key = (cfg, H, W, B, grid)
    if key not in _OUTS:
        x, _ = _input_and_oracle(xparams, B, H, W)
        _OUTS[key] = _run(xparams, cfg, x, B, H, W, grid)
    return _OUTS[key]


def _rel_err(y, ref):
    return ((y.float().cpu() - ref).abs().max() / ref.abs().max()).item()


# (H, W, B). (6, 6): one strip, 3 pooled rows, a run is mostly warm-up. (10, 30): OW 15 = a strip of 13
# pooled columns and a ragged one of 2. (30, 10): one strip of 5 columns, 15 pooled rows wrap the rings.
# (32, 56): OW 28 = strips of 13, 13 and 2, cut in mid-run by grids 3 and 7. The served 74 x 74 map is the
# engine and bench tests'.
SHAPES = [(6, 6, 2), (10, 30, 2), (30, 10, 2), (32, 56, 2)]
# grid 1: one workgroup walks every run back to back; 7 cuts runs in the middle; None: one per CU
GRIDS = [1, 2, 3, 7, None]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("H,W,B", SHAPES)
def test_dwm_matches_oracle_and_replays(xparams, H, W, B, grid):
    x, ref = _input_and_oracle(xparams, B, H, W)
    got = _out(xparams, NEW, H, W, B, grid)
    assert torch.isfinite(got.float()).all()                     # every NaN overwritten
    err, err_valu = _rel_err(got, ref), _rel_err(_out(xparams, VALU, H, W, B, None), ref)
    print(f"MFMA-depthwise cfg {NEW} ({H}x{W}, B={B}, grid={grid}): rel max err vs oracle {err:.2e} "
          f"(config {VALU}: {err_valu:.2e})")
    assert err < 2e-2, err
    again = _run(xparams, NEW, x, B, H, W, grid)                 # a second launch: the same bits
    assert again.view(torch.int16).equal(got.view(torch.int16))


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_dwm_output_does_not_depend_on_the_plan(xparams, H, W, B):
    """Every grid deals the same elements out differently (other run lengths, warm-up steps and ring
    slots); the bits must not move."""
    base = _out(xparams, NEW, H, W, B, GRIDS[0])
    for grid in GRIDS[1:]:
        got = _out(xparams, NEW, H, W, B, grid)
        ndiff = int((got.view(torch.int16) != base.view(torch.int16)).sum().item())
        assert ndiff == 0, (grid, ndiff, got.numel())


def test_dwm_refuses_an_odd_map(xparams):
    """Config 23 is built for the leading pool pad 0 (even maps), as config 21 is: the launcher returns
    hipErrorInvalidValue for a 9 x 9 map and the binding raises."""
    x = torch.randn(1, 9, 9, 128).to(torch.bfloat16).to(DEV)
    with pytest.raises(RuntimeError, match="(?i)invalid"):
        _run(xparams, NEW, x, 1, 9, 9, 1)
