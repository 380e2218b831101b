"""Two-phase schedule of the block-3 entry kernel (entry_block.hip config 21: a step skewed by one stage,
two barriers per step) against config 1 on the same input, bit for bit, and against the fp32
Keras-semantics oracle of the block with the bound of tests/test_entry_block_gpu.py.

The kernel takes H and W at run time, so the maps are small even ones (leading pool pad 0, what the
config is built for) with block 3's channels (128 -> 256). Inputs and weights are random with negative
values, so the leading ReLU and the -inf pool borders matter; every output buffer is filled with NaN
before the launch."""
import pytest
import torch

from kdl.models import xception as X
from kdl.models.layers import maxpool_same

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE = 1                  # the four-phase config the new one must reproduce
NEW = 21


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


# (H, W, B). (6, 6): one strip, 3 pooled rows, a run is mostly warm-up. (10, 30): OW 15 = a strip of 13
# pooled columns and a ragged one of 2. (30, 10): one strip of 5 columns, 15 pooled rows wrap the rings.
# (32, 56): OW 28 = strips of 13, 13 and 2. (74, 74) at batch 2: the served geometry.
SHAPES = [(6, 6, 2), (10, 30, 2), (30, 10, 2), (32, 56, 2), (74, 74, 2)]
# grid 1: one workgroup walks every run back to back; 7 cuts runs in the middle; None: one per CU.
# (74, 74) at batch 2 on ONE workgroup is 6 runs of 37 + 2 steps = 234 > EB_MAX_STEPS (128): the host
# refuses that plan for every config (asserted below), so that one pair runs at batch 1 instead
# (3 runs back to back, 117 steps)
GRIDS = [1, 2, 3, 7, None]
CASES = [(H, W, B, g) for H, W, B in SHAPES for g in GRIDS if (H, g) != (74, 1)] + [(74, 74, 1, 1)]


@pytest.mark.parametrize("H,W,B,grid", CASES)
def test_twophase_equals_config1_and_matches_oracle(xparams, H, W, B, grid):
    x, ref = _input_and_oracle(xparams, B, H, W)
    base = _run(xparams, BASE, x, B, H, W, grid)
    got = _run(xparams, NEW, x, B, H, W, grid)
    assert torch.isfinite(base.float()).all() and torch.isfinite(got.float()).all()   # every NaN overwritten
    err = ((got.float().cpu() - ref).abs().max() / ref.abs().max()).item()
    err_base = ((base.float().cpu() - ref).abs().max() / ref.abs().max()).item()
    ndiff = int((got.view(torch.int16) != base.view(torch.int16)).sum().item())
    print(f"two-phase cfg {NEW} ({H}x{W}, B={B}, grid={grid}): rel max err vs oracle {err:.2e} "
          f"(config {BASE}: {err_base:.2e}); {ndiff} of {got.numel()} differ from config {BASE}")
    assert err < 2e-2 and err_base < 2e-2, (err, err_base)
    assert torch.equal(got, base), ndiff


def test_twophase_one_workgroup_plan_of_the_served_map_is_refused(xparams):
    """(74, 74), B = 2 on one workgroup: 234 steps > EB_MAX_STEPS, the pair left out of CASES."""
    from kdl.ops.entry_block import EntryBlock
    s1, s2, r = _block3_layers(xparams)
    for cfg in (BASE, NEW):
        eb = EntryBlock("block3", s1, s2, r, device=DEV, grid=1, cfg=cfg)
        with pytest.raises(AssertionError, match="EB_MAX_STEPS"):
            eb.plan(2, 37, 37)


def test_twophase_refuses_an_odd_map(xparams):
    """Config 21 is built for the leading pool pad 0 (even maps), as config 1 is: the launcher returns
    hipErrorInvalidValue for a 9 x 9 map and the binding raises."""
    x = torch.randn(1, 9, 9, 128).to(torch.bfloat16).to(DEV)
    for cfg in (BASE, NEW):
        with pytest.raises(RuntimeError, match="(?i)invalid"):
            _run(xparams, cfg, x, 1, 9, 9, 1)


def test_twophase_replays_bit_identical(xparams):
    x, _ = _input_and_oracle(xparams, 2, 32, 56)
    y1 = _run(xparams, NEW, x, 2, 32, 56, None)
    y2 = _run(xparams, NEW, x, 2, 32, 56, None)
    assert torch.isfinite(y1.float()).all()
    assert y1.view(torch.int16).equal(y2.view(torch.int16))
