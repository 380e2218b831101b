"""Row-pair depthwise of the warp-specialized block-2 kernel (entry_block.hip configs 17 / 19: a step's
two adjacent rows share their depthwise tap reads) against config 15 on the same input, bit for bit, and
against the fp32 Keras-semantics oracle of the block with the bound of tests/test_entry_block_gpu.py.

The kernel takes H and W at run time, so the maps are small odd ones (leading pool pad 1) with block 2's
channels (64 -> 128); every output buffer is filled with NaN before the launch."""
import numpy as np
import pytest
import torch

from kdl.models import xception as X
from kdl.models.layers import maxpool_same

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE = 15                 # the config the row-pair builds must reproduce
NEW = [17, 19]            # row-pair builds: CDW 0 / 1 (dw2 items per consumer wave)


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


def _layers(p, blk):
    from kdl.engine.xception import XceptionEngine as XE
    b = X.SPEC[blk - 1]
    return XE._sep(p, b.main[0], DEV), XE._sep(p, b.main[1], DEV), XE._pw(p, b.res_conv, DEV)


_LAYERS = {}
_INPUTS = {}


def _block2_layers(xparams):
    if "l" not in _LAYERS:
        _LAYERS["l"] = _layers(xparams, 2)
    return _LAYERS["l"]


def _input_and_oracle(xparams, B, H, W):
    """One seeded post-ReLU input (block1_conv2's output is one) and its oracle per shape, shared."""
    key = (B, H, W)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(100 * H + W + B)
        x = torch.relu(torch.randn(B, H, W, 64, generator=gen)).to(torch.bfloat16)
        _INPUTS[key] = (x.to(DEV), _block_oracle(xparams, x.float(), 2))
    return _INPUTS[key]


def _run(xparams, cfg, x, B, H, W, grid):
    from kdl.ops.entry_block import EntryBlock
    s1, s2, r = _block2_layers(xparams)
    eb = EntryBlock("block2", s1, s2, r, device=DEV, grid=grid, cfg=cfg)
    y = torch.full((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 128), float("nan"), dtype=torch.bfloat16, device=DEV)
    eb.emit(None, x.data_ptr(), y.data_ptr(), B, H, W)
    torch.cuda.synchronize()
    return y


def _ulps(a, b):
    """|a - b| in bf16 units in the last place (distance of the ordered bit patterns), per element."""
    def key(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


# (H, W, B, grid). (5, 5): every row and column is a border, the first output step follows its two warm-ups
# directly. (9, 29): OW 15 = a strip of 13 pooled columns and one of 2; (29, 9): one strip of 5 columns, the
# second column fragment is empty. (31, 55): OW 28 = strips of 13, 13 and 2; 16 pooled rows wrap the x and
# y1 rings several times; grid 7 splits runs in mid-strip; grid 2 is the smallest whose step tables fit
# (grid 1 would need 3 x 3 x 18 = 162 steps: refused, see below); None = one workgroup per work item here.
CASES = [(5, 5, 1, 1),
         (9, 29, 2, 1), (9, 29, 2, 3), (29, 9, 2, 1), (29, 9, 2, 3),
         (31, 55, 3, 2), (31, 55, 3, 7), (31, 55, 3, None)]


@pytest.mark.parametrize("cfg", NEW)
@pytest.mark.parametrize("H,W,B,grid", CASES)
def test_rowpair_equals_config15_and_matches_oracle(xparams, H, W, B, grid, cfg):
    x, ref = _input_and_oracle(xparams, B, H, W)
    base = _run(xparams, BASE, x, B, H, W, grid)
    got = _run(xparams, cfg, x, B, H, W, grid)
    assert torch.isfinite(base.float()).all() and torch.isfinite(got.float()).all()   # every NaN overwritten
    err = ((got.float().cpu() - ref).abs().max() / ref.abs().max()).item()
    err_base = ((base.float().cpu() - ref).abs().max() / ref.abs().max()).item()
    d = _ulps(got, base)
    worst = int(d.max().item())
    where = [int(i) for i in np.unravel_index(int(d.argmax().item()), tuple(d.shape))]
    print(f"rowpair cfg {cfg} ({H}x{W}, B={B}, grid={grid}): rel max err vs oracle {err:.2e} (config {BASE}: {err_base:.2e}); vs config {BASE}: "
          f"{int((d > 0).sum().item())} of {d.numel()} differ, largest {worst} bf16 ulp at [b, row, col, ch] = {where}")
    assert err < 2e-2 and err_base < 2e-2, (err, err_base)
    assert torch.equal(got, base), (worst, where)


def test_rowpair_one_workgroup_plan_of_the_longest_table_is_refused(xparams):
    """(31, 55), B = 3 on one workgroup: 9 runs of 16 rows + 2 warm-ups = 162 steps > EB_MAX_STEPS."""
    from kdl.ops.entry_block import EntryBlock
    s1, s2, r = _block2_layers(xparams)
    for cfg in NEW:
        eb = EntryBlock("block2", s1, s2, r, device=DEV, grid=1, cfg=cfg)
        with pytest.raises(AssertionError, match="EB_MAX_STEPS"):
            eb.plan(3, 16, 28)


@pytest.mark.parametrize("cfg", NEW)
def test_rowpair_replays_bit_identical(xparams, cfg):
    x, _ = _input_and_oracle(xparams, 2, 31, 55)
    y1 = _run(xparams, cfg, x, 2, 31, 55, None)
    y2 = _run(xparams, cfg, x, 2, 31, 55, None)
    assert torch.isfinite(y1.float()).all()
    assert y1.view(torch.int16).equal(y2.view(torch.int16))
