"""Peeled-tail builds of the warp-specialized separable conv (sepconv_ws.hip TAIL: no padding
k-step, no load of a stage past the last one) against their parent ids, bit for bit, and against
the fp32 reference with the gate of tests/test_kernels_gpu.py.

K = 32 .. 224 and 736 give KT = 1 .. 7 and 23: below, at and just above STAGES - 1 = 4 (the
prologue must stop at KT stages), odd and even step counts (the unroll by two), and the shipped
depth. B = 2 at 5x7 is one ragged M tile; B = 3 at 9x9 several tiles, the last one ragged, image
borders inside a tile, and tiles that start K at a rotated offset (krot = 7 * tile % KT).
"""
import pytest
import torch

from kdl.ops import _lib
from kdl.ops.conv import MODE_DW, Geometry, cfg_tile, config_applicable
from kdl.ops.reference import conv_gemm_ref
from test_kernels_gpu import DEV, _check, _layer, _rand_act

pytestmark = pytest.mark.gpu

# new id -> the id it is built from
TWINS = {150: 148, 151: 149, 152: 156, 153: 157, 154: 158, 155: 125}
SHAPES = [(2, 5, 7), (3, 9, 9)]          # (B, H, W)
# n = 384: one N tile; n = 728: N = 768 computed in two tiles, 728 channels stored
NS = [384, 728]


def _run(lay, cfg, x, y, g, res, nstore):
    args = lay.args(_lib.ptr(x), _lib.ptr(y), g, _lib.ptr(res) if res is not None else None, cfg=cfg)
    args["nstore"] = nstore
    _lib.lib().conv_gemm(MODE_DW, cfg, args, _lib.stream_ptr())


@pytest.mark.parametrize("K", [32, 64, 96, 128, 160, 192, 224, 736])
def test_tail_equals_parent_and_reference(K):
    gen = torch.Generator().manual_seed(100 + K)
    for n in NS:
        for relu_in in (True, False):
            lay = _layer(MODE_DW, K, n, gen, relu_in=relu_in)
            assert lay.K == K
            for B, H, W in SHAPES:
                g = Geometry(B, H, W, H, W)
                x = _rand_act((B, H, W), lay.cin_pad, K, gen)
                for with_res in (False, True):
                    res = _rand_act((B, H, W), lay.ldy, n, gen) if with_res else None
                    ref = conv_gemm_ref(lay, x, g, res=res)
                    for cfg, parent in TWINS.items():
                        assert config_applicable(cfg, W, K, n) and (False, cfg) in lay.variants(W)
                        tag = f"cfg {cfg} K {K} n {n} B{B} {H}x{W} relu_in {relu_in} res {with_res}"
                        if B == 3:       # several M tiles: the rotated ids start K at a non-zero offset
                            assert -(-g.M // cfg_tile(cfg)[0]) >= 3, tag
                        y = torch.zeros(g.M * lay.ldy, dtype=torch.bfloat16, device=DEV)
                        yp = torch.zeros_like(y)
                        _run(lay, cfg, x, y, g, res, n)
                        _run(lay, parent, x, yp, g, res, n)
                        torch.cuda.synchronize()
                        assert torch.equal(y, yp), tag
                        try:
                            _check(y, ref, n)
                        except AssertionError as e:
                            raise AssertionError(f"{tag}: {e}") from None


@pytest.mark.parametrize("K", [96, 736])
def test_tail_replay_same_buffers(K):
    """One launch three times into the same buffers: a stale ring slot or A buffer would show."""
    gen = torch.Generator().manual_seed(7)
    lay = _layer(MODE_DW, K, 728, gen, relu_in=True)
    B, H, W = 3, 9, 9
    g = Geometry(B, H, W, H, W)
    x = _rand_act((B, H, W), lay.cin_pad, K, gen)
    res = _rand_act((B, H, W), lay.ldy, 728, gen)
    for cfg in TWINS:
        y = torch.zeros(g.M * lay.ldy, dtype=torch.bfloat16, device=DEV)
        outs = []
        for _ in range(3):
            _run(lay, cfg, x, y, g, res, 728)
            torch.cuda.synchronize()
            outs.append(y.clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"cfg {cfg} K {K}"
