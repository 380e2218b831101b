"""The classifier tails called directly, against float64 references at their edges: fc_mfma on
both sides of its 16-row fragments and its 64-row blocks, with one and three k-steps for its four
waves, ReLU and both types, and NaN in the rows of xb that only pad a fragment; head_dense with
one image, eight and nine, fewer pixels than pixel groups, a single K block, one hidden unit, 128
of them, more than 16 logits and padded rows; gap on both sides of its 8 pixel parts and its
four-deep unrolled loop. Inputs, references and bounds are in _tail_cases.py; test_tail_ops_cpu.py
shows what the bounds let through and what they catch. Every output sits between NaN guard rows."""
import pytest
import torch

import _tail_cases as TC
from kdl.ops import _lib
from kdl.ops.pack import pack_fragments

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
G = TC.GUARD


def _nan_guards_intact(buf: torch.Tensor) -> bool:
    return bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all())


# ---------------------------------------------------------------------------------------------
# fc_mfma

def _fc(B, F, N, relu, dt, nan_rows, over=None):
    x, w, bias = TC.fc_inputs(B, F, N, dt)
    nf = (N + 15) // 16
    rows = TC.round_up(B, 16)
    xb = torch.full((rows, F), NAN if nan_rows else 0.0, dtype=TC.DTYPES[dt], device=DEV)
    xb[:B] = x.to(TC.DTYPES[dt]).to(DEV)
    wp = pack_fragments(w, nf, F // 32, TC.DTYPES[dt]).to(DEV)
    bd = bias.to(DEV)
    obuf, omid = TC.guarded(B, N, torch.float32, NAN, DEV)
    args = dict(xb=xb.data_ptr(), wp=wp.data_ptr(), bias=bd.data_ptr(), out=omid.data_ptr(), B=B, F=F, N=N, NF=nf,
                relu=relu, dt=dt)
    args.update(over or {})
    try:
        _lib.lib().fc_mfma(args, _lib.stream_ptr())
    finally:
        torch.cuda.synchronize()
        assert _nan_guards_intact(obuf), ("fc_mfma wrote a row outside [0, B)", B, F, N)
    return omid.cpu()


def test_fc_mfma_every_edge():
    worst, missed = {}, []
    for B, F, N, relu, dt, nan_rows in TC.fc_launches():
        got = _fc(B, F, N, relu, dt, nan_rows)
        ref, bound = TC.fc_reference(*TC.fc_inputs(B, F, N, dt), relu)
        err = (got.double() - ref).abs()
        r = TC.ratio(err, bound)
        key = (F, N, "fp16" if dt else "bf16")
        worst[key] = max(worst.get(key, 0.0), r) if r == r else r
        if not TC.within(err, bound):
            missed.append((f"B {B} F {F} N {N} relu {relu} dt {dt} NaN rows {nan_rows}", "worst err / bound", r))
    for key, r in worst.items():
        print(f"fc_mfma_kernel F {key[0]} N {key[1]} {key[2]}: worst err / bound {r:.3f}")
    assert not missed, (len(missed), missed[:8])


@pytest.mark.parametrize("bad", [dict(B=0), dict(F=48), dict(NF=0), dict(dt=2), dict(dt=-1)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_fc_mfma_refuses(bad):
    with pytest.raises(RuntimeError):
        _fc(17, 96, 10, 0, 0, False, bad)
    _fc(17, 96, 10, 0, 0, False)


# ---------------------------------------------------------------------------------------------
# gap

@pytest.mark.parametrize("F", TC.GAP_F)
def test_gap_on_both_sides_of_its_parts(F):
    worst = 0.0
    for dt in (0, 1):
        for HW in TC.GAP_HW:
            for B, ldx in ((1, F), (2, F + 8)):
                x = TC.gap_inputs(B, HW, F, ldx, dt)
                xd = x.to(DEV)
                ybuf, ymid = TC.guarded(B, F, torch.float32, NAN, DEV)
                bbuf, bmid = TC.guarded(B, F, torch.int16, TC.SENTINEL16, DEV)
                _lib.lib().gap(dict(x=xd.data_ptr(), y=ymid.data_ptr(), yb=bmid.data_ptr(), B=B, HW=HW, ldx=ldx, F=F,
                                    dt=dt), _lib.stream_ptr())
                torch.cuda.synchronize()
                assert _nan_guards_intact(ybuf) and TC.guards_intact(bbuf, F, TC.SENTINEL16), (dt, HW, B, ldx)
                ref, b32, b16 = TC.gap_reference(x, F, dt)
                e32 = (ymid.cpu().double() - ref).abs()
                e16 = (bmid.view(TC.DTYPES[dt]).cpu().double() - ref).abs()
                r = max(TC.ratio(e32, b32), TC.ratio(e16, b16))
                assert TC.within(e32, b32) and TC.within(e16, b16), (f"gap dt {dt} HW {HW} B {B} ldx {ldx} F {F}", r)
                worst = max(worst, r)
    print(f"gap_kernel F {F}: worst err / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------
# head_dense

def _head(key, **over):
    x, w1t, b1, w2, b2 = TC.head_inputs(*key)
    _, B, HW, F, H1, NC, pad = key
    d = [t.to(DEV) for t in (x, w1t, b1, w2, b2)]
    hbuf, hmid = TC.guarded(F // 64 * B, H1, torch.float32, NAN, DEV)
    obuf, omid = TC.guarded(B, NC, torch.float32, NAN, DEV)
    args = dict(x=d[0].data_ptr(), w1=d[1].data_ptr(), b1=d[2].data_ptr(), w2=d[3].data_ptr(), b2=d[4].data_ptr(),
                out=omid.data_ptr(), hid=hmid.data_ptr(), B=B, HW=HW, ldx=F + pad, F=F, H1=H1, NC=NC)
    args.update(over)
    try:
        _lib.lib().head_dense(args, _lib.stream_ptr())
    finally:
        torch.cuda.synchronize()
        assert _nan_guards_intact(hbuf) and _nan_guards_intact(obuf), ("head_dense wrote outside hid or out", key)
        if over:
            assert bool(torch.isnan(hbuf).all()) and bool(torch.isnan(obuf).all())
    return omid.cpu()


@pytest.mark.parametrize("key", TC.HEAD_CASES, ids=lambda k: "-".join(str(v) for v in k))
def test_head_dense_edges(key):
    got = _head(key)
    ref, bound, _ = TC.head_reference(*TC.head_inputs(*key))
    err = (got.double() - ref).abs()
    r = TC.ratio(err, bound)
    print(f"head_dense {key}: worst err / bound {r:.4f}")
    assert TC.within(err, bound), (f"head_dense {key}", "worst err / bound", r)
    assert torch.equal(_head(key), got)


HEAD_OK = ("benign", 8, 3, 128, 100, 10, 8)      # H1 = 100, NC = 10: the engine's own head


@pytest.mark.parametrize("bad", [dict(ldx=120), dict(ldx=64), dict(HW=0), dict(HW=-3), dict(F=96, ldx=96), dict(B=0),
                                 dict(H1=0), dict(H1=129), dict(NC=0),
                                 dict(NC=127),       # (128 + 128 * 127 + 256) * 4 bytes > 64 KB
                                 dict(H1=100, NC=163)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_head_dense_refuses(bad):
    """Next to a launch of the same arguments without the fault; nothing is written by a refused one."""
    key = ("benign", 1, 100, 128, 128, 17, 0) if bad.get("NC", 0) == 127 else HEAD_OK
    with pytest.raises(RuntimeError):
        _head(key, **bad)
    got = _head(key)
    ref, bound, _ = TC.head_reference(*TC.head_inputs(*key))
    assert TC.within((got.double() - ref).abs(), bound)


def test_head_dense_largest_lds_request_that_fits():
    """H1 = 128, NC = 125: (128 + 128 * 125 + 256) * 4 = 65536 bytes, the limit itself."""
    gen = torch.Generator().manual_seed(3)
    B, HW, F, H1, NC = 2, 5, 64, 128, 125
    x = torch.randn(B, HW, F, generator=gen).to(torch.bfloat16)
    w1t, b1 = torch.randn(H1, F, generator=gen) / 8, torch.randn(H1, generator=gen) * 0.1
    w2, b2 = torch.randn(H1, NC, generator=gen) / 11, torch.randn(NC, generator=gen) * 0.1
    ref, bound, _ = TC.head_reference(x, w1t, b1, w2, b2)
    d = [t.to(DEV) for t in (x, w1t, b1, w2, b2)]
    hid = torch.zeros(B, H1, device=DEV)
    obuf, omid = TC.guarded(B, NC, torch.float32, NAN, DEV)
    _lib.lib().head_dense(dict(x=d[0].data_ptr(), w1=d[1].data_ptr(), b1=d[2].data_ptr(), w2=d[3].data_ptr(),
                               b2=d[4].data_ptr(), out=omid.data_ptr(), hid=hid.data_ptr(), B=B, HW=HW, ldx=F, F=F,
                               H1=H1, NC=NC), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _nan_guards_intact(obuf)
    assert TC.within((omid.cpu().double() - ref).abs(), bound)
