"""The MBConv kernels called directly, against float64 references at their edges: every
dispatched instance of the direct depthwise kernel (K, S, SEG, CB, PD, SiLU: 256) and of the
tiled one (K, S, SEG, SiLU: 40, times CG 1..8) on maps of 1 x 1, 2 x 9, 7 x 10 and 12 x 11 with
ordinary, strongly negative, large and cancelling data; the fused squeeze-excite pool part by
part; se_kernel on synthetic pools on both sides of its Cs = 256 branch; chscale_kernel bit for
bit; the launchers' refusals; and a walk over EfficientNet-B7 that finds every instance the
engine launches in that matrix. Inputs, references and bounds are in _mbconv_cases.py;
test_mbconv_ops_cpu.py shows what the bounds let through and what they catch.

Every input sits between NaN guard rows (padding must come from the kernel's zeros, never from
memory), every output between guard rows of a fixed bit pattern, and the pool is NaN before the
launch: a part that is not written stays NaN, a part written beyond the last is seen."""
import functools

import pytest
import torch

import _mbconv_cases as MC
from kdl.models import efficientnet as E
from kdl.ops import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
S16 = MC.SENTINEL16
G = MC.GUARD


def _sync():
    torch.cuda.synchronize()


def _nan_guards_intact(buf: torch.Tensor) -> bool:
    return bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[-G:]).all())


@functools.lru_cache(maxsize=8)
def _on_device(key):
    """(case, x between NaN rows, w, bias, w1) on the GPU; the x buffer is kept alive with its view."""
    c = MC.dw_case(*key)
    xbuf, xmid = MC.guarded(c.B * c.H, c.W * c.C, torch.bfloat16, NAN, DEV)
    xmid.copy_(c.x.view(c.B * c.H, c.W * c.C))
    return c, (xbuf, xmid), c.w.to(DEV), c.bias.to(DEV), c.w1.to(DEV)


def _dwk(key, over: dict, act: int, with_pool: bool = True):
    """One launch between guards. Returns (y [B][OH][OW][C] bf16, pool [B][ntiles][Cs] or None,
    plan), all on the CPU, after the guard checks."""
    c, (_, xmid), w, bias, w1 = _on_device(key)
    C_ = _lib.lib()
    args = dict(c.geom(), act=act, x=xmid.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), **over)
    ybuf, ymid = MC.guarded(c.B * c.OH, c.OW * c.C, torch.int16, S16, DEV)
    args["y"] = ymid.data_ptr()
    plan = C_.dwk_plan(args)
    nt = plan["ntiles"]
    if with_pool:
        pbuf, pmid = MC.guarded(c.B * nt, c.Cs, torch.float32, NAN, DEV)
        args.update(pool=pmid.data_ptr(), w1=w1.data_ptr())
        assert C_.dwk_plan(args) == plan
    else:
        args["Cs"] = 0
    C_.dwk(args, _lib.stream_ptr())
    _sync()
    assert MC.guards_intact(ybuf, c.OW * c.C, S16), ("dwk wrote outside its output rows", key, over, act)
    y = ymid.view(torch.bfloat16).cpu().view(c.B, c.OH, c.OW, c.C)
    pool = None
    if with_pool:
        assert _nan_guards_intact(pbuf), ("dwk wrote a pool part outside its ntiles", key, over, act)
        pool = pmid.cpu().view(c.B, nt, c.Cs)
        assert bool(torch.isfinite(pool).all()), ("a pool part was not written", key, over, act)
    return y, pool, plan


def _check(key, over, act, y, pool, worst, missed):
    """Both bounds of one launch; a miss is recorded, so that a run reports all of them."""
    c = MC.dw_case(*key)
    err, bound = (y.double() - c.ref(act)).abs(), c.bound(act)
    ry = MC.ratio(err, bound)
    if not MC.within(err, bound):
        missed.append(("output err / bound", ry, "share", MC.share_over(err, bound), key, over, act))
    ref, pb = MC.pool_reference(y, c.w1, pool.shape[1])
    perr = (pool.double().sum(1) - ref).abs()
    rp = MC.ratio(perr, pb)
    if not MC.within(perr, pb):
        missed.append(("pool err / bound", rp, key, over, act))
    worst[0], worst[1] = max(worst[0], ry), max(worst[1], rp)


def _run_matrix(name, K, S, launches, explicit=True):
    """Every launch under both bounds; the first launch on the two-block ragged map again (bit-equal
    y and pool) and without a pool (bit-equal y)."""
    worst, n, repeated, missed = [0.0, 0.0], 0, False, []
    for key, over, act in launches:
        y, pool, plan = _dwk(key, over, act)
        if explicit:
            assert (plan["algo"], plan["seg"], plan["cb"]) == (over["algo"], over["seg"], over["cg"]), (plan, over)
            assert plan["pd"] == over.get("pd", 0) and (over["rb"] == 0 or plan["rb"] == over["rb"]), (plan, over)
            assert plan["tw"] == over.get("tw", 0), (plan, over)
        _check(key, over, act, y, pool, worst, missed)
        if not repeated and key[2] >= 12 and key[1] == 3:
            y2, pool2, _ = _dwk(key, over, act)
            assert torch.equal(y2.view(torch.int16), y.view(torch.int16)) and torch.equal(pool2, pool), (key, over)
            y3, _, _ = _dwk(key, over, act, with_pool=False)
            assert torch.equal(y3.view(torch.int16), y.view(torch.int16)), (key, over)
            repeated = True
        n += 1
    print(f"{name} K {K} S {S}: {n} launches, worst err / bound: output {worst[0]:.3f}, pool {worst[1]:.3f}")
    assert repeated
    assert not missed, (f"{len(missed)} of {n} launches missed a bound", missed[:8])


@pytest.mark.parametrize("K,S", MC.KS)
def test_dwv_every_instance(K, S):
    _run_matrix("dwv_kernel", K, S, MC.dwv_launches(K, S))


@pytest.mark.parametrize("K,S", MC.KS)
def test_dwk_every_instance(K, S):
    _run_matrix("dwk_kernel", K, S, MC.dwt_launches(K, S))


@pytest.mark.parametrize("K,S", MC.KS)
def test_dwk_fallback_heuristic(K, S):
    _run_matrix("dwk_kernel (own tiles)", K, S, MC.dwt_fallback_launches(K, S), explicit=False)


def test_dwk_big_patch_loops_go_round_again():
    """The K 5 / S 1 launches of the matrix with CG 8, rb 8, tw 19 stage 12 x 23 x 8 = 2208 vectors
    (more than 256 threads x 8) and hold more than 256 items."""
    big = [(k, o, a) for k, o, a in MC.dwt_launches(5, 1) if o.get("tw") == 19]
    assert len(big) == 2
    for key, over, act in big:
        c = MC.dw_case(*key)
        plan = _lib.lib().dwk_plan(dict(c.geom(), act=act, **over))
        PR, PC = (plan["rb"] - 1) * c.S + c.K, (plan["tw"] - 1) * c.S + c.K
        assert PR * PC * plan["cb"] > 2048
        assert plan["cb"] * plan["rb"] * -(-plan["tw"] // plan["seg"]) > 256
        assert plan["lds"] == PR * PC * plan["cb"] * 16 + c.K * c.K * plan["cb"] * 32


def test_every_b7_depthwise_instance_is_in_the_matrix():
    """What the engine launches for EfficientNet-B7 at 600 x 600 (the measured table's rows) and
    at 256 x 256 (no row matches), asked of the launcher's own plan: each (K, S, algo, seg, CB or
    CG, pd, SiLU) is an instance test_dwv_every_instance / test_dwk_every_instance ran."""
    C_ = _lib.lib()
    keys = MC.matrix_keys()
    for size in (600, 256):
        H = (size + 2 - 3) // 2 + 1
        for blk in E.blocks():
            pad = (blk.k - 1) // 2
            oh = (H + 2 * pad - blk.k) // blk.stride + 1
            plan = C_.dwk_plan(dict(B=1, H=H, W=H, C=blk.cexp, OH=oh, OW=oh, K=blk.k, S=blk.stride, pad=pad,
                                    Cs=blk.csq, act=2))
            key = (blk.k, blk.stride, plan["algo"], plan["seg"], plan["cb"], plan["pd"], 2)
            print(f"B7 at {size}: {blk.prefix} {H}x{H}x{blk.cexp} {blk.k}x{blk.k}/{blk.stride} -> algo {plan['algo']} "
                  f"seg {plan['seg']} cb {plan['cb']} pd {plan['pd']} rb {plan['rb']} tw {plan['tw']} "
                  f"ntiles {plan['ntiles']} lds {plan['lds']}")
            assert key in keys, (size, blk.prefix, key)
            H = oh


# ---------------------------------------------------------------------------------------------
# depthwise launcher refusals

REF_KEY = MC.dw_key("benign", 1, 12, 11, 64, 3, 1, 3)
DWK_REFUSED = [
    dict(algo=3), dict(algo=-1), dict(H=0), dict(W=0), dict(OH=0), dict(OW=0), dict(H=-12), dict(OW=-11),
    dict(pad=-1), dict(pad=3), dict(OH=13), dict(OW=12), dict(OH=11), dict(OH=6, OW=6), dict(Cs=0), dict(Cs=-1),
    dict(H=4, K=5, S=2, pad=0, OH=1, OW=4),      # H + 2 pad < K: (4 - 5) / 2 + 1 truncates to 1
    dict(C=60), dict(K=4), dict(K=7), dict(S=3), dict(S=0), dict(B=0),
    dict(algo=1, cg=3, rb=4, tw=4), dict(algo=1, cg=16, rb=4, tw=4), dict(algo=1, C=48, cg=4, rb=4, tw=4),
    dict(algo=1, seg=6), dict(algo=1, seg=2), dict(algo=2, seg=3), dict(algo=2, seg=5), dict(algo=2, pd=2),
    dict(algo=2, pd=4), dict(algo=1, cg=8, rb=40, tw=40),
]


@pytest.mark.parametrize("bad", DWK_REFUSED, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_dwk_refuses(bad):
    """Valid pointers, and buffers that would hold the launch were the check missing."""
    c, (_, xmid), _, bias, w1 = _on_device(REF_KEY)
    w = torch.zeros(5 * 5, c.C, device=DEV)      # room for the 5 x 5 taps that one case asks for
    ybuf, ymid = MC.guarded(c.B * c.OH, c.OW * c.C, torch.int16, S16, DEV)
    pbuf, pmid = MC.guarded(64, 4, torch.float32, NAN, DEV)
    args = dict(c.geom(), act=2, x=xmid.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), y=ymid.data_ptr(),
                pool=pmid.data_ptr(), w1=w1.data_ptr())
    C_ = _lib.lib()
    assert C_.dwk_plan(args)["ntiles"] <= 64
    args.update(bad)
    with pytest.raises(RuntimeError):
        C_.dwk_plan(args)
    with pytest.raises(RuntimeError):
        C_.dwk(args, _lib.stream_ptr())
    _sync()
    assert bool((ybuf == S16).all()) and bool(torch.isnan(pbuf).all())


# ---------------------------------------------------------------------------------------------
# squeeze-excite tail

def _se(inp, HW: int, over: dict | None = None):
    """One launch; the pool between NaN parts, the scale between NaN rows. Returns scale [B][C] on the CPU."""
    pool, b1, w2t, b2 = inp
    B, nt, Cs = pool.shape
    C = b2.numel()
    pbuf, pmid = MC.guarded(B * nt, Cs, torch.float32, NAN, DEV)
    pmid.copy_(pool.view(B * nt, Cs))
    sbuf, smid = MC.guarded(B, C, torch.float32, NAN, DEV)
    d = [t.to(DEV) for t in (b1, w2t, b2)]
    args = dict(pool=pmid.data_ptr(), b1=d[0].data_ptr(), w2t=d[1].data_ptr(), b2=d[2].data_ptr(),
                scale=smid.data_ptr(), B=B, ntiles=nt, HW=HW, C=C, Cs=Cs)
    args.update(over or {})
    try:
        _lib.lib().squeeze_excite(args, _lib.stream_ptr())
    finally:
        _sync()
        assert _nan_guards_intact(sbuf), "squeeze_excite wrote outside its scale rows"
        if over:
            assert bool(torch.isnan(sbuf).all())
    return smid.cpu()


@pytest.mark.parametrize("Cs", MC.SE_CS)
def test_squeeze_excite(Cs):
    worst = 0.0
    for nt in MC.se_ntiles(Cs):
        for C in MC.SE_C:
            for B in MC.SE_B:
                inp = MC.se_inputs(B, nt, C, Cs)
                ref, bound = MC.se_reference(*inp, 132)
                err = (_se(inp, 132).double() - ref).abs()
                assert MC.within(err, bound), (Cs, nt, C, B, MC.ratio(err, bound))
                worst = max(worst, MC.ratio(err, bound))
    print(f"se_kernel Cs {Cs}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("Cs", [20, 300])
def test_squeeze_excite_extreme_logits(Cs):
    for B in MC.SE_B:
        inp = MC.se_inputs(B, 7, 264, Cs, logit=100.0)
        ref, bound = MC.se_reference(*inp, 132)
        got = _se(inp, 132)
        assert MC.within((got.double() - ref).abs(), bound)
        assert bool(((got == 0) | (got == 1)).all()) and bool((got == 0).any()) and bool((got == 1).any())


@pytest.mark.parametrize("bad", [dict(HW=0), dict(HW=-132), dict(B=0), dict(ntiles=0), dict(C=0), dict(Cs=0)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_squeeze_excite_refuses(bad):
    with pytest.raises(RuntimeError):
        _se(MC.se_inputs(1, 3, 264, 20), 132, bad)


def test_squeeze_excite_refuses_an_lds_request_over_160_kib():
    Cs = 41000                                   # (256 + Cs) floats > 160 KiB
    with pytest.raises(RuntimeError):
        _se((torch.zeros(1, 1, Cs), torch.zeros(Cs), torch.zeros(Cs, 8), torch.zeros(8)), 132, dict(Cs=Cs))


# ---------------------------------------------------------------------------------------------
# channel scale

def _chscale(y, scale, **over):
    B, HW, C = y.shape
    ybuf, ymid = MC.guarded(B * HW, C, torch.int16, S16, DEV)
    ymid.copy_(y.view(torch.int16).view(B * HW, C))
    before = ybuf.clone()
    sd = scale.to(DEV)
    args = dict(y=ymid.data_ptr(), scale=sd.data_ptr(), B=B, HW=HW, C=C)
    args.update(over)
    try:
        _lib.lib().channel_scale(args, _lib.stream_ptr())
    finally:
        _sync()
        assert MC.guards_intact(ybuf, C, S16), "channel_scale wrote outside its rows"
        if over:
            assert torch.equal(ybuf, before)
    return ymid.cpu().view(B, HW, C)


@pytest.mark.parametrize("HW,C", MC.CHS_SHAPES)
def test_channel_scale_is_exact(HW, C):
    for B in (1, 3):
        y, scale = MC.chscale_inputs(B, HW, C)
        got = _chscale(y, scale)
        assert torch.equal(got, MC.chscale_expected(y, scale).view(torch.int16)), (B, HW, C)


@pytest.mark.parametrize("bad", [dict(C=12), dict(B=0), dict(HW=0), dict(HW=-7)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_channel_scale_refuses(bad):
    y, scale = MC.chscale_inputs(1, 7, 264)
    with pytest.raises(RuntimeError):
        _chscale(y, scale, **bad)


def test_channel_scale_refuses_more_images_than_grid_rows():
    B = 65536                                    # blockIdx.y holds the image: at most 65535
    y = torch.ones(B, 1, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        _chscale(y, torch.ones(B, 8), B=B)
