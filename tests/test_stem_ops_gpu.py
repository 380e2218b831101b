"""stem_kernel and stem_rows_kernel called directly through stem_conv, every instance the launcher
dispatches, against float64 references on the smallest maps at which they can go wrong: one
output pixel, fewer pixels than a fragment / a wave / a block, 128 and 129 pixels, maps smaller
than the padding, non-square maps, a fragment that spans two images, and for the row-run kernel
an image pointer at every byte offset. Inputs, references and bounds are in _stem_cases.py;
test_stem_ops_cpu.py shows what the bounds let through and what they catch.

The output sits between guard rows of a fixed bit pattern, with ldy = cout + 8 in half of the
launches; a float image sits between NaN floats, so that an unmasked read outside the tensor
turns an output into NaN even through a zero weight."""
import pytest
import torch

import _stem_cases as SC
from kdl.ops import _lib
from kdl.ops.pack import pack_fragments, rowrun_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
S16 = SC.SENTINEL16
PAD = 64                    # guard bytes / floats on each side of an image


def _args(L: SC.Launch, keep: list) -> tuple:
    """(args of the launch, guarded y buffer, its middle rows). keep holds the device tensors."""
    c, i, p = SC.case(L), L.inst, L.prob
    nf, KT = i.cout // 16, SC.kt_of(i)
    wnk = c.w.reshape(i.cout, -1)
    if i.kernel == "rows":
        wnk = rowrun_weights(wnk, i.KW, 3 * i.KW, SC.rp_of(i.KW))
    wp = pack_fragments(wnk, nf, KT, SC.DTYPES[i.dt]).to(DEV)
    bias = c.bias.to(DEV)
    total = c.img.numel()
    if i.in_kind == 0:
        xbuf = torch.full((PAD + L.off + total + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
        xbuf[PAD + L.off:PAD + L.off + total] = c.img.reshape(-1).to(DEV)
        xptr = xbuf.data_ptr() + PAD + L.off
        assert xptr % 4 == L.off
    else:
        assert L.off == 0
        xbuf = torch.full((PAD + total + PAD,), float("nan"), dtype=torch.float32, device=DEV)
        xbuf[PAD:PAD + total] = c.img.reshape(-1).to(DEV)
        xptr = xbuf.data_ptr() + 4 * PAD
    ldy = i.cout + L.ldy_extra
    ybuf, ymid = SC.guarded(c.M, ldy, torch.int16, S16, DEV)
    keep += [wp, bias, xbuf, ybuf]
    args = dict(x=xptr, wp=wp.data_ptr(), bias=bias.data_ptr(), y=ymid.data_ptr(), B=p.B, H=p.H, W=p.W, OH=c.OH,
                OW=c.OW, ldy=ldy, in_kind=i.in_kind, KH=i.KW, KW=i.KW, stride=p.stride, pad=p.pad, cout=i.cout,
                relu=L.act, dt=i.dt, rows=int(i.kernel == "rows"))
    if i.generic:
        args.update(scale0=SC.SCALE[0], scale1=SC.SCALE[1], scale2=SC.SCALE[2],
                    shift0=SC.SHIFT[0], shift1=SC.SHIFT[1], shift2=SC.SHIFT[2])
    return args, ybuf, ymid


def _run(L: SC.Launch) -> torch.Tensor:
    """One launch between guards; [M][cout] in the output type, on the CPU, after the guard check."""
    keep = []
    args, ybuf, ymid = _args(L, keep)
    _lib.lib().stem_conv(args, _lib.stream_ptr())
    torch.cuda.synchronize()
    cout = L.inst.cout
    assert SC.guards_intact(ybuf, cout, S16), ("stem_conv wrote outside its rows or columns", SC.describe(L))
    return ymid[:, :cout].contiguous().view(SC.DTYPES[L.inst.dt]).cpu()


def _check(L: SC.Launch, y: torch.Tensor, worst: dict, missed: list):
    c = SC.case(L)
    err = c.err(y)
    r = SC.ratio(err, c.bound)
    worst[L.inst] = max(worst.get(L.inst, 0.0), r) if r == r else r
    if not SC.within(err, c.bound):
        missed.append((SC.describe(L), "worst err / bound", r, "share over", SC.share_over(err, c.bound)))


def _report(worst: dict, missed: list, n: int):
    for inst, r in worst.items():
        print(f"{SC.describe_instance(inst)}: worst err / bound {r:.3f}")
    assert not missed, (f"{len(missed)} of {n} launches missed their bound", missed[:8])


@pytest.mark.parametrize("kernel,KW", [(k, KW) for k in ("stem", "rows") for KW in (3, 7)])
def test_every_instance_on_every_edge(kernel, KW):
    worst, missed = {}, []
    ls = SC.launches(kernel, KW)
    for L in ls:
        _check(L, _run(L), worst, missed)
    _report(worst, missed, len(ls))


def test_rows_kernel_image_pointer_at_any_byte():
    """The engine hands stem_rows_kernel image k of a batch of 299 x 299 x 3 bytes: every window is
    addressed relative to x, and an image that starts 1, 2 or 3 bytes into a dword gives the bits
    of the aligned launch."""
    worst, missed, n = {}, [], 0
    for base, moved in SC.unaligned_launches():
        y0 = _run(base)
        _check(base, y0, worst, missed)
        for L in moved:
            y = _run(L)
            assert torch.equal(y.view(torch.int16), y0.view(torch.int16)), SC.describe(L)
            _check(L, y, worst, missed)
            n += 1
    _report(worst, missed, n)


def test_a_launch_is_deterministic():
    L = next(x for x in SC.launches("rows", 7) if SC.case(x).M == 540)
    assert torch.equal(_run(L).view(torch.int16), _run(L).view(torch.int16))


# ---------------------------------------------------------------------------------------------
# refusals

OK_3 = SC.Launch(SC.Instance("stem", 0, 3, 32, False, 0), SC.Problem(2, 9, 7, 2, 0), "benign", 1, 0, 0)     # OH 4, OW 3
OK_7 = SC.Launch(SC.Instance("rows", 0, 7, 64, True, 0), SC.Problem(2, 13, 9, 2, 3), "benign", 1, 8, 0)     # OH 7, OW 5
REFUSED = [
    (OK_3, dict(ldy=36)), (OK_3, dict(ldy=33)), (OK_7, dict(ldy=68)),
    (OK_3, dict(KH=1)), (OK_7, dict(KH=3)), (OK_3, dict(KH=7)),
    (OK_3, dict(in_kind=2)), (OK_3, dict(in_kind=-1)), (OK_7, dict(in_kind=1)),      # rows kernel: uint8 only
    (OK_7, dict(pad=-1)), (OK_3, dict(pad=-1)),
    (OK_3, dict(OH=5)), (OK_3, dict(OW=4)), (OK_7, dict(OH=8)), (OK_7, dict(OW=6)),
    (OK_3, dict(H=2, OH=1)), (OK_3, dict(W=2, OW=1)),          # H + 2 pad < KH: -1 / 2 truncates to 0, + 1
    (OK_3, dict(OH=0)), (OK_3, dict(OH=-4, OW=-3)), (OK_3, dict(H=0)), (OK_3, dict(stride=0)), (OK_3, dict(B=0)),
    (OK_3, dict(cout=48, ldy=48)), (OK_3, dict(ldy=24)), (OK_3, dict(dt=1)), (OK_3, dict(dt=2)),
]


@pytest.mark.parametrize("n", range(len(REFUSED)), ids=lambda n: ",".join(f"{k}={v}" for k, v in REFUSED[n][1].items()))
def test_stem_conv_refuses(n):
    """Next to a launch of the same arguments without the fault; a smaller OH / OW stays legal."""
    L, bad = REFUSED[n]
    keep = []
    args, ybuf, _ = _args(L, keep)
    C = _lib.lib()
    with pytest.raises(RuntimeError):
        C.stem_conv({**args, **bad}, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((ybuf == S16).all())
    C.stem_conv({**args, "OH": args["OH"] - 1}, _lib.stream_ptr())
    C.stem_conv(args, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert SC.guards_intact(ybuf, L.inst.cout, S16)
    y = ybuf[SC.GUARD:-SC.GUARD, :L.inst.cout].contiguous().view(SC.DTYPES[L.inst.dt]).cpu()
    assert SC.within(SC.case(L).err(y), SC.case(L).bound)


@pytest.mark.parametrize("name,size,over", [
    ("Xception 299", 299, dict(ldy=32)),
    ("Xception 299 rows", 299, dict(ldy=32, rows=1)),
    ("ResNet-50 224", 224, dict(ldy=64, KH=7, KW=7, pad=3, cout=64, rows=1, scale0=SC.SCALE[0], shift0=SC.SHIFT[0])),
    ("ResNet-50 224 fp16", 224, dict(ldy=64, KH=7, KW=7, pad=3, cout=64, dt=1, scale0=SC.SCALE[0], shift0=SC.SHIFT[0])),
    ("EfficientNet-B7 600", 600, dict(ldy=64, pad=1, cout=64, relu=2, scale0=SC.SCALE[0], shift0=SC.SHIFT[0])),
])
def test_the_engines_own_stem_launches_stay_legal(name, size, over):
    """The arguments each engine passes for its input size are accepted (a zero image, batch 1)."""
    K, pad = over.get("KW", 3), over.get("pad", 0)
    OH = (size + 2 * pad - K) // 2 + 1
    x = torch.zeros(size * size * 3, dtype=torch.uint8, device=DEV)
    cout = over.get("cout", 32)
    kt = (K * SC.rp_of(K) + 31) >> 5 if over.get("rows") else (K * K * 3 + 31) >> 5
    wp = torch.zeros(cout // 16 * kt * 512, dtype=torch.int16, device=DEV)
    bias = torch.full((cout,), 0.5, device=DEV)
    ybuf, ymid = SC.guarded(OH * OH, cout, torch.int16, S16, DEV)
    _lib.lib().stem_conv(dict(x=x.data_ptr(), wp=wp.data_ptr(), bias=bias.data_ptr(), y=ymid.data_ptr(), B=1, H=size,
                              W=size, OH=OH, OW=OH, in_kind=0, stride=2, **over), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert SC.guards_intact(ybuf, cout, S16), name
    got = ymid.view(torch.float16 if over.get("dt") else torch.bfloat16).float()
    want = 0.5 * torch.sigmoid(torch.tensor(0.5)).item() if over.get("relu") == 2 else 0.5
    assert bool(((got - want).abs() <= 2.0 ** -8 * want).all()), name
