"""ResNeXt-50 conv2 shapes at batch 32: grouped_conv against the dense MODE_CONV lowering of the
same weights (KDL_GROUPED_CONV=0), interleaved on one device, then the whole forward both ways.
The record is profiles/resnext50.txt.

    python tools/grouped_conv_ab.py [out.txt]

Per shape both kernels walk a set of input / output buffer pairs larger than ROTATE bytes, so no
launch finds its operands in the 256 MB MALL left by the one before: the byte rates are HBM
rates and comparable with the copy rate measured here. Bytes = padded input + output + packed
weights, once each; useful FLOP = 2 * B * OH * OW * C * cg * 9."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kdl.engine import registry
from kdl.engine.resnet import GroupedConvLayer
from kdl.models import resnet as R
from kdl.ops import _lib
from kdl.ops.conv import MODE_CONV, ConvGemmLayer, Geometry
from kdl.ops.pack import grouped_dense_weights

DEV = "cuda"
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else open(os.devnull, "w")
ROTATE = 1 << 30


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3     # us


def pairs(fa, fb, per, rounds=5, window_us=2e5):
    """fa / fb launch `per` kernels a call. Alternating windows of about 0.2 s each; median and
    range of the per-launch time."""
    na, nb = (max(3, int(window_us / timed(f, 3))) for f in (fa, fb))
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, na) / per)
        tb.append(timed(fb, nb) / per)
    ta.sort(), tb.sort()
    return ta[len(ta) // 2], tb[len(tb) // 2], (ta[0], ta[-1]), (tb[0], tb[-1])


# the box's copy rate: device-to-device copy of 512 MiB (read + write counted)
src = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
dst = torch.empty_like(src)
timed(lambda: dst.copy_(src), 5)
cp = sorted(timed(lambda: dst.copy_(src), 10) for _ in range(5))[2]
copy_rate = 2 * src.numel() / cp / 1e3      # GB/s
say(f"copy rate (512 MiB d2d, read+write): {copy_rate:.0f} GB/s")
del src, dst

B = 32
SHAPES = [("layer1.x", 4, 1, 56, 128), ("layer2.0", 8, 2, 56, 256), ("layer2.x", 8, 1, 28, 256),
          ("layer3.0", 16, 2, 28, 512), ("layer3.x", 16, 1, 14, 512), ("layer4.0", 32, 2, 14, 1024),
          ("layer4.x", 32, 1, 7, 1024)]
s = _lib.stream_ptr()
C_ = _lib.lib()
for dname, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
    for name, cg, st, H, C in SHAPES:
        gen = torch.Generator().manual_seed(H + C)
        OH = (H - 1) // st + 1
        x = torch.zeros(B, H + 2, H + 2, C)
        x[:, 1:-1, 1:-1] = torch.randn(B, H, H, C, generator=gen)
        xd = x.to(dtype).to(DEV)
        nbuf = ROTATE // ((x.numel() + B * OH * OH * C) * 2) + 1
        xs = [xd] + [xd.clone() for _ in range(nbuf - 1)]
        w = torch.randn(C, 9 * cg, generator=gen, dtype=torch.float64) / (9 * cg) ** 0.5
        bias = torch.randn(C, generator=gen) * 0.1
        gl = GroupedConvLayer(name, w, bias, groups=C // cg, stride=st, device=DEV, dtype=dtype)
        dl = ConvGemmLayer(name, MODE_CONV, grouped_dense_weights(w, cg), bias, cin_pad=C, n=C, stride=st,
                           relu_out=1, device=DEV, dtype=dtype)
        dl.krot = 1
        ys = [torch.zeros(B * OH * OH * C, dtype=dtype, device=DEV) for _ in range(nbuf)]
        yg, yd = ys[0], torch.zeros_like(ys[0])
        gas = [gl.args(a.data_ptr(), b.data_ptr(), B, H, H, OH, OH) for a, b in zip(xs, ys)]
        geo = Geometry(B, H + 2, H + 2, OH, OH)
        # one native Program per kernel, one op per buffer pair: a call launches all of them from C++
        pg, pd = C_.Program(), C_.Program()
        for i in range(nbuf):
            pg.add_grouped_conv(name, gas[i])
            dl.emit(pd, xs[i].data_ptr(), ys[i].data_ptr(), geo, ldx=C)
        fg, fd = (lambda: pg.run(s)), (lambda: pd.run(s))
        C_.grouped_conv(gas[0], s)
        dl.emit(None, xd.data_ptr(), yd.data_ptr(), geo, ldx=C)
        torch.cuda.synchronize()
        diff = (yg.float() - yd.float()).abs().max().item() / yd.float().abs().max().item()
        tg, td, rg, rd = pairs(fg, fd, nbuf)
        byts = (xd.numel() + yg.numel()) * 2 + gl.wp.numel() * 2
        macs = B * OH * OH * C * cg * 9
        say(f"{dname} {name} cg={cg} s={st} {H}x{H}x{C} ({nbuf} buffer pairs): grouped {tg:.1f} us [{rg[0]:.1f}..{rg[1]:.1f}] "
            f"dense(cfg {dl.cfg}) {td:.1f} us [{rd[0]:.1f}..{rd[1]:.1f}] x{td / tg:.2f}; "
            f"{byts / 1e6:.1f} MB -> {byts / tg / 1e3:.0f} GB/s = {byts / tg / 1e3 / copy_rate * 100:.0f}% of copy rate; "
            f"{2 * macs / tg / 1e6:.1f} TFLOP/s useful; max rel diff vs dense {diff:.2e}")
        del xd, xs, ys, yg, yd, gas, gl, dl, pg, pd

# whole forward, batch 32, graph replay, interleaved pairs
p = R.init_params(seed=0, **R.RESNEXT50_32X4D)
x = torch.randint(0, 256, (B, 224, 224, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(DEV)
for fam in ("resnext50_32x4d", "resnext50_32x4d_bf16"):
    info = registry.get(fam)
    os.environ["KDL_GROUPED_CONV"] = "1"
    eg = info.engine(p, B, DEV, buckets=[B])
    os.environ["KDL_GROUPED_CONV"] = "0"
    ed = info.engine(p, B, DEV, buckets=[B])
    os.environ["KDL_GROUPED_CONV"] = "1"
    og, od = eg.forward(x).clone(), ed.forward(x).clone()

    def sync_timed(e, iters=200):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            e.launch(B, e.stream)
        e.stream.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3
    for e in (eg, ed):
        sync_timed(e, 10)
    tg, td = [], []
    for _ in range(7):
        tg.append(sync_timed(eg))
        td.append(sync_timed(ed))
    tg.sort(), td.sort()
    say(f"{fam} forward b32 (graph replay, untuned 1x1 tiles): grouped {tg[3]:.3f} ms [{tg[0]:.3f}..{tg[-1]:.3f}] = "
        f"{B / tg[3] * 1e3:.0f} img/s; dense lowering {td[3]:.3f} ms [{td[0]:.3f}..{td[-1]:.3f}] = {B / td[3] * 1e3:.0f} img/s; "
        f"x{td[3] / tg[3]:.2f}; logits max rel diff {((og - od).abs().max() / od.abs().max()).item():.2e}")
    del eg, ed
out.close()
