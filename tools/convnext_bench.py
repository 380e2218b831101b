"""ConvNeXt-Tiny's four block-head shapes at batch 32: dwconv7_ln against torch eager
conv2d(groups=C) + layer_norm on the same device, interleaved, then the whole forward as one
engine's graph replay on one stream. The record is profiles/convnext.txt.

    python tools/convnext_bench.py [out.txt]

Per shape both sides walk a set of input / output buffer pairs larger than ROTATE bytes, so no launch
finds its operands in the 256 MB MALL left by the one before: the byte rates are HBM rates and
comparable with the copy rate measured here. Bytes = input + output, once each (the fused kernel's
minimum; the eager pair also writes and re-reads the conv output)."""
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kdl.engine import registry
from kdl.ops import _lib

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
    """Alternating windows of about 0.2 s each; median and range of the per-launch time."""
    na, nb = (max(3, int(window_us / timed(f, 3))) for f in (fa, fb))
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, na) / per)
        tb.append(timed(fb, nb) / per)
    ta.sort(), tb.sort()
    return ta[len(ta) // 2], tb[len(tb) // 2], (ta[0], ta[-1]), (tb[0], tb[-1])


src = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
dst = torch.empty_like(src)
timed(lambda: dst.copy_(src), 5)
cp = sorted(timed(lambda: dst.copy_(src), 10) for _ in range(5))[2]
copy_rate = 2 * src.numel() / cp / 1e3      # GB/s
say(f"copy rate (512 MiB d2d, read+write): {copy_rate:.0f} GB/s")
del src, dst

B = 32
s = _lib.stream_ptr()
C_ = _lib.lib()
for H, C in ((56, 96), (28, 192), (14, 384), (7, 768)):
    gen = torch.Generator().manual_seed(H)
    xd = torch.randn(B, H, H, C, generator=gen).to(torch.bfloat16).to(DEV)
    w = (torch.randn(49, C, generator=gen) / 7).to(DEV)
    bias, gamma, beta = (torch.randn(C, generator=gen).to(DEV) * k for k in (0.1, 1.0, 0.1))
    nbuf = ROTATE // (xd.numel() * 4) + 1
    xs = [xd] + [xd.clone() for _ in range(nbuf - 1)]
    ys = [torch.zeros_like(xd) for _ in range(nbuf)]
    base = dict(w=w.data_ptr(), bias=bias.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), B=B, H=H, W=H,
                C=C, ldx=C, ldy=C, eps=1e-6)
    plan = C_.dwconv7_ln_plan(dict(base, x=xd.data_ptr(), y=ys[0].data_ptr()))
    wt = w.t().reshape(C, 1, 7, 7).to(torch.bfloat16).contiguous()
    xn = [a.permute(0, 3, 1, 2) for a in xs]             # NCHW views of the NHWC storage (channels_last)
    bb, gb, eb = bias.to(torch.bfloat16), gamma.to(torch.bfloat16), beta.to(torch.bfloat16)

    def eager():
        for a in xn:
            F.layer_norm(F.conv2d(a, wt, bb, padding=3, groups=C).permute(0, 2, 3, 1), (C,), gb, eb, 1e-6)

    for rows in sorted({0, 1, 2, 4, 7, H} - {plan[0]}):  # 0 = the launcher's choice; then other band heights
        pg = C_.Program()
        for a, b in zip(xs, ys):
            pg.add_dwconv7_ln("dwln", dict(base, x=a.data_ptr(), y=b.data_ptr(), rows=rows))
        tg, te, rg, re = pairs(lambda: pg.run(s), eager, nbuf, rounds=5 if rows == 0 else 3)
        byts = xd.numel() * 4
        say(f"{H}x{H}x{C} rows={rows or plan[0]}{' (launcher, tw=%d)' % plan[1] if rows == 0 else ''} ({nbuf} buffer pairs): "
            f"dwconv7_ln {tg:.1f} us [{rg[0]:.1f}..{rg[1]:.1f}]; torch eager conv2d+layer_norm {te:.1f} us "
            f"[{re[0]:.1f}..{re[1]:.1f}] x{te / tg:.2f}; {byts / 1e6:.1f} MB -> {byts / tg / 1e3:.0f} GB/s = "
            f"{byts / tg / 1e3 / copy_rate * 100:.0f}% of copy rate; {2 * 49 * xd.numel() / tg / 1e6:.2f} TFLOP/s")
    del xs, ys, xn, pg

info = registry.get("convnext_tiny")
p = info.init_params(0)
x = torch.randint(0, 256, (B, 224, 224, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(DEV)
eng = info.engine(p, B, DEV, buckets=[B])
eng.forward(x)


def sync_timed(e, iters=100):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        e.launch(B, e.stream)
    e.stream.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


sync_timed(eng, 10)
t = sorted(sync_timed(eng) for _ in range(7))
say(f"convnext_tiny forward b32 (one engine's graph replay on one stream, default tiles): {t[3]:.3f} ms "
    f"[{t[0]:.3f}..{t[-1]:.3f}] = {B / t[3] * 1e3:.0f} img/s")
prof = {}
for name, ms in eng.profile(B, 10):
    k = "dwconv7_ln" if name.endswith("block.0") else "ln_s2d" if name.endswith(".0") and name[9] in "246" else \
        "gemm" if name[-1] in "135" and "block" in name or name.endswith(".1") or name == "features.0.0" else "other"
    prof[k] = prof.get(k, 0.0) + ms
say("per-op profile (eager launches, ms per forward): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(prof.items())))
out.close()
