"""Grad-CAM timings on one GPU (profiles/explain.txt).

  python -m tools.explain_bench [--out FILE]

1. The class_map op alone (kernels/explain.hip) at Xception's shape (B = 32, HW = 100, F = 2048, MLP
   head, H1 = 100, NC = 10) and ResNet-50's (B = 32, HW = 49, F = 2048, linear head, NC = 1000, fp16),
   with and without the normalising launch: microseconds per call. Beside it ``embed_rows`` on the
   same tensor, which reads the same bytes once, and the ratio. "same" re-reads one map (13 MB / 6 MB:
   it sits in the 256 MiB Infinity Cache, as block14's output does when the step runs behind the
   forward); "rotating" walks over copies of at least 1 GiB in total, so every call reads from HBM.
2. An Xception ``explain`` engine's batch-32 forward (captured graph) against a plain engine's, as
   interleaved pairs, and the two steps' own times from engine.profile.

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events,
after warm-up calls of the same shapes."""
from __future__ import annotations

import argparse
import statistics
import sys

import torch


def window(fn, iters: int, repeats: int, warm: int = 10) -> tuple[float, float]:
    """(median, min) microseconds per call of fn(i)."""
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for r in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(r * iters + i)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out), min(out)


def op_shape(name: str, B: int, HW: int, F: int, NC: int, H1: int, dt: int, iters: int, repeats: int, say) -> None:
    from kdl.ops import _lib
    lib = _lib.lib()
    dtype = torch.float16 if dt else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(7)
    nbytes = B * HW * F * 2
    copies = max(2, -(-(1 << 30) // nbytes))
    maps = [torch.randn((B, HW, F), generator=g, device="cuda").abs().to(dtype) for _ in range(copies)]
    top = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    top[:, 0] = torch.arange(B, device="cuda") % NC
    alpha = torch.zeros((B, F), dtype=torch.float32, device="cuda")
    out = torch.zeros((B, 2 + HW), dtype=torch.float32, device="cuda")
    emb = torch.zeros((B, F), dtype=torch.float32, device="cuda")
    if H1:
        head = dict(head=1, H1=H1, w1=torch.randn((H1, F), generator=g, device="cuda"),
                    w2=torch.randn((H1, NC), generator=g, device="cuda"),
                    b1=torch.randn((H1,), generator=g, device="cuda"),
                    hid=torch.randn((F // 64, B, H1), generator=g, device="cuda") / 8)
    else:
        head = dict(head=0, w=torch.randn((NC, F), generator=g, device="cuda").to(dtype))
    ptrs = {k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in head.items()}
    s = torch.cuda.current_stream().cuda_stream

    def cmap(x, norm):
        lib.class_map(dict(x=x.data_ptr(), top=top.data_ptr(), alpha=alpha.data_ptr(), out=out.data_ptr(), B=B, HW=HW,
                           F=F, ldx=F, ldo=2 + HW, NC=NC, dt=dt, norm=norm, **ptrs), s)

    def embed(x):
        lib.embed_rows(dict(x=x.data_ptr(), out=emb.data_ptr(), B=B, HW=HW, F=F, ldx=F, ldo=F, dt=dt, norm=0), s)
    say(f"-- {name}: B={B} HW={HW} F={F} NC={NC} {'MLP head H1=' + str(H1) if H1 else 'linear head'} "
        f"{'fp16' if dt else 'bf16'}, map {nbytes / 1e6:.1f} MB")
    for kind, pick in (("same", lambda i: maps[0]), ("rotating", lambda i: maps[i % copies])):
        t = {}
        nl = 2 if H1 else 1                  # the MLP head's gradient pass is a launch of its own
        for label, fn in ((f"class_map norm=1 ({nl + 1} launches)", lambda i: cmap(pick(i), 1)),
                          (f"class_map norm=0 ({nl} launch{'es' if nl > 1 else '  '})", lambda i: cmap(pick(i), 0)),
                          ("embed_rows raw   (1 launch)  ", lambda i: embed(pick(i)))):
            med, best = window(fn, iters, repeats)
            t[label[:16].strip()] = med
            say(f"{kind:8s} {label}: median {med:7.2f} us  min {best:7.2f} us  {nbytes / med / 1e6:5.2f} TB/s of map bytes")
        say(f"{kind:8s} class_map norm=1 / embed_rows = {t['class_map norm=1'] / t['embed_rows raw']:.2f}, "
            f"norm=0 / embed_rows = {t['class_map norm=0'] / t['embed_rows raw']:.2f}")


def engine_pairs(pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.tuning import tuning_path
    info = registry.get("xception")
    p = info.init_params(0)
    engines = {"plain": info.engine(p, 32, "cuda"), "explain": info.engine(p, 32, "cuda", explain=True)}
    x = torch.randint(0, 256, (32, info.input_size, info.input_size, 3), dtype=torch.uint8,
                      generator=torch.Generator().manual_seed(1)).cuda()
    tp = tuning_path(info.tuning or "xception", 32)
    for e in engines.values():
        if tp.exists():
            e.load_tuning(tp)
        e.forward(x)

    def timed(e) -> float:
        with torch.cuda.stream(e.stream):
            for _ in range(20):
                e.launch(32, e.stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(e.stream)
            for _ in range(100):
                e.launch(32, e.stream)
            e1.record(e.stream)
            e1.synchronize()
        return e0.elapsed_time(e1) / 100
    for i in range(pairs):
        order = ("plain", "explain") if i % 2 == 0 else ("explain", "plain")
        t = {k: timed(engines[k]) for k in order}
        d = (t["explain"] - t["plain"]) * 1e3
        say(f"pair {i}: plain {t['plain']:.4f} ms  explain {t['explain']:.4f} ms  diff {d:+.1f} us "
            f"({100 * d / 1e3 / t['plain']:+.2f} %)")
    prof = dict(engines["explain"].profile(32))
    say(f"explain engine.profile(32), eager launches, median of 20: head {prof['head'] * 1e3:.1f} us, "
        f"top1 {prof['top1'] * 1e3:.1f} us, class_map {prof['class_map'] * 1e3:.1f} us, "
        f"sum of all steps {sum(prof.values()):.3f} ms")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("explain_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say("== class_map alone and embed_rows on the same tensor")
    op_shape("xception", 32, 100, 2048, 10, 100, 0, a.iters, a.repeats, say)
    op_shape("resnet50", 32, 49, 2048, 1000, 0, 1, a.iters, a.repeats, say)
    if a.pairs:
        say("== xception b32 forward (captured graph, device events), plain vs explain, interleaved pairs")
        engine_pairs(a.pairs, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
