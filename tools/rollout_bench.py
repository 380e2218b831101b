"""Attention-rollout timings on one GPU (profiles/rollout.txt).

  python -m tools.rollout_bench [--out FILE]

1. The attn_rollout op alone (kernels/rollout.hip) at ViT-B/16's shape (B = 32, T = 197, H = 12): a
   middle layer (Tq = T, fp32 product with r_in), the first layer (r_in null), the last layer
   (Tq = 1) and rollout_map: microseconds per call. Beside it ``attention`` on the same QKV buffer,
   the yardstick: it does Q K^T and P V for the same bytes. "same" re-reads one QKV buffer (29 MB,
   it sits in the Infinity Cache, as the QKV GEMM's output does inside the forward); "rotating" walks
   over copies of at least 1 GiB in total, so every call reads QKV from HBM.
2. A ``rollout`` engine's batch-32 forward (captured graph) against a plain engine's, as interleaved
   pairs, for the bf16 and the fp8 build, and the steps' own times from engine.profile: the twelve
   rollout launches next to the twelve attention launches.

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


def op_alone(B: int, T: int, H: int, iters: int, repeats: int, say) -> None:
    from kdl.ops import _lib
    lib = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    ldr = (T + 3) // 4 * 4
    nbytes = B * T * 3 * H * 64 * 2
    copies = max(2, -(-(1 << 30) // nbytes))
    qkvs = [(torch.randn((B * T, 3 * H * 64), generator=g, device="cuda") * 1.7).to(torch.bfloat16)
            for _ in range(copies)]
    r0 = torch.zeros((B, T, ldr), dtype=torch.float32, device="cuda")
    r1 = torch.zeros((B, T, ldr), dtype=torch.float32, device="cuda")
    att = torch.zeros((B * T, H * 64), dtype=torch.bfloat16, device="cuda")
    top = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    rows = torch.zeros((B, T + 1), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def roll(x, r_in, Tq):
        lib.attn_rollout(dict(qkv=x.data_ptr(), r_in=r_in, r_out=r1.data_ptr(), B=B, T=T, Tq=Tq, H=H, dh=64,
                              scale=0.125, ldr=ldr), s)

    def attn(x):
        lib.attention(dict(qkv=x.data_ptr(), out=att.data_ptr(), B=B, T=T, H=H, dh=64, scale=0.125), s)
    roll(qkvs[0], None, T)
    r0.copy_(r1)                                     # a real state: rows that sum to 1
    flop = 2.0 * B * T * T * T                       # the fp32 product of one layer
    say(f"-- B={B} T={T} H={H}: QKV {nbytes / 1e6:.1f} MB, R {B * T * ldr * 4 / 1e6:.1f} MB, "
        f"fp32 product {flop / 1e9:.2f} GFLOP per layer, {copies} QKV copies when rotating")
    for kind, pick in (("same", lambda i: qkvs[0]), ("rotating", lambda i: qkvs[i % copies])):
        t = {}
        for label, fn in (("attn_rollout middle layer", lambda i: roll(pick(i), r0.data_ptr(), T)),
                          ("attn_rollout first layer ", lambda i: roll(pick(i), None, T)),
                          ("attn_rollout Tq = 1      ", lambda i: roll(pick(i), r0.data_ptr(), 1)),
                          ("attention                ", lambda i: attn(pick(i)))):
            med, best = window(fn, iters, repeats)
            t[label.strip()] = med
            say(f"{kind:8s} {label}: median {med:7.2f} us  min {best:7.2f} us")
        say(f"{kind:8s} middle layer / attention = {t['attn_rollout middle layer'] / t['attention']:.2f}; "
            f"the product alone would be {flop / t['attn_rollout middle layer'] / 1e6:.1f} TFLOP/s fp32 if the "
            f"launch did nothing else")
    med, best = window(lambda i: lib.rollout_map(dict(r=r0.data_ptr(), top=top.data_ptr(), out=rows.data_ptr(), B=B,
                                                      T=T, ldr=ldr, ldo=T + 1), s), iters, repeats)
    say(f"rollout_map: median {med:7.2f} us  min {best:7.2f} us")


def engine_pairs(family: str, pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.tuning import tuning_path
    info = registry.get(family)
    p = info.init_params(0)
    engines = {"plain": info.engine(p, 32, "cuda"), "rollout": info.engine(p, 32, "cuda", rollout=True)}
    x = torch.randint(0, 256, (32, info.input_size, info.input_size, 3), dtype=torch.uint8,
                      generator=torch.Generator().manual_seed(1)).cuda()
    tp = tuning_path(info.tuning or family, 32)
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
        order = ("plain", "rollout") if i % 2 == 0 else ("rollout", "plain")
        t = {k: timed(engines[k]) for k in order}
        d = (t["rollout"] - t["plain"]) * 1e3
        say(f"{family} pair {i}: plain {t['plain']:.4f} ms  rollout {t['rollout']:.4f} ms  diff {d:+.1f} us "
            f"({100 * d / 1e3 / t['plain']:+.2f} %)")
    prof = engines["rollout"].profile(32)
    roll = [v * 1e3 for k, v in prof if k.endswith(".rollout")]
    attn = [v * 1e3 for k, v in prof if k.endswith(".attn")]
    d = dict(prof)
    say(f"{family} rollout engine.profile(32), eager launches, median of 20: 12 rollout steps {sum(roll):.1f} us "
        f"(first {roll[0]:.1f}, middle {statistics.median(roll[1:-1]):.1f}, last {roll[-1]:.1f}), 12 attention steps "
        f"{sum(attn):.1f} us, top1 {d['top1'] * 1e3:.1f} us, rollout_map {d['rollout_map'] * 1e3:.1f} us, "
        f"sum of all steps {sum(v for _, v in prof):.3f} ms")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--families", default="vit_b16,vit_b16_fp8")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("rollout_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say("== attn_rollout alone and attention on the same QKV buffer")
    op_alone(32, 197, 12, a.iters, a.repeats, say)
    if a.pairs:
        say("== b32 forward (captured graph, device events), plain vs rollout, interleaved pairs")
        for fam in a.families.split(","):
            engine_pairs(fam, a.pairs, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
