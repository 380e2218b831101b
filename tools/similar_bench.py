"""Gallery search timings on one GPU (profiles/similar.txt).

  python -m tools.similar_bench [--rows 10000,100000,1000000] [--out FILE]

1. The gallery_topk op alone (kernels/similar.hip) at F = 2048, B = 32, K = 5: microseconds per call
   and gallery bytes / time. "same" re-reads one gallery (a 41 MB or 410 MB one then sits partly or
   wholly in the 256 MiB Infinity Cache); "rotating" walks over copies of at least 1 GiB in total,
   so every call reads from HBM.
2. The same answer from torch: (q @ g.T).topk(K) with both operands bf16, and with both fp32.
3. An Xception ``similar`` engine's batch-32 forward (captured graph) against an ``embed="l2"``
   engine's, as interleaved pairs.

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events,
after warm-up calls of the same shapes."""
from __future__ import annotations

import argparse
import statistics
import sys

import torch

F, B, K = 2048, 32, 5


def window(fn, iters: int, repeats: int, warm: int = 5) -> tuple[float, float]:
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


def random_gallery(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((n, F), dtype=torch.bfloat16, device="cuda")
    for lo in range(0, n, 65536):                       # unit rows, made in slices: no fp32 copy of the whole
        x = torch.randn((min(65536, n - lo), F), generator=g, device="cuda")
        out[lo:lo + x.shape[0]] = torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)
    return out


def op_rows(n: int, iters: int, repeats: int, say) -> None:
    from kdl.ops import _lib
    lib = _lib.lib()
    nbytes = n * F * 2
    copies = max(1, -(-(1 << 30) // nbytes))
    gals = [random_gallery(n, 17 + c) for c in range(copies)]
    q = torch.nn.functional.normalize(torch.randn((B, F), generator=torch.Generator().manual_seed(3)), dim=1).cuda()
    out = torch.zeros((B, 2 * K), dtype=torch.int32, device="cuda")
    work = torch.zeros(lib.gallery_topk_workspace(B, n, K), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(g):
        lib.gallery_topk(dict(q=q.data_ptr(), g=g.data_ptr(), out=out.data_ptr(), work=work.data_ptr(), B=B, N=n, F=F,
                              K=K, ldq=F, ldg=F), s)
    it = max(5, min(iters, (64 << 30) // nbytes))
    for name, pick in (("same", lambda i: gals[0]), ("rotating", lambda i: gals[i % copies])):
        if name == "rotating" and copies == 1:
            continue
        med, best = window(lambda i: call(pick(i)), it, repeats)
        say(f"N={n:8d} gallery_topk {name:8s} ({copies if name == 'rotating' else 1} x {nbytes / 1e6:7.1f} MB): "
            f"median {med:8.1f} us  min {best:8.1f} us  {nbytes / med / 1e6:6.2f} TB/s of gallery bytes")
    call(gals[0])
    torch.cuda.synchronize()
    mine = out[:, :K].clone()
    g = gals[0]
    qb = q.to(torch.bfloat16)
    med, best = window(lambda i: (qb @ g.T).topk(K), it, repeats)
    say(f"N={n:8d} torch bf16 (q @ g.T).topk({K}):            median {med:8.1f} us  min {best:8.1f} us  "
        f"{nbytes / med / 1e6:6.2f} TB/s of gallery bytes")
    gf = g.float()
    med, best = window(lambda i: (q @ gf.T).topk(K), it, repeats)
    say(f"N={n:8d} torch fp32 (q @ g.T).topk({K}):            median {med:8.1f} us  min {best:8.1f} us  "
        f"(reads {2 * nbytes / 1e6:.1f} MB of fp32: {2 * nbytes / med / 1e6:5.2f} TB/s)")
    ref = (q.double() @ gf.double().T).topk(K).indices
    say(f"N={n:8d} indices equal to a float64 torch top-{K}: gallery_topk {int((mine == ref).sum())}/{B * K}, "
        f"torch fp32 {int(((q @ gf.T).topk(K).indices == ref).sum())}/{B * K}, "
        f"torch bf16 {int(((qb @ g.T).topk(K).indices == ref).sum())}/{B * K}")
    del gals, gf


def engine_pairs(n: int, pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.base import Similar
    from kdl.engine.tuning import tuning_path
    info = registry.get("xception")
    p = info.init_params(0)
    gal = random_gallery(n, 5)
    engines = {"l2": info.engine(p, 32, "cuda", embed="l2"),
               "similar": info.engine(p, 32, "cuda", similar=Similar(gal, K, "cosine"))}
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
        order = ("l2", "similar") if i % 2 == 0 else ("similar", "l2")
        t = {k: timed(engines[k]) for k in order}
        d = (t["similar"] - t["l2"]) * 1e3
        say(f"pair {i}: embed=l2 {t['l2']:.4f} ms  similar(N={n}) {t['similar']:.4f} ms  diff {d:+.1f} us "
            f"({100 * d / 1e3 / t['l2']:+.2f} %)")
    prof = dict(engines["similar"].profile(32))
    say(f"similar engine.profile(32), eager launches, median of 20: embed_rows {prof['embed_rows'] * 1e3:.1f} us, "
        f"similar {prof['similar'] * 1e3:.1f} us, sum of all steps {sum(prof.values()):.3f} ms")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000,100000,1000000")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--engine-rows", type=int, default=100000)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("similar_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say(f"== gallery_topk alone and torch, F={F} B={B} K={K}")
    for n in (int(v) for v in a.rows.split(",")):
        op_rows(n, a.iters, a.repeats, say)
    say("== xception b32 forward (captured graph, device events), embed=l2 vs similar, interleaved pairs")
    engine_pairs(a.engine_rows, a.pairs, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
