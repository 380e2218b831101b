"""Dominant-colour timings on one GPU (profiles/palette.txt).

  python -m tools.palette_bench [--out FILE]

1. palette alone (kernels/palette.hip, both launches) for 32 pictures at S = 224, 299 and 600: microseconds
   per call on noise (every pixel its own bin: 4096 live bins to cluster), on a flat picture (every lane of a
   wave hits one bin: the worst case for LDS atomics, which the wave-level sum in front of them answers) and
   on blocks of 16 x 16 flat pixels, with the map's weights and with uniform ones. K = 5, T = 8 as served;
   K = 1, T = 1 beside it is the clustering launch at its shortest, so the difference is what rounds cost.
   The split between the two launches comes from a kernel trace of this same run (--alone).
2. A palette engine's batch-32 forward (captured graph) against the explain / rollout engine it rides on,
   as interleaved pairs, and the palette step's own time from engine.profile.

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events, after
warm-up calls of the same shapes."""
from __future__ import annotations

import argparse
import sys

import torch

from .overlay_bench import window

SHAPES = {"vit_b16": (224, 14), "xception": (299, 10), "efficientnet_b7": (600, 19)}


def pictures(B: int, S: int) -> dict:
    g = torch.Generator(device="cuda").manual_seed(3)
    noise = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=g)
    n = (S + 15) // 16
    blocks = torch.randint(0, 256, (B, n, n, 3), dtype=torch.uint8, device="cuda", generator=g)
    blocks = blocks.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :S, :S].contiguous()
    return {"noise": noise, "flat": torch.full((B, S, S, 3), 200, dtype=torch.uint8, device="cuda"), "blocks": blocks}


def op_alone(B: int, iters: int, repeats: int, say) -> None:
    from kdl.ops import _lib
    from kdl.serving import overlay as O
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    for family, (S, n) in SHAPES.items():
        host = dict(zip(("xb", "xk", "yb", "yk"), O.axis_tables(n, S, "bilinear") + O.axis_tables(n, S, "bilinear")))
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        work = torch.zeros(lib.palette_workspace(B), dtype=torch.uint8, device="cuda")
        for name, inp in pictures(B, S).items():
            for weight in (1, 0):
                for K, T in ((5, 8), (1, 1)):
                    ldo = 2 + n * n + 1 + 2 * K
                    rows = torch.rand((B, ldo), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
                    d = dict(inp=inp.data_ptr(), out=rows.data_ptr(), work=work.data_ptr(), xb=dev["xb"].data_ptr(),
                             xk=dev["xk"].data_ptr(), yb=dev["yb"].data_ptr(), yk=dev["yk"].data_ptr(),
                             h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=B, S=S, h=n, w=n, ldo=ldo,
                             xks=host["xk"].shape[1], yks=host["yk"].shape[1], K=K, T=T, weight=weight)
                    med, best = window(lambda i: lib.palette(d, s), iters, repeats)
                    say(f"{family:16s} S {S:3d} map {n:2d} x {n:2d} B {B} {name:6s} {'map' if weight else 'uniform':7s} "
                        f"K {K} T {T}: median {med:7.2f} us  min {best:7.2f} us  ({B * S * S * 3 / 1e6:.1f} MB read)")


def engine_pairs(family: str, pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.base import Palette
    from kdl.engine.tuning import tuning_path
    info = registry.get(family)
    p = info.init_params(0)
    mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
    engines = {"map": info.engine(p, 32, "cuda", **mode), "palette": info.engine(p, 32, "cuda", palette=Palette(), **mode)}
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
        order = ("map", "palette") if i % 2 == 0 else ("palette", "map")
        t = {k: timed(engines[k]) for k in order}
        d = (t["palette"] - t["map"]) * 1e3
        say(f"{family} pair {i}: {'rollout' if 'rollout' in mode else 'explain'} {t['map']:.4f} ms  palette "
            f"{t['palette']:.4f} ms  diff {d:+.1f} us ({100 * d / 1e3 / t['map']:+.2f} %)")
    prof = dict(engines["palette"].profile(32))
    say(f"{family} palette engine.profile(32), eager launches: palette step {prof['palette'] * 1e3:.1f} us, "
        f"sum of all steps {sum(prof.values()):.3f} ms")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--families", default="xception,vit_b16")
    ap.add_argument("--alone", action="store_true", help="part 1 only (the run to put under a kernel trace)")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("palette_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say("== palette alone (both launches), batch 32, bilinear")
    op_alone(32, a.iters, a.repeats, say)
    if a.pairs and not a.alone:
        say("== b32 forward (captured graph, device events), heatmap engine vs palette engine, interleaved pairs")
        for fam in a.families.split(","):
            engine_pairs(fam, a.pairs, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
