"""Garment-box timings on one GPU (profiles/locate.txt).

  python -m tools.locate_bench [--out FILE]

1. locate alone (kernels/locate.hip, both launches) for 32 maps at S = 224, 299 and 600: microseconds per call
   on realistic maps (smooth, one or two peaks, divided by their maximum: a few runs a row, the run tables in
   LDS) and on the worst case for the run tables, a 64 x 64 checkerboard upsampled with bicubic (thousands of
   runs an image, the tables in the workspace, one component). K = 3, threshold 51 as served, and K = 8. The
   runs per image and the workspace bytes per image are printed beside the times. The split between the two
   launches comes from a kernel trace of this same run (--alone).
2. A locate engine's batch-32 forward (captured graph) against the explain / rollout engine it rides on, as
   interleaved pairs, and the locate step's own time from engine.profile.

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events, after
warm-up calls of the same shapes."""
from __future__ import annotations

import argparse
import sys

import numpy as np
import torch

from .overlay_bench import window

SHAPES = {"vit_b16": (224, 14), "xception": (299, 10), "efficientnet_b7": (600, 19)}


def peaked(B: int, n: int) -> np.ndarray:
    """fp32 [B, n, n]: one or two Gaussian peaks per map at random places, divided by the maximum."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    out = np.zeros((B, n, n), np.float32)
    for b in range(B):
        for _ in range(1 + b % 2):
            cy, cx, s = rng.uniform(0.2, 0.8) * n, rng.uniform(0.2, 0.8) * n, rng.uniform(0.08, 0.2) * n
            out[b] += rng.uniform(0.5, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        out[b] /= out[b].max()
    return out


def board(B: int, n: int = 64) -> np.ndarray:
    yy, xx = np.indices((n, n))
    return np.broadcast_to(((yy + xx) % 2 == 0).astype(np.float32), (B, n, n)).copy()


def op_alone(B: int, iters: int, repeats: int, say) -> None:
    from kdl.engine.base import Locate
    from kdl.ops import _lib
    from kdl.serving import locate as L
    from kdl.serving import overlay as O
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    for family, (S, n) in SHAPES.items():
        work = torch.zeros(lib.locate_workspace(B, S), dtype=torch.uint8, device="cuda")
        say(f"{family:16s} S {S:3d}: workspace {work.numel() // B} bytes an image = {work.numel() / B / S / S:.3f} a pixel "
            f"(bitmask {S * ((S + 63) // 64) * 8})")
        for name, maps, flt, thr in (("peaked", peaked(B, n), "bilinear", 51), ("board", board(B), "bicubic", 128)):
            m = maps.shape[1]
            host = dict(zip(("xb", "xk", "yb", "yk"), O.axis_tables(m, S, flt) + O.axis_tables(m, S, flt)))
            dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
            runs = [len(L.runs_of(L.mask_of(maps[b], S, Locate(3, thr, flt)))[0]) for b in range(min(B, 4))]
            for K in (3, 8):
                ldo = 2 + m * m + 1 + 3 * K
                rows = torch.zeros((B, ldo), device="cuda")
                rows[:, 2:2 + m * m] = torch.from_numpy(maps.reshape(B, -1)).cuda()
                d = dict(out=rows.data_ptr(), work=work.data_ptr(), xb=dev["xb"].data_ptr(), xk=dev["xk"].data_ptr(),
                         yb=dev["yb"].data_ptr(), yk=dev["yk"].data_ptr(), h_xb=host["xb"].ctypes.data,
                         h_yb=host["yb"].ctypes.data, B=B, S=S, h=m, w=m, ldo=ldo, xks=host["xk"].shape[1],
                         yks=host["yk"].shape[1], K=K, threshold=thr)
                med, best = window(lambda i: lib.locate(d, s), iters, repeats)
                say(f"{family:16s} S {S:3d} map {m:2d} x {m:2d} B {B} {name:6s} {flt:8s} K {K}: median {med:7.2f} us  "
                    f"min {best:7.2f} us  (runs of images 0-3: {runs})")


def engine_pairs(family: str, pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.base import Locate
    from kdl.engine.tuning import tuning_path
    info = registry.get(family)
    p = info.init_params(0)
    mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
    engines = {"map": info.engine(p, 32, "cuda", **mode), "locate": info.engine(p, 32, "cuda", locate=Locate(), **mode)}
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
        order = ("map", "locate") if i % 2 == 0 else ("locate", "map")
        t = {k: timed(engines[k]) for k in order}
        d = (t["locate"] - t["map"]) * 1e3
        say(f"{family} pair {i}: {'rollout' if 'rollout' in mode else 'explain'} {t['map']:.4f} ms  locate "
            f"{t['locate']:.4f} ms  diff {d:+.1f} us ({100 * d / 1e3 / t['map']:+.2f} %)")
    prof = dict(engines["locate"].profile(32))
    say(f"{family} locate engine.profile(32), eager launches: locate step {prof['locate'] * 1e3:.1f} us, "
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
        print("locate_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say("== locate alone (both launches), batch 32")
    op_alone(32, a.iters, a.repeats, say)
    if a.pairs and not a.alone:
        say("== b32 forward (captured graph, device events), heatmap engine vs locate engine, interleaved pairs")
        for fam in a.families.split(","):
            engine_pairs(fam, a.pairs, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
