"""Garment-cutout timings on one GPU (profiles/cutout.txt).

  python -m tools.cutout_bench [--out FILE]

1. cutout alone (kernels/cutout.hip, all three launches) for 32 pictures at S = 224, 299 and 600: microseconds
   per call on noise (every colour bin live, the mask a random half of the gated area: the most LDS atomics and
   the most global table adds) and on a photograph (tests/data/pants.png resized: a few hundred live bins, long
   flat stretches), under one-peak maps divided by their maximum, with the served defaults and with the
   largest rounds and smooth. The workspace bytes per image and the rule's coverage of images 0-3 are printed
   beside the times. The split between the three launches comes from a kernel trace of this same run (--alone).
2. The copy of 32 result rows to pinned host memory, beside overlay's rows of the same pictures.
3. A cutout engine's batch-32 forward (captured graph) against the explain / rollout engine it rides on, as
   interleaved pairs, and the cutout step's own time from engine.profile.

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events, after
warm-up calls of the same shapes."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

from .locate_bench import SHAPES, peaked
from .overlay_bench import window

PHOTO = Path(__file__).resolve().parent.parent / "tests" / "data" / "pants.png"


def pictures(B: int, S: int) -> dict:
    from PIL import Image
    rng = np.random.default_rng(3)
    photo = np.asarray(Image.open(PHOTO).convert("RGB").resize((S, S), Image.BILINEAR), np.uint8)
    return {"noise": rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8),
            "photo": np.ascontiguousarray(np.broadcast_to(photo, (B, S, S, 3)))}


def op_alone(B: int, iters: int, repeats: int, say) -> None:
    from kdl.engine.base import Cutout
    from kdl.ops import _lib
    from kdl.serving import cutout as C
    from kdl.serving import overlay as O
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    for family, (S, n) in SHAPES.items():
        work = torch.zeros(lib.cutout_workspace(B, S), dtype=torch.uint8, device="cuda")
        say(f"{family:16s} S {S:3d}: workspace {work.numel() // B} bytes an image (tables 49152, colour bits 512, "
            f"gate mask {S * ((S + 63) // 64) * 8}); a result row is {4 * (2 + n * n + 1 + S * S)} bytes")
        maps = peaked(B, n)
        host = dict(zip(("xb", "xk", "yb", "yk"), O.axis_tables(n, S, "bilinear") + O.axis_tables(n, S, "bilinear")))
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        ldo = 2 + n * n + 1 + S * S
        rows = torch.zeros((B, ldo), device="cuda")
        rows[:, 2:2 + n * n] = torch.from_numpy(maps.reshape(B, -1)).cuda()
        for name, pics in pictures(B, S).items():
            inp = torch.from_numpy(pics).cuda()
            for spec in (Cutout(), Cutout(rounds=8, smooth=4)):
                cov = [round(C.cutout_rule(pics[b], maps[b], spec)[0] / S / S, 3) for b in range(min(B, 4))]
                d = dict(inp=inp.data_ptr(), out=rows.data_ptr(), work=work.data_ptr(), xb=dev["xb"].data_ptr(),
                         xk=dev["xk"].data_ptr(), yb=dev["yb"].data_ptr(), yk=dev["yk"].data_ptr(),
                         h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=B, S=S, h=n, w=n, ldo=ldo,
                         xks=host["xk"].shape[1], yks=host["yk"].shape[1], gate=spec.gate, rounds=spec.rounds,
                         smooth=spec.smooth, feather=int(spec.feather))
                med, best = window(lambda i: lib.cutout(d, s), iters, repeats)
                say(f"{family:16s} S {S:3d} map {n:2d} x {n:2d} B {B} {name:5s} rounds {spec.rounds} smooth {spec.smooth}: "
                    f"median {med:7.2f} us  min {best:7.2f} us  (coverage of images 0-3: {cov})")


def row_copies(B: int, repeats: int, say) -> None:
    """Device rows -> pinned host memory, one copy of all B rows, wall time around a synchronised copy."""
    import time

    from kdl.engine.base import overlay_words
    for family, (S, n) in SHAPES.items():
        for name, words in (("cutout", 2 + n * n + 1 + S * S), ("overlay", 2 + n * n + overlay_words(S))):
            dev = torch.zeros((B, words), device="cuda")
            pin = torch.empty((B, words), pin_memory=True)
            ts = []
            for _ in range(repeats + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pin.copy_(dev, non_blocking=True)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            ts = sorted(ts[2:])
            say(f"{family:16s} S {S:3d} {name:7s} rows: {4 * words} bytes a picture, {B} rows to pinned memory median "
                f"{ts[len(ts) // 2]:8.1f} us  min {ts[0]:8.1f} us  ({4 * words * B / ts[len(ts) // 2] / 1e3:.1f} GB/s)")


def engine_pairs(family: str, pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.base import Cutout
    from kdl.engine.tuning import tuning_path
    info = registry.get(family)
    p = info.init_params(0)
    mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
    engines = {"map": info.engine(p, 32, "cuda", **mode), "cutout": info.engine(p, 32, "cuda", cutout=Cutout(), **mode)}
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
        order = ("map", "cutout") if i % 2 == 0 else ("cutout", "map")
        t = {k: timed(engines[k]) for k in order}
        d = (t["cutout"] - t["map"]) * 1e3
        say(f"{family} pair {i}: {'rollout' if 'rollout' in mode else 'explain'} {t['map']:.4f} ms  cutout "
            f"{t['cutout']:.4f} ms  diff {d:+.1f} us ({100 * d / 1e3 / t['map']:+.2f} %)")
    prof = dict(engines["cutout"].profile(32))
    say(f"{family} cutout engine.profile(32), eager launches: cutout step {prof['cutout'] * 1e3:.1f} us, "
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
        print("cutout_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say("== cutout alone (all three launches), batch 32")
    op_alone(32, a.iters, a.repeats, say)
    if not a.alone:
        say("== result rows, device to pinned host memory")
        row_copies(32, a.repeats, say)
    if a.pairs and not a.alone:
        say("== b32 forward (captured graph, device events), heatmap engine vs cutout engine, interleaved pairs")
        for fam in a.families.split(","):
            engine_pairs(fam, a.pairs, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
