"""GPU-encoded PNG cutout timings on one GPU (profiles/cutout_png.txt).

  python -m tools.png_bench [--out FILE]

1. png_encode alone (kernels/png_encode.hip, all five launches) for 32 RGBA pictures at S = 224, 299 and 600:
   microseconds per call on noise (no matches, every literal live, the file overflows the default cap) and on a
   photograph (tests/data/pants.png resized, its bright backdrop transparent), with the file sizes of the rule
   beside ``png_bytes``' (filter 0, zlib level 6) and Pillow's. The split between the five launches comes from a
   kernel trace of this same run (--alone).
2. The copy of 32 narrow result rows to pinned host memory, beside the raw cutout rows of the same pictures.
3. A cutout_png engine's batch-32 forward (captured graph) against the cutout engine it rides on, as
   interleaved pairs, and the step's own time from engine.profile.

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events, after
warm-up calls of the same shapes."""
from __future__ import annotations

import argparse
import io
import sys
import time
from pathlib import Path

import numpy as np
import torch

from .overlay_bench import window

PHOTO = Path(__file__).resolve().parent.parent / "tests" / "data" / "pants.png"
SIZES = {"resnet50/vit_b16": (224, 7), "xception": (299, 10), "efficientnet_b7": (600, 19)}


def pictures(B: int, S: int) -> dict:
    from PIL import Image
    rng = np.random.default_rng(3)
    rgb = np.asarray(Image.open(PHOTO).convert("RGB").resize((S, S), Image.BILINEAR), np.uint8)
    alpha = np.where(rgb.astype(np.int64).sum(axis=2) < 700, 255, 0).astype(np.uint8)
    photo = np.dstack([rgb, alpha])
    return {"noise": rng.integers(0, 256, (B, S, S, 4), dtype=np.uint8),
            "photo": np.ascontiguousarray(np.broadcast_to(photo, (B, S, S, 4)))}


def op_alone(B: int, sizes, iters: int, repeats: int, say) -> None:
    from PIL import Image

    from kdl.gateway.client import png_bytes
    from kdl.ops import _lib
    from kdl.serving import png_encode as E
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    for S in sizes:
        cap = E.default_cap(S, S, 4)
        work = torch.zeros(lib.png_encode_workspace(B, S, S, 4, cap), dtype=torch.uint8, device="cuda")
        rows = torch.zeros((B, 1 + (cap + 3) // 4), dtype=torch.int32, device="cuda")
        say(f"S {S:3d}: workspace {work.numel() // B} bytes a picture (tokens {S * ((S * 4 + 8) & ~7) * 2}, stream "
            f"{4 * ((cap + 3) // 4 + 2)}); cap {cap} bytes, a raw picture is {S * S * 4}")
        for name, pics in pictures(B, S).items():
            inp = torch.from_numpy(pics).cuda()
            d = dict(inp=inp.data_ptr(), ldi=S * S * 4, row_stride=S * 4, front=None, nfront=0, ldf=0,
                     out=rows.data_ptr(), ldo=rows.shape[1], work=work.data_ptr(), B=B, H=S, W=S, C=4, cap=cap)
            med, best = window(lambda i: lib.png_encode(d, s), iters, repeats)
            rule = len(E.png_rule(pics[:1], 1 << 24)[0])
            b = io.BytesIO()
            Image.fromarray(pics[0]).save(b, "PNG")
            say(f"S {S:3d} B {B} {name:5s}: median {med:8.2f} us  min {best:8.2f} us  (length word {int(rows[0, 0])}; the "
                f"rule's file {rule} bytes, png_bytes {len(png_bytes(pics[0]))}, Pillow {len(b.getvalue())})")


def row_copies(B: int, repeats: int, say) -> None:
    """Device rows -> pinned host memory, one copy of all B rows, wall time around a synchronised copy."""
    from kdl.engine.base import cutout_png_cap
    for family, (S, n) in SIZES.items():
        front = 2 + n * n + 1
        for name, words in (("cutout_png", front + 1 + (cutout_png_cap(S) + 3) // 4), ("cutout", front + S * S)):
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
            say(f"{family:16s} S {S:3d} {name:10s} rows: {4 * words} bytes a picture, {B} rows to pinned memory median "
                f"{ts[len(ts) // 2]:8.1f} us  min {ts[0]:8.1f} us")


def engine_pairs(family: str, pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.base import Cutout, CutoutPng
    from kdl.engine.tuning import tuning_path
    info = registry.get(family)
    p = info.init_params(0)
    mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
    engines = {"cutout": info.engine(p, 32, "cuda", cutout=Cutout(), **mode),
               "png": info.engine(p, 32, "cuda", cutout=Cutout(), cutout_png=CutoutPng(), **mode)}
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
        order = ("cutout", "png") if i % 2 == 0 else ("png", "cutout")
        t = {k: timed(engines[k]) for k in order}
        d = (t["png"] - t["cutout"]) * 1e3
        say(f"{family} pair {i}: cutout {t['cutout']:.4f} ms  cutout_png {t['png']:.4f} ms  diff {d:+.1f} us "
            f"({100 * d / 1e3 / t['cutout']:+.2f} %)")
    prof = dict(engines["png"].profile(32))
    say(f"{family} cutout_png engine.profile(32), eager launches: cutout_png step {prof['cutout_png'] * 1e3:.1f} us, "
        f"cutout step {prof['cutout'] * 1e3:.1f} us, sum of all steps {sum(prof.values()):.3f} ms")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--sizes", default="224,299,600")
    ap.add_argument("--families", default="xception,vit_b16")
    ap.add_argument("--alone", action="store_true", help="part 1 only (the run to put under a kernel trace)")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("png_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say("== png_encode alone (all five launches), batch 32, RGBA")
    op_alone(32, [int(v) for v in a.sizes.split(",")], a.iters, a.repeats, say)
    if not a.alone:
        say("== result rows, device to pinned host memory")
        row_copies(32, a.repeats, say)
    if a.pairs and not a.alone:
        say("== b32 forward (captured graph, device events), cutout engine vs cutout_png engine, interleaved pairs")
        for fam in a.families.split(","):
            engine_pairs(fam, a.pairs, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
