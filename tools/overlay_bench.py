"""Rendered-overlay timings on one GPU (profiles/overlay.txt).

  python -m tools.overlay_bench [--out FILE]

1. The box's own fill and copy rates from this run (a 1 GiB ``fill_`` and a 1 GiB device-to-device
   ``copy_``), the yardsticks for a bandwidth-bound launch.
2. heat_overlay alone (kernels/overlay.hip) at the four family shapes and batch 32: microseconds per
   call and the implied bytes/s over 2 * B * S^2 * 3 (the photograph read, the picture written).
   "same" re-uses one input and one row buffer (both may sit in the Infinity Cache, as the input does
   inside a forward); "rotating" walks over copies of at least 1 GiB in total, so every call goes to HBM.
3. An overlay engine's batch-32 forward (captured graph) against the explain / rollout engine it rides
   on, as interleaved pairs, and the overlay step's own time from engine.profile.
4. The D2H of the wider rows into pinned memory, next to the explain rows'.
5. One closed-loop ``/overlay`` latency: a GPU model server, the gateway in ``bytes`` mode in this
   process, one request at a time.

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events,
after warm-up calls of the same shapes."""
from __future__ import annotations

import argparse
import statistics
import sys
import time

import numpy as np
import torch

SHAPES = {"xception": (299, 10), "resnet50": (224, 7), "efficientnet_b7": (600, 19), "vit_b16": (224, 14)}


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


def box_rates(say) -> None:
    n = 1 << 30
    a = torch.empty(n, dtype=torch.uint8, device="cuda")
    b = torch.empty(n, dtype=torch.uint8, device="cuda")
    med, best = window(lambda i: a.fill_(i & 255), 10, 5, warm=3)
    say(f"fill_ 1 GiB: median {med:8.1f} us = {n / med / 1e6:.2f} TB/s written")
    med, best = window(lambda i: b.copy_(a), 10, 5, warm=3)
    say(f"copy_ 1 GiB: median {med:8.1f} us = {2 * n / med / 1e6:.2f} TB/s read + written")


def op_alone(B: int, iters: int, repeats: int, say) -> None:
    from kdl.ops import _lib
    from kdl.serving import overlay as O
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    tab = torch.from_numpy(O.colormap_table("jet")).cuda()
    for family, (S, n) in SHAPES.items():
        host = dict(zip(("xb", "xk", "yb", "yk"), O.axis_tables(n, S, "bilinear") + O.axis_tables(n, S, "bilinear")))
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        ldo = 2 + n * n + (S * S * 3 + 3) // 4
        moved = 2 * B * S * S * 3
        copies = max(2, -(-(1 << 30) // moved))
        g = torch.Generator(device="cuda").manual_seed(3)
        inps = [torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(copies)]
        rows = [torch.rand((B, ldo), device="cuda", generator=g) for _ in range(copies)]

        def run(i, j):
            lib.heat_overlay(dict(inp=inps[j].data_ptr(), out=rows[j].data_ptr(), tab=tab.data_ptr(),
                                  xb=dev["xb"].data_ptr(), xk=dev["xk"].data_ptr(), yb=dev["yb"].data_ptr(),
                                  yk=dev["yk"].data_ptr(), h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data,
                                  B=B, S=S, h=n, w=n, ldo=ldo, xks=host["xk"].shape[1], yks=host["yk"].shape[1],
                                  a=128, blend=1), s)
        for kind, pick in (("same", lambda i: 0), ("rotating", lambda i: i % copies)):
            med, best = window(lambda i: run(i, pick(i)), iters, repeats)
            say(f"{family:16s} S {S:3d} map {n:2d} x {n:2d} B {B} {kind:8s}: median {med:7.2f} us  min {best:7.2f} us  "
                f"{moved / 1e6:.1f} MB -> {moved / med / 1e6:.2f} TB/s")
        del inps, rows


def engine_pairs(family: str, pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.base import Overlay
    from kdl.engine.tuning import tuning_path
    info = registry.get(family)
    p = info.init_params(0)
    mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
    engines = {"map": info.engine(p, 32, "cuda", **mode), "overlay": info.engine(p, 32, "cuda", overlay=Overlay(), **mode)}
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
        order = ("map", "overlay") if i % 2 == 0 else ("overlay", "map")
        t = {k: timed(engines[k]) for k in order}
        d = (t["overlay"] - t["map"]) * 1e3
        say(f"{family} pair {i}: {'rollout' if 'rollout' in mode else 'explain'} {t['map']:.4f} ms  overlay "
            f"{t['overlay']:.4f} ms  diff {d:+.1f} us ({100 * d / 1e3 / t['map']:+.2f} %)")
    prof = dict(engines["overlay"].profile(32))
    say(f"{family} overlay engine.profile(32), eager launches: overlay step {prof['overlay'] * 1e3:.1f} us, "
        f"sum of all steps {sum(prof.values()):.3f} ms")
    # the D2H of the rows, as the executors copy them: one async copy into pinned memory
    for k, e in engines.items():
        host = torch.zeros(tuple(e.logits.shape), dtype=torch.float32).pin_memory()
        med, best = window(lambda i: host.copy_(e.logits, non_blocking=True), 20, 5, warm=3)
        nb = e.logits.numel() * 4
        say(f"{family} D2H of 32 {k} rows ({e.logits.shape[1]} words, {nb / 1e6:.2f} MB): median {med:.1f} us = "
            f"{nb / med / 1e3:.1f} GB/s")


def gateway_latency(n: int, say) -> None:
    import io
    import tempfile
    from pathlib import Path

    import grpc
    from PIL import Image

    from kdl.gateway import preprocess as pp
    from kdl.gateway.app import GatewayConfig, create_app
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.server import ModelServer
    b = io.BytesIO()
    Image.open(Path(__file__).parent.parent / "tests" / "data" / "pants.png").convert("RGB").save(b, "JPEG", quality=90)
    jpeg = b.getvalue()
    pp.fetch = lambda url, timeout=10.0: jpeg                     # no network in the loop: the file is at hand
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(tmp) / "clothing-model"
        (base / "1").mkdir(parents=True)
        (base / "1" / "synthetic.json").write_text('{"seed": 0}')
        cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                           file_system_poll_wait_seconds=0,
                           batching=BatchingParams(max_batch_size=8, batch_timeout_micros=0, allowed_batch_sizes=[1, 8]))
        srv = ModelServer(cfg).start(block_until_loaded=True)
        try:
            with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
                c = create_app(GatewayConfig({"GATEWAY_MODE": "bytes"}), channel=ch).test_client()
                for route in ("/explain", "/overlay"):
                    ts = []
                    for i in range(n + 5):
                        t0 = time.perf_counter()
                        r = c.post(route, json={"url": "http://example.invalid/pants.jpg"})
                        ts.append((time.perf_counter() - t0) * 1e3)
                        assert r.status_code == 200, r.data
                    ts = ts[5:]
                    say(f"gateway {route:9s} closed loop, 1 client, {n} requests ({len(r.data)} byte answer): median "
                        f"{statistics.median(ts):.2f} ms  p90 {float(np.percentile(ts, 90)):.2f} ms  min {min(ts):.2f} ms")
        finally:
            srv.stop(0)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--families", default="xception,vit_b16")
    ap.add_argument("--requests", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("overlay_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say("== the box: fill and copy rates of this run")
    box_rates(say)
    say("== heat_overlay alone, batch 32, bilinear, jet, a = 128, heat-weighted")
    op_alone(32, a.iters, a.repeats, say)
    if a.pairs:
        say("== b32 forward (captured graph, device events), heatmap engine vs overlay engine, interleaved pairs")
        for fam in a.families.split(","):
            engine_pairs(fam, a.pairs, say)
    if a.requests:
        say("== gateway, GATEWAY_MODE=bytes, Xception on one GPU")
        gateway_latency(a.requests, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
