"""Overlay-as-JPEG timings on one GPU (profiles/overlay_jpeg.txt).

  python -m tools.overlay_jpeg_bench [--out FILE]

1. jpeg_encode alone (kernels/jpeg_encode.hip) for 32 pictures at S = 224, 299 and 600, quality 85, 4:2:0, the
   default cap: microseconds per call (its four launches together) on seeded noise and on the smooth picture
   ``tests/data/pants.png`` resized to S, and the mean file size of each.
2. An overlay_jpeg engine's batch-32 forward (captured graph) against the overlay engine it rides on, as
   interleaved pairs, and the encode step's own time from engine.profile.
3. The D2H of 32 narrow rows into pinned memory, next to the raw overlay rows'.
4. Closed-loop ``/overlay`` latency, ``"format": "jpeg"`` against ``png``: a GPU model server, the gateway in
   ``bytes`` mode in this process, one request at a time.

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events, after warm-up
calls of the same shapes (tools/overlay_bench.py ``window``)."""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

from .overlay_bench import window

PANTS = Path(__file__).parent.parent / "tests" / "data" / "pants.png"


def op_alone(B: int, iters: int, repeats: int, say) -> None:
    from PIL import Image

    from kdl.engine.base import overlay_jpeg_cap
    from kdl.ops import _lib
    from kdl.serving import jpeg_encode as J
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    for S in (224, 299, 600):
        cap = overlay_jpeg_cap(S)
        ldo = 1 + (cap + 3) // 4
        hdr = np.frombuffer(J.header(S, S, 85, "4:2:0"), np.uint8).copy()
        d_hdr = torch.from_numpy(hdr).cuda()
        work = torch.zeros(lib.jpeg_encode_workspace(B, S, S, 1, cap), dtype=torch.uint8, device="cuda")
        out = torch.zeros((B, ldo), dtype=torch.int32, device="cuda")
        pants = np.asarray(Image.open(PANTS).convert("RGB").resize((S, S), Image.BILINEAR))
        pics = {"noise": torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(S)),
                "pants": torch.from_numpy(np.ascontiguousarray(np.broadcast_to(pants, (B, S, S, 3))))}
        for kind, x in pics.items():
            x = x.cuda()
            d = dict(inp=x.data_ptr(), ldi=S * S * 3, hdr=d_hdr.data_ptr(), h_hdr=hdr.ctypes.data, out=out.data_ptr(),
                     ldo=ldo, work=work.data_ptr(), B=B, H=S, W=S, quality=85, sampling=1, cap=cap)
            med, best = window(lambda i: lib.jpeg_encode(d, s), iters, repeats)
            lens = out[:, 0].cpu().numpy()
            assert (lens > 0).all(), lens
            say(f"S {S:3d} B {B} {kind:5s}: median {med:8.2f} us  min {best:8.2f} us  mean file {lens.mean():9.0f} bytes "
                f"({lens.mean() / S / S:.3f} per pixel, cap {cap}), {B * S * S * 3 / med / 1e3:.1f} GB/s of pixels")


def engine_pairs(family: str, pairs: int, say) -> None:
    from kdl.engine import registry
    from kdl.engine.base import Overlay, OverlayJpeg
    from kdl.engine.tuning import tuning_path
    info = registry.get(family)
    p = info.init_params(0)
    mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
    engines = {"overlay": info.engine(p, 32, "cuda", overlay=Overlay(), **mode),
               "jpeg": info.engine(p, 32, "cuda", overlay=Overlay(), overlay_jpeg=OverlayJpeg(), **mode)}
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
        order = ("overlay", "jpeg") if i % 2 == 0 else ("jpeg", "overlay")
        t = {k: timed(engines[k]) for k in order}
        d = (t["jpeg"] - t["overlay"]) * 1e3
        say(f"{family} pair {i}: overlay {t['overlay']:.4f} ms  overlay_jpeg {t['jpeg']:.4f} ms  diff {d:+.1f} us "
            f"({100 * d / 1e3 / t['overlay']:+.2f} %)")
    prof = dict(engines["jpeg"].profile(32))
    say(f"{family} overlay_jpeg engine.profile(32), eager launches: overlay_jpeg step {prof['overlay_jpeg'] * 1e3:.1f} us, "
        f"overlay step {prof['overlay'] * 1e3:.1f} us, sum of all steps {sum(prof.values()):.3f} ms")
    for k, e in engines.items():      # the D2H of the rows, as the executors copy them: one async copy into pinned memory
        host = torch.zeros(tuple(e.logits.shape), dtype=torch.float32).pin_memory()
        med, best = window(lambda i: host.copy_(e.logits, non_blocking=True), 20, 5, warm=3)
        nb = e.logits.numel() * 4
        say(f"{family} D2H of 32 {k} rows ({e.logits.shape[1]} words, {nb / 1e6:.2f} MB): median {med:.1f} us = "
            f"{nb / med / 1e3:.1f} GB/s")


def gateway_latency(n: int, say) -> None:
    import io
    import tempfile

    import grpc
    from PIL import Image

    from kdl.gateway import preprocess as pp
    from kdl.gateway.app import GatewayConfig, create_app
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.server import ModelServer
    b = io.BytesIO()
    Image.open(PANTS).convert("RGB").save(b, "JPEG", quality=90)
    jpeg = b.getvalue()
    pp.fetch = lambda url, timeout=10.0: jpeg                     # no network in the loop: the file is at hand
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(tmp) / "clothing-model"
        (base / "1").mkdir(parents=True)
        (base / "1" / "synthetic.json").write_text('{"seed": 0, "overlay_jpeg": {}}')
        cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                           file_system_poll_wait_seconds=0,
                           batching=BatchingParams(max_batch_size=8, batch_timeout_micros=0, allowed_batch_sizes=[1, 8]))
        srv = ModelServer(cfg).start(block_until_loaded=True)
        try:
            with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
                c = create_app(GatewayConfig({"GATEWAY_MODE": "bytes"}), channel=ch).test_client()
                for fmt in ("png", "jpeg", "png", "jpeg"):
                    ts = []
                    for i in range(n + 5):
                        t0 = time.perf_counter()
                        r = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg", "format": fmt})
                        ts.append((time.perf_counter() - t0) * 1e3)
                        assert r.status_code == 200, r.data
                    ts = ts[5:]
                    say(f"gateway /overlay format {fmt:4s} closed loop, 1 client, {n} requests ({len(r.data)} byte answer): "
                        f"median {statistics.median(ts):.2f} ms  p90 {float(np.percentile(ts, 90)):.2f} ms  min {min(ts):.2f} ms")
        finally:
            srv.stop(0)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--families", default="xception,vit_b16")
    ap.add_argument("--requests", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("overlay_jpeg_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    say("== jpeg_encode alone, batch 32, quality 85, 4:2:0, cap ceil(S*S*3/2)")
    op_alone(32, a.iters, a.repeats, say)
    if a.pairs:
        say("== b32 forward (captured graph, device events), overlay engine vs overlay_jpeg engine, interleaved pairs")
        for fam in a.families.split(","):
            engine_pairs(fam, a.pairs, say)
    if a.requests:
        say("== gateway, GATEWAY_MODE=bytes, Xception on one GPU")
        gateway_latency(a.requests, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
