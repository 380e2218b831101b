#!/usr/bin/env python
"""serving_bytes micro-benchmarks (profiles/jpeg_serving.txt).

  python tools/jpeg_bench.py --size 534x400                  # host: jpeg_parse vs Pillow, one core
  python tools/jpeg_bench.py --size 534x400 --kernels --images 32   # MI355X: the two HIP kernels
  python tools/jpeg_bench.py --size 534x400 --kernels --images 32 --entropy gpu   # + the device entropy decode

The image is tests/data/pants.png scaled to --size (HxW) and encoded as a quality-90 4:2:0 JPEG.
Host: median microseconds per image of the entropy decode (kdl._rt.jpeg_parse into a reused
buffer) against Pillow's full decode (Image.open().convert("RGB")) on the same core. --kernels:
--images copies decoded in one call, device-event times of jpeg_idct_u8 and jpeg_sample_rgb_u8
(-> 299x299) and the bytes each has to move over that time; needs a GPU, no fallback.
--entropy gpu adds the device entropy decode (profiles/jpeg_entropy_gpu.txt): on the host
jpeg_scan_prepare beside jpeg_parse, on the GPU jpeg_huff_decode + jpeg_dc_scan in front of
jpeg_idct_u8 in the same loop, with the fixed-point rounds the decode took.
--restart rows:N | blocks:N encodes the file with restart markers every N MCU rows / N MCUs
(profiles/jpeg_restart_gpu.txt): the host numbers are of that file, the entropy kernels are
jpeg_huff_rst_decode + jpeg_dc_rst_scan, and "yardstick_entropy_kernels" times jpeg_huff_decode +
jpeg_dc_scan on the same image encoded without markers, in the same run.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402


def restart_kw(spec: str | None) -> dict:
    """--restart rows:N | blocks:N -> the keyword of Pillow's JPEG encoder."""
    if not spec:
        return {}
    kind, _, n = spec.partition(":")
    if kind not in ("rows", "blocks") or not n.isdigit() or int(n) < 1:
        raise SystemExit(f"--restart {spec!r}: expected rows:N or blocks:N")
    return {f"restart_marker_{kind}": int(n)}


def make_file(H: int, W: int, restart: str | None = None) -> bytes:
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    im = Image.open(os.path.join(root, "tests", "data", "pants.png")).convert("RGB").resize((W, H), Image.BILINEAR)
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=90, subsampling=2, **restart_kw(restart))
    return buf.getvalue()


def _median_us(fn, iters: int) -> float:
    fn()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e6


def host(data: bytes, iters: int) -> dict:
    from kdl.ops import _lib
    rt = _lib.rt()
    st, hd = rt.jpeg_probe(data)
    assert st == rt.JPEG_OK, hd.why
    coef = np.empty(hd.ncoef, np.int16)
    parse = _median_us(lambda: rt.jpeg_parse(data, coef), iters)
    pil = _median_us(lambda: Image.open(io.BytesIO(data)).convert("RGB"), iters)
    return {"file_bytes": len(data), "jpeg_parse_us": round(parse, 1), "pillow_decode_us": round(pil, 1),
            "parse_over_pillow": round(parse / pil, 3)}


def host_prepare(data: bytes, iters: int) -> dict:
    """jpeg_scan_prepare -- all the host does for the device entropy decode -- into a reused buffer."""
    from kdl.ops import _lib
    rt = _lib.rt()
    from kdl.serving.jpeg import _intervals
    out = np.empty(rt.jpeg_prepare_bound(len(data), _intervals(data, rt.jpeg_probe(data)[1])), np.uint8)
    st, hd, info = rt.jpeg_scan_prepare(data, out)
    assert st == rt.JPEG_OK and (info.device_ok or info.restart_ok), hd.why
    prep = _median_us(lambda: rt.jpeg_scan_prepare(data, out), iters)
    res = {"jpeg_scan_prepare_us": round(prep, 1), "staged_bytes": info.nbytes, "coefficient_bytes": 2 * hd.ncoef}
    if info.restart_ok:
        res.update(restart_interval=info.ri, intervals=info.nint, groups=info.ngroup)
    return res


def entropy_kernels(data: bytes, n: int, iters: int) -> dict:
    """Device-event times of jpeg_huff_decode, jpeg_dc_scan and jpeg_idct_u8 over ``n`` copies; of
    jpeg_huff_rst_decode and jpeg_dc_rst_scan for a file with restart intervals."""
    import torch

    from kdl.ops import _lib
    if not torch.cuda.is_available():
        raise SystemExit("--kernels needs a GPU")
    from kdl.serving.jpeg import CallLayout, _intervals
    rt, C = _lib.rt(), _lib.lib()
    st, hd = rt.jpeg_probe(data)
    assert st == rt.JPEG_OK, hd.why
    lay = CallLayout([hd.ncoef] * n, [rt.jpeg_prepare_bound(len(data), _intervals(data, hd))] * n)
    hin = np.zeros(lay.nbytes, np.uint8)
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")      # jpeg_idct_u8 reads no resize table
    for k in range(n):
        st, h, info = rt.jpeg_scan_prepare(data, lay.prep(hin, k))
        assert st == rt.JPEG_OK and (info.device_ok or info.restart_ok)
        lay.add(hin, k, h, k, idx, idx)
        lay.add_huff(hin, k, h, info)
    d_in = torch.from_numpy(hin).cuda()
    coef = torch.empty(lay.ncoef, dtype=torch.int16, device="cuda")
    planes = torch.empty(lay.ncoef, dtype=torch.uint8, device="cuda")
    out = torch.empty((n, 1, 1, 3), dtype=torch.uint8, device="cuda")
    status = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    rst = bool(info.restart_ok)
    ha = (lay.huff_rst_args if rst else lay.huff_args)(hin.ctypes.data, d_in.data_ptr(), coef.data_ptr(),
                                                       status.data_ptr(), 2 * n)
    huff, dc = (C.jpeg_huff_rst_decode, C.jpeg_dc_rst_scan) if rst else (C.jpeg_huff_decode, C.jpeg_dc_scan)
    ia = lay.args(hin.ctypes.data, d_in.data_ptr(), planes.data_ptr(), lay.ncoef, out.data_ptr(), n, 1, 1,
                  coef=coef.data_ptr())
    s = torch.cuda.current_stream().cuda_stream
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(iters)]

    def once(e=None):
        for i, fn in enumerate((lambda: huff(ha, s), lambda: dc(ha, s),
                                lambda: C.jpeg_idct_u8(ia, s))):
            if e:
                e[i].record()
            fn()
        if e:
            e[3].record()
    for _ in range(10):
        once()
    torch.cuda.synchronize()
    for e in ev:
        once(e)
    torch.cuda.synchronize()
    st = status.cpu().numpy().reshape(n, 2)
    assert not st[:, 0].any(), "the device decoder rejected the benchmark's own file"
    us = [round(statistics.median(e[i].elapsed_time(e[i + 1]) for e in ev) * 1e3, 1) for i in range(3)]
    shape = ({"intervals": info.nint, "groups_per_image": info.ngroup} if rst else
             {"chunks_per_image": -(-info.nbits // (rt.JPEG_HUFF_SUB_BITS * rt.JPEG_HUFF_CHUNK))})
    return {"images": n, "sub_bits": rt.JPEG_HUFF_SUB_BITS, "chunk": rt.JPEG_HUFF_CHUNK, **shape,
            "most_rounds_of_a_chunk": int(st[:, 1].max()), "huff_decode_us": us[0], "dc_scan_us": us[1],
            "idct_us": us[2], "entropy_us_per_image": round((us[0] + us[1]) / n, 2)}


def kernels(data: bytes, n: int, iters: int, S: int = 299) -> dict:
    import torch

    from kdl.gateway.preprocess import nearest_indices
    from kdl.ops import _lib
    if not torch.cuda.is_available():
        raise SystemExit("--kernels needs a GPU")
    from kdl.serving.jpeg import CallLayout
    rt, C = _lib.rt(), _lib.lib()
    st, hd = rt.jpeg_probe(data)
    assert st == rt.JPEG_OK, hd.why
    lay = CallLayout([hd.ncoef] * n)
    hin = np.zeros(lay.nbytes, np.uint8)
    ys = torch.from_numpy(nearest_indices(hd.H, S)).cuda()
    xs = torch.from_numpy(nearest_indices(hd.W, S)).cuda()
    for k in range(n):
        st, h = rt.jpeg_parse(data, lay.coef(hin, k, hd.ncoef))
        assert st == rt.JPEG_OK
        lay.add(hin, k, h, k, ys, xs)
    d_in = torch.from_numpy(hin).cuda()
    planes = torch.empty(lay.ncoef, dtype=torch.uint8, device="cuda")
    out = torch.empty((n, S, S, 3), dtype=torch.uint8, device="cuda")
    args = lay.args(hin.ctypes.data, d_in.data_ptr(), planes.data_ptr(), lay.ncoef, out.data_ptr(), n, S, S)
    s = torch.cuda.current_stream().cuda_stream
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for _ in range(10):
        C.jpeg_idct_u8(args, s)
        C.jpeg_sample_rgb_u8(args, s)
    torch.cuda.synchronize()
    for e in ev:
        e[0].record()
        C.jpeg_idct_u8(args, s)
        e[1].record()
        C.jpeg_sample_rgb_u8(args, s)
        e[2].record()
    torch.cuda.synchronize()
    idct = statistics.median(e[0].elapsed_time(e[1]) for e in ev) * 1e3
    samp = statistics.median(e[1].elapsed_time(e[2]) for e in ev) * 1e3
    # bytes the algorithm has to move: coefficients in (2 B) + samples out (1 B); then at most all
    # samples in + the resized RGB out
    b_idct, b_samp = 3 * hd.ncoef * n, hd.ncoef * n + n * S * S * 3
    return {"images": n, "blocks": hd.ncoef // 64 * n, "idct_us": round(idct, 1), "sample_rgb_us": round(samp, 1),
            "idct_GBps": round(b_idct / idct / 1e3, 1), "sample_rgb_GBps_upper": round(b_samp / samp / 1e3, 1),
            "both_us_per_image": round((idct + samp) / n, 2)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="534x400", help="HxW")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--entropy", choices=["host", "gpu"], default="host",
                    help="gpu: also time jpeg_scan_prepare and, with --kernels, the device entropy decode")
    ap.add_argument("--restart", default=None, metavar="rows:N|blocks:N",
                    help="encode the file with restart markers every N MCU rows / N MCUs; with --entropy gpu the "
                         "restart kernels are timed, and the plain ones on the file without markers beside them")
    a = ap.parse_args(argv)
    H, W = map(int, a.size.split("x"))
    data = make_file(H, W, a.restart)
    res = {"size": a.size, **host(data, a.iters)}
    if a.entropy == "gpu":
        res.update(host_prepare(data, a.iters))
        res["parse_over_prepare"] = round(res["jpeg_parse_us"] / res["jpeg_scan_prepare_us"], 1)
    if a.kernels:
        res["kernels"] = kernels(data, a.images, a.iters)
        if a.entropy == "gpu":
            res["entropy_kernels"] = entropy_kernels(data, a.images, a.iters)
            if a.restart:
                res["yardstick_entropy_kernels"] = entropy_kernels(make_file(H, W), a.images, a.iters)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
