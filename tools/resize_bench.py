#!/usr/bin/env python
"""Filtered resize micro-benchmark (profiles/resize_filters.txt).

  python tools/resize_bench.py                      # every step, each in a child under `timeout`
  python tools/resize_bench.py --step raw:squash    # one step in this process

32 images of 534x400 (HxW; tests/data/pants.png scaled, for the JPEG source a quality-90 4:2:0
file) become model inputs on one MI355X. Steps: source raw | jpeg x shape squash (-> 299x299) |
crop (shorter side 256, center 224). Each step times nearest, bilinear, bicubic and lanczos:
medians of device-event intervals around resample_h_u8 and resample_v_u8 (nearest: the one
resize_nearest_u8 / jpeg_sample_rgb_u8 launch), the bytes each launch has to move over that time,
and beside them what a user pays today: the single-thread Pillow time of the same operation on the
same machine (apply_spec_pil on decoded pixels). jpeg_idct_u8 is the same for every filter and is
listed on its own. Needs a GPU, no fallback; the driver stops at the first step that fails.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

FILTERS = ("nearest", "bilinear", "bicubic", "lanczos")
SHAPES = {"squash": (None, 299), "crop": (256, 224)}
STEPS = [f"{src}:{shape}" for src in ("raw", "jpeg") for shape in SHAPES]
H, W = 400, 534


def image() -> Image.Image:
    return Image.open(os.path.join(ROOT, "tests", "data", "pants.png")).convert("RGB").resize((W, H), Image.BILINEAR)


def _events(torch, launches, iters: int) -> list[float]:
    """Median microseconds of each launch of ``launches`` (callables), timed back to back."""
    for _ in range(10):
        for fn in launches:
            fn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(launches) + 1)] for _ in range(iters)]
    for e in ev:
        e[0].record()
        for k, fn in enumerate(launches):
            fn()
            e[k + 1].record()
    torch.cuda.synchronize()
    return [statistics.median(e[k].elapsed_time(e[k + 1]) for e in ev) * 1e3 for k in range(len(launches))]


def step(name: str, n: int, iters: int) -> dict:
    import torch

    from kdl.gateway.preprocess import ResizeSpec, apply_spec_pil, nearest_indices
    from kdl.ops import _lib
    from kdl.serving.jpeg import CallLayout
    from kdl.serving.resize import FilterTables
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench needs a GPU")
    rt, C = _lib.rt(), _lib.lib()
    source, shape = name.split(":")
    R, S = SHAPES[shape]
    im = image()
    dev = torch.device("cuda")
    s = torch.cuda.current_stream().cuda_stream
    out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    res = {"step": name, "images": n, "source_hw": [H, W], "S": S, "R": R}
    plane_bytes = H * W * 3                         # per image: what the horizontal pass can read at most
    if source == "raw":
        src = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(im)] * n))).cuda()
        jpeg = {}
    else:
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=90, subsampling=2)
        data = buf.getvalue()
        st, hd = rt.jpeg_probe(data)
        assert st == rt.JPEG_OK, hd.why
        lay = CallLayout([hd.ncoef] * n)
        hin = np.zeros(lay.nbytes, np.uint8)
        plane_bytes = hd.ncoef
    rows = []
    for flt in FILTERS:
        spec = ResizeSpec(flt, R)
        nh, nw, top, left = spec.geometry(H, W, S)
        pil_im = im.copy()
        apply_spec_pil(pil_im, spec, S)
        ts = []
        for _ in range(20):
            t = time.perf_counter()
            apply_spec_pil(pil_im, spec, S)
            ts.append(time.perf_counter() - t)
        row = {"filter": flt, "pillow_us_per_image": round(statistics.median(ts) * 1e6, 1)}
        if flt == "nearest":
            ys = torch.from_numpy(np.ascontiguousarray(nearest_indices(H, nh)[top:top + S])).cuda()
            xs = torch.from_numpy(np.ascontiguousarray(nearest_indices(W, nw)[left:left + S])).cuda()
        else:
            t = FilterTables.for_spec(H, W, spec, S, dev)
            tmp = torch.empty(n * t.tmp_bytes, dtype=torch.uint8, device=dev)
            row.update(ksize=[int(t.xk.shape[1]), int(t.yk.shape[1])], rows=t.rows)
        if source == "jpeg":
            lay.n_desc = lay.n_wg = 0
            tabs = (ys, xs) if flt == "nearest" else (t.dev[2], t.dev[0])
            for k in range(n):
                st, h = rt.jpeg_parse(data, lay.coef(hin, k, hd.ncoef))
                assert st == rt.JPEG_OK
                lay.add(hin, k, h, k, *tabs)
            d_in = torch.from_numpy(hin).cuda()
            planes = torch.empty(lay.ncoef, dtype=torch.uint8, device=dev)
            jargs = lay.args(hin.ctypes.data, d_in.data_ptr(), planes.data_ptr(), lay.ncoef, out.data_ptr(), n, S, S)
            jpeg = dict(jdesc=d_in.data_ptr(), h_jdesc=hin.ctypes.data, n_jdesc=n, planes=planes.data_ptr(),
                        plane_cap=lay.ncoef)
            C.jpeg_idct_u8(jargs, s)
            if "jpeg_idct_us" not in res:
                res["jpeg_idct_us"] = round(_events(torch, [lambda: C.jpeg_idct_u8(jargs, s)], iters)[0], 1)
        if flt == "nearest":
            if source == "raw":
                a = dict(src=src.data_ptr(), dst=out.data_ptr(), ytab=ys.data_ptr(), xtab=xs.data_ptr(), SH=H, SW=W,
                         OH=S, OW=S, n=n)
                us = _events(torch, [lambda: C.resize_nearest_u8(a, s)], iters)
            else:
                us = _events(torch, [lambda: C.jpeg_sample_rgb_u8(jargs, s)], iters)
            row.update(launch_us=[round(us[0], 1)], total_us=round(us[0], 1))
        else:
            h_desc = np.concatenate([t.desc(k if source == "jpeg" else src.data_ptr() + k * H * W * 3,
                                            k * t.tmp_bytes, k) for k in range(n)])
            d_desc = torch.from_numpy(h_desc).cuda()
            a = dict(desc=d_desc.data_ptr(), h_desc=h_desc.ctypes.data, tmp=tmp.data_ptr(), tmp_cap=tmp.numel(),
                     out=out.data_ptr(), out_rows=n, OH=S, OW=S, n=n, **jpeg)
            kind = 1 if source == "jpeg" else 0
            us = _events(torch, [lambda: C.resample_h_u8(a, kind, s), lambda: C.resample_v_u8(a, s)], iters)
            # bytes each launch has to move: the source rows it reads (an upper bound: only the
            # crop window's columns are read) + the intermediate; the intermediate + the batch
            b_h = n * (plane_bytes * t.rows // H + t.tmp_bytes)
            b_v = n * (t.tmp_bytes + S * S * 3)
            row.update(launch_us=[round(u, 1) for u in us], total_us=round(sum(us), 1),
                       h_MB=round(b_h / 1e6, 2), v_MB=round(b_v / 1e6, 2),
                       h_GBps_upper=round(b_h / us[0] / 1e3, 1), v_GBps=round(b_v / us[1] / 1e3, 1))
        row["us_per_image"] = round(row["total_us"] / n, 2)
        row["pillow_over_gpu"] = round(row["pillow_us_per_image"] * n / row["total_us"], 1)
        rows.append(row)
    torch.cuda.synchronize()
    res["filters"] = rows
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step_timeout", type=int, default=120, help="seconds per step (driver)")
    a = ap.parse_args(argv)
    if a.step:
        print(json.dumps(step(a.step, a.images, a.iters)), flush=True)
        return 0
    for name in STEPS:                  # one child per step, each under its own time limit
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--images", str(a.images), "--iters", str(a.iters)]
        print(f"$ python tools/resize_bench.py --step {name} --images {a.images} --iters {a.iters}", flush=True)
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"step {name} ended with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
