"""``serving_image``: uint8 images of ANY size, resized to the model input on the GPU.

The reference resizes in the gateway, on the CPU: keras_image_helper's PIL
``Image.NEAREST`` to 299x299 (`model_server.py:18,53`), then ships
f32 pixels. Here the gateway may ship the decoded pixels as they are
(``GATEWAY_MODE=raw``) and the model server resizes them with the table-driven
``resize_nearest_u8`` kernel (kdl/csrc/kernels/preprocess.hip; the row / column
tables are PIL's own double-precision rule, ``gateway.preprocess.nearest_indices``,
so the result is bit-identical to PIL) before the resized batch joins the
``serving_uint8`` batcher. Without a GPU the same tables drive a numpy gather.

With native GPU executors behind the batcher the resized images never come back to the
host: the kernel writes them into a device buffer, the request is queued as a
device-resident batcher item (``DynamicBatcher.submit_device``) and the executor's backend
copies its rows device-to-device into the engine's input slot (``HipExecBackend::issue_dev``,
kdl/csrc/runtime/hip_backend.cpp) while the other rows of the batch come from the pinned
staging as usual.

NEAREST squashed to S x S is the default. A model version may name another preprocess spec
(``gateway.preprocess.ResizeSpec``: ``"<filter>[:<R>]"``): the filters of Pillow's ``Image.resize``
and torchvision's ``Resize(R)`` + ``CenterCrop(S)``. A filter runs as two launches over all images
of the request (kdl/csrc/kernels/resample.hip): ``resample_h_u8``, Pillow's horizontal pass over
the source rows and output columns the crop window needs, and ``resample_v_u8``, its vertical
pass into the batch, both driven by Pillow's own coefficient tables (``kdl._rt.resample_coeffs``),
so the result equals ``gateway.preprocess.apply_spec_pil`` bit for bit. CPU servers call that.
"""
from __future__ import annotations

import contextlib
import os
import threading
from collections import OrderedDict

import numpy as np
import torch

from ..gateway.preprocess import NEAREST_SPEC, ResizeSpec, apply_spec_pil, nearest_indices
from ..ops import _lib
from .metrics import METRICS

IMAGE_SIGNATURE = "serving_image"
MAX_PIXELS = int(os.environ.get("KDL_MAX_IMAGE_PIXELS", str(64 << 20)))   # per request, all images


FILTER_IDS = {"box": 0, "bilinear": 1, "hamming": 2, "bicubic": 3, "lanczos": 4}   # kdl._rt.resample_coeffs
# what one output column of resample_h_u8 may need (its LDS budget, kernels/resample.hip: kCoefMax,
# kSpanMax): 65535 pixels across to 224 with LANCZOS are 1757 taps
MAX_TAPS, MAX_SPAN = 4096, 2048


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


class FilterTables:
    """The tables of one filtered resize + crop: H x W resized to nh x nw with ``flt``, of which
    the OH x OW window at (top, left) is kept. Per axis Pillow's bounds / coefficient pair
    (``kdl._rt.resample_coeffs``) sliced to the window, as host arrays (the launchers check the
    bounds) and, with ``dev``, as device tensors (the kernels follow them)."""

    def __init__(self, H: int, W: int, nh: int, nw: int, flt: str, dev: torch.device | None,
                 window: tuple[int, int, int, int] | None = None):
        rt = _lib.rt()
        top, left, OH, OW = window or (0, 0, nh, nw)
        assert 0 <= top and top + OH <= nh and 0 <= left and left + OW <= nw and OH > 0 and OW > 0
        f = FILTER_IDS[flt]
        xb, xk = rt.resample_coeffs(W, nw, f)
        yb, yk = rt.resample_coeffs(H, nh, f)
        self.H, self.W, self.OH, self.OW = H, W, OH, OW
        self.xb, self.xk = np.ascontiguousarray(xb[left:left + OW]), np.ascontiguousarray(xk[left:left + OW])
        self.yb, self.yk = np.ascontiguousarray(yb[top:top + OH]), np.ascontiguousarray(yk[top:top + OH])
        # the source rows the vertical pass reads: all the horizontal pass has to produce
        self.row0 = int(self.yb[0, 0])
        self.rows = int(self.yb[-1, 0] + self.yb[-1, 1]) - self.row0
        self.tmp_bytes = self.rows * _align(OW * 3, 4)
        self.dev = [] if dev is None else [torch.from_numpy(t).to(dev) for t in (self.xb, self.xk, self.yb, self.yk)]

    @classmethod
    def for_spec(cls, H: int, W: int, spec: ResizeSpec, S: int, dev: torch.device | None) -> "FilterTables":
        nh, nw, top, left = spec.geometry(H, W, S)
        return cls(H, W, nh, nw, spec.filter, dev, (top, left, S, S))

    def desc(self, src: int, tmp_off: int, out_row: int) -> np.ndarray:
        """The raw ResampleDesc of one image: ``src`` its pixels' device address (raw kind) or the
        index of its JpegDesc; its intermediate at ``tmp_off``; its output row."""
        d_xb, d_xk, d_yb, d_yk = (_lib.ptr(t) for t in self.dev)
        return np.frombuffer(_lib.rt().resample_desc(
            src, d_xb, d_xk, d_yb, d_yk, self.xb.ctypes.data, self.yb.ctypes.data, tmp_off, self.W, self.H,
            self.xk.shape[1], self.yk.shape[1], self.row0, self.rows, out_row), np.uint8)


class _Ctx:
    """One in-flight resize: its own stream and pinned / device buffers (grown on demand).
    Outgrown device output buffers are kept, not freed: a device-resident batcher item whose
    request hit its deadline returns before the executor's device-to-device copy of it ran,
    so its buffer must stay valid (a later request may overwrite it: only the abandoned row
    reads garbage)."""

    def __init__(self, dev: torch.device):
        self.dev = dev
        self.stream = torch.cuda.Stream(device=dev)
        self.cap_in = self.cap_out = 0
        self._retired: list[torch.Tensor] = []
        # serving_bytes (jpeg.py): sample-plane scratch of the JPEG kernels, and what the stream
        # still reads (resize tables, fallback pixels) until the request has synchronised
        self.cap_planes = 0
        self.d_planes: torch.Tensor | None = None
        self.keep: list | None = None
        # intermediate of the filtered resize (csrc/kernels/resample.hip): the horizontal pass's rows
        self.cap_tmp = 0
        self.d_tmp: torch.Tensor | None = None
        # device entropy decode (csrc/kernels/jpeg_huff.hip): the coefficient planes never leave the
        # device; per image an error word and a round count come back (n_status images in flight)
        self.cap_coef = 0
        self.d_coef: torch.Tensor | None = None
        self.cap_status = self.n_status = 0
        self.d_status: torch.Tensor | None = None
        self.h_status: torch.Tensor | None = None

    def grow_coef(self, n: int, images: int) -> None:
        if n > self.cap_coef:
            self.cap_coef = max(n, 2 * self.cap_coef)
            self.d_coef = torch.empty(self.cap_coef, dtype=torch.int16, device=self.dev)
        if 2 * images > self.cap_status:
            self.cap_status = max(2 * images, 2 * self.cap_status)
            self.d_status = torch.empty(self.cap_status, dtype=torch.int32, device=self.dev)
            self.h_status = torch.empty(self.cap_status, dtype=torch.int32).pin_memory()

    def grow_tmp(self, n: int) -> None:
        if n > self.cap_tmp:
            self.cap_tmp = max(n, 2 * self.cap_tmp)
            self.d_tmp = torch.empty(self.cap_tmp, dtype=torch.uint8, device=self.dev)

    def grow_planes(self, n: int) -> None:
        if n > self.cap_planes:
            self.cap_planes = max(n, 2 * self.cap_planes)
            self.d_planes = torch.empty(self.cap_planes, dtype=torch.uint8, device=self.dev)

    def grow(self, n_in: int, n_out: int) -> None:
        if n_in > self.cap_in:
            self.cap_in = max(n_in, 2 * self.cap_in)
            self.h_in = torch.empty(self.cap_in, dtype=torch.uint8).pin_memory()
            self.d_in = torch.empty(self.cap_in, dtype=torch.uint8, device=self.dev)
        if n_out > self.cap_out:
            if self.cap_out:
                self._retired.append(self.d_out)
            self.cap_out = max(n_out, 2 * self.cap_out)
            self.h_out = torch.empty(self.cap_out, dtype=torch.uint8).pin_memory()
            self.d_out = torch.empty(self.cap_out, dtype=torch.uint8, device=self.dev)


class Resizer:
    """[n, H, W, 3] uint8 -> [n, S, S, 3] uint8 under ``spec`` (default: NEAREST, squashed),
    Pillow-exact. ``device``: a GPU index (HIP kernels), a list of them (contexts spread over the
    GPUs), or None (numpy for NEAREST, Pillow itself for the filters). Concurrent
    requests do not serialise: each call takes one of up to ``KDL_RESIZE_CTX`` (default 4) per
    GPU contexts -- stream + pinned staging -- from a free list, so the H2D, kernel and D2H of
    different requests overlap on the GPU."""

    def __init__(self, size: int, device: int | list[int] | None, contexts: int | None = None,
                 spec: ResizeSpec | str | None = None):
        self.S = size
        # how the image becomes S x S (gateway.preprocess.ResizeSpec): the default is PIL NEAREST,
        # squashed; a filter runs as resample_h_u8 + resample_v_u8 (Pillow's Image.resize, exact),
        # and with ``:R`` only the center crop's window of the resized image is computed
        self.spec = ResizeSpec.parse(spec, size)
        self.filtered = self.spec.filter != "nearest"
        devs = [] if device is None else [device] if isinstance(device, int) else list(device)
        self.device = devs[0] if devs else None
        self._tab_lock = threading.Lock()
        self._tabs: OrderedDict[tuple[int, int, int], tuple] = OrderedDict()
        if devs:
            import queue
            n = contexts or int(os.environ.get("KDL_RESIZE_CTX", "4"))
            self._free: queue.SimpleQueue = queue.SimpleQueue()
            for _ in range(max(1, n)):
                for d in devs:
                    self._free.put(_Ctx(torch.device("cuda", d)))

    def _tables(self, H: int, W: int, dev: torch.device | None):
        key = (H, W, -1 if dev is None else dev.index)
        with self._tab_lock:
            t = self._tabs.get(key)
            if t is None:
                S = self.S
                if self.filtered:
                    t = FilterTables.for_spec(H, W, self.spec, S, dev)
                    if dev is not None and (t.xk.shape[1] > MAX_TAPS or int(t.xb[:, 1].max()) > MAX_SPAN):
                        from .backend import ServingError
                        raise ServingError("INVALID_ARGUMENT", f"a {H}x{W} image is too wide for {self.spec} to "
                                           f"{S}x{S}: {t.xk.shape[1]} taps per output pixel")
                else:
                    nh, nw, top, left = self.spec.geometry(H, W, S)     # a crop window is a slice of the tables
                    ys, xs = nearest_indices(H, nh)[top:top + S], nearest_indices(W, nw)[left:left + S]
                    if dev is not None:
                        ys = torch.from_numpy(np.ascontiguousarray(ys)).to(dev)
                        xs = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
                    t = (ys, xs)
                self._tabs[key] = t
                if len(self._tabs) > 256:
                    self._tabs.popitem(last=False)
            else:
                self._tabs.move_to_end(key)
            return t

    def _check(self, x: np.ndarray) -> None:
        assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[3] == 3, (x.dtype, x.shape)
        n, H, W, _ = x.shape
        if n * H * W > MAX_PIXELS:
            raise ValueError(f"{n} images of {H}x{W} exceed the {MAX_PIXELS}-pixel request limit")

    def _resize_on(self, c: _Ctx, x: np.ndarray) -> int:
        """H2D + resize kernel on context ``c``'s stream; returns the output's element count."""
        n, H, W, _ = x.shape
        S = self.S
        n_in, n_out = x.size, n * S * S * 3
        METRICS.inc("kdl_resize_total", filter=self.spec.filter)
        if self.filtered:
            return self._resample_on(c, x)
        ys, xs = self._tables(H, W, c.dev)
        c.grow(n_in, n_out)
        c.h_in[:n_in].numpy()[:] = x.reshape(-1)
        with torch.cuda.device(c.dev), torch.cuda.stream(c.stream):
            c.d_in[:n_in].copy_(c.h_in[:n_in], non_blocking=True)
            _lib.lib().resize_nearest_u8(
                dict(src=_lib.ptr(c.d_in), dst=_lib.ptr(c.d_out), ytab=_lib.ptr(ys), xtab=_lib.ptr(xs),
                     SH=H, SW=W, OH=S, OW=S, n=n), int(c.stream.cuda_stream))
        return n_out

    def _resample_on(self, c: _Ctx, x: np.ndarray) -> int:
        """The filtered spec: H2D, then the horizontal and the vertical pass over all n images.
        Staging: [pixels | one ResampleDesc per image]."""
        C, D = _lib.lib(), _lib.rt().RESAMPLE_DESC_BYTES
        n, H, W, _ = x.shape
        S = self.S
        tabs = self._tables(H, W, c.dev)
        off_desc = _align(x.size, 256)
        n_in, n_out = off_desc + n * D, n * S * S * 3
        c.grow(n_in, n_out)
        c.grow_tmp(n * tabs.tmp_bytes)
        hin = c.h_in.numpy()
        hin[:x.size] = x.reshape(-1)
        for i in range(n):
            hin[off_desc + i * D: off_desc + (i + 1) * D] = tabs.desc(_lib.ptr(c.d_in) + i * H * W * 3,
                                                                     i * tabs.tmp_bytes, i)
        c.keep = [tabs]                                 # its device tables, until the next request of the context
        stream = int(c.stream.cuda_stream)
        with torch.cuda.device(c.dev), torch.cuda.stream(c.stream):
            c.d_in[:n_in].copy_(c.h_in[:n_in], non_blocking=True)
            args = dict(desc=_lib.ptr(c.d_in) + off_desc, h_desc=_lib.ptr(c.h_in) + off_desc, tmp=_lib.ptr(c.d_tmp),
                        tmp_cap=c.cap_tmp, out=_lib.ptr(c.d_out), out_rows=n, OH=S, OW=S, n=n)
            C.resample_h_u8(args, 0, stream)
            C.resample_v_u8(args, stream)
        return n_out

    def __call__(self, x: np.ndarray) -> np.ndarray:
        self._check(x)
        n, H, W, _ = x.shape
        S = self.S
        if self.device is None:
            METRICS.inc("kdl_resize_total", filter=self.spec.filter)
            if self.filtered:                       # CPU servers: Pillow itself
                from PIL import Image
                return np.stack([apply_spec_pil(Image.fromarray(im), self.spec, S) for im in x])
            ys, xs = self._tables(H, W, None)
            return np.ascontiguousarray(x[:, ys][:, :, xs])
        c = self._free.get()
        try:
            n_out = self._resize_on(c, x)
            with torch.cuda.device(c.dev), torch.cuda.stream(c.stream):
                c.h_out[:n_out].copy_(c.d_out[:n_out], non_blocking=True)
            c.stream.synchronize()
            return c.h_out[:n_out].numpy().reshape(n, S, S, 3).copy()
        finally:
            self._free.put(c)

    @contextlib.contextmanager
    def on_device(self, x: np.ndarray):
        """Resize into a device buffer and yield its address ([n, S, S, 3] uint8, valid inside
        the block; the kernel has finished when the block starts)."""
        assert self.device is not None
        self._check(x)
        c = self._free.get()
        try:
            self._resize_on(c, x)
            c.stream.synchronize()
            yield _lib.ptr(c.d_out)
        finally:
            self._free.put(c)


class ImageRunner:
    """The ``serving_image`` signature: resize (GPU when the servable has one), then the
    ``serving_uint8`` runner's batcher and executors; images already at the model size
    skip the resize, unless the spec resizes to another size before its crop."""

    def __init__(self, sig, inner, devices: list[int], spec: ResizeSpec | None = None):
        self.sig, self.inner = sig, inner
        self.source = inner.source
        self.spec = spec if spec is not None else getattr(inner.source, "preprocess", NEAREST_SPEC)
        self.resizer = Resizer(inner.source.input_size, devices or None, spec=self.spec)
        self.device_path = bool(devices) and inner.takes_device_items()

    def predict(self, x, n: int, deadline_us: int) -> np.ndarray:
        x = np.asarray(x)
        S = self.source.input_size
        # a squash of an S x S image is the image itself (Pillow returns a copy); with a resize
        # target R != S the image is still resized and cropped
        if x.shape[1:3] == (S, S) and self.spec.resize_to in (None, S):
            return self.inner.predict(np.ascontiguousarray(x), n, deadline_us)
        if self.device_path:           # resized straight into device memory: no host round trip
            with self.resizer.on_device(x) as ptr:
                return self.inner.predict_device(ptr, n, deadline_us)
        return self.inner.predict(self.resizer(x), n, deadline_us)

    def healthy(self) -> bool:
        return self.inner.healthy()

    def close(self) -> None:       # the inner runner belongs to the servable
        pass
