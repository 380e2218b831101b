"""``serving_bytes``: encoded image files in, decoded on the model server.

TF-Serving models commonly take the image file itself as a ``DT_STRING`` tensor
(``{"b64": ...}`` over REST); with it the gateway is a plain proxy (``GATEWAY_MODE=bytes``):
about 50 KB per image cross the wire instead of 640 KB of pixels, and no gateway core decodes.

Baseline JPEG -- what the web serves -- is split at its serial part. The host Huffman-decodes
each file into quantised coefficient planes (``kdl._rt.jpeg_parse``, csrc/runtime/jpeg.cpp,
GIL released, straight into pinned staging); everything per pixel is two HIP launches per
request (csrc/kernels/jpeg.hip): ``jpeg_idct_u8`` for all blocks of all images, then
``jpeg_sample_rgb_u8``, which reads only the source pixels that PIL's NEAREST resize would keep
(the tables of ``resize_nearest_u8``), upsamples the chroma at those positions, converts to RGB
and writes the image's row of the model batch. The full-size RGB image never exists and, with
native executors, the batch never returns to the host. The arithmetic is libjpeg-turbo's
default decode, so each row equals ``gateway.preprocess.to_uint8(load_image(data), (S, S))``
bit for bit and the logits equal ``serving_image``'s for the PIL-decoded pixels.

Under a filtered preprocess spec (serving/resize.py) the second launch is replaced by Pillow's two
resize passes: ``jpeg_idct_u8`` -> ``resample_h_u8`` (JPEG kind: the horizontal pass reads the
sample planes and converts each source pixel once on its way into LDS) -> ``resample_v_u8``; the
rows then equal ``apply_spec_pil(load_image(data), spec, S)``.

With ``entropy="gpu"`` (``--jpeg_entropy gpu``, env ``KDL_JPEG_ENTROPY``; the default is ``host``)
the Huffman decode moves to the device too (csrc/kernels/jpeg_huff.hip). The host only walks the
markers, builds the code tables and removes the byte stuffing (``kdl._rt.jpeg_scan_prepare``); the
tables and scans -- about the size of the files -- are staged instead of the coefficients, and
``jpeg_huff_decode`` + ``jpeg_dc_scan`` fill the coefficient planes, which live in a device-only
buffer, in front of the unchanged ``jpeg_idct_u8``. Each image's error word returns with the
request's synchronise; if one is set the whole request is decoded again through the host path,
whose answer (success, or ``INVALID_ARGUMENT`` with its message) is the request's. A request that
holds a file with restart intervals takes the host path as a whole.

``entropy="gpu_rst"`` is ``gpu``, and files with restart intervals (a ``DRI`` segment: cameras,
phones, hardware encoders) are decoded on the device too. Every interval starts byte-aligned at a
known MCU with its DC predictors at zero, so ``jpeg_scan_prepare`` carries its unstuffing on through
the ``RSTm`` markers and adds a table of the intervals, and ``jpeg_huff_rst_decode`` +
``jpeg_dc_rst_scan`` give each group of intervals a workgroup of its own. In one request the plain
files go through ``jpeg_huff_decode`` and the restart files through ``jpeg_huff_rst_decode``. A file
whose markers are not exactly ``RST0, RST1, ...`` in order and in number (``restart_ok`` false)
sends the request to the host decoder, as a restart file does under ``gpu``.

Files the decoder does not cover (progressive or arithmetic JPEG, CMYK, PNG, ...) are decoded by
PIL on the host and resized by ``resize_nearest_u8`` into the same batch. Without a GPU the same
arithmetic runs on the CPU (``jpeg_pixels_cpu``) followed by the numpy gather.
"""
from __future__ import annotations

import concurrent.futures as cf
import io
import os
import time

import numpy as np
import torch
from PIL import Image

from ..gateway.preprocess import NEAREST_SPEC, ResizeSpec, apply_spec_pil, load_image
from ..ops import _lib
from . import protos as P
from .metrics import METRICS
from .resize import MAX_PIXELS, Resizer

BYTES_SIGNATURE = "serving_bytes"
BYTES_INPUT_KEY = "image_bytes"

THREADS = int(os.environ.get("KDL_JPEG_THREADS", "4"))
_POOL: cf.ThreadPoolExecutor | None = None


def _pool() -> cf.ThreadPoolExecutor:
    """Entropy-decode threads shared by all requests: the images of one request are spread over
    them. A request of one image, and every request when KDL_JPEG_THREADS <= 1, decodes on its own
    handler thread (the GIL is released either way, so handlers decode side by side)."""
    global _POOL
    if _POOL is None:
        _POOL = cf.ThreadPoolExecutor(max_workers=THREADS, thread_name_prefix="jpeg")
    return _POOL


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


def _intervals(data: bytes, header) -> int:
    """An upper bound of the restart intervals of a file, for ``jpeg_prepare_bound``: its MCUs over
    the smallest interval that anything in it that reads as a DRI segment defines (the probed header
    ends at the frame header, and encoders write DRI behind it). 0: no DRI segment."""
    ri, at = 0, data.find(b"\xff\xdd\x00\x04")
    while at >= 0:
        r = int.from_bytes(data[at + 4:at + 6], "big")
        ri = min(ri, r) if ri and r else ri or r
        at = data.find(b"\xff\xdd\x00\x04", at + 2)
    if not ri:
        return 0
    _, h, v, _, bw, bh = header.comps[0][:6]
    return -(-((bw // h) * (bh // v)) // ri)


def _bad(msg: str):
    from .backend import ServingError
    return ServingError("INVALID_ARGUMENT", msg)


class CallLayout:
    """Where one GPU decode call keeps its inputs in the staging buffer (pinned on the host, mirrored
    on the device): [descriptors | 4 quantisation tables per image | coefficient planes, each
    128-byte aligned]. ``ncoefs``: the coefficient count of every image that may join the call.

    The second form, for the device entropy decode (``prepared``: per image the bound of its prepared
    buffer, ``kdl._rt.jpeg_prepare_bound``): [descriptors | quantisation tables | one JpegHuffDesc per
    image | per image its Huffman tables and unstuffed scan]. The coefficient planes then are not
    staged: they live in a device buffer of ``ncoef`` int16 with the same ``coef_at`` offsets."""

    def __init__(self, ncoefs: list[int], prepared: list[int] | None = None):
        self.desc_bytes = _lib.rt().JPEG_DESC_BYTES
        n = len(ncoefs)
        self.off_qt = _align(n * self.desc_bytes, 256)
        self.off_coef = _align(self.off_qt + n * 512, 256)
        self.coef_at, self.ncoef = [], 0            # int16 units from the coefficient base
        for k in ncoefs:
            self.coef_at.append(self.ncoef)
            self.ncoef += _align(k, 64)
        self.nbytes = self.off_coef + 2 * self.ncoef
        self.n_desc = self.n_wg = 0
        self.device_entropy = prepared is not None
        if prepared is not None:
            self.huff_bytes = _lib.rt().JPEG_HUFF_DESC_BYTES
            # descriptors of plain files from the front, of restart files from the back: each
            # launcher gets a contiguous range
            self.off_huff, self.n_huff, self.n_rst, self.n_slots = self.off_coef, 0, 0, n
            self.prep_at, o = [], _align(self.off_huff + n * self.huff_bytes, 256)
            for b in prepared:
                self.prep_at.append(o)
                o += _align(b, 256)
            self.nbytes = o

    def prep(self, hin: np.ndarray, k: int) -> np.ndarray:
        """Slot ``k``'s room for its prepared tables and scan inside the staging array ``hin``."""
        end = self.prep_at[k + 1] if k + 1 < len(self.prep_at) else self.nbytes
        return hin[self.prep_at[k]:end]

    def add_huff(self, hin: np.ndarray, k: int, header, info) -> None:
        """Stage the entropy-decode descriptor of slot ``k``; call in the order of ``add``."""
        D = self.huff_bytes
        desc = _lib.rt().jpeg_huff_desc(header, info, self.prep_at[k], self.coef_at[k])
        if info.restart_ok:
            self.n_rst += 1
            j = self.n_slots - self.n_rst
        else:
            j = self.n_huff
            self.n_huff = j + 1
        assert self.n_huff + self.n_rst <= self.n_slots
        hin[self.off_huff + j * D:self.off_huff + (j + 1) * D] = np.frombuffer(desc, np.uint8)

    def huff_args(self, h_in: int, d_in: int, coef: int, status: int, status_cap: int) -> dict:
        """The argument dict of kdl._C.jpeg_huff_decode / jpeg_dc_scan (addresses as ints)."""
        return dict(desc=d_in + self.off_huff, h_desc=h_in + self.off_huff, stage=d_in, stage_cap=self.nbytes, coef=coef,
                    coef_cap=self.ncoef, status=status, status_cap=status_cap, n=self.n_huff)

    def huff_rst_args(self, h_in: int, d_in: int, coef: int, status: int, status_cap: int) -> dict:
        """The argument dict of kdl._C.jpeg_huff_rst_decode / jpeg_dc_rst_scan for the restart files of
        the call; ``status``: where their status words start (behind the plain files')."""
        at = self.off_huff + (self.n_slots - self.n_rst) * self.huff_bytes
        return dict(desc=d_in + at, h_desc=h_in + at, stage=d_in, h_stage=h_in, stage_cap=self.nbytes, coef=coef,
                    coef_cap=self.ncoef, status=status, status_cap=status_cap, n=self.n_rst)

    def coef(self, hin: np.ndarray, k: int, ncoef: int) -> np.ndarray:
        """The int16 coefficient buffer of slot ``k`` inside the uint8 staging array ``hin``."""
        o = self.off_coef + 2 * self.coef_at[k]
        return hin[o:o + 2 * ncoef].view(np.int16)

    def add(self, hin: np.ndarray, k: int, header, out_row: int, ys: torch.Tensor, xs: torch.Tensor) -> None:
        """Stage the descriptor and tables of the parsed image in slot ``k``; it goes to ``out_row``
        through the device tables ``ys`` / ``xs`` (PIL-NEAREST source rows / columns)."""
        j, D = self.n_desc, self.desc_bytes
        desc, self.n_wg = _lib.rt().jpeg_desc(header, self.coef_at[k], self.coef_at[k], j * 256, self.n_wg, out_row,
                                              _lib.ptr(ys), _lib.ptr(xs))
        hin[j * D:(j + 1) * D] = np.frombuffer(desc, np.uint8)
        hin[self.off_qt + j * 512: self.off_qt + (j + 1) * 512].view(np.uint16)[:] = header.qt.reshape(-1)
        self.n_desc = j + 1

    def args(self, h_in: int, d_in: int, planes: int, plane_cap: int, out: int, out_rows: int, OH: int, OW: int,
             coef: int | None = None) -> dict:
        """The argument dict of kdl._C.jpeg_idct_u8 / jpeg_sample_rgb_u8 (addresses as ints); ``coef``:
        the device coefficient buffer of the second form."""
        return dict(desc=d_in, h_desc=h_in, qt=d_in + self.off_qt, coef=d_in + self.off_coef if coef is None else coef,
                    planes=planes, out=out,
                    coef_cap=self.ncoef, plane_cap=plane_cap, qt_cap=self.n_desc * 256, n=self.n_desc, n_wg=self.n_wg,
                    out_rows=out_rows, OH=OH, OW=OW)


class BytesRunner:
    """The ``serving_bytes`` signature: decode + resize (GPU when the servable has one), then the
    ``serving_uint8`` runner's batcher and executors."""

    def __init__(self, sig, inner, devices: list[int], spec: ResizeSpec | None = None, entropy: str = "host"):
        if entropy not in ("host", "gpu", "gpu_rst"):
            raise ValueError(f"jpeg entropy decode {entropy!r}: expected 'host', 'gpu' or 'gpu_rst'")
        self.sig, self.inner = sig, inner
        self.entropy = entropy if devices else "host"       # CPU servers decode on the host
        self.source = inner.source
        self.S = inner.source.input_size
        self.spec = spec if spec is not None else getattr(inner.source, "preprocess", NEAREST_SPEC)
        # contexts, table cache, PIL-fallback resize
        self.resizer = Resizer(self.S, devices or None, spec=self.spec)
        self.gpu = bool(devices)
        self.device_path = self.gpu and inner.takes_device_items()

    # ------------------------------------------------------------------ per image
    def _probe(self, images) -> list:
        """[file bytes, JPEG header | None (= a file for PIL)] per image, after the request's pixel
        limit: nothing is allocated from a header before the sum of W x H has passed it."""
        rt = _lib.rt()
        plan, total = [], 0
        for i, data in enumerate(images):
            if not isinstance(data, (bytes, bytearray, memoryview)):
                raise _bad(f"image {i}: expected the bytes of an image file")
            data = bytes(data)
            st, hd = rt.jpeg_probe(data, 1 << 62)
            if st == rt.JPEG_MALFORMED:
                raise _bad(f"image {i}: malformed JPEG ({hd.why})")
            if st == rt.JPEG_OK:
                plan.append([data, hd])
                total += hd.W * hd.H
            else:
                try:
                    w, h = Image.open(io.BytesIO(data)).size      # lazy: the header only
                except Exception as e:  # noqa: BLE001 - PIL raises many types
                    raise _bad(f"image {i}: not a decodable image file ({hd.why}; PIL: {e})") from e
                plan.append([data, None])
                total += w * h
            if total > MAX_PIXELS:
                raise _bad(f"the images of the request exceed the {MAX_PIXELS}-pixel request limit")
        return plan

    @staticmethod
    def _pil(i: int, data: bytes) -> np.ndarray:
        try:
            px = np.array(load_image(data), dtype=np.uint8)      # a writable copy (torch.from_numpy)
        except Exception as e:  # noqa: BLE001
            raise _bad(f"image {i}: not a decodable image file (PIL: {e})") from e
        METRICS.inc("kdl_jpeg_decoded_total", path="pil")
        return px

    def _parse_all(self, plan, buffers, where: str = "host") -> None:
        """Entropy-decode every JPEG of ``plan`` into its int16 buffer; a file that turns out to be
        outside the decoder after its frame header (e.g. several scans) falls back to PIL."""
        rt = _lib.rt()
        jobs = [(i, p) for i, p in enumerate(plan) if p[1] is not None]
        if jobs:                    # counted as work done, whether or not a file then turns out malformed
            METRICS.inc("kdl_jpeg_entropy_total", len(jobs), where=where)
        t0 = time.perf_counter()

        def one(job):
            i, p = job
            return rt.jpeg_parse(p[0], buffers[i], MAX_PIXELS)
        results = [one(j) for j in jobs] if len(jobs) < 2 or THREADS <= 1 else list(_pool().map(one, jobs))
        for (i, p), (st, hd) in zip(jobs, results):
            if st == rt.JPEG_MALFORMED:
                raise _bad(f"image {i}: malformed JPEG ({hd.why})")
            p[1] = hd if st == rt.JPEG_OK else None
        if jobs:
            METRICS.observe("kdl_stage_ms", (time.perf_counter() - t0) * 1e3, stage="jpeg_entropy")

    def _prepare_all(self, plan, lay, hin, slot) -> dict | None:
        """Stage tables and scan of every JPEG of ``plan`` for the device decode -> {image: info}, or
        None when a file is not for the device (restart intervals under ``gpu``; under ``gpu_rst`` only
        those whose markers are out of order or number): the request then is the host decoder's. As in
        ``_parse_all`` a file outside the decoder falls back to PIL and a malformed header is rejected."""
        rt = _lib.rt()
        t0 = time.perf_counter()
        infos, ok = {}, True
        for i, k in slot.items():
            st, hd, info = rt.jpeg_scan_prepare(plan[i][0], lay.prep(hin, k), MAX_PIXELS)
            if st == rt.JPEG_MALFORMED and hd.why == "prepare buffer too small":
                ok = False                              # more intervals than its headers let expect
                continue
            if st == rt.JPEG_MALFORMED:
                raise _bad(f"image {i}: malformed JPEG ({hd.why})")
            if st != rt.JPEG_OK:
                plan[i][1] = None
                continue
            plan[i][1], infos[i] = hd, info
            ok = ok and (info.device_ok or (self.entropy == "gpu_rst" and info.restart_ok))
        METRICS.observe("kdl_stage_ms", (time.perf_counter() - t0) * 1e3, stage="jpeg_prepare")
        return infos if ok else None

    def _stage(self, c, plan, slot, extra: int, n_out: int, host: bool, where: str):
        """Lay out and fill the request's staging (``extra`` bytes of room behind it): the scans for
        the device decode when the runner has it and every file allows it, else the host-decoded
        coefficients -> (layout, {image: JpegHuffInfo} | None, offset of the extra room)."""
        ncoefs = [plan[i][1].ncoef for i in slot]
        c.n_status = 0
        if self.entropy != "host" and not host and slot:
            rt = _lib.rt()
            rst = self.entropy == "gpu_rst"
            lay = CallLayout(ncoefs, [rt.jpeg_prepare_bound(len(plan[i][0]), _intervals(*plan[i]) if rst else 0)
                                      for i in slot])
            off = _align(lay.nbytes, 256)
            c.grow(off + extra, n_out)
            infos = self._prepare_all(plan, lay, c.h_in.numpy(), slot)
            if infos is not None:
                c.grow_coef(max(lay.ncoef, 1), len(slot))
                return lay, infos, off
            for i in slot:                              # the host decoder starts from the probed headers
                plan[i][1] = rt.jpeg_probe(plan[i][0], 1 << 62)[1]
        lay = CallLayout(ncoefs)
        off = _align(lay.nbytes, 256)
        c.grow(max(off + extra, 1), n_out)
        hin = c.h_in.numpy()
        self._parse_all(plan, {i: lay.coef(hin, k, plan[i][1].ncoef) for i, k in slot.items()}, where)
        return lay, None, off

    def _entropy_on(self, c, lay, stream: int) -> int | None:
        """Launch the device entropy decode of a second-form layout (inside the stream context, after
        the staging copy) -> the coefficient buffer's address for ``CallLayout.args``."""
        n = lay.n_huff + lay.n_rst if lay.device_entropy else 0
        if not n:
            return None
        C = _lib.lib()
        if lay.n_huff:
            ha = lay.huff_args(_lib.ptr(c.h_in), _lib.ptr(c.d_in), _lib.ptr(c.d_coef), _lib.ptr(c.d_status), c.cap_status)
            C.jpeg_huff_decode(ha, stream)
            C.jpeg_dc_scan(ha, stream)
        if lay.n_rst:                                   # their status words follow the plain files'
            ha = lay.huff_rst_args(_lib.ptr(c.h_in), _lib.ptr(c.d_in), _lib.ptr(c.d_coef),
                                   _lib.ptr(c.d_status) + 8 * lay.n_huff, c.cap_status - 2 * lay.n_huff)
            C.jpeg_huff_rst_decode(ha, stream)
            C.jpeg_dc_rst_scan(ha, stream)
        c.n_status = n
        c.h_status[:2 * n].copy_(c.d_status[:2 * n], non_blocking=True)
        METRICS.inc("kdl_jpeg_entropy_total", n, where="gpu")
        return _lib.ptr(c.d_coef)

    @staticmethod
    def _rejected(c) -> bool:
        """After the stream's synchronise: did the device decoder set an image's error word?"""
        return bool(c.n_status) and bool(c.h_status[:2 * c.n_status:2].any())

    # ------------------------------------------------------------------ CPU
    def _decode_cpu(self, plan) -> np.ndarray:
        rt = _lib.rt()
        S = self.S
        bufs = {i: np.empty(p[1].ncoef, np.int16) for i, p in enumerate(plan) if p[1] is not None}
        self._parse_all(plan, bufs)
        out = np.empty((len(plan), S, S, 3), np.uint8)
        for i, (data, hd) in enumerate(plan):
            if hd is not None:
                px = rt.jpeg_pixels_cpu(hd, bufs[i])
                METRICS.inc("kdl_jpeg_decoded_total", path="cpu")
            else:
                px = self._pil(i, data)
            if self.resizer.filtered:               # Pillow itself: the definition of the filtered specs
                out[i] = apply_spec_pil(Image.fromarray(px), self.spec, S)
            else:
                ys, xs = self.resizer._tables(px.shape[0], px.shape[1], None)
                out[i] = px[ys][:, xs]
        METRICS.inc("kdl_resize_total", filter=self.spec.filter)
        return out

    # ------------------------------------------------------------------ GPU
    def _decode_on(self, c, plan, host: bool = False) -> int:
        """Decode + resize the request into ``c.d_out`` ([n, S, S, 3]) on the context's stream;
        returns the output's element count. The caller synchronises the stream and, under
        ``entropy="gpu"``, asks ``_rejected``: a set error word means this call again with ``host``
        (the retry through the host decoder) on a fresh plan."""
        C = _lib.lib()
        S, n = self.S, len(plan)
        slot = {i: k for k, i in enumerate(i for i, p in enumerate(plan) if p[1] is not None)}
        where = "retry" if host and self.entropy != "host" else "host"
        METRICS.inc("kdl_resize_total", filter=self.spec.filter)
        if self.resizer.filtered:
            return self._resample_on(c, plan, slot, host, where)
        n_out = n * S * S * 3
        lay, infos, _ = self._stage(c, plan, slot, 0, n_out, host, where)
        n_in = lay.nbytes
        c.grow_planes(max(lay.ncoef, 1))                # sample planes: one byte per coefficient
        hin = c.h_in.numpy()
        # every host step that can fail comes before the first launch: the stream never runs a
        # request that was rejected half way
        pil = {i: self._pil(i, p[0]) for i, p in enumerate(plan) if p[1] is None}
        keep = []                                   # tables / fallback pixels in use by the stream
        for i, k in slot.items():
            hd = plan[i][1]
            if hd is None:                          # fell back to PIL after its frame header
                continue
            ys, xs = self.resizer._tables(hd.H, hd.W, c.dev)
            keep += [ys, xs]
            lay.add(hin, k, hd, i, ys, xs)
            if infos is not None:
                lay.add_huff(hin, k, hd, infos[i])
        stream = int(c.stream.cuda_stream)
        with torch.cuda.device(c.dev), torch.cuda.stream(c.stream):
            if lay.n_desc:
                c.d_in[:n_in].copy_(c.h_in[:n_in], non_blocking=True)
                args = lay.args(_lib.ptr(c.h_in), _lib.ptr(c.d_in), _lib.ptr(c.d_planes), c.cap_planes,
                                _lib.ptr(c.d_out), n, S, S, coef=self._entropy_on(c, lay, stream))
                C.jpeg_idct_u8(args, stream)
                C.jpeg_sample_rgb_u8(args, stream)
                METRICS.inc("kdl_jpeg_decoded_total", lay.n_desc, path="gpu")
            for i, px in pil.items():               # what the decoder does not cover: PIL + the resize kernel
                ys, xs = self.resizer._tables(px.shape[0], px.shape[1], c.dev)
                src = torch.from_numpy(np.ascontiguousarray(px)).to(c.dev)
                keep += [ys, xs, src]
                C.resize_nearest_u8(dict(src=_lib.ptr(src), dst=_lib.ptr(c.d_out) + i * S * S * 3, ytab=_lib.ptr(ys),
                                         xtab=_lib.ptr(xs), SH=px.shape[0], SW=px.shape[1], OH=S, OW=S, n=1), stream)
        c.keep = keep
        return n_out

    def _resample_on(self, c, plan, slot, host: bool, where: str) -> int:
        """``_decode_on`` of a filtered spec: jpeg_idct_u8, then the horizontal pass straight from the
        sample planes (resample_h_u8, JPEG kind; raw kind for what PIL decoded), then one vertical pass
        over all images of the request. Staging: [the CallLayout | one ResampleDesc per image]."""
        C, D = _lib.lib(), _lib.rt().RESAMPLE_DESC_BYTES
        S, n = self.S, len(plan)
        n_out = n * S * S * 3
        lay, infos, off_desc = self._stage(c, plan, slot, n * D, n_out, host, where)
        n_in = off_desc + n * D
        c.grow_planes(max(lay.ncoef, 1))
        hin = c.h_in.numpy()
        # every host step that can fail comes before the first launch (see _decode_on)
        pil = {i: self._pil(i, p[0]) for i, p in enumerate(plan) if p[1] is None}
        keep, descs, raw, tmp = [], [], [], 0       # JPEG descriptors first, then the PIL-decoded images
        for i, k in slot.items():
            hd = plan[i][1]
            if hd is None:
                continue
            t = self.resizer._tables(hd.H, hd.W, c.dev)
            keep.append(t)
            descs.append(t.desc(lay.n_desc, tmp, i))
            lay.add(hin, k, hd, i, t.dev[2], t.dev[0])      # the nearest tables of the descriptor: unused here
            if infos is not None:
                lay.add_huff(hin, k, hd, infos[i])
            tmp += t.tmp_bytes
        for i, px in pil.items():
            t = self.resizer._tables(px.shape[0], px.shape[1], c.dev)
            src = torch.empty(px.shape, dtype=torch.uint8, device=c.dev)     # filled on the stream below
            keep += [t, src]
            raw.append((src, px))
            descs.append(t.desc(_lib.ptr(src), tmp, i))
            tmp += t.tmp_bytes
        c.grow_tmp(tmp)
        hin[off_desc:off_desc + n * D] = np.concatenate(descs)
        nj, stream = lay.n_desc, int(c.stream.cuda_stream)
        with torch.cuda.device(c.dev), torch.cuda.stream(c.stream):
            c.d_in[:n_in].copy_(c.h_in[:n_in], non_blocking=True)
            rs = dict(desc=_lib.ptr(c.d_in) + off_desc, h_desc=_lib.ptr(c.h_in) + off_desc, jdesc=_lib.ptr(c.d_in),
                      h_jdesc=_lib.ptr(c.h_in), n_jdesc=nj, planes=_lib.ptr(c.d_planes), plane_cap=c.cap_planes,
                      tmp=_lib.ptr(c.d_tmp), tmp_cap=c.cap_tmp, out=_lib.ptr(c.d_out), out_rows=n, OH=S, OW=S, n=n)
            if nj:
                C.jpeg_idct_u8(lay.args(_lib.ptr(c.h_in), _lib.ptr(c.d_in), _lib.ptr(c.d_planes), c.cap_planes,
                                        _lib.ptr(c.d_out), n, S, S, coef=self._entropy_on(c, lay, stream)), stream)
                C.resample_h_u8({**rs, "n": nj}, 1, stream)
                METRICS.inc("kdl_jpeg_decoded_total", nj, path="gpu")
            if n > nj:
                for src, px in raw:
                    src.copy_(torch.from_numpy(np.ascontiguousarray(px)))
                C.resample_h_u8({**rs, "desc": rs["desc"] + nj * D, "h_desc": rs["h_desc"] + nj * D, "n": n - nj},
                                0, stream)
            C.resample_v_u8(rs, stream)
        c.keep = keep
        return n_out

    def decode(self, images) -> np.ndarray:
        """[n, S, S, 3] uint8 model inputs of the encoded ``images`` (host array)."""
        plan = self._probe(images)
        if not self.gpu:
            return self._decode_cpu(plan)
        c = self.resizer._free.get()
        try:
            n_out = self._decode_on(c, plan)
            with torch.cuda.device(c.dev), torch.cuda.stream(c.stream):
                c.h_out[:n_out].copy_(c.d_out[:n_out], non_blocking=True)
            c.stream.synchronize()
            if self._rejected(c):           # the device decoder refused a scan: the host decoder's answer counts
                n_out = self._decode_on(c, self._probe(images), host=True)
                with torch.cuda.device(c.dev), torch.cuda.stream(c.stream):
                    c.h_out[:n_out].copy_(c.d_out[:n_out], non_blocking=True)
                c.stream.synchronize()
            return c.h_out[:n_out].numpy().reshape(len(plan), self.S, self.S, 3).copy()
        finally:
            self._release(c)

    # ------------------------------------------------------------------ runner interface
    def predict(self, images, n: int, deadline_us: int) -> np.ndarray:
        if len(images) != n or n < 1:
            raise _bad(f"expected {n} encoded images, got {len(images)}")
        if not self.device_path:
            return self.inner.predict(self.decode(images), n, deadline_us)
        plan = self._probe(images)
        c = self.resizer._free.get()
        try:                           # decoded straight into device memory: no host round trip
            self._decode_on(c, plan)
            c.stream.synchronize()
            if self._rejected(c):
                self._decode_on(c, self._probe(images), host=True)
                c.stream.synchronize()
            return self.inner.predict_device(_lib.ptr(c.d_out), n, deadline_us)
        finally:
            self._release(c)

    def _release(self, c) -> None:
        """Hand the context back idle: the next request rewrites its pinned staging, which an
        unfinished host-to-device copy of this one must not still be reading."""
        try:
            c.stream.synchronize()
        finally:
            c.keep = None
            self.resizer._free.put(c)

    def healthy(self) -> bool:
        return self.inner.healthy()

    def close(self) -> None:       # the inner runner belongs to the servable
        pass


def bytes_signature(output_key: str, classes: int):
    from .backend import SignatureInfo
    return SignatureInfo(BYTES_SIGNATURE, BYTES_INPUT_KEY, P.DT_STRING, output_key, input_shape=(-1,),
                         output_shape=(-1, classes))
