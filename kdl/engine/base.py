"""Model-agnostic MI355X executor machinery shared by every model family.

A model engine lowers its network into a list of ``Step`` s (fused HIP launches
over statically planned NHWC bf16 buffers). This base class owns what does not
depend on the network: one native ``Program`` per (batch bucket, capture) with
a hipGraph per bucket, per-op profiling, per-layer tile autotuning over the
conv-GEMM config table, and the tuning-table round trip
(``kdl/tuning/<model>_b<batch>.json``). The reference equivalent is a
TF-Serving servable's session run (`tf-serving.dockerfile:2-5`).
"""
from __future__ import annotations

import contextlib
import json
from dataclasses import dataclass, field
from pathlib import Path

import torch

from ..ops import _lib
from ..ops.conv import MODE_DW, STREAM_IDS, ConvGemmLayer, is_splitk, splitk_parts


@dataclass
class Step:
    kind: str                  # conv | stem | pool | head | gap | fc | ...
    name: str
    layer: object = None
    src: str = ""
    dst: str = ""
    res: str | None = None
    geom: tuple = ()           # (H, W, OH, OW) per image
    extra: dict = field(default_factory=dict)


def unpack_topk(rows) -> tuple:
    """Packed top-k rows [n, 2K] (a torch tensor or numpy array of 32-bit words) ->
    (classes int32 [n, K], scores fp32 [n, K]) as numpy arrays."""
    import numpy as np
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    a = np.ascontiguousarray(a)
    k = a.shape[-1] // 2
    return a[..., :k].view(np.int32).copy(), a[..., k:].view(np.float32).copy()


def unpack_explain(rows, h: int, w: int) -> tuple:
    """Packed explain rows [n, 2 + h*w] (a torch tensor or numpy array of 32-bit words) ->
    (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w]) as numpy arrays."""
    import numpy as np
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    a = np.ascontiguousarray(a)
    assert a.shape[-1] == 2 + h * w, (a.shape, h, w)
    return (a[..., 0].view(np.int32).copy(), a[..., 1].view(np.float32).copy(),
            a[..., 2:].view(np.float32).reshape(*a.shape[:-1], h, w).copy())


def pack_explain(classes, scores, heat):
    """The inverse of ``unpack_explain``: numpy rows [n, 2 + h*w] of fp32 words."""
    import numpy as np
    heat = np.asarray(heat, dtype=np.float32)
    n = heat.shape[0]
    rows = np.empty((n, 2 + heat[0].size), dtype=np.float32)
    rows[:, 0] = np.asarray(classes, dtype=np.int32).reshape(n).view(np.float32)
    rows[:, 1] = np.asarray(scores, dtype=np.float32).reshape(n)
    rows[:, 2:] = heat.reshape(n, -1)
    return rows


def overlay_words(S: int) -> int:
    """32-bit words that hold the S x S x 3 picture bytes of an overlay row."""
    return (S * S * 3 + 3) // 4


def unpack_overlay(rows, h: int, w: int, S: int) -> tuple:
    """Packed overlay rows [n, 2 + h*w + ceil(S*S*3/4)] (a torch tensor or numpy array of 32-bit words)
    -> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], pictures uint8 [n, S, S, 3])."""
    import numpy as np
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    a = np.ascontiguousarray(a)
    assert a.ndim == 2 and a.shape[1] == 2 + h * w + overlay_words(S), (a.shape, h, w, S)
    pics = np.ascontiguousarray(a[:, 2 + h * w:]).view(np.uint8)[:, :S * S * 3].reshape(-1, S, S, 3).copy()
    return unpack_explain(a[:, :2 + h * w], h, w) + (pics,)


def pack_overlay(classes, scores, heat, pictures):
    """The inverse of ``unpack_overlay``: numpy rows of fp32 words (the pad bytes of the last word 0).
    The picture bytes are copied as bytes, never through a float."""
    import numpy as np
    pics = np.ascontiguousarray(pictures, dtype=np.uint8)
    n, S = pics.shape[0], pics.shape[1]
    front = pack_explain(classes, scores, heat)
    rows = np.zeros((n, front.shape[1] + overlay_words(S)), dtype=np.float32)
    rows[:, :front.shape[1]] = front
    rows.view(np.uint8)[:, 4 * front.shape[1]:4 * front.shape[1] + S * S * 3] = pics.reshape(n, -1)
    return rows


def overlay_jpeg_cap(S: int, max_bytes: int | None = None) -> int:
    """Bytes an overlay_jpeg row keeps for the file of an S x S picture: ``max_bytes``, or ceil(S*S*3/2)."""
    return int(max_bytes) if max_bytes is not None else (S * S * 3 + 1) // 2


def unpack_overlay_jpeg(rows, h: int, w: int, max_bytes: int) -> tuple:
    """Packed overlay_jpeg rows [n, 2 + h*w + 1 + ceil(max_bytes/4)] (a torch tensor or numpy array of 32-bit
    words) -> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], files: a list of n bytes objects, a
    row's length word of them; b"" for a file that did not fit)."""
    import numpy as np
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    a = np.ascontiguousarray(a)
    front = 2 + h * w
    assert a.ndim == 2 and a.shape[1] == front + 1 + (max_bytes + 3) // 4, (a.shape, h, w, max_bytes)
    lens = np.ascontiguousarray(a[:, front]).view(np.int32)
    body = np.ascontiguousarray(a[:, front + 1:]).view(np.uint8).reshape(a.shape[0], -1)
    assert ((0 <= lens) & (lens <= max_bytes)).all(), lens
    return unpack_explain(a[:, :front], h, w) + ([body[i, :n].tobytes() for i, n in enumerate(lens)],)


def pack_overlay_jpeg(classes, scores, heat, files, max_bytes: int):
    """The inverse of ``unpack_overlay_jpeg``: numpy rows of fp32 words, the bytes behind a file 0. A file
    longer than ``max_bytes`` is an overflow row: length 0 and no bytes."""
    import numpy as np
    front = pack_explain(classes, scores, heat)
    n, f = front.shape
    rows = np.zeros((n, f + 1 + (max_bytes + 3) // 4), dtype=np.float32)
    rows[:, :f] = front
    by = rows.view(np.uint8)
    for i, data in enumerate(files):
        if len(data) > max_bytes:
            continue
        rows.view(np.int32)[i, f] = len(data)
        by[i, 4 * (f + 1):4 * (f + 1) + len(data)] = np.frombuffer(bytes(data), np.uint8)
    return rows


def unpack_palette(rows, h: int, w: int, K: int) -> tuple:
    """Packed palette rows [n, 2 + h*w + 1 + 2K] (a torch tensor or numpy array of 32-bit words) ->
    (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], W uint32 [n], colours uint8 [n, K, 3],
    weights uint32 [n, K])."""
    import numpy as np
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    a = np.ascontiguousarray(a)
    front = 2 + h * w
    assert a.ndim == 2 and a.shape[1] == front + 1 + 2 * K, (a.shape, h, w, K)
    tail = np.ascontiguousarray(a[:, front:]).view(np.uint32)
    packed = tail[:, 1::2]
    cols = np.stack([packed & 255, (packed >> 8) & 255, (packed >> 16) & 255], axis=-1).astype(np.uint8)
    return unpack_explain(a[:, :front], h, w) + (tail[:, 0].copy(), cols, tail[:, 2::2].copy())


def pack_palette(classes, scores, heat, totals, colours, weights):
    """The inverse of ``unpack_palette``: numpy rows of fp32 words; the integers are copied as bits, never
    through a float."""
    import numpy as np
    front = pack_explain(classes, scores, heat)
    n, f = front.shape
    c = np.asarray(colours, dtype=np.uint32).reshape(n, -1, 3)
    K = c.shape[1]
    rows = np.zeros((n, f + 1 + 2 * K), dtype=np.float32)
    rows[:, :f] = front
    tail = rows.view(np.uint32)[:, f:]
    tail[:, 0] = np.asarray(totals, dtype=np.uint32).reshape(n)
    tail[:, 1::2] = c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)
    tail[:, 2::2] = np.asarray(weights, dtype=np.uint32).reshape(n, K)
    return rows


def unpack_locate(rows, h: int, w: int, K: int) -> tuple:
    """Packed locate rows [n, 2 + h*w + 1 + 3K] (a torch tensor or numpy array of 32-bit words) ->
    (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], counts uint32 [n], boxes int32 [n, K, 4] as
    (y0, x0, y1, x1), areas uint32 [n, K])."""
    import numpy as np
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    a = np.ascontiguousarray(a)
    front = 2 + h * w
    assert a.ndim == 2 and a.shape[1] == front + 1 + 3 * K, (a.shape, h, w, K)
    tail = np.ascontiguousarray(a[:, front:]).view(np.uint32)
    lo, hi = tail[:, 1::3], tail[:, 2::3]
    boxes = np.stack([lo & 0xFFFF, lo >> 16, hi & 0xFFFF, hi >> 16], axis=-1).astype(np.int32)
    return unpack_explain(a[:, :front], h, w) + (tail[:, 0].copy(), boxes, tail[:, 3::3].copy())


def pack_locate(classes, scores, heat, counts, boxes, areas):
    """The inverse of ``unpack_locate``: numpy rows of fp32 words; the integers are copied as bits, never
    through a float."""
    import numpy as np
    front = pack_explain(classes, scores, heat)
    n, f = front.shape
    bx = np.asarray(boxes, dtype=np.uint32).reshape(n, -1, 4)
    K = bx.shape[1]
    rows = np.zeros((n, f + 1 + 3 * K), dtype=np.float32)
    rows[:, :f] = front
    tail = rows.view(np.uint32)[:, f:]
    tail[:, 0] = np.asarray(counts, dtype=np.uint32).reshape(n)
    tail[:, 1::3] = bx[..., 0] | (bx[..., 1] << 16)
    tail[:, 2::3] = bx[..., 2] | (bx[..., 3] << 16)
    tail[:, 3::3] = np.asarray(areas, dtype=np.uint32).reshape(n, K)
    return rows


def unpack_cutout(rows, h: int, w: int, S: int) -> tuple:
    """Packed cutout rows [n, 2 + h*w + 1 + S*S] (a torch tensor or numpy array of 32-bit words) ->
    (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], counts uint32 [n], rgba uint8 [n, S, S, 4])."""
    import numpy as np
    a = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    a = np.ascontiguousarray(a)
    front = 2 + h * w
    assert a.ndim == 2 and a.shape[1] == front + 1 + S * S, (a.shape, h, w, S)
    tail = np.ascontiguousarray(a[:, front:]).view(np.uint32)
    pics = np.ascontiguousarray(tail[:, 1:]).view(np.uint8).reshape(-1, S, S, 4).copy()   # r | g << 8 | b << 16 | a << 24
    return unpack_explain(a[:, :front], h, w) + (tail[:, 0].copy(), pics)


def pack_cutout(classes, scores, heat, counts, pictures):
    """The inverse of ``unpack_cutout``: numpy rows of fp32 words; the pixel bytes and the count are copied as
    bits, never through a float."""
    import numpy as np
    pics = np.ascontiguousarray(pictures, dtype=np.uint8)
    n, S = pics.shape[0], pics.shape[1]
    assert pics.shape == (n, S, S, 4), pics.shape
    front = pack_explain(classes, scores, heat)
    f = front.shape[1]
    rows = np.zeros((n, f + 1 + S * S), dtype=np.float32)
    rows[:, :f] = front
    rows.view(np.uint32)[:, f] = np.asarray(counts, dtype=np.uint32).reshape(n)
    rows.view(np.uint8)[:, 4 * (f + 1):] = pics.reshape(n, -1)
    return rows


EMBED_MODES = ("", "raw", "l2")
SIMILAR_METRICS = ("cosine", "dot")


@dataclass
class Similar:
    """Gallery search outputs of an engine (``EngineBase(similar=...)``). ``gallery`` is the device
    tensor [N, ldg] of stored bf16 rows (``kdl.serving.similar.load_gallery``'s values), ldg a
    multiple of 8 and at least the family's F. It is shared: every engine on that device built
    from this object reads the same copy. ``k`` neighbours per image (clipped to N); ``metric``
    "cosine" normalises the query rows (the stored rows are already unit length), "dot" does not."""
    gallery: torch.Tensor
    k: int = 5
    metric: str = "cosine"


@dataclass(frozen=True)
class Overlay:
    """Rendered overlay outputs of an ``explain`` / ``rollout`` engine (``EngineBase(overlay=...)``): the
    heatmap upsampled to the input size with ``filter`` ("bilinear" | "bicubic", Pillow's), coloured
    through ``colormap`` ("jet" | "hot" | "gray") and blended onto the input picture with ``alpha``
    (0..1), ``blend`` "flat" or weighted by the "heat". kdl/serving/overlay.py defines the rule."""
    colormap: str = "jet"
    alpha: float = 0.5
    blend: str = "heat"
    filter: str = "bilinear"


@dataclass(frozen=True)
class OverlayJpeg:
    """The rendered overlay as a baseline JPEG file (``EngineBase(overlay=..., overlay_jpeg=...)``):
    ``quality`` 1..100, ``subsampling`` "4:4:4" | "4:2:0", at most ``max_bytes`` per file (None =
    ceil(S*S*3/2)). kdl/serving/jpeg_encode.py defines the rule."""
    quality: int = 85
    subsampling: str = "4:2:0"
    max_bytes: int | None = None


@dataclass(frozen=True)
class Palette:
    """Dominant-colour outputs of an ``explain`` / ``rollout`` engine (``EngineBase(palette=...)``): the
    ``colors`` (1..8) dominant colours of the input picture after ``rounds`` (1..16) clustering rounds over
    its 4096-bin histogram, every pixel weighted by the heatmap upsampled with ``filter`` ("bilinear" |
    "bicubic", Pillow's) when ``weight`` is "map", or all alike when it is "uniform".
    kdl/serving/palette.py defines the rule."""
    colors: int = 5
    weight: str = "map"
    filter: str = "bilinear"
    rounds: int = 8


@dataclass(frozen=True)
class Locate:
    """Garment-box outputs of an ``explain`` / ``rollout`` engine (``EngineBase(locate=...)``): the ``boxes``
    (1..8) largest 8-connected regions of the heatmap upsampled with ``filter`` ("bilinear" | "bicubic",
    Pillow's) and cut at ``threshold`` (1..255 of the quantised map; 51 is 20 % of the peak).
    kdl/serving/locate.py defines the rule."""
    boxes: int = 3
    threshold: int = 51
    filter: str = "bilinear"


@dataclass(frozen=True)
class Cutout:
    """Garment-cutout outputs of an ``explain`` / ``rollout`` engine (``EngineBase(cutout=...)``): the input
    picture with an alpha channel. The heatmap, upsampled with ``filter`` ("bilinear" | "bicubic", Pillow's),
    seeds a two-histogram colour model over the picture's 4096 colour bins that is re-estimated ``rounds``
    (0..8) times; a pixel below ``gate`` (1..255 of the upsampled map) is never garment; the mask takes
    ``smooth`` (0..4) 3 x 3 majority rounds and, with ``feather``, its alpha is the 3 x 3 mean of the mask.
    kdl/serving/cutout.py defines the rule."""
    gate: int = 26
    rounds: int = 2
    smooth: int = 1
    feather: bool = True
    filter: str = "bilinear"


class EngineBase:
    model_name = "model"
    # tail step kind -> the method that emits it; every other kind is the family's (_emit)
    TAIL_EMITTERS = {"topk": "_emit_topk", "similar": "_emit_similar", "top1": "_emit_top1",
                     "explain": "_emit_explain", "overlay": "_emit_overlay", "overlay_jpeg": "_emit_overlay_jpeg",
                     "palette": "_emit_palette", "locate": "_emit_locate", "cutout": "_emit_cutout"}

    def __init__(self, device, max_batch: int, buckets=None, topk: int = 0, embed: str = "", similar=None,
                 explain: bool = False, rollout: bool = False, overlay: Overlay | None = None,
                 overlay_jpeg: OverlayJpeg | None = None, palette: Palette | None = None,
                 locate: Locate | None = None, cutout: Cutout | None = None):
        if cutout is not None:       # before anything touches the device
            if not (explain or rollout):
                raise ValueError("cutout seeds its colour model with a heatmap: it needs explain=True or rollout=True")
            if overlay is not None or palette is not None or locate is not None:
                raise ValueError("cutout, locate, palette and overlay each extend the heatmap rows: set one of them")
            from ..serving.cutout import check as check_cutout
            check_cutout(cutout)
        if locate is not None:       # before anything touches the device
            if not (explain or rollout):
                raise ValueError("locate cuts boxes out of a heatmap: it needs explain=True or rollout=True")
            if overlay is not None or palette is not None:
                raise ValueError("locate, palette and overlay each extend the heatmap rows: set one of them")
            from ..serving.locate import check as check_locate
            check_locate(locate)
        if palette is not None:      # before anything touches the device
            if not (explain or rollout):
                raise ValueError("palette weighs the picture by a heatmap: it needs explain=True or rollout=True")
            if overlay is not None:
                raise ValueError("palette and overlay both extend the heatmap rows: set one of them")
            from ..serving.palette import check as check_palette
            check_palette(palette)
        if overlay_jpeg is not None:
            if overlay is None:
                raise ValueError("overlay_jpeg encodes the rendered overlay: it needs overlay=Overlay(...)")
            from ..serving.jpeg_encode import check as check_jpeg
            check_jpeg(overlay_jpeg)
        if overlay is not None:      # before anything touches the device
            if not (explain or rollout):
                raise ValueError("overlay paints a heatmap: it needs explain=True or rollout=True")
            from ..serving.overlay import check
            check(overlay)
        if sum(map(bool, (topk, embed, similar is not None, explain, rollout))) > 1:
            raise ValueError("rollout, explain, similar, embed and topk all replace the output rows: set one of them")
        self.device = torch.device(device)
        self.max_batch = max_batch
        self.buckets = sorted(set(buckets or [max_batch]))
        assert self.buckets[-1] <= max_batch
        self.steps: list[Step] = []
        self.programs: dict[tuple[int, bool, int], object] = {}
        self.stream = torch.cuda.Stream(device=self.device)
        self.inputs: list[torch.Tensor] = []   # input slots (self.inp is slot 0)
        self.outputs: list[torch.Tensor] = []  # per-slot logits (self.logits is slot 0)
        self._slot = 0
        self._remap: dict[str, str] = {}      # buffer-name overrides while emitting (stages.py)
        # classification outputs: 0 = the output is the fp32 logits; K = one more step packs the
        # top-K classes and softmax scores of the logits into the output rows (_enable_topk)
        if topk < 0:
            raise ValueError(f"topk must be >= 0, got {topk}")
        self.topk = int(topk)
        self.logit_slots: list[torch.Tensor] = []   # topk / embed only: per-slot fp32 logits the head writes
        # embedding outputs: "" = the output is the fp32 logits; "raw" / "l2" = one more step writes
        # the pooled features in front of the head into the output rows (_enable_embed)
        if embed not in EMBED_MODES:
            raise ValueError(f"embed must be one of {EMBED_MODES}, got {embed!r}")
        self.embed = embed
        self._embed_step: Step | None = None
        # gallery search outputs: None = the output is the fp32 logits; a ``Similar`` = two more
        # steps write the K nearest gallery rows of each image's features (_enable_similar)
        self.similar: Similar | None = similar
        self.feature_slots: list[torch.Tensor] = []   # similar only: per-slot fp32 features [max_batch, F]
        self._similar_work: list[torch.Tensor] = []   # similar only: per-slot gallery_topk workspace
        # Grad-CAM outputs: False = the output is the fp32 logits; True = two more steps write the
        # predicted class, its score and the class's heatmap over the last feature map (_enable_explain)
        self.explain = bool(explain)
        self.top1_slots: list[torch.Tensor] = []      # explain only: per-slot [max_batch, 2] class and score
        self._cam_alpha: list[torch.Tensor] = []      # explain only: per-slot class_map workspace [max_batch, F]
        # attention-rollout outputs (ViT): False = the output is the fp32 logits; True = one more step
        # beside every layer's attention, then "top1" and "rollout_map" behind the head write the
        # predicted class, its score and the rollout heatmap, explain's row layout (ViTEngine._enable_heatmap)
        self.rollout = bool(rollout)
        # rendered overlays: None = the rows end with the map; an ``Overlay`` = the rows also carry the
        # S x S x 3 picture bytes, written by one more step behind the map's (_enable_overlay)
        self.overlay: Overlay | None = overlay
        self._overlay_tabs: dict = {}                 # overlay only: device tables and their host copies
        # overlays as JPEG files: None = the rows carry the picture bytes; an ``OverlayJpeg`` = the steps
        # above write those raw rows into a device-only buffer, and one more step writes narrow output rows:
        # the raw row's front words, a length word and the encoded file (_enable_overlay_jpeg)
        self.overlay_jpeg: OverlayJpeg | None = overlay_jpeg
        self._jpeg: dict = {}                         # overlay_jpeg only: header, cap, per-slot raw rows and workspaces
        # dominant colours: None = the rows end with the map; a ``Palette`` = the rows also carry W and K x
        # (colour, weight), written by one more step behind the map's (_enable_palette)
        self.palette: Palette | None = palette
        self._palette_tabs: dict = {}                 # palette only: device tables, their host copies, per-slot histograms
        # garment boxes: None = the rows end with the map; a ``Locate`` = the rows also carry the region count
        # and K x (corner, corner, area), written by one more step behind the map's (_enable_locate)
        self.locate: Locate | None = locate
        self._locate_tabs: dict = {}                  # locate only: device tables, their host copies, per-slot workspaces
        # garment cutouts: None = the rows end with the map; a ``Cutout`` = the rows also carry the garment's
        # pixel count and the S x S RGBA words, written by one more step behind the map's (_enable_cutout)
        self.cutout: Cutout | None = cutout
        self._cutout_tabs: dict = {}                  # cutout only: device tables, their host copies, per-slot workspaces

    # ---------------------------------------------------------------- input slots
    def input_ptr(self) -> int:
        """Device pointer of the input slot the program being built reads."""
        return _lib.ptr(self.inputs[self._slot] if self.inputs else self.inp)

    def _rows_replaced(self) -> bool:
        """The head writes per-slot logits, not the output rows: a tail step writes those."""
        return bool(self.topk or self.embed or self.similar or self.explain or self.rollout)

    def _out_rows(self) -> torch.Tensor:
        """The rows the tail steps of the program being built write: the slot's output rows, or with
        ``overlay_jpeg`` the slot's raw overlay rows, which never leave the device."""
        if self._jpeg:
            return self._jpeg_slot(self._slot)[0]
        return self.outputs[self._slot] if self.outputs else self.logits

    def output_ptr(self) -> int:
        """Device pointer of the logits buffer the program being built writes."""
        return _lib.ptr(self._logit_slot(self._slot) if self._rows_replaced() else self._out_rows())

    def slot_logits(self, slot: int) -> torch.Tensor:
        """Output buffer of a slot: fp32 logits, the packed top-k rows of a ``topk`` engine, the
        feature rows of an ``embed`` engine, the packed neighbour rows of a ``similar`` engine, or the
        packed heatmap rows of an ``explain`` or ``rollout`` engine."""
        return self.outputs[slot] if self.outputs else self.logits

    # ---------------------------------------------------------------- output tails
    def _enable_outputs(self) -> None:
        """Called once by a family's constructor when ``self.logits`` [max_batch, classes] exists:
        appends the tail steps of the one row-replacing mode that is set, and behind a heatmap the
        overlay step."""
        self._enable_topk()
        self._enable_embed()
        self._enable_similar()
        hw = self._enable_heatmap()
        if hw:
            self._enable_overlay(*hw)
            self._enable_overlay_jpeg(*hw)
            self._enable_palette(*hw)
            self._enable_locate(*hw)
            self._enable_cutout(*hw)

    def _enable_heatmap(self) -> tuple:
        """The family's heatmap tail: (h, w) of the map it appended, () without one. Grad-CAM here;
        ViT overrides it with attention rollout."""
        if not self.explain:
            return ()
        self._enable_explain()
        return self.cam_source()[1:3]

    # ---------------------------------------------------------------- classification outputs
    def _enable_topk(self) -> None:
        """Called by ``_enable_outputs``. With
        ``topk = K`` (clipped to the class count) the head keeps writing that buffer, a last
        step of kind "topk" (kernels/classify.hip) reads it, and ``self.logits`` -- the output
        the executor copies to the host and ``forward`` returns -- becomes [max_batch, 2K]
        32-bit words per row: K int32 class indices, then K fp32 scores (``unpack_topk``)."""
        if not self.topk:
            return
        assert not self.inputs, "topk is set at construction, before input slots exist"
        classes = self.logits.shape[1]
        if classes > _lib.lib().TOPK_MAX_NC:
            raise ValueError(f"topk: {classes} classes exceed the kernel's {_lib.lib().TOPK_MAX_NC}")
        self.topk = min(self.topk, classes)
        if self.topk > _lib.lib().TOPK_MAX_K:
            raise ValueError(f"topk must be <= {_lib.lib().TOPK_MAX_K}, got {self.topk}")
        self.logit_slots = [self.logits]
        self.logits = torch.zeros((self.max_batch, 2 * self.topk), dtype=torch.float32, device=self.device)
        self.steps.append(Step("topk", "topk", src="logits"))

    def _logit_slot(self, slot: int) -> torch.Tensor:
        while len(self.logit_slots) <= slot:      # one per input slot, whoever added the slots
            self.logit_slots.append(torch.zeros_like(self.logit_slots[0]))
        return self.logit_slots[slot]

    def _emit_topk(self, prog, step: Step, b: int) -> None:
        lg, out = self._logit_slot(self._slot), self._out_rows()
        prog.add_softmax_topk(step.name, dict(x=_lib.ptr(lg), out=_lib.ptr(out), B=b, NC=lg.shape[1],
                                              K=self.topk, ldx=lg.shape[1]))

    def last_logits(self, slot: int = 0) -> torch.Tensor:
        """fp32 logits [max_batch, classes] of the last forward in ``slot``, with or without
        ``topk`` / ``embed`` / ``similar`` / ``explain`` / ``rollout``."""
        return self._logit_slot(slot) if self._rows_replaced() else self.slot_logits(slot)

    # ---------------------------------------------------------------- embedding outputs
    def embed_source(self) -> tuple:
        """A family's pooled-feature source: (buffer name, HW, row stride in elements, F, element
        type: 0 bf16 / 1 fp16). The embedding of an image is the mean over the buffer's HW pixels
        of its first F channels: what the head pools before its dense layers."""
        raise NotImplementedError

    @property
    def embed_dim(self) -> int:
        """F: floats per embedding row (whether or not this engine was built with ``embed``)."""
        return self.embed_source()[3]

    def _enable_embed(self) -> None:
        """Called by ``_enable_outputs``. With ``embed`` "raw" or "l2"
        the head keeps writing the per-slot logits, a last step of kind "embed" (kernels/embed.hip)
        pools ``embed_source()`` and ``self.logits`` -- the output the executor copies to the host
        and ``forward`` returns -- becomes [max_batch, F] fp32: the mean over the pixels, for "l2"
        divided by max(its L2 norm, 1e-12). The step is named "embed_rows" (ViT's token
        embedding is the step "embed") and names its source in ``src``, so the stage pipeline's
        buffer renaming reaches it through ``_ptr``."""
        if not self.embed:
            return
        assert not self.inputs, "embed is set at construction, before input slots exist"
        src, _, _, F, _ = self.embed_source()
        if F % 8 or F > _lib.lib().EMBED_MAX_F:
            raise ValueError(f"embed: {F} features; the kernel takes a multiple of 8 up to {_lib.lib().EMBED_MAX_F}")
        self.logit_slots = [self.logits]
        self.logits = torch.zeros((self.max_batch, F), dtype=torch.float32, device=self.device)
        self._embed_step = Step("embed", "embed_rows", src=src)
        self.steps.append(self._embed_step)

    def _emit_embed(self, prog, step: Step, b: int) -> None:
        _, hw, ldx, F, dt = self.embed_source()
        if self.similar is not None:       # the query rows of the "similar" step
            out, norm = self.feature_slot(self._slot), int(self.similar.metric == "cosine")
        else:
            out, norm = self._out_rows(), int(self.embed == "l2")
        prog.add_embed_rows(step.name, dict(x=self._ptr(step.src), out=_lib.ptr(out), B=b, HW=hw, F=F, ldx=ldx,
                                            ldo=out.shape[1], dt=dt, norm=norm))

    # ---------------------------------------------------------------- gallery search outputs
    def _enable_similar(self) -> None:
        """Called by ``_enable_outputs``. With ``similar`` the head keeps
        writing the per-slot logits, a step "embed_rows" pools ``embed_source()`` into a per-slot
        fp32 feature buffer [max_batch, F] (L2-normalised for "cosine"), and a last step of kind
        "similar" (kernels/similar.hip) scores those rows against the gallery. ``self.logits`` --
        the output the executor copies to the host and ``forward`` returns -- becomes
        [max_batch, 2K] 32-bit words per row: K int32 gallery row indices, then K fp32 scores
        (``unpack_topk``). Feature buffers and workspaces are per slot, like the logits."""
        sim = self.similar
        if sim is None:
            return
        assert not self.inputs, "similar is set at construction, before input slots exist"
        lib = _lib.lib()
        src, _, _, F, _ = self.embed_source()
        g = sim.gallery
        if sim.metric not in SIMILAR_METRICS:
            raise ValueError(f"similar: metric must be one of {SIMILAR_METRICS}, got {sim.metric!r}")
        if F % 8 or F > lib.EMBED_MAX_F:
            raise ValueError(f"similar: {F} features; the kernel takes a multiple of 8 up to {lib.EMBED_MAX_F}")
        if (g.dim() != 2 or g.dtype != torch.bfloat16 or not self._on_device(g) or not g.is_contiguous()
                or g.shape[1] < F or g.shape[1] % 8 or not 1 <= g.shape[0] <= lib.GALLERY_MAX_N):
            raise ValueError(f"similar: the gallery must be a contiguous bf16 [N, >= {F}] tensor on {self.device} "
                             f"with 1 <= N <= {lib.GALLERY_MAX_N} and a row stride that is a multiple of 8, got "
                             f"{tuple(g.shape)} {g.dtype} on {g.device}")
        if sim.k < 1:
            raise ValueError(f"similar: k must be >= 1, got {sim.k}")
        self.similar_k = min(int(sim.k), g.shape[0])
        if self.similar_k > lib.TOPK_MAX_K:
            raise ValueError(f"similar: k must be <= {lib.TOPK_MAX_K}, got {self.similar_k}")
        self.logit_slots = [self.logits]
        self.feature_slots = [torch.zeros((self.max_batch, F), dtype=torch.float32, device=self.device)]
        self.logits = torch.zeros((self.max_batch, 2 * self.similar_k), dtype=torch.float32, device=self.device)
        self._embed_step = Step("embed", "embed_rows", src=src)
        self.steps.append(self._embed_step)
        self.steps.append(Step("similar", "similar", src="features"))

    def _on_device(self, t: torch.Tensor) -> bool:
        d = self.device
        return t.device.type == d.type and (d.index is None or t.device.index == d.index)

    def feature_slot(self, slot: int = 0) -> torch.Tensor:
        """fp32 query rows [max_batch, F] of the last forward of a ``similar`` engine in ``slot``."""
        while len(self.feature_slots) <= slot:
            self.feature_slots.append(torch.zeros_like(self.feature_slots[0]))
        return self.feature_slots[slot]

    def _similar_workspace(self, slot: int) -> torch.Tensor:
        while len(self._similar_work) <= slot:
            n = _lib.lib().gallery_topk_workspace(self.max_batch, self.similar.gallery.shape[0], self.similar_k)
            self._similar_work.append(torch.zeros(n, dtype=torch.uint8, device=self.device))
        return self._similar_work[slot]

    def _emit_similar(self, prog, step: Step, b: int) -> None:
        g, feat, out = self.similar.gallery, self.feature_slot(self._slot), self._out_rows()
        prog.add_gallery_topk(step.name, dict(q=_lib.ptr(feat), g=_lib.ptr(g), out=_lib.ptr(out),
                                              work=_lib.ptr(self._similar_workspace(self._slot)), B=b,
                                              N=g.shape[0], F=feat.shape[1], K=self.similar_k,
                                              ldq=feat.shape[1], ldg=g.shape[1]))

    # ---------------------------------------------------------------- Grad-CAM outputs
    def cam_source(self) -> tuple:
        """A family's last feature map: (buffer name, h, w, row stride in elements, F, element type:
        0 bf16 / 1 fp16). It is ``embed_source()``'s buffer with its two spatial sizes. A family
        without a spatial map in front of its head raises ValueError."""
        raise NotImplementedError

    def cam_head(self) -> dict:
        """A family's head as ``class_map`` takes it (launch.h ClassMapArgs): ``head=0, w, NC`` for a
        linear classifier on the pooled features, ``head=1, w1, w2, b1, hid, H1, NC`` for the MLP."""
        raise NotImplementedError

    def _enable_explain(self) -> None:
        """Called by ``_enable_heatmap``. With ``explain`` the head
        keeps writing the per-slot logits, a step "top1" (softmax_topk, K = 1) fills a per-slot
        [max_batch, 2] buffer with the predicted class and its score, and a last step "class_map"
        (kernels/explain.hip) writes the output rows. ``self.logits`` -- the output the executor
        copies to the host and ``forward`` returns -- becomes [max_batch, 2 + h*w] fp32 words: the
        class (int32 bits), its score, then the Grad-CAM map of that class over ``cam_source()``,
        divided by its maximum (``unpack_explain``). The class-map step names the map in ``src``, so
        the stage pipeline's buffer renaming reaches it through ``_ptr``; what else it reads (the
        logits through "top1", the head's weights and partials) belongs to the head's own stage."""
        assert not self.inputs, "explain is set at construction, before input slots exist"
        lib = _lib.lib()
        src, h, w, _, F, _ = self.cam_source()
        classes = self.logits.shape[1]
        if classes > lib.TOPK_MAX_NC:
            raise ValueError(f"explain: {classes} classes exceed the top-1 kernel's {lib.TOPK_MAX_NC}")
        if F % 8 or F > lib.CLASS_MAP_MAX_F or h * w > lib.CLASS_MAP_MAX_HW:
            raise ValueError(f"explain: a {h} x {w} map of {F} features; the kernel takes a multiple of 8 up to "
                             f"{lib.CLASS_MAP_MAX_F} features and {lib.CLASS_MAP_MAX_HW} pixels")
        self.logit_slots = [self.logits]
        self.top1_slots = [torch.zeros((self.max_batch, 2), dtype=torch.float32, device=self.device)]
        self._cam_alpha = [torch.zeros((self.max_batch, F), dtype=torch.float32, device=self.device)]
        self.logits = torch.zeros((self.max_batch, 2 + h * w), dtype=torch.float32, device=self.device)
        self.steps.append(Step("top1", "top1", src="logits"))
        self.steps.append(Step("explain", "class_map", src=src))

    # ---------------------------------------------------------------- rendered overlays
    def _enable_overlay(self, h: int, w: int) -> None:
        """Called by ``_enable_outputs`` behind the heatmap tail. With
        ``overlay`` the output rows grow to 2 + h*w + ceil(S*S*3/4) words: ``class_map`` / ``rollout_map``
        take ``ldo`` and write the front of the wider row unchanged, and one more step "overlay"
        (kernels/overlay.hip) reads the map from the row and the slot's uint8 input (``src="input"``,
        through ``_ptr``) and writes the picture bytes behind the map (``unpack_overlay``). The input
        slot is not a planned buffer: a slot's input is only rewritten after that slot's rows were
        copied out (the executors complete a slot before they refill it), so the last stage of a
        stage pipeline may read it."""
        if self.overlay is None:
            return
        assert not self.inputs, "overlay is set at construction, before input slots exist"
        from ..serving import overlay as O
        lib = _lib.lib()
        S = self.inp.shape[1]
        if self.inp.dtype != torch.uint8:
            raise ValueError("overlay paints the uint8 picture the model saw: a float-input engine has none")
        if self.inp.shape[2] != S or S < max(h, w) or S > lib.OVERLAY_MAX_S:
            raise ValueError(f"overlay: a {h} x {w} map on a {tuple(self.inp.shape[1:3])} input; the kernel "
                             f"upsamples onto square inputs up to {lib.OVERLAY_MAX_S}")
        ov = self.overlay
        xb, xk = O.axis_tables(w, S, ov.filter)
        yb, yk = O.axis_tables(h, S, ov.filter)
        host = dict(xb=xb, xk=xk, yb=yb, yk=yk, tab=O.colormap_table(ov.colormap))
        self._overlay_tabs = dict(host=host, dev={k: torch.from_numpy(v).to(self.device) for k, v in host.items()},
                                  hw=(h, w), a=O.alpha_fixed(ov.alpha), blend=O.BLENDS.index(ov.blend))
        assert self.logits.shape[1] == 2 + h * w, (self.logits.shape, h, w)
        self.logits = torch.zeros((self.max_batch, 2 + h * w + overlay_words(S)), dtype=torch.float32,
                                  device=self.device)
        self.steps.append(Step("overlay", "overlay", src="input"))

    def _emit_overlay(self, prog, step: Step, b: int) -> None:
        t = self._overlay_tabs
        host, dev, (h, w), out = t["host"], t["dev"], t["hw"], self._out_rows()
        prog.add_heat_overlay(step.name, dict(
            inp=self._ptr(step.src), out=_lib.ptr(out), tab=_lib.ptr(dev["tab"]), xb=_lib.ptr(dev["xb"]),
            xk=_lib.ptr(dev["xk"]), yb=_lib.ptr(dev["yb"]), yk=_lib.ptr(dev["yk"]),
            h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=b, S=self.inp.shape[1], h=h, w=w,
            ldo=out.shape[1], xks=host["xk"].shape[1], yks=host["yk"].shape[1], a=t["a"], blend=t["blend"]))

    # ---------------------------------------------------------------- overlays as JPEG files
    def _enable_overlay_jpeg(self, h: int, w: int) -> None:
        """Called by ``_enable_outputs`` behind ``_enable_overlay``. With ``overlay_jpeg`` the wide rows
        that step made stay on the device (one buffer per slot; ``class_map`` / ``rollout_map`` / ``overlay``
        write them as before, through ``_out_rows``), and one more step "overlay_jpeg"
        (kernels/jpeg_encode.hip) writes the output rows: the 2 + h*w front words copied from the raw row,
        a length word, then the file in ceil(max_bytes/4) words, the bytes behind it 0
        (``unpack_overlay_jpeg``). The file header is built here, once, and kept on the device."""
        if self.overlay_jpeg is None:
            return
        assert not self.inputs, "overlay_jpeg is set at construction, before input slots exist"
        from ..serving import jpeg_encode as J
        lib = _lib.lib()
        S, spec = self.inp.shape[1], self.overlay_jpeg
        cap = overlay_jpeg_cap(S, spec.max_bytes)
        if S > lib.JPEG_ENC_MAX_SIDE or cap > lib.JPEG_ENC_MAX_CAP:
            raise ValueError(f"overlay_jpeg: a {S} x {S} picture in at most {cap} bytes; the kernel takes sides up "
                             f"to {lib.JPEG_ENC_MAX_SIDE} and {lib.JPEG_ENC_MAX_CAP} bytes")
        import numpy as np
        host = np.frombuffer(J.header(S, S, spec.quality, spec.subsampling), np.uint8).copy()
        sampling = J.SUBSAMPLINGS.index(spec.subsampling)
        self._jpeg = dict(cap=cap, hw=(h, w), sampling=sampling, host=host, dev=torch.from_numpy(host).to(self.device),
                          work=lib.jpeg_encode_workspace(self.max_batch, S, S, sampling, cap),
                          slots=[(self.logits, None)])
        self.logits = torch.zeros((self.max_batch, 2 + h * w + 1 + (cap + 3) // 4), dtype=torch.float32,
                                  device=self.device)
        self.steps.append(Step("overlay_jpeg", "overlay_jpeg"))

    def _jpeg_slot(self, slot: int) -> tuple:
        """(raw overlay rows, encoder workspace) of a slot, both device-only."""
        sl = self._jpeg["slots"]
        while len(sl) <= slot:
            sl.append((torch.zeros_like(sl[0][0]), None))
        if sl[slot][1] is None:
            sl[slot] = (sl[slot][0], torch.zeros(self._jpeg["work"], dtype=torch.uint8, device=self.device))
        return sl[slot]

    def overlay_raw(self, slot: int = 0) -> torch.Tensor:
        """The raw overlay rows (``unpack_overlay``) of the last forward of an ``overlay_jpeg`` engine in ``slot``."""
        return self._jpeg_slot(slot)[0]

    def _emit_overlay_jpeg(self, prog, step: Step, b: int) -> None:
        j, (h, w), S = self._jpeg, self._jpeg["hw"], self.inp.shape[1]
        raw, work = self._jpeg_slot(self._slot)
        out = self.slot_logits(self._slot)
        front = 2 + h * w
        prog.add_jpeg_encode(step.name, dict(
            inp=_lib.ptr(raw) + 4 * front, ldi=4 * raw.shape[1], hdr=_lib.ptr(j["dev"]), h_hdr=j["host"].ctypes.data,
            front=_lib.ptr(raw), ldf=raw.shape[1], nfront=front, out=_lib.ptr(out), ldo=out.shape[1],
            work=_lib.ptr(work), B=b, H=S, W=S, quality=self.overlay_jpeg.quality, sampling=j["sampling"],
            cap=j["cap"]))

    # ---------------------------------------------------------------- dominant colours
    def _enable_palette(self, h: int, w: int) -> None:
        """Called by ``_enable_outputs`` behind the heatmap tail. With ``palette`` the output rows grow to
        2 + h*w + 1 + 2K words: ``class_map`` / ``rollout_map`` take ``ldo`` and write the front of the wider
        row unchanged, and one more step "palette" (kernels/palette.hip) reads the map from the row and the
        slot's uint8 input (``src="input"``, through ``_ptr``, with the lifetime ``_enable_overlay``
        describes) and writes W and the K (colour, weight) pairs behind the map (``unpack_palette``). Each
        slot has its own histogram workspace, which the step leaves zeroed."""
        if self.palette is None:
            return
        assert not self.inputs, "palette is set at construction, before input slots exist"
        from ..serving import overlay as O
        from ..serving import palette as PL
        lib = _lib.lib()
        S, pal = self.inp.shape[1], self.palette
        if self.inp.dtype != torch.uint8:
            raise ValueError("palette reads the uint8 picture the model saw: a float-input engine has none")
        if self.inp.shape[2] != S or S < max(h, w) or S > lib.OVERLAY_MAX_S:
            raise ValueError(f"palette: a {h} x {w} map on a {tuple(self.inp.shape[1:3])} input; the kernel "
                             f"upsamples onto square inputs up to {lib.OVERLAY_MAX_S}")
        xb, xk = O.axis_tables(w, S, pal.filter)
        yb, yk = O.axis_tables(h, S, pal.filter)
        host = dict(xb=xb, xk=xk, yb=yb, yk=yk)
        self._palette_tabs = dict(host=host, dev={k: torch.from_numpy(v).to(self.device) for k, v in host.items()},
                                  hw=(h, w), weight=PL.WEIGHTS.index(pal.weight), work=[])
        assert self.logits.shape[1] == 2 + h * w, (self.logits.shape, h, w)
        self.logits = torch.zeros((self.max_batch, 2 + h * w + 1 + 2 * pal.colors), dtype=torch.float32,
                                  device=self.device)
        self.steps.append(Step("palette", "palette", src="input"))

    def _palette_workspace(self, slot: int) -> torch.Tensor:
        work = self._palette_tabs["work"]
        while len(work) <= slot:
            work.append(torch.zeros(_lib.lib().palette_workspace(self.max_batch), dtype=torch.uint8,
                                    device=self.device))
        return work[slot]

    def _emit_palette(self, prog, step: Step, b: int) -> None:
        t = self._palette_tabs
        host, dev, (h, w), out = t["host"], t["dev"], t["hw"], self._out_rows()
        prog.add_palette(step.name, dict(
            inp=self._ptr(step.src), out=_lib.ptr(out), work=_lib.ptr(self._palette_workspace(self._slot)),
            xb=_lib.ptr(dev["xb"]), xk=_lib.ptr(dev["xk"]), yb=_lib.ptr(dev["yb"]), yk=_lib.ptr(dev["yk"]),
            h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=b, S=self.inp.shape[1], h=h, w=w,
            ldo=out.shape[1], xks=host["xk"].shape[1], yks=host["yk"].shape[1], K=self.palette.colors,
            T=self.palette.rounds, weight=t["weight"]))

    # ---------------------------------------------------------------- garment boxes
    def _enable_locate(self, h: int, w: int) -> None:
        """Called by ``_enable_outputs`` behind the heatmap tail. With ``locate`` the output rows grow to
        2 + h*w + 1 + 3K words: ``class_map`` / ``rollout_map`` take ``ldo`` and write the front of the wider
        row unchanged, and one more step "locate" (kernels/locate.hip) reads the map from the row, never the
        picture, and writes the region count and the K (corner, corner, area) triples behind the map
        (``unpack_locate``). Each slot has its own workspace (the bitmask and the run tables), which every
        launch initialises before it reads it."""
        if self.locate is None:
            return
        assert not self.inputs, "locate is set at construction, before input slots exist"
        from ..serving import overlay as O
        lib = _lib.lib()
        S, loc = self.inp.shape[1], self.locate
        if self.inp.shape[2] != S or S < max(h, w) or S > lib.OVERLAY_MAX_S:
            raise ValueError(f"locate: a {h} x {w} map on a {tuple(self.inp.shape[1:3])} input; the kernel "
                             f"upsamples onto square inputs up to {lib.OVERLAY_MAX_S}")
        xb, xk = O.axis_tables(w, S, loc.filter)
        yb, yk = O.axis_tables(h, S, loc.filter)
        host = dict(xb=xb, xk=xk, yb=yb, yk=yk)
        self._locate_tabs = dict(host=host, dev={k: torch.from_numpy(v).to(self.device) for k, v in host.items()},
                                 hw=(h, w), work=[])
        assert self.logits.shape[1] == 2 + h * w, (self.logits.shape, h, w)
        self.logits = torch.zeros((self.max_batch, 2 + h * w + 1 + 3 * loc.boxes), dtype=torch.float32,
                                  device=self.device)
        self.steps.append(Step("locate", "locate"))

    def _locate_workspace(self, slot: int) -> torch.Tensor:
        work = self._locate_tabs["work"]
        while len(work) <= slot:
            work.append(torch.zeros(_lib.lib().locate_workspace(self.max_batch, self.inp.shape[1]), dtype=torch.uint8,
                                    device=self.device))
        return work[slot]

    def _emit_locate(self, prog, step: Step, b: int) -> None:
        t = self._locate_tabs
        host, dev, (h, w), out = t["host"], t["dev"], t["hw"], self._out_rows()
        prog.add_locate(step.name, dict(
            out=_lib.ptr(out), work=_lib.ptr(self._locate_workspace(self._slot)),
            xb=_lib.ptr(dev["xb"]), xk=_lib.ptr(dev["xk"]), yb=_lib.ptr(dev["yb"]), yk=_lib.ptr(dev["yk"]),
            h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=b, S=self.inp.shape[1], h=h, w=w,
            ldo=out.shape[1], xks=host["xk"].shape[1], yks=host["yk"].shape[1], K=self.locate.boxes,
            threshold=self.locate.threshold))

    # ---------------------------------------------------------------- garment cutouts
    def _enable_cutout(self, h: int, w: int) -> None:
        """Called by ``_enable_outputs`` behind the heatmap tail. With ``cutout`` the output rows grow to
        2 + h*w + 1 + S*S words: ``class_map`` / ``rollout_map`` take ``ldo`` and write the front of the wider
        row unchanged, and one more step "cutout" (kernels/cutout.hip) reads the map from the row and the
        slot's uint8 input (``src="input"``, through ``_ptr``, with the lifetime ``_enable_overlay``
        describes) and writes the garment's pixel count and the RGBA words behind the map
        (``unpack_cutout``). Each slot has its own workspace: the colour tables, which the step leaves zeroed,
        and the colour bits and the gate's bitmask, which every launch writes before it reads them."""
        if self.cutout is None:
            return
        assert not self.inputs, "cutout is set at construction, before input slots exist"
        from ..serving import overlay as O
        lib = _lib.lib()
        S, cut = self.inp.shape[1], self.cutout
        if self.inp.dtype != torch.uint8:
            raise ValueError("cutout reads the uint8 picture the model saw: a float-input engine has none")
        if self.inp.shape[2] != S or S < max(h, w) or S > lib.OVERLAY_MAX_S:
            raise ValueError(f"cutout: a {h} x {w} map on a {tuple(self.inp.shape[1:3])} input; the kernel "
                             f"upsamples onto square inputs up to {lib.OVERLAY_MAX_S}")
        xb, xk = O.axis_tables(w, S, cut.filter)
        yb, yk = O.axis_tables(h, S, cut.filter)
        host = dict(xb=xb, xk=xk, yb=yb, yk=yk)
        self._cutout_tabs = dict(host=host, dev={k: torch.from_numpy(v).to(self.device) for k, v in host.items()},
                                 hw=(h, w), work=[])
        assert self.logits.shape[1] == 2 + h * w, (self.logits.shape, h, w)
        self.logits = torch.zeros((self.max_batch, 2 + h * w + 1 + S * S), dtype=torch.float32, device=self.device)
        self.steps.append(Step("cutout", "cutout", src="input"))

    def _cutout_workspace(self, slot: int) -> torch.Tensor:
        work = self._cutout_tabs["work"]
        while len(work) <= slot:
            work.append(torch.zeros(_lib.lib().cutout_workspace(self.max_batch, self.inp.shape[1]), dtype=torch.uint8,
                                    device=self.device))
        return work[slot]

    def _emit_cutout(self, prog, step: Step, b: int) -> None:
        t = self._cutout_tabs
        host, dev, (h, w), out, cut = t["host"], t["dev"], t["hw"], self._out_rows(), self.cutout
        prog.add_cutout(step.name, dict(
            inp=self._ptr(step.src), out=_lib.ptr(out), work=_lib.ptr(self._cutout_workspace(self._slot)),
            xb=_lib.ptr(dev["xb"]), xk=_lib.ptr(dev["xk"]), yb=_lib.ptr(dev["yb"]), yk=_lib.ptr(dev["yk"]),
            h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=b, S=self.inp.shape[1], h=h, w=w,
            ldo=out.shape[1], xks=host["xk"].shape[1], yks=host["yk"].shape[1], gate=cut.gate, rounds=cut.rounds,
            smooth=cut.smooth, feather=int(bool(cut.feather))))

    def top1_slot(self, slot: int = 0) -> torch.Tensor:
        """[max_batch, 2] class (int32 bits) and score of the last forward of an ``explain`` or
        ``rollout`` engine."""
        while len(self.top1_slots) <= slot:
            self.top1_slots.append(torch.zeros_like(self.top1_slots[0]))
            if self._cam_alpha:
                self._cam_alpha.append(torch.zeros_like(self._cam_alpha[0]))
        return self.top1_slots[slot]

    def _emit_top1(self, prog, step: Step, b: int) -> None:
        lg = self._logit_slot(self._slot)
        prog.add_softmax_topk(step.name, dict(x=_lib.ptr(lg), out=_lib.ptr(self.top1_slot(self._slot)), B=b,
                                              NC=lg.shape[1], K=1, ldx=lg.shape[1]))

    def _emit_explain(self, prog, step: Step, b: int) -> None:
        _, h, w, ldx, F, dt = self.cam_source()
        top, out = self.top1_slot(self._slot), self._out_rows()
        prog.add_class_map(step.name, dict(x=self._ptr(step.src), top=_lib.ptr(top),
                                           alpha=_lib.ptr(self._cam_alpha[self._slot]), out=_lib.ptr(out), B=b,
                                           HW=h * w, F=F, ldx=ldx, ldo=out.shape[1], dt=dt, norm=1,
                                           **self.cam_head()))

    def add_input_slots(self, n: int) -> list[torch.Tensor]:
        """Extra static input AND logits buffers, each slot with its own captured
        graphs, so a pipelined caller can H2D batch i+1 into one slot while the graph
        of batch i reads another, and D2H batch i's logits while batch i+1's graph
        writes its own (no device-to-device copies on the compute stream)."""
        if not self.inputs:
            self.inputs = [self.inp]
            self.outputs = [self.logits]
        while len(self.inputs) < n:
            self.inputs.append(torch.zeros_like(self.inp))
            self.outputs.append(torch.zeros_like(self.logits))
        return self.inputs

    # ---------------------------------------------------------------- hooks
    def _emit(self, prog, step: Step, b: int) -> None:
        raise NotImplementedError

    def _emit_conv(self, prog, step: Step, b: int, split=None, cfg=None) -> None:
        """Emit (prog) or launch now (prog=None) one conv step with an explicit variant."""
        raise NotImplementedError

    # ---------------------------------------------------------------- programs
    def conv_steps(self) -> list[Step]:
        """Steps with a tunable GEMM layer (bf16 conv-GEMM or fp8 linear)."""
        return [s for s in self.steps if s.kind in ("conv", "f8")]

    def program(self, b: int, capture: bool = True, slot: int = 0):
        key = (b, capture, slot)
        if key in self.programs:
            return self.programs[key]
        assert 1 <= b <= self.max_batch
        prog = _lib.lib().Program()
        self._slot = slot
        try:
            self._emit_steps(prog, self.steps, [{}] * len(self.steps), b)
        finally:
            self._slot, self._remap = 0, {}
        if capture:
            with torch.cuda.device(self.device):
                prog.capture(int(self.stream.cuda_stream))
        self.programs[key] = prog
        return prog

    def _wptr(self, name: str) -> int:
        """Destination pointer of a step: a residual GEMM (res == dst) may write a different
        physical copy than it reads (stages.py versioning puts that under ``name@w``)."""
        return self._ptr(name + "@w") if (name + "@w") in self._remap else self._ptr(name)

    def alias_buffer(self, name: str, alias: str) -> None:
        """Another physical copy of an activation buffer (``stages.StagePipe`` gives each
        pipeline stage / batch parity its own copy of the buffers it shares)."""
        if alias not in self.bufs:
            self.bufs[alias] = torch.zeros_like(self.bufs[name])

    def program_range(self, b: int, lo: int, hi: int, capture: bool = True, slot: int = 0,
                      remap=None):
        """Program of steps[lo:hi] only, with buffer names remapped (``stages.py``):
        ``remap`` is one dict for all steps or a list with one dict per step."""
        n = hi - lo
        maps = list(remap) if isinstance(remap, (list, tuple)) else [dict(remap or {})] * n
        assert len(maps) == n
        key = (b, capture, slot, lo, hi, tuple(tuple(sorted(m.items())) for m in maps))
        if key in self.programs:
            return self.programs[key]
        prog = _lib.lib().Program()
        self._slot = slot
        try:
            self._emit_steps(prog, self.steps[lo:hi], maps, b)
        finally:
            self._slot, self._remap = 0, {}
        if capture:
            with torch.cuda.device(self.device):
                prog.capture(int(self.stream.cuda_stream))
        self.programs[key] = prog
        return prog

    def _emit_steps(self, prog, steps: list[Step], maps: list[dict], b: int) -> None:
        """Emit a run of steps, each with its buffer remap, on the engine's device (a vendor
        GEMM node builds its plan and workspace for the CURRENT device at emission time)."""
        ctx = torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()
        with ctx:
            for st, m in zip(steps, maps):
                self._remap = m
                if st is self._embed_step:     # by identity: ViT has its own step of kind "embed"
                    self._emit_embed(prog, st, b)
                else:
                    getattr(self, self.TAIL_EMITTERS.get(st.kind, "_emit"))(prog, st, b)

    def invalidate(self) -> None:
        self.programs.clear()

    def bucket_for(self, n: int) -> int:
        for b in self.buckets:
            if b >= n:
                return b
        raise ValueError(f"batch {n} exceeds max bucket {self.buckets[-1]}")

    def launch(self, b: int, stream: torch.cuda.Stream | None = None, capture: bool = True,
               slot: int = 0) -> None:
        """Run the forward for the first ``b`` images already in input slot ``slot``."""
        s = stream or self.stream
        self.program(b, capture, slot).launch(int(s.cuda_stream))

    @torch.no_grad()
    def forward(self, x: torch.Tensor, capture: bool = True) -> torch.Tensor:
        """x: [n, H, W, 3] in the engine's input dtype, any device -> fp32 logits [n, classes]
        (a ``topk`` or ``similar`` engine: the packed rows [n, 2K], see ``unpack_topk``; an ``embed``
        engine: the fp32 feature rows [n, F]; an ``explain`` or ``rollout`` engine: the packed rows
        [n, 2 + h*w], see ``unpack_explain``; with ``overlay`` the wider rows of ``unpack_overlay``, with
        ``overlay_jpeg`` the rows of ``unpack_overlay_jpeg``, with ``palette`` the rows of ``unpack_palette``,
        with ``locate`` the rows of ``unpack_locate``, with ``cutout`` the rows of ``unpack_cutout``)."""
        n = x.shape[0]
        assert tuple(x.shape[1:]) == tuple(self.inp.shape[1:]), (x.shape, self.inp.shape)
        assert x.dtype == self.inp.dtype, (x.dtype, self.inp.dtype)
        b = self.bucket_for(n)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self.inp[:n].copy_(x, non_blocking=True)
            self.launch(b, self.stream, capture)
            out = self.logits[:n].clone()
        cur.wait_stream(self.stream)
        return out

    # ---------------------------------------------------------------- observability / tuning
    def profile(self, b: int, iters: int = 20) -> list[tuple[str, float]]:
        prog = self.program(b, capture=False)
        ms = prog.profile(int(self.stream.cuda_stream), iters)
        return list(zip(prog.op_names(), ms))

    def _variants(self, step: Step) -> list[tuple[bool, int]]:
        v = step.layer.variants(step.geom[1])
        if step.res and not getattr(step.layer, "stream_ok", lambda res=False: True)(res=True):
            v = [x for x in v if x[1] not in STREAM_IDS]
        return v

    def autotune(self, b: int, iters: int = 10, verbose: bool = False) -> dict[str, list[int]]:
        """Pick the fastest (split, tile config) per conv layer by timing on the device."""
        s = self.stream
        chosen = {}
        with torch.cuda.stream(s):
            for step in self.conv_steps():
                lay: ConvGemmLayer = step.layer
                best = None
                for split, cfg in self._variants(step):
                    def run():
                        self._emit_conv(None, step, b, split=split, cfg=cfg)
                    for _ in range(2):
                        run()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(iters):
                        run()
                    e1.record(s)
                    e1.synchronize()
                    t = e0.elapsed_time(e1) / iters
                    if best is None or t < best[0]:
                        best = (t, split, cfg)
                    if verbose:
                        print(f"  {step.name:24s} split={int(split)} cfg {cfg}: {t * 1e3:8.1f} us", flush=True)
                lay.split, lay.cfg = best[1], best[2]
                chosen[step.name] = [int(best[1]), best[2]]
        self.invalidate()
        return chosen

    def tuning(self) -> dict[str, list[int]]:
        return {s.name: [int(s.layer.split), s.layer.cfg] for s in self.conv_steps()}

    def save_tuning(self, path) -> None:
        Path(path).write_text(json.dumps(self.tuning(), indent=1))

    def load_tuning(self, path) -> None:
        self.apply_tuning(json.loads(Path(path).read_text()))

    def apply_tuning(self, d: dict) -> None:
        for s in self.conv_steps():
            v = d.get(s.name)
            if v is None:
                continue
            split, cfg = (False, v) if isinstance(v, int) else (bool(v[0]), int(v[1]))
            ok = cfg in s.layer.candidates       # (ids 1000-1999, the retired hipBLASLt node, are refused)
            if cfg in STREAM_IDS:
                ok = getattr(s.layer, "stream_ok", lambda res=False: False)(res=bool(s.res))
            if is_splitk(cfg):
                sk, base = splitk_parts(cfg)
                ok = sk in getattr(s.layer, "ksplit", ()) and base in s.layer.candidates
            if ok and (not split or getattr(s.layer, "mode", -1) == MODE_DW):
                s.layer.split, s.layer.cfg = split, cfg
        self.invalidate()
