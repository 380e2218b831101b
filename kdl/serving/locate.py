"""Garment boxes: the ``locate`` / ``locate_image`` / ``locate_bytes`` signatures.

"Where is it?" beside "what is it?". They ride on the family's heatmap method (Grad-CAM where
``ModelInfo.cam_oracle`` exists, attention rollout where ``rollout_oracle`` does): the classic use of a class
activation map (CAM localisation, Zhou et al. 2016) is to threshold it, take the connected regions and answer
their bounding boxes, so a caller can crop a product shot to the garment. Outputs: ``classes`` DT_STRING
[-1, 1], ``scores`` DT_FLOAT [-1, 1], ``boxes`` DT_FLOAT [-1, K, 4] (``[ymin, xmin, ymax, xmax]`` as fractions
of the picture the model saw, TensorFlow's box convention), ``areas`` DT_FLOAT [-1, K] (each region's share of
the picture), ``num_boxes`` DT_INT32 [-1, 1] (all regions, not clipped to K). The rule uses integers only
and is defined HERE, once: ``locate_rule`` in numpy is what CPU servers answer and what the GPU kernels
(kernels/locate.hip, ``EngineBase(locate=...)``) reproduce bit for bit.

1. upsample   u = overlay.upsample(overlay.quantise(heat), S, filter), uint8 [S, S] (steps 1-2 of the overlay
              rule, unchanged).
2. mask       u >= threshold, an integer in 1..255. The default is 51: the maps are divided by their
              maximum, so 51 is CAM's 20 % of the peak.
3. components of the mask under 8-connectivity. A component's identity is its first pixel in raster
              order: its smallest y*S + x.
4. measures   per component its pixel count ``area`` and its box (y0, x0, y1, x1), y1 and x1 exclusive.
5. count      the number of all components; it may exceed K.
6. order      by area descending, ties to the earlier first pixel; the answer is the first K. Absent boxes
              are (0, 0, 0, 0) with area 0.

An all-zero, all-NaN or below-threshold map gives count 0 and zeros.

Configuration (opt-in): ``"locate": {"boxes": 3, "threshold": 51, "filter": "bilinear"}`` in the version's
``kdl_model.json`` / ``synthetic.json`` (these are the defaults of a present block), or ``--locate_boxes K``,
which turns the signatures on and overrides ``boxes``. A result row is 2 + h*w + 1 + 3K words: explain's
front, count, then K x (y0 | x0 << 16, y1 | x1 << 16, area) (``pack_rows`` / ``unpack_rows``). S <= 1024 keeps
every coordinate in 16 bits and every area in 21.
"""
from __future__ import annotations

from bisect import bisect_left
from pathlib import Path

import numpy as np

from ..engine.base import Locate, pack_locate, unpack_locate  # noqa: F401
from . import overlay
from . import protos as P

LOCATE_SIGNATURE = "locate"
LOCATE_IMAGE_SIGNATURE = "locate_image"
LOCATE_BYTES_SIGNATURE = "locate_bytes"
LOCATE_SIGNATURES = (LOCATE_SIGNATURE, LOCATE_IMAGE_SIGNATURE, LOCATE_BYTES_SIGNATURE)
OUTPUT_KEYS = ("classes", "scores", "boxes", "areas", "num_boxes")
MAX_BOXES = 8
MAX_S = 1024                                   # kOverlayMaxS: coordinates in 16 bits, areas in 21


def _int_in(v, lo: int, hi: int) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= int(v) <= hi


def check(spec: Locate) -> Locate:
    """ValueError for boxes outside 1..8, a threshold outside 1..255, an unknown filter."""
    if not _int_in(spec.boxes, 1, MAX_BOXES):
        raise ValueError(f"locate boxes must be an integer in 1..{MAX_BOXES}, got {spec.boxes!r}")
    if not _int_in(spec.threshold, 1, 255):
        raise ValueError(f"locate threshold must be an integer in 1..255, got {spec.threshold!r}")
    if spec.filter not in overlay.FILTERS:
        raise ValueError(f"locate filter must be one of {tuple(overlay.FILTERS)}, got {spec.filter!r}")
    return spec


def mask_of(heat_f32, S: int, spec: Locate) -> np.ndarray:
    """Steps 1-2: bool [S, S]."""
    return overlay.upsample(overlay.quantise(heat_f32), S, spec.filter) >= int(spec.threshold)


def runs_of(mask: np.ndarray) -> tuple:
    """The maximal horizontal runs of a bool mask in raster order: (y, x0, x1) int64 arrays, x1 exclusive."""
    m = np.asarray(mask, dtype=bool)
    pad = np.zeros((m.shape[0], m.shape[1] + 2), dtype=np.int8)
    pad[:, 1:-1] = m
    d = np.diff(pad, axis=1)
    y, x0 = np.nonzero(d == 1)                                  # np.nonzero walks in raster order
    _, x1 = np.nonzero(d == -1)
    return y.astype(np.int64), x0.astype(np.int64), x1.astype(np.int64)


def components(mask: np.ndarray) -> tuple:
    """Steps 3-4 on a bool mask [H, W]: (first int64 [n], areas int64 [n], boxes int64 [n, 4]) of its
    8-connected components in the raster order of their first pixels (``first`` = y*W + x of that pixel).
    Union-find over runs: a run of row y joins every run of row y - 1 whose column range widened by one
    overlaps it; the smaller run index becomes the parent, so a root is its component's first run."""
    W = mask.shape[1]
    y, x0, x1 = runs_of(mask)
    n = len(y)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    row_off = np.searchsorted(y, np.arange(mask.shape[0] + 1))
    ys, a0, a1 = y.tolist(), x0.tolist(), x1.tolist()
    for r in range(n):
        yy = ys[r]
        if yy == 0:
            continue
        hi = int(row_off[yy])
        p = bisect_left(a1, a0[r], int(row_off[yy - 1]), hi)      # behind the runs above that end left of x0 - 1
        while p < hi and a0[p] <= a1[r]:
            i, j = find(r), find(p)
            if i != j:
                parent[max(i, j)] = min(i, j)
            p += 1
    root = np.array([find(i) for i in range(n)], dtype=np.int64)
    ids, inv = np.unique(root, return_inverse=True)             # ascending: raster order of the first pixels
    k = len(ids)
    areas = np.zeros(k, dtype=np.int64)
    np.add.at(areas, inv, x1 - x0)
    box = np.empty((k, 4), dtype=np.int64)
    box[:, :2] = np.iinfo(np.int64).max
    box[:, 2:] = 0
    np.minimum.at(box[:, 0], inv, y)
    np.minimum.at(box[:, 1], inv, x0)
    np.maximum.at(box[:, 2], inv, y + 1)
    np.maximum.at(box[:, 3], inv, x1)
    return y[ids] * W + x0[ids], areas, box


def select(first, areas, box, K: int) -> tuple:
    """Steps 5-6: (count, boxes int32 [K, 4], areas uint32 [K])."""
    boxes, out = np.zeros((K, 4), dtype=np.int32), np.zeros(K, dtype=np.uint32)
    order = np.lexsort((first, -areas))[:K]                     # area descending, ties to the earlier first pixel
    boxes[:len(order)] = box[order]
    out[:len(order)] = areas[order]
    return len(areas), boxes, out


def locate_rule(heat_f32, S: int, spec: Locate | None = None) -> tuple:
    """THE definition: fp32 heat [h, w] and the side S of the picture the model saw -> (count, boxes int32
    [K, 4] as (y0, x0, y1, x1), areas uint32 [K])."""
    spec = check(spec or Locate())
    heat = np.asarray(heat_f32)
    if heat.ndim != 2:
        raise ValueError(f"the map must be [h, w], got {heat.shape}")
    S = int(S)
    if S > MAX_S:
        raise ValueError(f"locate: a side of {S} pixels is refused, the packed coordinates hold up to {MAX_S}")
    return select(*components(mask_of(heat, S, spec)), int(spec.boxes))


# ------------------------------------------------------------------------------------------ host-side helpers
def boxes_of(boxes, S: int) -> np.ndarray:
    """float32(v / S) per coordinate, the division in float64: [ymin, xmin, ymax, xmax]."""
    return (np.asarray(boxes, dtype=np.float64) / float(S)).astype(np.float32)


def areas_of(areas, S: int) -> np.ndarray:
    """float32(area / (S*S)), the division in float64."""
    return (np.asarray(areas, dtype=np.float64) / float(S * S)).astype(np.float32)


# ------------------------------------------------------------------------------------------ rows
def pack_rows(classes, scores, heat, counts, boxes, areas) -> np.ndarray:
    """The engine's row layout [n, 2 + h*w + 1 + 3K] fp32 words."""
    return pack_locate(classes, scores, heat, counts, boxes, areas)


def unpack_rows(rows, h: int, w: int, K: int) -> tuple:
    """-> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], counts uint32 [n], boxes int32 [n, K, 4],
    areas uint32 [n, K])."""
    return unpack_locate(np.ascontiguousarray(rows, dtype=np.float32), h, w, K)


# ------------------------------------------------------------------------------------------ config
def resolve(path: Path, boxes_flag: int | None = None) -> Locate | None:
    """The version's ``Locate``: its "locate" block over the defaults, ``--locate_boxes`` over that; None
    where neither is there. ValueError (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    if "locate" not in meta and boxes_flag is None:
        return None
    block = meta.get("locate", {})
    if not isinstance(block, dict):
        raise ValueError(f"{path / name}: \"locate\" must be an object like {{\"boxes\": 3, \"threshold\": 51}}")
    unknown = sorted(set(block) - {"boxes", "threshold", "filter"})
    if unknown:
        raise ValueError(f"{path / name}: unknown \"locate\" keys {unknown}")
    try:
        spec = check(Locate(**block))
    except ValueError as e:
        raise ValueError(f"{path / name}: {e}") from e
    if boxes_flag is not None:
        if not _int_in(boxes_flag, 1, MAX_BOXES):
            raise ValueError(f"--locate_boxes must be an integer in 1..{MAX_BOXES}, got {boxes_flag!r}")
        spec = Locate(int(boxes_flag), spec.threshold, spec.filter)
    return spec


def add_signatures(src, path, boxes_flag: int | None = None) -> None:
    """Give a loaded ModelSource with a "locate" block (or the flag) its three locate signatures. They are
    explain-kind signatures told from the others by their ``boxes`` output, whose shape carries K."""
    from ..engine import registry
    from .outputs import add_trio
    spec = resolve(path, boxes_flag)
    if spec is None:
        return
    info = registry.get(src.family)
    if info.cam_oracle is None and info.rollout_oracle is None:
        raise ValueError(f"{path}: \"locate\" needs a heatmap method, which the {src.family} family does not have")
    h, w = info.map_size
    S, K = src.input_size, int(spec.boxes)
    if S < max(h, w) or S > MAX_S:
        raise ValueError(f"{path}: locate takes inputs from the {h} x {w} map's size up to {MAX_S}, not {S} x {S}")
    src.locate = spec
    outs = (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)), ("boxes", P.DT_FLOAT, (-1, K, 4)),
            ("areas", P.DT_FLOAT, (-1, K)), ("num_boxes", P.DT_INT32, (-1, 1)))
    add_trio(src, LOCATE_SIGNATURES, "classes", (-1, 1), outputs=outs, explain=(h, w),
             rollout=info.cam_oracle is None)
