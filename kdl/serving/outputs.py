"""One description per kind of result row.

A signature answers with one of ten kinds of row: the fp32 ``logits``, or what the ``classify``,
``embed``, ``similar``, ``explain``, ``attention``, ``overlay``, ``overlay_jpeg``, ``palette`` and ``locate``
trios pack into the same fp32 words. An eleventh, what the ``cutout`` trio packs, is ``CUTOUT`` beside the
table: the picture itself with an alpha channel, a word per pixel.
Everything that differs between the kinds is in ``KINDS`` and ``CUTOUT``; runners, executors, answer builders
and the loader ask ``kind_of`` and name no kind. Per kind:

  trio       its three signature names: uint8 pixels, any-size image, encoded file
  counter    what an answered request bumps (``signature=`` label)
  engine     (sig, src, device) -> the keywords a GPU engine is built with, so the rows come out of
             the captured program
  gpu_words  (sig, src) -> 32-bit words per row from a GPU engine
  cpu_rows   (sig, src, x) -> what the CPU executor returns for the staged batch x; its width
             (``host_words``, gpu_words when None) is also the null device's
  host_step  (sig, src, rows) -> packed rows, applied after ``_run`` where no engine packed them
             (CPU and null device); None = the executor's rows are the answer
  null_zero  the null device's rows are zeroed (class 0, score 0, an empty map)
  columns    (src, sig, rows) -> the named outputs [(key, dtype, array, nested list of strings or flat
             list of bytes)]; None = the single fp32 output, built natively
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path
from typing import Callable

import numpy as np
import torch

from ..engine.base import overlay_jpeg_cap, overlay_words
from . import classify, cutout, embed, explain, jpeg_encode, locate, overlay, palette, rollout, similar
from . import protos as P
from .jpeg import BYTES_SIGNATURE
from .metrics import METRICS
from .resize import IMAGE_SIGNATURE

NATIVE_SIGNATURE = "serving_uint8"     # native fast path: uint8 HWC images (4x fewer bytes)
NATIVE_INPUT_KEY = "images"


# ---------------------------------------------------------------------- GPU engine keywords
def _similar_kw(sig, src, dev) -> dict:
    from ..engine.base import Similar
    return dict(similar=Similar(similar.device_gallery(src, dev), sig.top_k, src.similar_metric))


def _map_kw(sig, src, dev) -> dict:
    kw = dict(rollout=True) if sig.rollout else dict(explain=True)
    return dict(kw, overlay=src.overlay) if sig.overlay else kw


def _jpeg_kw(sig, src, dev) -> dict:
    return dict(_map_kw(sig, src, dev), overlay_jpeg=src.overlay_jpeg)


def _palette_kw(sig, src, dev) -> dict:
    return dict(_map_kw(sig, src, dev), palette=src.palette)


def _locate_kw(sig, src, dev) -> dict:
    return dict(_map_kw(sig, src, dev), locate=src.locate)


def _cutout_kw(sig, src, dev) -> dict:
    return dict(_map_kw(sig, src, dev), cutout=src.cutout)


# ---------------------------------------------------------------------- CPU executor rows
def _info(src):
    from ..engine import registry
    return registry.get(src.family)


def _logit_rows(sig, src, x):
    if src.family != "xception":
        return _info(src).oracle(src.params, x)
    from ..models import xception as X
    return X.xception_forward(src.params, x.float() / 127.5 - 1.0 if sig.input_dtype == P.DT_UINT8 else x,
                              head=src.head)


def _feature_rows(sig, src, x):
    rows = _info(src).feature_oracle(src.params, x)
    return embed.l2_rule(rows.numpy()) if sig.embed == "l2" else rows


def _map_rows(sig, src, x):
    """Autograd through the family's own head (Grad-CAM) or its fp32 rollout; an overlay is the rule
    on the very tensor the oracle was fed."""
    oracle = _info(src).rollout_oracle if sig.rollout else _info(src).cam_oracle
    kw = dict(head=src.head) if src.family == "xception" and src.head is not None else {}
    k, score, heat = (t.numpy() for t in oracle(src.params, x, **kw))
    if _is_palette(sig):
        ans = [palette.palette_rule(img, m, src.palette) for img, m in zip(x.numpy(), heat)]
        return palette.pack_rows(k, score, heat, *(np.stack([a[i] for a in ans]) for i in range(3)))
    if _is_locate(sig):
        ans = [locate.locate_rule(m, src.input_size, src.locate) for m in heat]
        return locate.pack_rows(k, score, heat, *(np.stack([a[i] for a in ans]) for i in range(3)))
    if _is_cutout(sig):
        ans = [cutout.cutout_rule(img, m, src.cutout) for img, m in zip(x.numpy(), heat)]
        return cutout.pack_rows(k, score, heat, *(np.stack([a[i] for a in ans]) for i in range(2)))
    if not sig.overlay:
        return explain.pack_rows(k, score, heat)
    pics = [overlay.overlay_rule(img, m, src.overlay) for img, m in zip(x.numpy(), heat)]
    if not _is_jpeg(sig):
        return overlay.pack_rows(k, score, heat, np.stack(pics))
    spec = src.overlay_jpeg
    files = [jpeg_encode.encode_rule(p, spec.quality, spec.subsampling) for p in pics]
    return jpeg_encode.pack_rows(k, score, heat, files, _jpeg_cap(sig, src))


def _map_words(sig, src) -> int:
    return 2 + sig.explain[0] * sig.explain[1] + (overlay_words(sig.overlay) if sig.overlay else 0)


def _is_palette(sig) -> bool:
    """An explain-kind signature with a ``fractions`` output answers colours."""
    return bool(sig.explain and any(o[0] == "fractions" for o in sig.outputs))


def _palette_k(sig) -> int:
    return next(o[2][1] for o in sig.outputs if o[0] == "fractions")


def _palette_words(sig, src) -> int:
    return 2 + sig.explain[0] * sig.explain[1] + 1 + 2 * _palette_k(sig)


def _is_locate(sig) -> bool:
    """An explain-kind signature with a ``boxes`` output answers regions."""
    return bool(sig.explain and any(o[0] == "boxes" for o in sig.outputs))


def _locate_k(sig) -> int:
    return next(o[2][1] for o in sig.outputs if o[0] == "boxes")


def _locate_words(sig, src) -> int:
    return 2 + sig.explain[0] * sig.explain[1] + 1 + 3 * _locate_k(sig)


def _is_cutout(sig) -> bool:
    """An explain-kind signature with a ``coverage`` output answers the picture with an alpha channel."""
    return bool(sig.explain and any(o[0] == "coverage" for o in sig.outputs))


def _cutout_s(sig) -> int:
    return next(o[2][1] for o in sig.outputs if o[0] == "cutout")


def _cutout_words(sig, src) -> int:
    return 2 + sig.explain[0] * sig.explain[1] + 1 + _cutout_s(sig) ** 2


def _is_jpeg(sig) -> bool:
    """An overlay signature whose last output is a DT_STRING answers the picture as a file."""
    return bool(sig.overlay and sig.outputs and sig.outputs[-1][1] == P.DT_STRING)


def _jpeg_cap(sig, src) -> int:
    return overlay_jpeg_cap(sig.overlay, src.overlay_jpeg.max_bytes)


def _jpeg_words(sig, src) -> int:
    return 2 + sig.explain[0] * sig.explain[1] + 1 + (_jpeg_cap(sig, src) + 3) // 4


# ---------------------------------------------------------------------- named output columns
def _ranked(names: Callable):
    def columns(src, sig, rows) -> list:
        idx, scores = classify.unpack_rows(rows)
        return [(sig.output_key, P.DT_STRING, names(src, idx)), ("scores", P.DT_FLOAT, scores)]
    return columns


def _front_columns(src, classes, scores, heat) -> list:
    """A class index outside the label list (the null device's rows) is answered as its decimal."""
    lab = src.labels
    return [("classes", P.DT_STRING, [[lab[int(c)] if 0 <= int(c) < len(lab) else str(int(c))] for c in classes]),
            ("scores", P.DT_FLOAT, scores.reshape(-1, 1)), ("heatmap", P.DT_FLOAT, heat)]


def _map_columns(src, sig, rows) -> list:
    if sig.overlay:
        classes, scores, heat, pics = overlay.unpack_rows(rows, *sig.explain, sig.overlay)
    else:
        classes, scores, heat = explain.unpack_rows(rows, *sig.explain)
    cols = _front_columns(src, classes, scores, heat)
    return cols + [("overlay", P.DT_UINT8, pics)] if sig.overlay else cols


def _jpeg_columns(src, sig, rows) -> list:
    """The map's three outputs and each row's file; a row whose file did not fit answers b""."""
    classes, scores, heat, files = jpeg_encode.unpack_rows(rows, *sig.explain, _jpeg_cap(sig, src))
    lost = sum(not f for f in files)
    if lost:
        METRICS.inc("kdl_overlay_jpeg_overflow_total", lost, signature=sig.name)
    return _front_columns(src, classes, scores, heat) + [("jpeg_bytes", P.DT_STRING, files)]


def _palette_columns(src, sig, rows) -> list:
    classes, scores, heat, totals, colours, weights = palette.unpack_rows(rows, *sig.explain, _palette_k(sig))
    return _front_columns(src, classes, scores, heat)[:2] + [
        ("colors", P.DT_UINT8, colours), ("fractions", P.DT_FLOAT, palette.fractions_of(weights, totals)),
        ("names", P.DT_STRING, palette.names_of(colours))]


def _locate_columns(src, sig, rows) -> list:
    classes, scores, heat, counts, boxes, areas = locate.unpack_rows(rows, *sig.explain, _locate_k(sig))
    S = src.input_size
    return _front_columns(src, classes, scores, heat)[:2] + [
        ("boxes", P.DT_FLOAT, locate.boxes_of(boxes, S)), ("areas", P.DT_FLOAT, locate.areas_of(areas, S)),
        ("num_boxes", P.DT_INT32, counts.astype(np.int32).reshape(-1, 1))]


def _cutout_columns(src, sig, rows) -> list:
    S = _cutout_s(sig)
    classes, scores, heat, counts, pics = cutout.unpack_rows(rows, *sig.explain, S)
    return _front_columns(src, classes, scores, heat)[:2] + [
        ("cutout", P.DT_UINT8, pics), ("coverage", P.DT_FLOAT, cutout.coverage_of(counts, S).reshape(-1, 1))]


@dataclass(frozen=True)
class Kind:
    name: str
    trio: tuple
    counter: str = ""
    engine: Callable = lambda sig, src, dev: {}
    gpu_words: Callable = lambda sig, src: src.classes
    host_words: Callable | None = None
    cpu_rows: Callable = _logit_rows
    host_step: Callable | None = None
    null_zero: bool = False
    columns: Callable | None = None


_MAP = dict(engine=_map_kw, gpu_words=_map_words, cpu_rows=_map_rows, null_zero=True, columns=_map_columns)
KINDS = {k.name: k for k in (
    Kind("logits", (NATIVE_SIGNATURE, IMAGE_SIGNATURE, BYTES_SIGNATURE)),
    Kind("classify", classify.CLASSIFY_SIGNATURES, "kdl_classify_total",
         engine=lambda sig, src, dev: dict(topk=sig.top_k), gpu_words=lambda sig, src: 2 * sig.top_k,
         host_words=lambda sig, src: src.classes,
         host_step=lambda sig, src, rows: classify.pack_rows(*classify.topk_rule(rows, sig.top_k)),
         columns=_ranked(classify.labels_of)),
    Kind("embed", embed.EMBED_SIGNATURES, "kdl_embed_total",
         engine=lambda sig, src, dev: dict(embed=sig.embed), gpu_words=lambda sig, src: sig.output_shape[1],
         cpu_rows=_feature_rows),
    Kind("similar", similar.SIMILAR_SIGNATURES, "kdl_similar_total",
         engine=_similar_kw, gpu_words=lambda sig, src: 2 * sig.top_k,
         host_words=lambda sig, src: src.gallery.shape[1], cpu_rows=_feature_rows,
         host_step=lambda sig, src, rows: classify.pack_rows(
             *similar.similar_rule(rows, src.gallery, sig.top_k, src.similar_metric)),
         columns=_ranked(similar.ids_of)),
    Kind("explain", explain.EXPLAIN_SIGNATURES, "kdl_explain_total", **_MAP),
    Kind("attention", rollout.ATTENTION_SIGNATURES, "kdl_attention_total", **_MAP),
    Kind("overlay", overlay.OVERLAY_SIGNATURES, "kdl_overlay_total", **_MAP),
    Kind("overlay_jpeg", jpeg_encode.OVERLAY_JPEG_SIGNATURES, "kdl_overlay_jpeg_total",
         **dict(_MAP, engine=_jpeg_kw, gpu_words=_jpeg_words, columns=_jpeg_columns)),
    Kind("palette", palette.PALETTE_SIGNATURES, "kdl_palette_total",
         **dict(_MAP, engine=_palette_kw, gpu_words=_palette_words, columns=_palette_columns)),
    Kind("locate", locate.LOCATE_SIGNATURES, "kdl_locate_total",
         **dict(_MAP, engine=_locate_kw, gpu_words=_locate_words, columns=_locate_columns)),
)}
CUTOUT = Kind("cutout", cutout.CUTOUT_SIGNATURES, "kdl_cutout_total",
              **dict(_MAP, engine=_cutout_kw, gpu_words=_cutout_words, columns=_cutout_columns))
# the second and third name of every trio -> (0 any-size image / 1 encoded file, the trio's first name)
WRAPPED = {name: (i, k.trio[0]) for k in (*KINDS.values(), CUTOUT) for i, name in enumerate(k.trio[1:])}


def kind_of(sig) -> Kind:
    """The kind of a signature's rows, from the fields SignatureInfo has."""
    if _is_cutout(sig):
        return CUTOUT
    name = ("locate" if _is_locate(sig) else "palette" if _is_palette(sig) else "overlay_jpeg" if _is_jpeg(sig) else "overlay" if sig.overlay else "attention" if sig.explain and sig.rollout else
            "explain" if sig.explain else "similar" if sig.similar else "classify" if sig.top_k else
            "embed" if sig.embed else "logits")
    return KINDS[name]


def engine_kwargs(sig, src, device) -> dict:
    return kind_of(sig).engine(sig, src, device)


def out_cols(sig, src, gpu: bool) -> int:
    """32-bit words per result row, from the executor to the waiting handler."""
    k = kind_of(sig)
    return (k.gpu_words if gpu or k.host_words is None else k.host_words)(sig, src)


def cpu_rows(sig, src, x) -> torch.Tensor:
    return torch.as_tensor(kind_of(sig).cpu_rows(sig, src, x))


def host_rows(sig, src, rows: np.ndarray, null: bool) -> np.ndarray:
    """The answer's packed rows from what a CPU or null executor returned."""
    k = kind_of(sig)
    if null and k.null_zero:
        return np.zeros_like(rows)
    return rows if k.host_step is None else k.host_step(sig, src, rows)


def answered(sig) -> None:
    """Count one answered request of the signature's kind."""
    k = kind_of(sig)
    if k.counter:
        METRICS.inc(k.counter, signature=sig.name)


def columns(src, sig, rows):
    """The named outputs of an answered request (counted here), or None for a kind whose single fp32
    output is the rows themselves."""
    k = kind_of(sig)
    if k.columns is None:
        return None
    answered(sig)
    return k.columns(src, sig, rows)


# ---------------------------------------------------------------------- loading
def _meta(path: Path) -> tuple[dict, str]:
    """(the version's kdl_model.json / synthetic.json, its file name)."""
    for name in ("kdl_model.json", "synthetic.json"):
        if (path / name).exists():
            return json.loads((path / name).read_text()), name
    return {}, "kdl_model.json"


def add_trio(src, names, output_key: str, output_shape: tuple, **fields) -> None:
    """The trio ``names`` = (uint8 pixels, any-size image, encoded file) beside the source's
    ``serving_uint8`` / ``serving_image`` / ``serving_bytes``: each takes its base's input, a
    missing base or an existing name is skipped."""
    from .backend import SignatureInfo
    S = src.input_size
    for name, base in zip(names, KINDS["logits"].trio):
        b = src.signatures.get(base)
        if b is None or name in src.signatures:
            continue
        key = b.input_key if b.input_dtype != P.DT_FLOAT else NATIVE_INPUT_KEY
        shape = b.input_shape if name != names[0] else (-1, S, S, 3)
        src.signatures[name] = SignatureInfo(name, key, b.input_dtype, output_key, input_shape=shape,
                                             output_shape=output_shape, **fields)
