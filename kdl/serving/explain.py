"""Grad-CAM outputs: the ``explain`` / ``explain_image`` / ``explain_bytes`` signatures.

Each answers the question after a prediction, "which part of the picture made the model say
that?": the predicted class (``classes`` DT_STRING [-1, 1], the label ``classify`` resolves), its
softmax score (``scores`` DT_FLOAT [-1, 1]) and the class's Grad-CAM map over the last feature map
(``heatmap`` DT_FLOAT [-1, h, w]: 10 x 10 for Xception's block14_sepconv2_act, 7 x 7 for ResNet-50's
layer4, 19 x 19 for EfficientNet-B7's features.8), as the keras.io Grad-CAM example defines it:
max(sum_c alpha_c A[p][c], 0) divided by its largest value, all zeros when that is 0. Upsampling
and colouring are the client's job. On a GPU the rows come out of the captured program itself
(``EngineBase(explain=True)``, kernels/explain.hip: the gradient in closed form, no backward pass);
CPU servers run ``torch.autograd`` through the family's own head (``ModelInfo.cam_oracle``); the
null device answers zero rows. A family without a spatial map in front of its head (ViT) has no
explain signatures.
"""
from __future__ import annotations

import numpy as np

from . import protos as P

EXPLAIN_SIGNATURE = "explain"
EXPLAIN_IMAGE_SIGNATURE = "explain_image"
EXPLAIN_BYTES_SIGNATURE = "explain_bytes"
EXPLAIN_SIGNATURES = (EXPLAIN_SIGNATURE, EXPLAIN_IMAGE_SIGNATURE, EXPLAIN_BYTES_SIGNATURE)
OUTPUT_KEYS = ("classes", "scores", "heatmap")


def pack_rows(classes, scores, heat) -> np.ndarray:
    """The engine's row layout, [n, 2 + h*w] fp32 words: the class (int32 bits), the score, the map."""
    from ..engine.base import pack_explain
    return pack_explain(classes, scores, heat)


def unpack_rows(rows, h: int, w: int) -> tuple:
    """-> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w])."""
    from ..engine.base import unpack_explain
    return unpack_explain(np.ascontiguousarray(rows, dtype=np.float32), h, w)


def add_signatures(src, path=None) -> None:
    """Give a loaded ModelSource its three explain signatures (beside the existing ones), when its
    family has a ``cam_oracle``."""
    from ..engine import registry
    info = registry.get(src.family)
    if info.cam_oracle is None:
        return
    add_map_signatures(src, EXPLAIN_SIGNATURES, info.map_size)


def add_map_signatures(src, names, hw, rollout: bool = False) -> None:
    """The trio ``names`` = (uint8 pixels, any-size image, encoded file) of a heatmap method with an
    h x w map, beside the source's existing signatures. ``rollout`` marks the attention signatures
    (serving/rollout.py); rows, responses and bodies are the same for both methods."""
    from .backend import NATIVE_INPUT_KEY, NATIVE_SIGNATURE, SignatureInfo
    from .jpeg import BYTES_SIGNATURE
    from .resize import IMAGE_SIGNATURE
    h, w = hw
    S = src.input_size
    outs = (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)), ("heatmap", P.DT_FLOAT, (-1, h, w)))
    like = dict(zip(names, (NATIVE_SIGNATURE, IMAGE_SIGNATURE, BYTES_SIGNATURE)))
    for name, base in like.items():
        b = src.signatures.get(base)
        if b is None or name in src.signatures:
            continue
        key = b.input_key if b.input_dtype != P.DT_FLOAT else NATIVE_INPUT_KEY
        shape = b.input_shape if name != names[0] else (-1, S, S, 3)
        kw = dict(rollout=True) if rollout else {}
        src.signatures[name] = SignatureInfo(name, key, b.input_dtype, "classes", input_shape=shape,
                                             output_shape=(-1, 1), outputs=outs, explain=(h, w), **kw)


def explain_outputs(s, sig, rows) -> tuple:
    """Packed rows of an explain signature -> (labels [n], scores fp32 [n], heat fp32 [n, h, w]).
    A class index outside the label list (the null device's rows) is answered as its decimal."""
    from .metrics import METRICS
    classes, scores, heat = unpack_rows(rows, *sig.explain)
    METRICS.inc("kdl_attention_total" if sig.rollout else "kdl_explain_total", signature=sig.name)
    lab = s.source.labels
    return [lab[int(c)] if 0 <= int(c) < len(lab) else str(int(c)) for c in classes], scores, heat


def explain_response(s, sig, rows, output_filter) -> bytes:
    """PredictResponse of an explain signature: ``classes`` DT_STRING [n, 1], ``scores`` DT_FLOAT
    [n, 1] and ``heatmap`` DT_FLOAT [n, h, w], or the subset ``output_filter`` names."""
    labels, scores, heat = explain_outputs(s, sig, rows)
    n, (h, w) = len(labels), sig.explain
    resp = P.PredictResponse()
    resp.model_spec.name = s.name
    resp.model_spec.version.value = s.version
    resp.model_spec.signature_name = sig.name
    want = list(output_filter) or list(OUTPUT_KEYS)
    if "classes" in want:
        t = resp.outputs["classes"]
        t.dtype = P.DT_STRING
        t.string_val.extend(name.encode() for name in labels)
    if "scores" in want:
        t = resp.outputs["scores"]
        t.dtype = P.DT_FLOAT
        t.float_val.extend(scores.reshape(-1).tolist())
    if "heatmap" in want:
        t = resp.outputs["heatmap"]
        t.dtype = P.DT_FLOAT
        t.float_val.extend(heat.reshape(-1).tolist())
    for key in resp.outputs:
        for d in ((n, h, w) if key == "heatmap" else (n, 1)):
            resp.outputs[key].tensor_shape.dim.add(size=d)
    return resp.SerializeToString()


def explain_body(s, sig, rows, by_row: bool) -> dict:
    """REST ``:predict`` answer of an explain signature, per instance or by column."""
    labels, scores, heat = explain_outputs(s, sig, rows)
    if by_row:
        return {"predictions": [{"classes": [c], "scores": [float(v)], "heatmap": m.tolist()}
                                for c, v, m in zip(labels, scores, heat)]}
    return {"outputs": {"classes": [[c] for c in labels], "scores": [[float(v)] for v in scores],
                        "heatmap": heat.tolist()}}
