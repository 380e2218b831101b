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


def map_outputs(h: int, w: int) -> tuple:
    """The three outputs of a heatmap method with an h x w map (explain's, attention's, and the
    front of overlay's)."""
    return (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)), ("heatmap", P.DT_FLOAT, (-1, h, w)))


def add_signatures(src, path=None) -> None:
    """Give a loaded ModelSource its three explain signatures (beside the existing ones), when its
    family has a ``cam_oracle``."""
    from ..engine import registry
    from .outputs import add_trio
    info = registry.get(src.family)
    if info.cam_oracle is not None:
        add_trio(src, EXPLAIN_SIGNATURES, "classes", (-1, 1), outputs=map_outputs(*info.map_size),
                 explain=tuple(info.map_size))
