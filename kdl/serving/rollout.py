"""Attention-rollout outputs: the ``attention`` / ``attention_image`` / ``attention_bytes`` signatures.

ViT's answer to "where did the model look?". Grad-CAM (serving/explain.py) needs a spatial feature map
in front of the head; a class-token head has none, so the two ViT families answer with attention
rollout instead (Abnar & Zuidema 2020): per layer the head-averaged attention probabilities with the
identity added for the residual path, A^ = (mean_h P_h + I) / 2, multiplied through the twelve layers;
the map is the class token's row of the product over the 14 x 14 patches, divided by its largest
value. The outputs are explain's: ``classes`` DT_STRING [-1, 1], ``scores`` DT_FLOAT [-1, 1] and
``heatmap`` DT_FLOAT [-1, 14, 14], from the same packed rows [class, score, 196 values], so the
response and body builders are explain's own. On a GPU the rows come out of the captured program
(``ViTEngine(rollout=True)``, kernels/rollout.hip); CPU servers run ``ModelInfo.rollout_oracle``; the
null device answers zero rows. A family without a ``rollout_oracle`` (the CNNs) has no attention
signatures, as ViT has no explain signatures.
"""
from __future__ import annotations

from .explain import map_outputs, pack_rows, unpack_rows  # noqa: F401  (the row layout is shared)

ATTENTION_SIGNATURE = "attention"
ATTENTION_IMAGE_SIGNATURE = "attention_image"
ATTENTION_BYTES_SIGNATURE = "attention_bytes"
ATTENTION_SIGNATURES = (ATTENTION_SIGNATURE, ATTENTION_IMAGE_SIGNATURE, ATTENTION_BYTES_SIGNATURE)


def add_signatures(src, path=None) -> None:
    """Give a loaded ModelSource its three attention signatures (beside the existing ones), when its
    family has a ``rollout_oracle``."""
    from ..engine import registry
    from .outputs import add_trio
    info = registry.get(src.family)
    if info.rollout_oracle is not None:
        add_trio(src, ATTENTION_SIGNATURES, "classes", (-1, 1), outputs=map_outputs(*info.map_size),
                 explain=tuple(info.map_size), rollout=True)
