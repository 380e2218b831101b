"""Embedding outputs: the ``embed`` / ``embed_image`` / ``embed_bytes`` signatures.

Each answers with the pooled feature vector in front of the model's head instead of its logits:
one output ``embedding``, DT_FLOAT [-1, F] (Xception and ResNet-50 2048, EfficientNet-B7 2560,
ViT-B/16 768: the normalised class token). It is what Keras ``pooling="avg"`` gives, the vector
a new head is trained on, and what similarity search and de-duplication compare. On a GPU the
rows come out of the captured program itself (``EngineBase(embed=...)``, kernels/embed.hip); CPU
servers return the family's fp32 ``feature_oracle`` rows, normalised in numpy by the same rule.

Normalisation comes from the version's ``kdl_model.json`` / ``synthetic.json`` key
``"embedding": {"normalize": "none" | "l2"}``, overridden by ``--embedding_normalize``; default
``none``. ``l2`` divides each row by max(its L2 norm, 1e-12) (``torch.nn.functional.normalize``).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np


EMBED_SIGNATURE = "embed"
EMBED_IMAGE_SIGNATURE = "embed_image"
EMBED_BYTES_SIGNATURE = "embed_bytes"
EMBED_SIGNATURES = (EMBED_SIGNATURE, EMBED_IMAGE_SIGNATURE, EMBED_BYTES_SIGNATURE)
OUTPUT_KEY = "embedding"
NORMALIZE = ("none", "l2")
ENGINE_MODE = {"none": "raw", "l2": "l2"}        # "normalize" value -> EngineBase(embed=...)


def l2_rule(rows: np.ndarray) -> np.ndarray:
    """fp32 rows [n, F] -> each divided by max(its L2 norm, 1e-12), in float64, as fp32."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    n = np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return (x / n).astype(np.float32)


def resolve(path: Path, normalize_flag: str | None = None) -> str:
    """"none" or "l2" for the version in ``path``; ValueError (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    spec = meta.get("embedding", {})
    if not isinstance(spec, dict):
        raise ValueError(f"{path / name}: \"embedding\" must be an object like {{\"normalize\": \"l2\"}}")
    if normalize_flag:
        if normalize_flag not in NORMALIZE:
            raise ValueError(f"--embedding_normalize must be one of {NORMALIZE}, got {normalize_flag!r}")
        return normalize_flag
    norm = spec.get("normalize", "none")
    if not isinstance(norm, str) or norm not in NORMALIZE:
        raise ValueError(f"{path / name}: embedding normalize must be one of {NORMALIZE}, got {norm!r}")
    return norm


def add_signatures(src, path: Path, normalize_flag: str | None = None) -> None:
    """Give a loaded ModelSource its three embed signatures (beside the existing ones)."""
    from ..engine import registry
    from .outputs import add_trio
    norm = resolve(path, normalize_flag)
    F = src.head.features if src.head is not None else registry.get(src.family).features
    src.embed_normalize, src.embed_dim = norm, F
    add_trio(src, EMBED_SIGNATURES, OUTPUT_KEY, (-1, F), embed=ENGINE_MODE[norm])
