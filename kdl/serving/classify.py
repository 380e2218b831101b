"""Classification outputs: the ``classify`` / ``classify_image`` / ``classify_bytes`` signatures.

Each answers with the top-K classes (label strings) and their softmax scores instead of the
raw logits. On a GPU the K indices and scores come out of the captured program itself
(``EngineBase(topk=K)``, kernels/classify.hip: 2K words per image cross the PCIe link instead of
``classes`` floats); CPU and ``--device null`` servers apply the same rule to their logits in
numpy (``topk_rule``). The rule: classes by descending logit, equal logits by ascending index
(TF ``top_k``), score_i = exp(x_i - max) / sum_j exp(x_j - max) over all logits.

K comes from the version's ``kdl_model.json`` / ``synthetic.json`` key ``"classify": {"top_k": K}``,
overridden by ``--classify_top_k``; default 5, clipped to the class count. Labels come from
``labels.txt`` in the version directory (one per line, as many as classes), else ``"labels"`` in
``kdl_model.json``, else the decimal class index. The TF-Serving ``Classify`` RPC and REST
``:classify`` (tf.Example input) are served by the ``classify_bytes`` signature: each example
carries one encoded image under the feature ``image/encoded`` (``"classify": {"feature": ...}``).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from . import protos as P

CLASSIFY_SIGNATURE = "classify"
CLASSIFY_IMAGE_SIGNATURE = "classify_image"
CLASSIFY_BYTES_SIGNATURE = "classify_bytes"
CLASSIFY_SIGNATURES = (CLASSIFY_SIGNATURE, CLASSIFY_IMAGE_SIGNATURE, CLASSIFY_BYTES_SIGNATURE)
DEFAULT_TOP_K = 5
MAX_TOP_K = 32                     # kTopkMaxK of kernels/launch.h
DEFAULT_FEATURE = "image/encoded"


def topk_rule(logits: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """fp32 logits [n, classes] -> (classes int32 [n, k], scores fp32 [n, k])."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    order = np.argsort(-x, axis=1, kind="stable")[:, :k]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return order.astype(np.int32), np.take_along_axis(p, order, axis=1).astype(np.float32)


def pack_rows(classes: np.ndarray, scores: np.ndarray) -> np.ndarray:
    """The engine's row layout: K int32 indices then K fp32 scores, in a float32 container."""
    return np.concatenate([np.ascontiguousarray(classes, dtype=np.int32).view(np.float32),
                           np.ascontiguousarray(scores, dtype=np.float32)], axis=1)


def unpack_rows(rows: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    k = rows.shape[1] // 2
    return np.ascontiguousarray(rows[:, :k]).view(np.int32), np.ascontiguousarray(rows[:, k:])


def resolve(path: Path, classes: int, top_k_flag: int | None = None) -> tuple[int, str, list[str]]:
    """(K, tf.Example feature key, labels) of the version in ``path``; ValueError fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, _ = _meta(path)
    spec = meta.get("classify", {})
    if not isinstance(spec, dict):
        raise ValueError(f"{path}: \"classify\" must be an object like {{\"top_k\": 5}}")
    k = top_k_flag if top_k_flag is not None else spec.get("top_k", DEFAULT_TOP_K)
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > MAX_TOP_K:
        raise ValueError(f"{path}: classify top_k must be an integer in 1..{MAX_TOP_K}, got {k!r}")
    feature = spec.get("feature", DEFAULT_FEATURE)
    if not isinstance(feature, str) or not feature:
        raise ValueError(f"{path}: classify feature must be a non-empty string, got {feature!r}")
    if (path / "labels.txt").exists():
        labels = (path / "labels.txt").read_text().splitlines()
        where = "labels.txt"
    elif (path / "kdl_model.json").exists() and "labels" in meta:
        labels, where = meta["labels"], "\"labels\" of kdl_model.json"
        if not isinstance(labels, list) or not all(isinstance(v, str) for v in labels):
            raise ValueError(f"{path}: \"labels\" must be a list of strings")
    else:
        labels, where = [str(i) for i in range(classes)], ""
    if len(labels) != classes:
        raise ValueError(f"{path}: {where} has {len(labels)} labels, the model has {classes} classes")
    return min(k, classes), feature, list(labels)


def add_signatures(src, path: Path, top_k_flag: int | None = None) -> None:
    """Give a loaded ModelSource its three classify signatures (beside the existing ones)."""
    from .outputs import add_trio
    k, feature, labels = resolve(path, src.classes, top_k_flag)
    src.labels, src.classify_k, src.classify_feature = labels, k, feature
    outs = (("classes", P.DT_STRING, (-1, k)), ("scores", P.DT_FLOAT, (-1, k)))
    add_trio(src, CLASSIFY_SIGNATURES, "classes", (-1, k), outputs=outs, top_k=k)


def labels_of(src, classes: np.ndarray) -> list[list[str]]:
    lab = src.labels
    return [[lab[int(c)] for c in row] for row in classes]


def examples_to_images(examples, feature: str) -> list[bytes]:
    """The encoded image of every tf.Example; ServingError INVALID_ARGUMENT names the bad index."""
    from .backend import ServingError
    images = []
    for i, ex in enumerate(examples):
        f = ex.features.feature.get(feature)
        if f is None:
            raise ServingError("INVALID_ARGUMENT", f"example {i}: feature '{feature}' is missing")
        if f.WhichOneof("kind") != "bytes_list":
            raise ServingError("INVALID_ARGUMENT", f"example {i}: feature '{feature}' must be a bytes_list")
        if len(f.bytes_list.value) != 1:
            raise ServingError("INVALID_ARGUMENT", f"example {i}: feature '{feature}' must hold exactly one "
                               f"bytes value, got {len(f.bytes_list.value)}")
        images.append(bytes(f.bytes_list.value[0]))
    return images
