"""Gallery search: the ``similar`` / ``similar_image`` / ``similar_bytes`` signatures.

Each answers with the K stored items nearest to the image: ``ids`` DT_STRING [-1, K] and ``scores``
DT_FLOAT [-1, K], best first. The stored items are the version's *gallery*: one pooled feature
vector per catalogue item (what the ``embed`` signatures return), kept next to the weights. On a
GPU the gallery lives on the device, once per (version, device), and the scan and the ranking
run inside the captured program (``EngineBase(similar=...)``, kernels/similar.hip): 2K words per
image cross the PCIe link. CPU and ``--device null`` servers apply ``similar_rule`` to their
``feature_oracle`` rows in numpy. The signatures exist only when the version has a gallery.

Files in the version directory: ``gallery.npy``, float32 or float16 [N, F] in C order (loaded with
``allow_pickle=False``), F the family's feature count; optionally ``gallery_ids.txt``, N lines,
else the ids are the decimal row indices. ``python -m kdl.cli build-gallery`` writes both.
Configuration: ``"similar": {"top_k": 5, "metric": "cosine" | "dot", "gallery": "gallery.npy"}`` in
``kdl_model.json`` / ``synthetic.json``; ``--similar_top_k`` overrides K, which is clipped to N.

The rule. ``load_gallery`` defines the stored values: for cosine each row is divided in float64 by
max(its L2 norm, 1e-12); the rows are cast to fp32 and rounded to bf16 (nearest even). score[j] =
sum_i q_i * g_ji with the query as fp32 (for cosine L2-normalised first, ``embed.l2_rule``) and the
bf16 values as they stand; rows rank by descending score, equal scores by ascending row index."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from . import protos as P

SIMILAR_SIGNATURE = "similar"
SIMILAR_IMAGE_SIGNATURE = "similar_image"
SIMILAR_BYTES_SIGNATURE = "similar_bytes"
SIMILAR_SIGNATURES = (SIMILAR_SIGNATURE, SIMILAR_IMAGE_SIGNATURE, SIMILAR_BYTES_SIGNATURE)
DEFAULT_TOP_K = 5
MAX_TOP_K = 32                     # kTopkMaxK of kernels/launch.h
GALLERY_MAX_N = 1 << 24            # kGalleryMaxN of kernels/launch.h
METRICS = ("cosine", "dot")
DEFAULT_GALLERY = "gallery.npy"
IDS_FILE = "gallery_ids.txt"


def bf16_to_f64(bits: np.ndarray) -> np.ndarray:
    """uint16 bf16 patterns -> the values they stand for, as float64."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def load_gallery(path: Path, features: int, metric: str = "cosine") -> np.ndarray:
    """The stored values of the gallery file ``path`` as uint16 bf16 patterns [N, F], C order.
    ValueError (naming the file) for anything but a finite float32 / float16 [N, features] array
    with 1 <= N <= GALLERY_MAX_N."""
    import torch
    path = Path(path)
    if metric not in METRICS:
        raise ValueError(f"similar metric must be one of {METRICS}, got {metric!r}")
    try:
        a = np.load(path, allow_pickle=False)
    except Exception as e:  # noqa: BLE001 - a missing, truncated or pickled file
        raise ValueError(f"{path}: cannot be read as a .npy array ({e})") from e
    if not isinstance(a, np.ndarray) or a.dtype not in (np.float32, np.float16):
        raise ValueError(f"{path}: must be a float32 or float16 array, got {getattr(a, 'dtype', type(a))}")
    if a.ndim != 2 or a.shape[1] != features:
        raise ValueError(f"{path}: must be [N, {features}] (the model's feature count), got {list(a.shape)}")
    if a.shape[0] < 1:
        raise ValueError(f"{path}: the gallery has no rows")
    if a.shape[0] > GALLERY_MAX_N:
        raise ValueError(f"{path}: {a.shape[0]} rows exceed the kernel's {GALLERY_MAX_N}")
    if not np.isfinite(a).all():
        raise ValueError(f"{path}: the gallery holds NaN or infinite values")
    x = a.astype(np.float64)
    if metric == "cosine":
        x = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    bits = torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    if not np.isfinite(bf16_to_f64(bits)).all():
        raise ValueError(f"{path}: a value is too large for bf16")
    return np.ascontiguousarray(bits)


def similar_rule(features_fp32: np.ndarray, gallery_bf16: np.ndarray, k: int,
                 metric: str = "cosine") -> tuple[np.ndarray, np.ndarray]:
    """fp32 feature rows [n, F] and the gallery's bf16 patterns [N, F] -> (row indices int32 [n, k],
    scores fp32 [n, k]): float64 scores, ranked by a stable argsort of their negation."""
    q = np.asarray(features_fp32, dtype=np.float32)
    if metric == "cosine":
        from .embed import l2_rule
        q = l2_rule(q)
    s = q.astype(np.float64) @ bf16_to_f64(gallery_bf16).T
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(s, order, axis=1).astype(np.float32)


def resolve(path: Path, features: int, top_k_flag: int | None = None):
    """None for a version without a gallery, else (K, metric, bf16 patterns [N, F], ids [N]) of the
    version in ``path``; ValueError (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    spec = meta.get("similar", {})
    if not isinstance(spec, dict):
        raise ValueError(f"{path / name}: \"similar\" must be an object like {{\"top_k\": 5, \"metric\": \"cosine\"}}")
    gname = spec.get("gallery", DEFAULT_GALLERY)
    if not isinstance(gname, str) or not gname or Path(gname).name != gname:
        raise ValueError(f"{path / name}: similar gallery must be a file name in the version directory, got {gname!r}")
    if not (path / gname).exists():
        if "gallery" in spec:
            raise ValueError(f"{path / gname}: the gallery named in {name} does not exist")
        return None
    k = top_k_flag if top_k_flag is not None else spec.get("top_k", DEFAULT_TOP_K)
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > MAX_TOP_K:
        raise ValueError(f"{path / name}: similar top_k must be an integer in 1..{MAX_TOP_K}, got {k!r}")
    metric = spec.get("metric", "cosine")
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError(f"{path / name}: similar metric must be one of {METRICS}, got {metric!r}")
    bits = load_gallery(path / gname, features, metric)
    n = bits.shape[0]
    if (path / IDS_FILE).exists():
        ids = (path / IDS_FILE).read_text().splitlines()
        if len(ids) != n:
            raise ValueError(f"{path / IDS_FILE}: {len(ids)} ids for the {n} rows of {gname}")
    else:
        ids = [str(i) for i in range(n)]
    return min(k, n), metric, bits, ids


def add_signatures(src, path: Path, top_k_flag: int | None = None) -> None:
    """Give a loaded ModelSource with a gallery its three similar signatures (beside the others)."""
    from ..engine import registry
    from .outputs import add_trio
    F = src.head.features if src.head is not None else registry.get(src.family).features
    got = resolve(path, F, top_k_flag)
    if got is None:
        return
    k, src.similar_metric, src.gallery, src.gallery_ids = got
    src.similar_k = k
    outs = (("ids", P.DT_STRING, (-1, k)), ("scores", P.DT_FLOAT, (-1, k)))
    add_trio(src, SIMILAR_SIGNATURES, "ids", (-1, k), outputs=outs, top_k=k, similar=True)


def ids_of(src, rows: np.ndarray) -> list[list[str]]:
    ids = src.gallery_ids           # (NaN features give unspecified rows: an index out of range names nothing)
    return [[ids[int(j)] if 0 <= int(j) < len(ids) else "" for j in row] for row in rows]


def device_gallery(src, device):
    """The version's gallery as a bf16 tensor on ``device``: one copy per (version, device), shared
    by every engine there."""
    import torch
    dev = torch.device(device)
    with src.gallery_lock:
        t = src.gallery_device.get(dev)
        if t is None:
            t = torch.from_numpy(src.gallery.view(np.int16)).to(dev).view(torch.bfloat16)
            src.gallery_device[dev] = t
        return t
