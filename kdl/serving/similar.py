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
``"dtype": "bf16" | "fp8"`` in the same block (``--similar_dtype`` / ``KDL_SIMILAR_DTYPE`` overrides
it, default bf16) chooses how the rows are stored; the gallery file is the same for both.

The rule. ``load_gallery`` defines the stored values: for cosine each row is divided in float64 by
max(its L2 norm, 1e-12); the rows are cast to fp32 and rounded to bf16 (nearest even). score[j] =
sum_i q_i * g_ji with the query as fp32 (for cosine L2-normalised first, ``embed.l2_rule``) and the
bf16 values as they stand; rows rank by descending score, equal scores by ascending row index.

The fp8 rule. ``load_gallery_fp8`` stores one byte per value and one fp32 scale per row
(``quantize_fp8``): rows normalised in float64 as above; s_j = fp32(max_i |x_ji| / 448), 1.0 for an
all-zero row; e_ji the OCP e4m3 code nearest to x_ji / s_j (the quotient taken in float64, cast
to fp32, clipped to +-448, then torch's round-to-nearest-even ``float8_e4m3fn`` cast, which does
not saturate by itself), never a NaN code (0x7F, 0xFF). score[j] = s_j * sum_i q_i * val(e_ji),
query and ranking as above; every e4m3 value is a bf16 value, so the GPU scan
(kernels/similar_f8.hip) keeps the exact-query arithmetic of the bf16 one at half the bytes.

The index. A version may carry an inverted-file index over its (bf16) gallery, so that a query is
scored against a few lists of rows instead of all of them: ``gallery_centroids.npy``, float32
[L, F], and ``gallery_lists.npy``, int32 [N] with the list 0..L-1 of each row (``build-gallery
--ivf_lists L`` writes both: ``build_ivf``, spherical k-means in numpy). ``"similar": {"index":
"ivf", "nprobe": 8, "centroids": ..., "lists": ...}`` turns it on; ``--similar_nprobe`` overrides
``nprobe``, 1 <= nprobe <= min(L, 32); without ``"index"`` every row is scanned as before. An fp8
gallery cannot have an index. ``load_ivf`` defines the stored form: the rows (and their ids) are
stably sorted by list, so a list is a run of stored positions in ascending original row order,
``offsets`` int32 [L + 1] says where each starts, and the centroids are normalised (cosine) and
rounded to bf16 as ``load_gallery`` does rows. ``ivf_rule``: the coarse score of a list is q .
centroid; the probed lists are the ``nprobe`` best by (score descending, list ascending); the
candidates are their rows, ranked by (q . g_j descending, stored position ascending); when they
are fewer than K the missing places are index -1 (id "") with score -inf. On a GPU both stages run
inside the captured program (``Similar(ivf=...)``, kernels/similar_ivf.hip)."""
from __future__ import annotations

from dataclasses import dataclass
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
DTYPES = ("bf16", "fp8")
FP8_MAX = 448.0                    # the largest e4m3 value
DEFAULT_GALLERY = "gallery.npy"
IDS_FILE = "gallery_ids.txt"
CENTROIDS_FILE = "gallery_centroids.npy"
LISTS_FILE = "gallery_lists.npy"
GALLERY_CHUNK = 256                # kGalleryChunk of kernels/launch.h
DEFAULT_NPROBE = 8
KMEANS_ROUNDS = 10


def bf16_to_f64(bits: np.ndarray) -> np.ndarray:
    """uint16 bf16 patterns -> the values they stand for, as float64."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def fp8_to_f64(codes: np.ndarray) -> np.ndarray:
    """uint8 e4m3 codes -> the values they stand for, as float64 (NaN for 0x7F / 0xFF)."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    v[(c & 0x7F) == 0x7F] = np.nan
    return np.where(c & 0x80, -v, v)[np.asarray(codes, dtype=np.uint8)]


def _read_rows(path: Path, features: int, metric: str) -> np.ndarray:
    """The rows of the gallery file ``path`` as float64 [N, F], for cosine of unit length.
    ValueError (naming the file) for anything but a finite float32 / float16 [N, features] array
    with 1 <= N <= GALLERY_MAX_N."""
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
    return x


def load_gallery(path: Path, features: int, metric: str = "cosine") -> np.ndarray:
    """The stored values of the gallery file ``path`` as uint16 bf16 patterns [N, F], C order.
    ValueError (naming the file) for anything but a finite float32 / float16 [N, features] array
    with 1 <= N <= GALLERY_MAX_N."""
    import torch
    path = Path(path)
    x32 = np.ascontiguousarray(_read_rows(path, features, metric), dtype=np.float32)
    bits = torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    if not np.isfinite(bf16_to_f64(bits)).all():
        raise ValueError(f"{path}: a value is too large for bf16")
    return np.ascontiguousarray(bits)


def quantize_fp8(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """float64 rows [N, F] -> (e4m3 codes uint8 [N, F], row scales float32 [N]): the fp8 rule of
    the module docstring."""
    import torch
    x = np.asarray(x, dtype=np.float64)
    scale = (np.abs(x).max(axis=1) / FP8_MAX).astype(np.float32)
    scale[scale == 0] = 1.0
    y = np.clip((x / scale.astype(np.float64)[:, None]).astype(np.float32), -FP8_MAX, FP8_MAX)
    codes = torch.from_numpy(np.ascontiguousarray(y)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return np.ascontiguousarray(codes), scale


def load_gallery_fp8(path: Path, features: int, metric: str = "cosine") -> tuple[np.ndarray, np.ndarray]:
    """The fp8 stored values of the gallery file ``path``: (codes uint8 [N, F], scales float32 [N]);
    the file and its checks are ``load_gallery``'s, and F must be a multiple of 16 (the kernel's)."""
    path = Path(path)
    x = _read_rows(path, features, metric)
    if features % 16:
        raise ValueError(f"{path}: an fp8 gallery needs a feature count that is a multiple of 16, got {features}")
    codes, scale = quantize_fp8(x)
    if not np.isfinite(scale).all():
        raise ValueError(f"{path}: a value is too large for an fp32 row scale")
    return codes, scale


def similar_rule(features_fp32: np.ndarray, gallery_bf16: np.ndarray, k: int,
                 metric: str = "cosine", scale: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
    """fp32 feature rows [n, F] and the gallery's bf16 patterns [N, F] -> (row indices int32 [n, k],
    scores fp32 [n, k]): float64 scores, ranked by a stable argsort of their negation. With
    ``scale`` (float32 [N]) the gallery is fp8: uint8 e4m3 codes [N, F] and their row scales."""
    q = np.asarray(features_fp32, dtype=np.float32)
    if metric == "cosine":
        from .embed import l2_rule
        q = l2_rule(q)
    if scale is None:
        s = q.astype(np.float64) @ bf16_to_f64(gallery_bf16).T
    else:
        s = (q.astype(np.float64) @ fp8_to_f64(gallery_bf16).T) * np.asarray(scale, dtype=np.float32).astype(np.float64)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(s, order, axis=1).astype(np.float32)


@dataclass
class IvfIndex:
    """A version's index in stored form (``load_ivf``) and its ``nprobe``; ``order[p]`` is the
    gallery file's row at stored position p."""
    centroids: np.ndarray          # uint16 bf16 patterns [L, F]
    offsets: np.ndarray            # int32 [L + 1]
    order: np.ndarray              # int64 [N]
    nprobe: int


def build_ivf(rows: np.ndarray, lists: int, rounds: int = KMEANS_ROUNDS) -> tuple[np.ndarray, np.ndarray]:
    """Spherical k-means of the gallery rows [N, F] -> (centroids float32 [L, F], list of each row
    int32 [N]). The centroids start as the first L distinct rows; a round gives every row to the
    centroid of largest cosine (the lowest such list on a tie) and replaces each centroid by the
    unit-length sum of its rows, an empty list keeping its centroid; after ``rounds`` rounds the rows
    are assigned once more. No random numbers: the same rows give the same index."""
    x = np.asarray(rows, dtype=np.float32)
    n = x.shape[0]
    if not 1 <= lists <= min(n, GALLERY_MAX_N):
        raise ValueError(f"ivf_lists must be in 1..{min(n, GALLERY_MAX_N)} (the row count), got {lists}")
    x = x / np.maximum(np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True), 1e-12).astype(np.float32)
    seen, first = set(), []
    for i in range(n):
        key = x[i].tobytes()
        if key not in seen:
            seen.add(key)
            first.append(i)
            if len(first) == lists:
                break
    if len(first) < lists:
        raise ValueError(f"ivf_lists = {lists}, but the gallery has only {len(first)} distinct rows")
    c = x[first].copy()

    def assign() -> np.ndarray:
        return np.concatenate([np.argmax(x[lo:lo + 8192] @ c.T, axis=1) for lo in range(0, n, 8192)]).astype(np.int32)
    for _ in range(rounds):
        a = assign()
        sums = np.zeros(c.shape, np.float64)
        np.add.at(sums, a, x)
        norm = np.linalg.norm(sums, axis=1, keepdims=True)
        keep = (np.bincount(a, minlength=lists) == 0)[:, None] | (norm == 0)
        c = np.where(keep, c, sums / np.where(norm == 0, 1.0, norm)).astype(np.float32)
    return c, assign()


def load_ivf(centroids: Path, lists: Path, rows: int, features: int, metric: str = "cosine"):
    """The stored form of an index over a gallery of ``rows`` rows: (centroid bf16 patterns uint16
    [L, F], offsets int32 [L + 1], order int64 [rows]); stored position p holds the file's row
    order[p] and list l the positions offsets[l] .. offsets[l + 1] - 1. ValueError (naming the file)
    for anything but finite float32 [L, features] centroids with 1 <= L <= GALLERY_MAX_N and int32
    [rows] list ids in 0..L-1."""
    centroids, lists = Path(centroids), Path(lists)

    def read(f: Path) -> np.ndarray:
        try:
            return np.load(f, allow_pickle=False)
        except Exception as e:  # noqa: BLE001 - a missing, truncated or pickled file
            raise ValueError(f"{f}: cannot be read as a .npy array ({e})") from e
    c, a = read(centroids), read(lists)
    if c.dtype != np.float32 or c.ndim != 2 or c.shape[1] != features:
        raise ValueError(f"{centroids}: must be a float32 [L, {features}] array, got {c.dtype} {list(c.shape)}")
    cbits = load_gallery(centroids, features, metric)      # its checks: 1 <= L <= GALLERY_MAX_N, finite
    L = cbits.shape[0]
    if a.dtype != np.int32 or a.shape != (rows,):
        raise ValueError(f"{lists}: must be an int32 [{rows}] array (one list per gallery row), got {a.dtype} {list(a.shape)}")
    if a.min() < 0 or a.max() >= L:
        raise ValueError(f"{lists}: list ids must be in 0..{L - 1}, got {int(a.min())}..{int(a.max())}")
    order = np.argsort(a, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=L))]).astype(np.int32)
    return cbits, offsets, order


def chunk_table(offsets: np.ndarray) -> np.ndarray:
    """The scan's static work list, int32 [C, 3] of (list, first stored position, row count): every
    list cut into chunks of at most GALLERY_CHUNK rows, in ascending position order."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    per = -(-lens // GALLERY_CHUNK)
    lst = np.repeat(np.arange(len(lens)), per)
    j = np.arange(int(per.sum())) - np.repeat(np.cumsum(per) - per, per)      # chunk number within its list
    first = offsets[lst] + j * GALLERY_CHUNK
    return np.ascontiguousarray(np.stack([lst, first, np.minimum(GALLERY_CHUNK, offsets[lst + 1] - first)], axis=1),
                                dtype=np.int32)


def ivf_rule(features_fp32: np.ndarray, centroids_bf16: np.ndarray, gallery_bf16: np.ndarray, offsets: np.ndarray,
             k: int, nprobe: int, metric: str = "cosine") -> tuple[np.ndarray, np.ndarray]:
    """``similar_rule`` over the rows of each query's ``nprobe`` best lists: fp32 feature rows [n, F],
    the bf16 patterns of the centroids [L, F] and of the stored rows [N, F] and the list offsets ->
    (stored positions int32 [n, k], scores fp32 [n, k]), (-1, -inf) where the lists run out."""
    q = np.asarray(features_fp32, dtype=np.float32)
    if metric == "cosine":
        from .embed import l2_rule
        q = l2_rule(q)
    q64 = q.astype(np.float64)
    probes = np.argsort(-(q64 @ bf16_to_f64(centroids_bf16).T), axis=1, kind="stable")[:, :nprobe]
    list_of = np.repeat(np.arange(len(offsets) - 1), np.diff(np.asarray(offsets, dtype=np.int64)))
    probed = np.zeros((q.shape[0], len(offsets) - 1), dtype=bool)
    np.put_along_axis(probed, probes, True, axis=1)
    cand = probed[:, list_of]
    s = np.where(cand, q64 @ bf16_to_f64(gallery_bf16).T, -np.inf)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    real = np.take_along_axis(cand, order, axis=1)
    return (np.where(real, order, -1).astype(np.int32),
            np.where(real, np.take_along_axis(s, order, axis=1), -np.inf).astype(np.float32))


def resolve_ivf(path: Path, rows: int, features: int, metric: str, dtype: str, nprobe_flag: int | None = None):
    """None for a version whose "similar" block has no "index", else its ``IvfIndex``; ValueError
    (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    spec = meta.get("similar", {})
    if "index" not in spec:
        return None
    if spec["index"] != "ivf":
        raise ValueError(f"{path / name}: similar index must be \"ivf\", got {spec['index']!r}")
    files = []
    for key, default in (("centroids", CENTROIDS_FILE), ("lists", LISTS_FILE)):
        f = spec.get(key, default)
        if not isinstance(f, str) or not f or Path(f).name != f:
            raise ValueError(f"{path / name}: similar {key} must be a file name in the version directory, got {f!r}")
        files.append(path / f)
    if dtype == "fp8":
        raise ValueError(f"{files[0]}: an fp8 gallery (\"dtype\": \"fp8\") cannot have an index; store it as bf16")
    cbits, offsets, order = load_ivf(files[0], files[1], rows, features, metric)
    nprobe = nprobe_flag if nprobe_flag is not None else spec.get("nprobe", DEFAULT_NPROBE)
    top = min(cbits.shape[0], MAX_TOP_K)
    if not isinstance(nprobe, int) or isinstance(nprobe, bool) or not 1 <= nprobe <= top:
        raise ValueError(f"{path / name}: similar nprobe must be an integer in 1..{top} "
                         f"(the {cbits.shape[0]} lists of {files[0].name}, at most {MAX_TOP_K}), got {nprobe!r}")
    return IvfIndex(cbits, offsets, order, nprobe)


def resolve(path: Path, features: int, top_k_flag: int | None = None):
    """None for a version without a gallery, else (K, metric, bf16 patterns [N, F], ids [N]) of the
    version in ``path``; ValueError (naming the file) fails the load. (An fp8 version: the first
    four of ``resolve_stored``.)"""
    got = resolve_stored(path, features, top_k_flag)
    return None if got is None else got[:4]


def resolve_stored(path: Path, features: int, top_k_flag: int | None = None, dtype_flag: str | None = None):
    """None for a version without a gallery, else (K, metric, stored values [N, F], ids [N], dtype,
    scales): bf16 patterns and None, or for "fp8" e4m3 codes and their float32 [N] row scales.
    ``dtype_flag`` overrides the version's "dtype"; ValueError (naming the file) fails the load."""
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
    dtype = dtype_flag if dtype_flag is not None else spec.get("dtype", "bf16")
    if not isinstance(dtype, str) or dtype not in DTYPES:
        raise ValueError(f"{path / name}: similar dtype must be one of {DTYPES}, got {dtype!r}")
    if dtype == "fp8":
        bits, scale = load_gallery_fp8(path / gname, features, metric)
    else:
        bits, scale = load_gallery(path / gname, features, metric), None
    n = bits.shape[0]
    if (path / IDS_FILE).exists():
        ids = (path / IDS_FILE).read_text().splitlines()
        if len(ids) != n:
            raise ValueError(f"{path / IDS_FILE}: {len(ids)} ids for the {n} rows of {gname}")
    else:
        ids = [str(i) for i in range(n)]
    return min(k, n), metric, bits, ids, dtype, scale


def add_signatures(src, path: Path, top_k_flag: int | None = None, dtype_flag: str | None = None,
                   nprobe_flag: int | None = None) -> None:
    """Give a loaded ModelSource with a gallery its three similar signatures (beside the others).
    With an index the gallery and its ids are kept in stored order (``load_ivf``)."""
    from ..engine import registry
    from .outputs import add_trio
    F = src.head.features if src.head is not None else registry.get(src.family).features
    got = resolve_stored(path, F, top_k_flag, dtype_flag)
    if got is None:
        return
    k, src.similar_metric, src.gallery, src.gallery_ids, src.similar_dtype, src.gallery_scale = got
    src.similar_k = k
    src.gallery_ivf = ivf = resolve_ivf(path, src.gallery.shape[0], F, src.similar_metric, src.similar_dtype, nprobe_flag)
    if ivf is not None:
        src.gallery = np.ascontiguousarray(src.gallery[ivf.order])
        src.gallery_ids = [src.gallery_ids[i] for i in ivf.order]
    outs = (("ids", P.DT_STRING, (-1, k)), ("scores", P.DT_FLOAT, (-1, k)))
    add_trio(src, SIMILAR_SIGNATURES, "ids", (-1, k), outputs=outs, top_k=k, similar=True)


def rule_rows(src, rows: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """What a CPU or null server answers for the feature rows: ``ivf_rule`` for an indexed version,
    else ``similar_rule``."""
    ivf = src.gallery_ivf
    if ivf is None:
        return similar_rule(rows, src.gallery, k, src.similar_metric, src.gallery_scale)
    return ivf_rule(rows, ivf.centroids, src.gallery, ivf.offsets, k, ivf.nprobe, src.similar_metric)


def ids_of(src, rows: np.ndarray) -> list[list[str]]:
    # NaN features give unspecified rows, a short candidate set index -1: an index out of range names nothing
    ids = src.gallery_ids
    return [[ids[int(j)] if 0 <= int(j) < len(ids) else "" for j in row] for row in rows]


def device_gallery(src, device):
    """The version's gallery as a bf16 tensor on ``device`` (an fp8 gallery: its uint8 codes): one
    copy per (version, device), shared by every engine there."""
    import torch
    dev = torch.device(device)
    with src.gallery_lock:
        t = src.gallery_device.get(dev)
        if t is None:
            if src.gallery_scale is not None:
                t = torch.from_numpy(src.gallery).to(dev)
            else:
                t = torch.from_numpy(src.gallery.view(np.int16)).to(dev).view(torch.bfloat16)
            src.gallery_device[dev] = t
        return t


def device_scale(src, device):
    """The row scales of the version's fp8 gallery as an fp32 tensor on ``device``, one copy per
    (version, device) like the codes; None for a bf16 gallery."""
    import torch
    if src.gallery_scale is None:
        return None
    key = (torch.device(device), "scale")
    with src.gallery_lock:
        t = src.gallery_device.get(key)
        if t is None:
            t = src.gallery_device[key] = torch.from_numpy(src.gallery_scale).to(key[0])
        return t


def device_ivf(src, device):
    """The engine form (``kdl.engine.base.Ivf``) of the version's index on ``device``, one copy per
    (version, device) like the gallery; None without an index."""
    import torch
    from ..engine.base import Ivf
    ivf = src.gallery_ivf
    if ivf is None:
        return None
    key = (torch.device(device), "ivf")
    with src.gallery_lock:
        t = src.gallery_device.get(key)
        if t is None:
            t = src.gallery_device[key] = Ivf(
                torch.from_numpy(ivf.centroids.view(np.int16)).to(key[0]).view(torch.bfloat16),
                torch.from_numpy(chunk_table(ivf.offsets)).to(key[0]), torch.from_numpy(ivf.offsets), ivf.nprobe)
        return t
