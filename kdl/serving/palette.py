"""Dominant colours: the ``palette`` / ``palette_image`` / ``palette_bytes`` signatures.

"What colour is it?" beside "what is it?". They ride on the family's heatmap method (Grad-CAM where
``ModelInfo.cam_oracle`` exists, attention rollout where ``rollout_oracle`` does) because the map already
says which pixels are the garment and which the backdrop: the answer is the picture's colour histogram
weighted by the map, clustered into K colours. Outputs: ``classes`` DT_STRING [-1, 1], ``scores`` DT_FLOAT
[-1, 1], ``colors`` DT_UINT8 [-1, K, 3], ``fractions`` DT_FLOAT [-1, K] (each colour's share of the weight),
``names`` DT_STRING [-1, K] (the nearest of twenty CSS colour names). The rule uses integers only, so any
summation order gives the same bits, and is defined HERE, once: ``palette_rule`` in numpy is what CPU
servers answer and what the GPU kernels (kernels/palette.hip, ``EngineBase(palette=...)``) reproduce bit
for bit.

1. weight     "map": u = overlay.upsample(overlay.quantise(heat), S, filter) (steps 1-2 of the overlay
              rule), w = u >> 4, 0..15; "uniform": w = 15.
2. histogram  bin = (r >> 4) << 8 | (g >> 4) << 4 | (b >> 4), 4096 bins; per bin four uint32 sums
              n = sum w, sr = sum w*r, sg, sb over the full 8-bit channels. 15 * 255 * S*S + 15 * S*S / 2 <
              2^32 for S <= 1024, so no sum (and no s + n/2 below) overflows; S > 1024 is refused.
3. total      W = sum n; W = 0 (an all-zero map): all K colours and weights are 0.
4. bin means  m = (s + n/2) // n per channel for every bin with n > 0.
5. centres    c_0 = m of the bin with the largest n; c_j = m of the bin with the largest n_i * D_i, D_i the
              smallest squared RGB distance from m_i to the centres chosen so far (a 64-bit product); every
              tie to the lowest bin. A largest product of 0 means fewer distinct bin means than K: stop with
              k < K centres, the other K - k answers are colour (0, 0, 0), weight 0.
6. T rounds   assign every live bin to the centre nearest to its m (ties to the lowest centre); N_j = sum n,
              S_j = sum s over the cluster's bins (the true sums, not the means); c_j = (S_j + N_j/2) // N_j;
              an empty cluster keeps its centre with N_j = 0. The answer is the T-th round's N_j and c_j.
7. order      by N_j descending, ties to the lower j.

Configuration (opt-in): ``"palette": {"colors": 5, "weight": "map", "filter": "bilinear", "rounds": 8}`` in the
version's ``kdl_model.json`` / ``synthetic.json`` (these are the defaults of a present block), or
``--palette_colors K``, which turns the signatures on and overrides ``colors``. A result row is
2 + h*w + 1 + 2K words: explain's front, W, then K x (r | g << 8 | b << 16, N) (``pack_rows`` / ``unpack_rows``).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from ..engine.base import Palette, pack_palette, unpack_palette  # noqa: F401
from . import overlay
from . import protos as P

PALETTE_SIGNATURE = "palette"
PALETTE_IMAGE_SIGNATURE = "palette_image"
PALETTE_BYTES_SIGNATURE = "palette_bytes"
PALETTE_SIGNATURES = (PALETTE_SIGNATURE, PALETTE_IMAGE_SIGNATURE, PALETTE_BYTES_SIGNATURE)
OUTPUT_KEYS = ("classes", "scores", "colors", "fractions", "names")
WEIGHTS = ("uniform", "map")                   # index = PaletteArgs.weight
MAX_COLORS = 8
MAX_ROUNDS = 16
MAX_S = 1024                                   # kOverlayMaxS: the uint32 bound of step 2
BINS = 4096

# the CSS values of the names ``names_of`` answers
CSS_COLORS = (
    ("black", (0, 0, 0)), ("white", (255, 255, 255)), ("gray", (128, 128, 128)), ("silver", (192, 192, 192)),
    ("red", (255, 0, 0)), ("maroon", (128, 0, 0)), ("orange", (255, 165, 0)), ("yellow", (255, 255, 0)),
    ("olive", (128, 128, 0)), ("green", (0, 128, 0)), ("lime", (0, 255, 0)), ("teal", (0, 128, 128)),
    ("aqua", (0, 255, 255)), ("blue", (0, 0, 255)), ("navy", (0, 0, 128)), ("purple", (128, 0, 128)),
    ("fuchsia", (255, 0, 255)), ("pink", (255, 192, 203)), ("brown", (165, 42, 42)), ("beige", (245, 245, 220)),
)


def _int_in(v, lo: int, hi: int) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= int(v) <= hi


def check(spec: Palette) -> Palette:
    """ValueError for colors outside 1..8, rounds outside 1..16, an unknown weight or filter."""
    if not _int_in(spec.colors, 1, MAX_COLORS):
        raise ValueError(f"palette colors must be an integer in 1..{MAX_COLORS}, got {spec.colors!r}")
    if not _int_in(spec.rounds, 1, MAX_ROUNDS):
        raise ValueError(f"palette rounds must be an integer in 1..{MAX_ROUNDS}, got {spec.rounds!r}")
    if spec.weight not in WEIGHTS:
        raise ValueError(f"palette weight must be one of {WEIGHTS}, got {spec.weight!r}")
    if spec.filter not in overlay.FILTERS:
        raise ValueError(f"palette filter must be one of {tuple(overlay.FILTERS)}, got {spec.filter!r}")
    return spec


def pixel_weights(heat_f32, S: int, spec: Palette) -> np.ndarray:
    """Step 1: the weight 0..15 of every pixel, int64 [S, S]."""
    if spec.weight == "uniform":
        return np.full((S, S), 15, dtype=np.int64)
    return overlay.upsample(overlay.quantise(heat_f32), S, spec.filter).astype(np.int64) >> 4


def histogram(image_u8: np.ndarray, w: np.ndarray) -> np.ndarray:
    """Step 2: int64 [4096, 4] of n, sr, sg, sb (every value < 2^32)."""
    px = image_u8.reshape(-1, 3).astype(np.int64)
    w = w.reshape(-1)
    bins = ((px[:, 0] >> 4) << 8) | ((px[:, 1] >> 4) << 4) | (px[:, 2] >> 4)
    hist = np.zeros((BINS, 4), dtype=np.int64)
    np.add.at(hist[:, 0], bins, w)
    for c in range(3):
        np.add.at(hist[:, 1 + c], bins, w * px[:, c])
    return hist


def cluster(hist: np.ndarray, K: int, T: int) -> tuple:
    """Steps 3-7 on a histogram: (W, colours uint8 [K, 3], weights uint32 [K])."""
    colours, weights = np.zeros((K, 3), dtype=np.uint8), np.zeros(K, dtype=np.uint32)
    W = int(hist[:, 0].sum())
    if W == 0:
        return 0, colours, weights
    live = np.flatnonzero(hist[:, 0] > 0)                      # ascending: the first of equals is the lowest bin
    n, s = hist[live, 0], hist[live, 1:]
    m = (s + (n // 2)[:, None]) // n[:, None]
    cen = [m[int(np.argmax(n))]]                               # np.argmax: the first of equals
    D = np.full(len(live), np.iinfo(np.int64).max)
    while len(cen) < K:
        D = np.minimum(D, ((m - cen[-1]) ** 2).sum(axis=1))
        prod = n * D                                           # < 2^24 * 2^18: int64 holds it
        i = int(np.argmax(prod))
        if prod[i] == 0:
            break
        cen.append(m[i])
    cen = np.stack(cen)
    k = len(cen)
    N = np.zeros(k, dtype=np.int64)
    for _ in range(T):
        d = ((m[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2)
        asg = np.argmin(d, axis=1)                             # the first of equals: the lowest centre
        N = np.zeros(k, dtype=np.int64)
        Ssum = np.zeros((k, 3), dtype=np.int64)
        np.add.at(N, asg, n)
        np.add.at(Ssum, asg, s)
        full = N > 0
        cen = cen.copy()
        cen[full] = (Ssum[full] + (N[full] // 2)[:, None]) // N[full][:, None]
    order = np.argsort(-N, kind="stable")                      # ties to the lower j
    colours[:k] = cen[order]
    weights[:k] = N[order]
    return W, colours, weights


def palette_rule(image_u8, heat_f32, spec: Palette | None = None) -> tuple:
    """THE definition: uint8 image [S, S, 3] and fp32 heat [h, w] -> (W, colours uint8 [K, 3], weights
    uint32 [K])."""
    spec = check(spec or Palette())
    img = np.asarray(image_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] != img.shape[1] or img.shape[2] != 3:
        raise ValueError(f"the picture must be uint8 [S, S, 3], got {img.dtype} {img.shape}")
    S = img.shape[0]
    if S > MAX_S:
        raise ValueError(f"palette: a side of {S} pixels is refused, the uint32 sums hold up to {MAX_S}")
    return cluster(histogram(img, pixel_weights(heat_f32, S, spec)), int(spec.colors), int(spec.rounds))


# ------------------------------------------------------------------------------------------ host-side helpers
def fractions_of(weights, totals) -> np.ndarray:
    """float32(N / W) per colour, the division in float64; W = 0 gives 0."""
    n = np.asarray(weights, dtype=np.float64)
    w = np.asarray(totals, dtype=np.float64).reshape(n.shape[:-1] + (1,))
    return np.divide(n, w, out=np.zeros_like(n), where=w > 0).astype(np.float32)


def names_of(colours) -> list:
    """The nearest CSS name of every colour by squared RGB distance (the first of equals): nested lists of
    str shaped like ``colours`` without its last axis."""
    c = np.asarray(colours, dtype=np.int64)
    table = np.array([v for _, v in CSS_COLORS], dtype=np.int64)
    idx = np.argmin(((c[..., None, :] - table) ** 2).sum(axis=-1), axis=-1)
    return np.array([name for name, _ in CSS_COLORS], dtype=object)[idx].tolist()


# ------------------------------------------------------------------------------------------ rows
def pack_rows(classes, scores, heat, totals, colours, weights) -> np.ndarray:
    """The engine's row layout [n, 2 + h*w + 1 + 2K] fp32 words."""
    return pack_palette(classes, scores, heat, totals, colours, weights)


def unpack_rows(rows, h: int, w: int, K: int) -> tuple:
    """-> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], W uint32 [n], colours uint8 [n, K, 3],
    weights uint32 [n, K])."""
    return unpack_palette(np.ascontiguousarray(rows, dtype=np.float32), h, w, K)


# ------------------------------------------------------------------------------------------ config
def resolve(path: Path, colors_flag: int | None = None) -> Palette | None:
    """The version's ``Palette``: its "palette" block over the defaults, ``--palette_colors`` over that; None
    where neither is there. ValueError (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    if "palette" not in meta and colors_flag is None:
        return None
    block = meta.get("palette", {})
    if not isinstance(block, dict):
        raise ValueError(f"{path / name}: \"palette\" must be an object like {{\"colors\": 5, \"weight\": \"map\"}}")
    unknown = sorted(set(block) - {"colors", "weight", "filter", "rounds"})
    if unknown:
        raise ValueError(f"{path / name}: unknown \"palette\" keys {unknown}")
    try:
        spec = check(Palette(**block))
    except ValueError as e:
        raise ValueError(f"{path / name}: {e}") from e
    if colors_flag is not None:
        if not _int_in(colors_flag, 1, MAX_COLORS):
            raise ValueError(f"--palette_colors must be an integer in 1..{MAX_COLORS}, got {colors_flag!r}")
        spec = Palette(int(colors_flag), spec.weight, spec.filter, spec.rounds)
    return spec


def add_signatures(src, path, colors_flag: int | None = None) -> None:
    """Give a loaded ModelSource with a "palette" block (or the flag) its three palette signatures. They are
    explain-kind signatures told from the others by their ``fractions`` output, whose shape carries K."""
    from ..engine import registry
    from .outputs import add_trio
    spec = resolve(path, colors_flag)
    if spec is None:
        return
    info = registry.get(src.family)
    if info.cam_oracle is None and info.rollout_oracle is None:
        raise ValueError(f"{path}: \"palette\" needs a heatmap method, which the {src.family} family does not have")
    h, w = info.map_size
    S, K = src.input_size, int(spec.colors)
    if S < max(h, w) or S > MAX_S:
        raise ValueError(f"{path}: palette takes inputs from the {h} x {w} map's size up to {MAX_S}, not {S} x {S}")
    src.palette = spec
    outs = (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)), ("colors", P.DT_UINT8, (-1, K, 3)),
            ("fractions", P.DT_FLOAT, (-1, K)), ("names", P.DT_STRING, (-1, K)))
    add_trio(src, PALETTE_SIGNATURES, "classes", (-1, 1), outputs=outs, explain=(h, w),
             rollout=info.cam_oracle is None)
