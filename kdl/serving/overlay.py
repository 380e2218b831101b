"""Rendered heatmap overlays: the ``overlay`` / ``overlay_image`` / ``overlay_bytes`` signatures.

They ride on the family's heatmap method (Grad-CAM where ``ModelInfo.cam_oracle`` exists, attention
rollout where ``rollout_oracle`` does; a client calls one name whatever is deployed) and answer its
three outputs plus ``overlay`` DT_UINT8 [-1, S, S, 3]: the exact picture the model saw with the map
upsampled, coloured and blended onto it. The rule is integer arithmetic and is defined HERE, once:
``overlay_rule`` in numpy is what CPU servers answer and what the GPU kernel (kernels/overlay.hip,
``EngineBase(overlay=...)``) reproduces bit for bit.

1. quantise  q = rint(clamp(heat, 0, 1) * 255) as uint8: one fp32 multiply, round-half-even, NaN -> 0.
2. upsample  q from h x w to S x S exactly as Pillow's ``Image.fromarray(q, "L").resize((S, S), filter)``:
             the horizontal pass, then the vertical one, 22-bit coefficients (``kdl._rt.resample_coeffs``),
             a uint8 intermediate, accumulators from 1 << 21, ``>> 22`` clamped to 0..255. ``filter`` is
             bilinear or bicubic; only S >= h and S >= w.
3. colour    the upsampled value u through a 256 x 3 uint8 table (``colormap_table``: jet, hot, gray,
             from integer formulas).
4. blend     a = round(alpha * 256); flat: a_p = a; heat: a_p = (a * u + 127) // 255 (cold regions stay the
             photograph); out = (img * (256 - a_p) + colour * a_p + 128) >> 8.

Configuration: ``"overlay": {"colormap": "jet", "alpha": 0.5, "blend": "heat", "filter": "bilinear"}`` in
the version's ``kdl_model.json`` / ``synthetic.json`` (these are the defaults); ``--overlay_colormap`` and
``--overlay_alpha`` override it. A result row is 2 + h*w + ceil(S*S*3 / 4) words: class, score, the map,
the picture bytes (``pack_rows`` / ``unpack_rows``).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from ..engine.base import Overlay, overlay_words, pack_overlay, unpack_overlay  # noqa: F401
from . import protos as P

OVERLAY_SIGNATURE = "overlay"
OVERLAY_IMAGE_SIGNATURE = "overlay_image"
OVERLAY_BYTES_SIGNATURE = "overlay_bytes"
OVERLAY_SIGNATURES = (OVERLAY_SIGNATURE, OVERLAY_IMAGE_SIGNATURE, OVERLAY_BYTES_SIGNATURE)
OUTPUT_KEYS = ("classes", "scores", "heatmap", "overlay")
COLORMAPS = ("jet", "hot", "gray")
BLENDS = ("flat", "heat")                      # index = HeatOverlayArgs.blend
FILTERS = {"bilinear": 1, "bicubic": 3}        # kdl._rt.resample_coeffs ids
PRECISION_BITS = 22


def colormap_table(name: str) -> np.ndarray:
    """The 256 x 3 uint8 colour table of ``name``, from integer formulas (u = 0..255):
    jet  channel k (k = 3, 2, 1 for r, g, b) = clip(383 - |4u - 255k|, 0, 255);
    hot  clip(3u - 255k, 0, 255) with k = 0, 1, 2;   gray  u for all three."""
    u = np.arange(256, dtype=np.int64)
    if name == "jet":
        cols = [np.clip(383 - np.abs(4 * u - 255 * k), 0, 255) for k in (3, 2, 1)]
    elif name == "hot":
        cols = [np.clip(3 * u - 255 * k, 0, 255) for k in (0, 1, 2)]
    elif name == "gray":
        cols = [u, u, u]
    else:
        raise ValueError(f"colormap must be one of {COLORMAPS}, got {name!r}")
    return np.ascontiguousarray(np.stack(cols, axis=1).astype(np.uint8))


def alpha_fixed(alpha: float) -> int:
    """a = round(alpha * 256), 0..256."""
    a = int(round(float(alpha) * 256))
    if not 0 <= a <= 256:
        raise ValueError(f"alpha must lie in 0..1, got {alpha!r}")
    return a


def check(spec: Overlay) -> Overlay:
    """ValueError for an unknown colour table, blend or filter, or an alpha outside 0..1."""
    if spec.colormap not in COLORMAPS:
        raise ValueError(f"overlay colormap must be one of {COLORMAPS}, got {spec.colormap!r}")
    if spec.blend not in BLENDS:
        raise ValueError(f"overlay blend must be one of {BLENDS}, got {spec.blend!r}")
    if spec.filter not in FILTERS:
        raise ValueError(f"overlay filter must be one of {tuple(FILTERS)}, got {spec.filter!r}")
    if isinstance(spec.alpha, bool) or not isinstance(spec.alpha, (int, float)) or not 0.0 <= spec.alpha <= 1.0:
        raise ValueError(f"overlay alpha must be a number in 0..1, got {spec.alpha!r}")
    return spec


def quantise(heat) -> np.ndarray:
    """Step 1: fp32 heat -> uint8, rint(clamp(heat, 0, 1) * 255), NaN -> 0."""
    x = np.asarray(heat, dtype=np.float32)
    x = np.where(x > 0, x, np.float32(0))                      # NaN -> 0
    x = np.where(x < 1, x, np.float32(1)).astype(np.float32)
    return np.rint(np.float32(x) * np.float32(255)).astype(np.uint8)


def axis_tables(n_in: int, S: int, filter: str) -> tuple:
    """Pillow's (bounds int32 [S, 2], coefficients int32 [S, ksize]) of one axis, n_in -> S."""
    from ..ops import _lib
    if S < n_in:
        raise ValueError(f"overlays only upsample: a map of {n_in} onto {S} pixels is refused")
    b, k = _lib.rt().resample_coeffs(int(n_in), int(S), FILTERS[filter])
    return np.ascontiguousarray(b, dtype=np.int32), np.ascontiguousarray(k, dtype=np.int32)


def _pass(src: np.ndarray, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """One pass along the LAST axis of uint8 ``src`` [..., n_in] -> uint8 [..., S]."""
    S = bounds.shape[0]
    out = np.empty(src.shape[:-1] + (S,), dtype=np.uint8)
    s64 = src.astype(np.int64)
    for x in range(S):
        mn, n = int(bounds[x, 0]), int(bounds[x, 1])
        acc = (1 << (PRECISION_BITS - 1)) + (s64[..., mn:mn + n] * kk[x, :n].astype(np.int64)).sum(axis=-1)
        out[..., x] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def upsample(q: np.ndarray, S: int, filter: str = "bilinear") -> np.ndarray:
    """Step 2: uint8 [h, w] -> uint8 [S, S], Pillow's ``L`` resize bit for bit."""
    q = np.asarray(q, dtype=np.uint8)
    h, w = q.shape
    xb, xk = axis_tables(w, S, filter)
    yb, yk = axis_tables(h, S, filter)
    tmp = _pass(q, xb, xk)                                     # [h, S]
    return np.ascontiguousarray(_pass(np.ascontiguousarray(tmp.T), yb, yk).T)


def overlay_rule(image_u8, heat_f32, spec: Overlay | None = None) -> np.ndarray:
    """THE definition: uint8 image [S, S, 3] and fp32 heat [h, w] -> uint8 [S, S, 3]."""
    spec = check(spec or Overlay())
    img = np.asarray(image_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] != img.shape[1] or img.shape[2] != 3:
        raise ValueError(f"the picture must be uint8 [S, S, 3], got {img.dtype} {img.shape}")
    S = img.shape[0]
    u = upsample(quantise(heat_f32), S, spec.filter).astype(np.int64)
    col = colormap_table(spec.colormap)[u].astype(np.int64)   # [S, S, 3]
    a = alpha_fixed(spec.alpha)
    ap = ((a * u + 127) // 255 if spec.blend == "heat" else np.full_like(u, a))[..., None]
    return ((img.astype(np.int64) * (256 - ap) + col * ap + 128) >> 8).astype(np.uint8)


# ------------------------------------------------------------------------------------------ rows
def pack_rows(classes, scores, heat, pictures) -> np.ndarray:
    """The engine's row layout [n, 2 + h*w + ceil(S*S*3/4)] fp32 words."""
    return pack_overlay(classes, scores, heat, pictures)


def unpack_rows(rows, h: int, w: int, S: int) -> tuple:
    """-> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], pictures uint8 [n, S, S, 3])."""
    return unpack_overlay(np.ascontiguousarray(rows, dtype=np.float32), h, w, S)


# ------------------------------------------------------------------------------------------ config
def resolve(path: Path, colormap_flag: str | None = None, alpha_flag: float | None = None) -> Overlay:
    """The version's ``Overlay``: its "overlay" block over the defaults, the two flags over that.
    ValueError (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    block = meta.get("overlay", {})
    if not isinstance(block, dict):
        raise ValueError(f"{path / name}: \"overlay\" must be an object like {{\"colormap\": \"jet\", \"alpha\": 0.5}}")
    unknown = sorted(set(block) - {"colormap", "alpha", "blend", "filter"})
    if unknown:
        raise ValueError(f"{path / name}: unknown \"overlay\" keys {unknown}")
    try:
        spec = check(Overlay(**block))
    except ValueError as e:
        raise ValueError(f"{path / name}: {e}") from e
    if colormap_flag:
        if colormap_flag not in COLORMAPS:
            raise ValueError(f"--overlay_colormap must be one of {COLORMAPS}, got {colormap_flag!r}")
        spec = Overlay(colormap_flag, spec.alpha, spec.blend, spec.filter)
    if alpha_flag is not None:
        if not 0.0 <= float(alpha_flag) <= 1.0:
            raise ValueError(f"--overlay_alpha must lie in 0..1, got {alpha_flag!r}")
        spec = Overlay(spec.colormap, float(alpha_flag), spec.blend, spec.filter)
    return spec


def add_signatures(src, path, colormap_flag: str | None = None, alpha_flag: float | None = None) -> None:
    """Give a loaded ModelSource its three overlay signatures (beside the existing ones): the family's
    heatmap method (Grad-CAM or rollout) and one more output."""
    from ..engine import registry
    from .explain import map_outputs
    from .outputs import add_trio
    info = registry.get(src.family)
    if info.cam_oracle is None and info.rollout_oracle is None:
        return
    src.overlay = resolve(path, colormap_flag, alpha_flag)
    h, w = info.map_size
    S = src.input_size
    if S < max(h, w):
        raise ValueError(f"{path}: overlays only upsample, the {h} x {w} map is larger than the {S} x {S} input")
    outs = map_outputs(h, w) + (("overlay", P.DT_UINT8, (-1, S, S, 3)),)
    add_trio(src, OVERLAY_SIGNATURES, "classes", (-1, 1), outputs=outs, explain=(h, w),
             rollout=info.cam_oracle is None, overlay=S)
