"""Garment cutouts: the ``cutout`` / ``cutout_image`` / ``cutout_bytes`` signatures.

"Give me the garment itself": the picture the model saw with the backdrop made transparent, for catalogue
tiles and listing thumbnails. They ride on the family's heatmap method (Grad-CAM where
``ModelInfo.cam_oracle`` exists, attention rollout where ``rollout_oracle`` does). The map says roughly where
the garment is (10 x 10 for Xception, 14 x 14 for ViT); the picture sharpens it with a CAM-seeded colour
model: one histogram describes the colours of the hot area, one the colours of the cold area, and each pixel
goes to the side its colour is more typical of (what GrabCut does, without the cut). Outputs: ``classes``
DT_STRING [-1, 1], ``scores`` DT_FLOAT [-1, 1], ``cutout`` DT_UINT8 [-1, S, S, 4] (the picture the model saw,
with alpha), ``coverage`` DT_FLOAT [-1, 1] (the share of the picture that is garment). The rule uses integers
only and is defined HERE, once: ``cutout_rule`` in numpy is what CPU servers answer and what the GPU kernels
(kernels/cutout.hip, ``EngineBase(cutout=...)``) reproduce bit for bit.

1. upsample   u = overlay.upsample(overlay.quantise(heat), S, filter), uint8 [S, S] (steps 1-2 of the overlay
              rule, unchanged; NaN becomes 0).
2. gate       ok = u >= gate, an integer in 1..255. A pixel with ok false is never garment.
3. tables     over the 4096 colour bins (palette's: (r >> 4) << 8 | (g >> 4) << 4 | (b >> 4)):
              N[b] = pixels of the bin, G[b] = gated pixels of the bin, F_0[b] = the sum of u over the bin's
              pixels. For S <= 1024 every sum is below 2^28: uint32 holds it. S > 1024 is refused.
4. rounds     t = 0..R: B_t[b] = 255 N[b] - F_t[b], TF_t = sum F_t, TB_t = 255 S^2 - TF_t. Bin b is
              garment-coloured in round t iff N[b] > 0 and F_t[b] TB_t >= B_t[b] TF_t (64-bit products:
              F TB <= TF TB <= (255 S^2)^2 / 4 < 2^54). F_{t+1}[b] = 255 G[b] where b is garment-coloured in
              round t, else 0: the histogram of the hard mask fg_t[bin] & ok. Ties go to the garment, which
              keeps an all-ones map (TB = 0) and a one-colour picture defined: the mask is the gate.
              ROUNDS AFTER THE FIRST NEED NO PIXELS, only the three tables N, G and F: the kernels run them in
              one workgroup per image, and tests/test_cutout_cpu.py checks the table form against a
              pixel-level second implementation.
5. raw mask   m = fg_R[bin] & ok.
6. smooth     M times: c(y, x) = the set pixels of the 3 x 3 window around (y, x), pixels outside the picture
              unset; m <- c >= 5.
7. alpha      with ``feather`` a = (255 c + 4) // 9, c taken on the final mask; without it a = 255 m.
              count = sum m of the final mask, whatever ``feather`` is.
8. answer     rgba = image || a.

An all-zero, all-NaN or below-gate map gives count 0 and alpha 0 everywhere.

Configuration (opt-in): ``"cutout": {"gate": 26, "rounds": 2, "smooth": 1, "feather": true, "filter":
"bilinear"}`` in the version's ``kdl_model.json`` / ``synthetic.json`` (these are the defaults of a present
block), or ``--cutout_gate G``, which turns the signatures on and overrides ``gate``. A result row is
2 + h*w + 1 + S*S words: explain's front, count, then one word per pixel, r | g << 8 | b << 16 | a << 24
(``pack_rows`` / ``unpack_rows``).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from ..engine.base import Cutout, pack_cutout, unpack_cutout  # noqa: F401
from . import overlay
from . import protos as P

CUTOUT_SIGNATURE = "cutout"
CUTOUT_IMAGE_SIGNATURE = "cutout_image"
CUTOUT_BYTES_SIGNATURE = "cutout_bytes"
CUTOUT_SIGNATURES = (CUTOUT_SIGNATURE, CUTOUT_IMAGE_SIGNATURE, CUTOUT_BYTES_SIGNATURE)
OUTPUT_KEYS = ("classes", "scores", "cutout", "coverage")
BINS = 4096
MAX_ROUNDS = 8
MAX_SMOOTH = 4
MAX_S = 1024                                   # kOverlayMaxS: every table sum below 2^28
KEYS = ("gate", "rounds", "smooth", "feather", "filter")


def _int_in(v, lo: int, hi: int) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= int(v) <= hi


def check(spec: Cutout) -> Cutout:
    """ValueError for a gate outside 1..255, rounds outside 0..8, smooth outside 0..4, a feather that is no
    bool, an unknown filter."""
    if not _int_in(spec.gate, 1, 255):
        raise ValueError(f"cutout gate must be an integer in 1..255, got {spec.gate!r}")
    if not _int_in(spec.rounds, 0, MAX_ROUNDS):
        raise ValueError(f"cutout rounds must be an integer in 0..{MAX_ROUNDS}, got {spec.rounds!r}")
    if not _int_in(spec.smooth, 0, MAX_SMOOTH):
        raise ValueError(f"cutout smooth must be an integer in 0..{MAX_SMOOTH}, got {spec.smooth!r}")
    if not isinstance(spec.feather, (bool, np.bool_)):
        raise ValueError(f"cutout feather must be true or false, got {spec.feather!r}")
    if spec.filter not in overlay.FILTERS:
        raise ValueError(f"cutout filter must be one of {tuple(overlay.FILTERS)}, got {spec.filter!r}")
    return spec


def bins_of(image_u8) -> np.ndarray:
    """palette's colour bin of every pixel: int64 [S, S] in 0..4095."""
    p = np.asarray(image_u8).astype(np.int64) >> 4
    return (p[..., 0] << 8) | (p[..., 1] << 4) | p[..., 2]


def tables_of(bins: np.ndarray, u: np.ndarray, ok: np.ndarray) -> tuple:
    """Step 3: (N, G, F_0), int64 [4096] each."""
    b = bins.reshape(-1)
    N = np.bincount(b, minlength=BINS).astype(np.int64)
    G = np.bincount(b[ok.reshape(-1)], minlength=BINS).astype(np.int64)
    F = np.bincount(b, weights=u.reshape(-1), minlength=BINS).astype(np.int64)   # sums below 2^28: exact in float64
    return N, G, F


def colour_table(N, G, F0, S: int, rounds: int) -> np.ndarray:
    """Step 4 on the three tables alone: bool [4096], fg_R. Every product is below 2^54."""
    N, G, F = (np.asarray(a, dtype=np.int64) for a in (N, G, F0))
    full = 255 * int(S) * int(S)
    fg = np.zeros(BINS, dtype=bool)
    for _ in range(int(rounds) + 1):
        TF = int(F.sum())
        TB = full - TF
        fg = (N > 0) & (F * TB >= (255 * N - F) * TF)
        F = np.where(fg, 255 * G, 0)
    return fg


def window_counts(mask: np.ndarray) -> np.ndarray:
    """c of step 6: the set pixels of every 3 x 3 window, int64 [S, S]; outside the picture counts as unset."""
    m = np.asarray(mask, dtype=np.int64)
    pad = np.zeros((m.shape[0] + 2, m.shape[1] + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = m
    H, W = m.shape
    return sum(pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))


def finish(mask: np.ndarray, spec: Cutout) -> tuple:
    """Steps 6-7 on a raw bool mask: (count, alpha uint8 [S, S])."""
    m = np.asarray(mask, dtype=bool)
    for _ in range(int(spec.smooth)):
        m = window_counts(m) >= 5
    if spec.feather:
        a = (255 * window_counts(m) + 4) // 9
    else:
        a = 255 * m.astype(np.int64)
    return int(m.sum()), a.astype(np.uint8)


def cutout_rule(image_u8, heat_f32, spec: Cutout | None = None) -> tuple:
    """THE definition: uint8 [S, S, 3] and fp32 heat [h, w] -> (count, rgba uint8 [S, S, 4])."""
    spec = check(spec or Cutout())
    img = np.asarray(image_u8)
    heat = np.asarray(heat_f32)
    if img.ndim != 3 or img.shape[0] != img.shape[1] or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f"the picture must be uint8 [S, S, 3], got {img.dtype} {img.shape}")
    if heat.ndim != 2:
        raise ValueError(f"the map must be [h, w], got {heat.shape}")
    S = img.shape[0]
    if S > MAX_S:
        raise ValueError(f"cutout: a side of {S} pixels is refused, the uint32 tables hold up to {MAX_S}")
    u = overlay.upsample(overlay.quantise(heat), S, spec.filter)
    ok = u >= int(spec.gate)
    bins = bins_of(img)
    fg = colour_table(*tables_of(bins, u, ok), S, spec.rounds)
    count, alpha = finish(fg[bins] & ok, spec)
    return count, np.concatenate([img, alpha[..., None]], axis=-1)


# ------------------------------------------------------------------------------------------ host-side helpers
def coverage_of(counts, S: int) -> np.ndarray:
    """float32(count / (S*S)), the division in float64."""
    return (np.asarray(counts, dtype=np.float64) / float(S * S)).astype(np.float32)


# ------------------------------------------------------------------------------------------ rows
def pack_rows(classes, scores, heat, counts, pictures) -> np.ndarray:
    """The engine's row layout [n, 2 + h*w + 1 + S*S] fp32 words."""
    return pack_cutout(classes, scores, heat, counts, pictures)


def unpack_rows(rows, h: int, w: int, S: int) -> tuple:
    """-> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], counts uint32 [n], rgba uint8 [n, S, S, 4])."""
    return unpack_cutout(np.ascontiguousarray(rows, dtype=np.float32), h, w, S)


# ------------------------------------------------------------------------------------------ config
def resolve(path: Path, gate_flag: int | None = None) -> Cutout | None:
    """The version's ``Cutout``: its "cutout" block over the defaults, ``--cutout_gate`` over that; None where
    neither is there. ValueError (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    if "cutout" not in meta and gate_flag is None:
        return None
    block = meta.get("cutout", {})
    if not isinstance(block, dict):
        raise ValueError(f"{path / name}: \"cutout\" must be an object like {{\"gate\": 26, \"rounds\": 2}}")
    unknown = sorted(set(block) - set(KEYS))
    if unknown:
        raise ValueError(f"{path / name}: unknown \"cutout\" keys {unknown}")
    try:
        spec = check(Cutout(**block))
    except ValueError as e:
        raise ValueError(f"{path / name}: {e}") from e
    if gate_flag is not None:
        if not _int_in(gate_flag, 1, 255):
            raise ValueError(f"--cutout_gate must be an integer in 1..255, got {gate_flag!r}")
        spec = Cutout(int(gate_flag), spec.rounds, spec.smooth, spec.feather, spec.filter)
    return spec


def add_signatures(src, path, gate_flag: int | None = None) -> None:
    """Give a loaded ModelSource with a "cutout" block (or the flag) its three cutout signatures. They are
    explain-kind signatures told from the others by their ``coverage`` output."""
    from ..engine import registry
    from .outputs import add_trio
    spec = resolve(path, gate_flag)
    if spec is None:
        return
    info = registry.get(src.family)
    if info.cam_oracle is None and info.rollout_oracle is None:
        raise ValueError(f"{path}: \"cutout\" needs a heatmap method, which the {src.family} family does not have")
    h, w = info.map_size
    S = src.input_size
    if S < max(h, w) or S > MAX_S:
        raise ValueError(f"{path}: cutout takes inputs from the {h} x {w} map's size up to {MAX_S}, not {S} x {S}")
    src.cutout = spec
    outs = (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)), ("cutout", P.DT_UINT8, (-1, S, S, 4)),
            ("coverage", P.DT_FLOAT, (-1, 1)))
    add_trio(src, CUTOUT_SIGNATURES, "classes", (-1, 1), outputs=outs, explain=(h, w),
             rollout=info.cam_oracle is None)
