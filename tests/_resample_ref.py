"""A numpy reference of Pillow's filtered resize driven only by ``kdl._rt.resample_coeffs`` tables:
what the HIP kernels compute, written the slow and obvious way. Shared by the CPU and GPU tests."""
import numpy as np
from PIL import Image

from kdl.gateway.preprocess import PIL_FILTERS, ResizeSpec

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")
FILTER_IDS = {f: i for i, f in enumerate(FILTERS)}

# H, W -> out_h, out_w
SQUASH_SHAPES = [(400, 534, 299, 299), (37, 53, 224, 224), (1, 1, 8, 8), (300, 7, 16, 16), (64, 64, 32, 64),
                 (97, 131, 24, 24), (513, 257, 256, 224)]
# H, W, R, S
CROP_SHAPES = [(400, 534, 256, 224), (9, 17, 24, 16), (1, 1, 8, 8), (300, 7, 16, 16), (7, 300, 16, 16),
               (700, 500, 64, 56), (37, 53, 40, 40), (65, 33, 33, 32)]


def noise(h: int, w: int, seed: int = 0) -> np.ndarray:
    """Random uint8 noise: smooth images hide off-by-one taps."""
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _pass(a: np.ndarray, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """One pass along axis 0 of ``a`` [n, ...] uint8: int32 accumulator from 1 << 21, wraparound
    as in C, arithmetic shift, clip to 0..255."""
    out = np.empty((len(bounds),) + a.shape[1:], np.uint8)
    for i, (mn, n) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << 21, np.int64)
        acc += np.tensordot(kk[i, :n].astype(np.int64), a[mn:mn + n].astype(np.int64), axes=1)
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)          # int32 wraparound
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def resize_ref(rt, a: np.ndarray, out_h: int, out_w: int, flt: str, window=None) -> np.ndarray:
    """``a`` [H, W, 3] resized to out_h x out_w; ``window`` = (top, left, S) keeps that crop only
    (by slicing the tables, as the kernels do)."""
    H, W, _ = a.shape
    xb, xk = rt.resample_coeffs(W, out_w, FILTER_IDS[flt])
    yb, yk = rt.resample_coeffs(H, out_h, FILTER_IDS[flt])
    if window is not None:
        top, left, S = window
        xb, xk, yb, yk = xb[left:left + S], xk[left:left + S], yb[top:top + S], yk[top:top + S]
    h = _pass(a.transpose(1, 0, 2), xb, xk).transpose(1, 0, 2)     # horizontal first, uint8 intermediate
    return _pass(h, yb, yk)


def spec_ref(rt, a: np.ndarray, spec: ResizeSpec, S: int) -> np.ndarray:
    nh, nw, top, left = spec.geometry(a.shape[0], a.shape[1], S)
    return resize_ref(rt, a, nh, nw, spec.filter, (top, left, S))


def pil_resize(a: np.ndarray, out_h: int, out_w: int, flt: str) -> np.ndarray:
    return np.asarray(Image.fromarray(a).resize((out_w, out_h), PIL_FILTERS[flt]))
