"""The pictures of the PNG encoder's tests, shared by the CPU and GPU files."""
import numpy as np

from _jpeg_cases import pants

SIZES = ((1, 1), (1, 70), (3, 65), (2, 300), (17, 299))     # a run past 258, tails shorter than the minimum match
CONTENTS = ("zero", "constant", "period", "noise", "photo")


def cutout_like(rgb: np.ndarray) -> np.ndarray:
    """RGBA with the bright backdrop of the photograph made transparent (and black, as a cutout's is not)."""
    alpha = np.where(rgb.astype(np.int64).sum(axis=2) < 700, 255, 0).astype(np.uint8)
    return np.dstack([rgb, alpha])


def picture(content: str, H: int, W: int, C: int, seed: int = 0) -> np.ndarray:
    if content == "zero":
        return np.zeros((H, W, C), np.uint8)
    if content == "constant":                                  # one literal and end-of-block once the filter is Sub
        return np.full((H, W, C), 200, np.uint8)
    if content == "period":                                    # period C: matches of the distance C only
        return np.broadcast_to((np.arange(C) * 37 + 5).astype(np.uint8), (H, W, C)).copy()
    if content == "noise":
        return np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)
    rgba = cutout_like(np.asarray(pants(W, H)))
    return np.ascontiguousarray(rgba[:, :, :C])


def cap_of(content: str, H: int, W: int, C: int) -> int:
    """The default cap, ceil(H*W*C / 2); noise cannot fit it and gets 2*H*W*C. A PNG has 63 bytes of framing, so
    below 256 raw bytes no file fits either cap: those pictures get 128 bytes on top. So do the few-pixel crops
    of the photograph, which are noise at these sizes and take the noise cap."""
    raw = H * W * C
    cap = 2 * raw if content in ("noise", "photo") else (raw + 1) // 2
    return cap + 128 if raw < 256 or content == "photo" else cap
