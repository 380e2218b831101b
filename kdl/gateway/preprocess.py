"""Xception image preprocessing, bit-compatible with keras_image_helper 0.0.1.

The reference gateway calls ``create_preprocessor('xception', target_size=(299,
299)).from_url(url)`` (`model_server.py:8,18,53`): download -> PIL open ->
convert('RGB') -> resize(target, Image.NEAREST) -> float32 -> x/127.5 - 1
(SURVEY.md §2.3 X5, §2.9.4). ``nearest_indices`` reproduces PIL's NEAREST
source-index rule (double-precision accumulation, *not* floor((i+0.5)*s)); the
same tables drive the GPU resize kernel (``resize_nearest_u8``).
"""
from __future__ import annotations

import io
import urllib.request
from dataclasses import dataclass

import numpy as np
from PIL import Image

TARGET = (299, 299)


def nearest_indices(src: int, dst: int) -> np.ndarray:
    """PIL Image.NEAREST source index for each destination pixel on one axis."""
    scale = src / dst
    xx = 0.5 * scale
    out = np.empty(dst, dtype=np.int32)
    for i in range(dst):
        out[i] = min(int(xx), src - 1)
        xx += scale
    return out


def load_image(data: bytes) -> Image.Image:
    img = Image.open(io.BytesIO(data))
    if img.mode != "RGB":
        img = img.convert("RGB")
    return img


def to_uint8(img: Image.Image, target=TARGET) -> np.ndarray:
    """uint8 HWC after NEAREST resize (the native serving_uint8 payload)."""
    return np.asarray(img.resize(target, Image.NEAREST), dtype=np.uint8)


def resize_nearest_np(arr: np.ndarray, target=TARGET) -> np.ndarray:
    """Same as PIL NEAREST via the index tables (used to validate the tables)."""
    h, w = arr.shape[:2]
    ys, xs = nearest_indices(h, target[1]), nearest_indices(w, target[0])
    return arr[ys][:, xs]


PIL_FILTERS = {"nearest": Image.NEAREST, "box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING,
               "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


@dataclass(frozen=True)
class ResizeSpec:
    """How an image of any size becomes the model's S x S input: ``"<filter>[:<R>]"``.

    Without ``R`` the image is resized to S x S (squash). With ``R >= S`` it is torchvision's
    ``Resize(R)`` + ``CenterCrop(S)``: the shorter side becomes R, the longer ``int(R * long /
    short)``, and the S x S window starts at ``int(round((side - S) / 2.0))``. ``nearest`` alone
    is the default and the reference's keras_image_helper contract."""
    filter: str = "nearest"
    resize_to: int | None = None

    def __post_init__(self):
        if self.filter not in PIL_FILTERS:
            raise ValueError(f"unknown resize filter {self.filter!r} (one of {', '.join(PIL_FILTERS)})")
        if self.resize_to is not None and (not isinstance(self.resize_to, int) or self.resize_to < 1):
            raise ValueError(f"resize target must be a positive integer, got {self.resize_to!r}")

    @classmethod
    def parse(cls, text: "str | ResizeSpec | None", size: int | None = None) -> "ResizeSpec":
        """The spec of ``text`` ('' / None: the default); with ``size`` (the model input S) given,
        ``R < S`` is rejected here."""
        if isinstance(text, cls):
            spec = text
        else:
            text = "" if text is None else str(text).strip()
            name, sep, r = text.partition(":")
            if sep and not (r.isascii() and r.isdigit()):
                raise ValueError(f"bad preprocess spec {text!r}: expected '<filter>[:<R>]' with an integer R")
            spec = cls((name or "nearest") if not sep else name, int(r) if sep else None)
        if size is not None:
            spec.check(size)
        return spec

    def check(self, S: int) -> None:
        if self.resize_to is not None and self.resize_to < S:
            raise ValueError(f"preprocess spec {self}: the resize target {self.resize_to} is smaller than the "
                             f"model input {S}, a center crop of {S} does not fit")

    @property
    def squash(self) -> bool:
        return self.resize_to is None

    def geometry(self, H: int, W: int, S: int) -> tuple[int, int, int, int]:
        """(nh, nw, top, left): the size the H x W image is resized to and the S x S window of it."""
        self.check(S)
        R = self.resize_to
        if R is None:
            return S, S, 0, 0
        if W <= H:
            nw, nh = R, int(R * H / W)
        else:
            nh, nw = R, int(R * W / H)
        return nh, nw, int(round((nh - S) / 2.0)), int(round((nw - S) / 2.0))

    def __str__(self) -> str:
        return self.filter if self.resize_to is None else f"{self.filter}:{self.resize_to}"


NEAREST_SPEC = ResizeSpec()


def apply_spec_pil(img: Image.Image, spec: ResizeSpec, S: int) -> np.ndarray:
    """uint8 [S, S, 3] of ``img`` under ``spec`` through Pillow itself: the definition of correct
    for the GPU kernels, and the path of CPU servers and of the gateway's compat / uint8 modes."""
    if img.mode != "RGB":
        img = img.convert("RGB")
    nh, nw, top, left = spec.geometry(img.height, img.width, S)
    out = img.resize((nw, nh), PIL_FILTERS[spec.filter])
    if (nh, nw) != (S, S):
        out = out.crop((left, top, left + S, top + S))
    return np.asarray(out, dtype=np.uint8)


def xception_preprocess(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float32)
    x /= 127.5
    x -= 1.0
    return x


def image_to_tensor(img: Image.Image, target=TARGET) -> np.ndarray:
    """float32 [1, 299, 299, 3] in [-1, 1] (the reference's input_8 payload)."""
    x = np.array(img.resize(target, Image.NEAREST), dtype="float32")
    return xception_preprocess(np.array([x]))


def fetch(url: str, timeout: float = 10.0) -> bytes:
    with urllib.request.urlopen(url, timeout=timeout) as resp:
        return resp.read()


class XceptionPreprocessor:
    """Drop-in for keras_image_helper's ``create_preprocessor('xception', ...)``."""

    def __init__(self, target_size=TARGET):
        self.target_size = target_size

    def from_url(self, url: str) -> np.ndarray:
        return self.convert_to_tensor(load_image(fetch(url)))

    def from_bytes(self, data: bytes) -> np.ndarray:
        return self.convert_to_tensor(load_image(data))

    def convert_to_tensor(self, img: Image.Image) -> np.ndarray:
        if img.mode != "RGB":
            img = img.convert("RGB")
        return image_to_tensor(img, self.target_size)


def create_preprocessor(name: str, target_size=TARGET) -> XceptionPreprocessor:
    if name != "xception":
        raise ValueError(f"unsupported preprocessor {name!r} (this framework serves Xception)")
    return XceptionPreprocessor(target_size)
