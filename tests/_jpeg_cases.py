"""Inputs of the serving_bytes tests: images made here and encoded by Pillow (no binary fixtures)."""
import io
from pathlib import Path

import numpy as np
from PIL import Image, ImageFile

DATA = Path(__file__).parent / "data"


def smooth_noise(w: int, h: int, seed: int = 0, mode: str = "RGB") -> Image.Image:
    """Seeded smooth gradients plus noise: every coefficient band and both DC signs occur."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)], -1)
    a = np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
    return Image.fromarray(a).convert(mode)


def pants(w: int, h: int) -> Image.Image:
    return Image.open(DATA / "pants.png").convert("RGB").resize((w, h), Image.BILINEAR)


def encode(im: Image.Image, fmt: str = "JPEG", **kw) -> bytes:
    b = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 22        # Pillow's encoder buffer: tiny optimised / q100 files outgrow the default
    try:
        im.save(b, fmt, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return b.getvalue()


def pil_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def with_segments(data: bytes) -> bytes:
    """The file with a COM and an APP1 segment added behind its JFIF APP0."""
    assert data[:4] == b"\xff\xd8\xff\xe0"
    at = 4 + int.from_bytes(data[4:6], "big")
    com = b"a comment, skipped"
    app1 = b"kdl-test\0" + bytes(range(200))
    extra = (b"\xff\xfe" + (len(com) + 2).to_bytes(2, "big") + com
             + b"\xff\xe1" + (len(app1) + 2).to_bytes(2, "big") + app1)
    return data[:at] + extra + data[at:]


def decode_cpu(rt, data: bytes):
    """(status, header, RGB | None) through jpeg_probe + jpeg_parse + jpeg_pixels_cpu."""
    st, hd = rt.jpeg_probe(data)
    if st != rt.JPEG_OK:
        return st, hd, None
    coef = np.full(hd.ncoef, 0x5A5A, np.int16)      # dirty: the parser must write every coefficient
    st, hd = rt.jpeg_parse(data, coef)
    if st != rt.JPEG_OK:
        return st, hd, None
    return st, hd, rt.jpeg_pixels_cpu(hd, coef)
