"""Overlays as JPEG files: the ``overlay_jpeg`` / ``overlay_jpeg_image`` / ``overlay_jpeg_bytes`` signatures.

They answer what the ``overlay`` trio answers, with the rendered picture as a finished baseline JPEG file
(``jpeg_bytes`` DT_STRING [-1]) instead of raw pixels. The encoder is integer arithmetic and is defined
HERE, once: ``encode_rule`` in numpy is what CPU servers answer and what the GPU kernel
(kernels/jpeg_encode.hip, ``EngineBase(overlay_jpeg=...)``) reproduces byte for byte. Its oracle is Pillow:
the file is what ``Image.save(buf, "JPEG", quality=Q, subsampling=s, optimize=False)`` writes.

1. colour    libjpeg's 16-bit fixed point: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
             Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
2. sampling  "4:4:4" or "4:2:0" (the default). Y and 4:4:4 chroma are padded to whole 8 x 8 blocks by
             replicating the last column and row. 4:2:0 chroma replicates the last full-resolution row only
             to make H even and the last column as far as needed, averages 2 x 2 as (a + b + c + d + bias) >> 2
             with bias 1, 2, 1, 2 ... along each output row, THEN replicates the last downsampled row.
3. DCT       libjpeg's ``islow`` on sample - 128 (rows, then columns; 8 x the true DCT).
4. quantise  Annex K tables scaled by the quality (``quant_tables``); q8 = 8 * entry,
             coefficient = sign(c) * ((|c| + (q8 >> 1)) // q8).
5. scan      one interleaved scan, no restart markers, the four Annex K Huffman tables. A Y block outside
             the component's ceil(H/8) x ceil(W/8) grid is a dummy: no AC, the DC of the block before it in
             its MCU. The last byte is filled with 1 bits, 0x00 follows every 0xFF.
6. file      SOI, APP0 (JFIF 1.01, density 1 x 1), two DQT, SOF0, four DHT, SOS: ``HEADER_BYTES`` = 623
             bytes (``header``), the scan, EOI.

Configuration: ``"overlay_jpeg": {"quality": 85, "subsampling": "4:2:0", "max_bytes": null}`` in the
version's ``kdl_model.json`` / ``synthetic.json`` turns the trio on (an empty object: these defaults, and
``max_bytes`` = ceil(S*S*3/2)); so does ``--overlay_jpeg_quality``. A result row is 2 + h*w words (class,
score, map), one length word and ceil(max_bytes/4) words of file (``pack_rows`` / ``unpack_rows``); a file
longer than ``max_bytes`` has length 0 and is answered as the empty string.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from ..engine.base import (OverlayJpeg, overlay_jpeg_cap, pack_overlay_jpeg,  # noqa: F401
                           unpack_overlay_jpeg)
from . import protos as P

OVERLAY_JPEG_SIGNATURES = ("overlay_jpeg", "overlay_jpeg_image", "overlay_jpeg_bytes")
OUTPUT_KEYS = ("classes", "scores", "heatmap", "jpeg_bytes")
SUBSAMPLINGS = ("4:4:4", "4:2:0")              # index = JpegEncodeArgs.sampling; Pillow's subsampling 0 and 2
HEADER_BYTES = 623

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                   13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                   45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
QUANT_BASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)
_AC_LUM = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435"
    "363738393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798"
    "999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4"
    "f5f6f7f8f9fa")
_AC_CHR = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a"
    "35363738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a9293949596"
    "9798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4"
    "f5f6f7f8f9fa")
# (class << 4 | id, code counts per length 1..16, symbols) in the file's order: DC0, AC0, DC1, AC1
HUFF_SPECS = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), _AC_LUM),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), _AC_CHR),
)


def _codes(bits, vals) -> tuple:
    """(code [256], length [256]) of a table's symbols, 0 where a symbol has no code."""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for n, cnt in enumerate(bits, start=1):
        for _ in range(cnt):
            code[vals[k]], length[vals[k]] = c, n
            c, k = c + 1, k + 1
        c <<= 1
    return code, length


# [table 0 luminance / 1 chrominance] -> (code, length)
DC_CODES = (_codes(*HUFF_SPECS[0][1:]), _codes(*HUFF_SPECS[2][1:]))
AC_CODES = (_codes(*HUFF_SPECS[1][1:]), _codes(*HUFF_SPECS[3][1:]))


def check(spec: OverlayJpeg) -> OverlayJpeg:
    """ValueError for a quality outside 1..100, an unknown sampling or a ``max_bytes`` that is no positive integer."""
    q = spec.quality
    if isinstance(q, bool) or not isinstance(q, int) or not 1 <= q <= 100:
        raise ValueError(f"overlay_jpeg quality must be an integer in 1..100, got {q!r}")
    if spec.subsampling not in SUBSAMPLINGS:
        raise ValueError(f"overlay_jpeg subsampling must be one of {SUBSAMPLINGS}, got {spec.subsampling!r}")
    m = spec.max_bytes
    if m is not None and (isinstance(m, bool) or not isinstance(m, int) or m < 1):
        raise ValueError(f"overlay_jpeg max_bytes must be a positive integer or null, got {m!r}")
    return spec


def quant_tables(quality: int) -> np.ndarray:
    """int64 [2, 64] in natural order: the Annex K tables at ``quality`` (1..100)."""
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must lie in 1..100, got {quality!r}")
    s = 5000 // int(quality) if quality < 50 else 200 - 2 * int(quality)
    return np.clip((np.asarray(QUANT_BASE, np.int64) * s + 50) // 100, 1, 255)


def header(H: int, W: int, quality: int, subsampling: str = "4:2:0") -> bytes:
    """The ``HEADER_BYTES`` bytes in front of the scan."""
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"a JPEG picture is 1..65535 pixels a side, got {H} x {W}")
    q = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in q[i][ZIGZAG])
    ys = 0x22 if subsampling == "4:2:0" else 0x11
    out += (b"\xff\xc0\x00\x11\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + b"\x03"
            + bytes([1, ys, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, bits, vals in HUFF_SPECS:
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc]) + bytes(bits) + vals
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def _planes(rgb: np.ndarray, subsampling: str) -> tuple:
    """Steps 1 and 2: (Y, Cb, Cr) int64 planes, each padded to whole 8 x 8 blocks."""
    H, W = rgb.shape[:2]
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16

    def pad(p, h, w):
        return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")

    def down(p):
        h2, w2 = (H + 1) // 2, (W + 1) // 2
        p = pad(p, 2 * h2, 16 * -(-w2 // 8))
        bias = 1 + (np.arange(p.shape[1] // 2) & 1)
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        return pad(d, 8 * -(-h2 // 8), d.shape[1])

    h8, w8 = 8 * -(-H // 8), 8 * -(-W // 8)
    if subsampling == "4:2:0":
        return pad(y, h8, w8), down(cb), down(cr)
    return pad(y, h8, w8), pad(cb, h8, w8), pad(cr, h8, w8)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first: bool):
    """libjpeg jfdctint.c, one pass along the LAST axis of int64 [..., 8]."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = np.empty_like(d)
    out[..., 0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[..., 4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = _descale(z1 + t13 * 6270, n)
    out[..., 6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def _coefficients(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """Steps 3 and 4: a padded plane -> int64 [block rows, block columns, 64] in zig-zag order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = (plane - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)               # [bh, bw, row, column]
    d = _dct_pass(d, True)
    d = _dct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
    q8 = 8 * q.reshape(8, 8)
    c = np.sign(d) * ((np.abs(d) + (q8 >> 1)) // q8)
    return c.reshape(bh, bw, 64)[..., ZIGZAG]


def _nbits(v):
    """Bits of |v| (0 for 0), for |v| < 2**16."""
    a = np.abs(v)
    n = np.zeros(a.shape, np.int64)
    for k in range(16):
        n += a >= (1 << k)
    return n


def scan_blocks(rgb: np.ndarray, quality: int, subsampling: str) -> tuple:
    """Steps 1 to 4 and the scan's order: (coefficients int64 [blocks, 64] zig-zag, the DC already a difference;
    table int64 [blocks]: 0 luminance, 1 chrominance)."""
    H, W = rgb.shape[:2]
    q = quant_tables(quality)
    y, cb, cr = _planes(rgb, subsampling)
    cy, ccb, ccr = _coefficients(y, q[0]), _coefficients(cb, q[1]), _coefficients(cr, q[1])
    hs = 2 if subsampling == "4:2:0" else 1
    my, mx = -(-H // (8 * hs)), -(-W // (8 * hs))
    gy, gx = cy.shape[:2]                                                        # ceil(H/8), ceil(W/8)
    full = np.zeros((my * hs, mx * hs, 64), np.int64)
    full[:gy, :gx] = cy
    # [MCU row, MCU column, block of the MCU in raster order, 64]
    ym = full.reshape(my, hs, mx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, hs * hs, 64)
    for i in range(1, hs * hs):                                                  # dummies: the DC of the block before
        by = np.arange(my)[:, None] * hs + i // hs
        bx = np.arange(mx)[None, :] * hs + i % hs
        dummy = (by >= gy) | (bx >= gx)
        ym[..., i, 0] = np.where(dummy, ym[..., i - 1, 0], ym[..., i, 0])
    mcus = np.concatenate([ym, ccb[:my, :mx, None], ccr[:my, :mx, None]], axis=2).reshape(my * mx, hs * hs + 2, 64)
    ny = hs * hs
    ydc = mcus[:, :ny, 0].reshape(-1)
    mcus[:, :ny, 0] = (ydc - np.concatenate([[0], ydc[:-1]])).reshape(-1, ny)
    for c in (ny, ny + 1):
        mcus[:, c, 0] -= np.concatenate([[0], mcus[:-1, c, 0]])
    table = np.tile(np.array([0] * ny + [1, 1]), my * mx)
    return mcus.reshape(-1, 64), table


def entropy_bits(blocks: np.ndarray, table: np.ndarray) -> tuple:
    """Step 5's tokens in scan order: (value int64 [n], bit length int64 [n]); a token is a Huffman code with
    the value bits that follow it."""
    n = blocks.shape[0]
    dc = blocks[:, 0]
    nb = _nbits(dc)
    dcode = np.where(table == 0, DC_CODES[0][0][nb], DC_CODES[1][0][nb])
    dlen = np.where(table == 0, DC_CODES[0][1][nb], DC_CODES[1][1][nb])
    val = (dcode << nb) | ((dc - (dc < 0)) & ((1 << nb) - 1))
    keys, vals, lens = [np.arange(n) * 256], [val], [dlen + nb]
    bi, ki = np.nonzero(blocks[:, 1:])
    ki = ki + 1
    first = np.concatenate([[True], bi[1:] != bi[:-1]]) if bi.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate([[0], ki[:-1]]))
    run = ki - prev - 1
    v = blocks[bi, ki]
    nb = _nbits(v)
    t = table[bi]
    sym = ((run & 15) << 4) | nb
    code = np.where(t == 0, AC_CODES[0][0][sym], AC_CODES[1][0][sym])
    clen = np.where(t == 0, AC_CODES[0][1][sym], AC_CODES[1][1][sym])
    keys.append(bi * 256 + ki * 4 + 3)
    vals.append((code << nb) | ((v - (v < 0)) & ((1 << nb) - 1)))
    lens.append(clen + nb)
    for z in range(3):                                                           # up to three ZRL in front of a symbol
        m = run >= 16 * (z + 1)
        keys.append(bi[m] * 256 + ki[m] * 4 + z)
        vals.append(np.where(t[m] == 0, AC_CODES[0][0][0xF0], AC_CODES[1][0][0xF0]))
        lens.append(np.where(t[m] == 0, AC_CODES[0][1][0xF0], AC_CODES[1][1][0xF0]))
    eob = np.nonzero(blocks[:, 63] == 0)[0]
    keys.append(eob * 256 + 255)
    vals.append(np.where(table[eob] == 0, AC_CODES[0][0][0], AC_CODES[1][0][0]))
    lens.append(np.where(table[eob] == 0, AC_CODES[0][1][0], AC_CODES[1][1][0]))
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    order = np.argsort(keys, kind="stable")
    return vals[order], lens[order]


def pack_scan(vals: np.ndarray, lens: np.ndarray) -> bytes:
    """Tokens -> the scan's bytes: most significant bit first, the last byte filled with 1 bits, 0x00 behind
    every 0xFF."""
    total = int(lens.sum())
    tok = np.repeat(np.arange(lens.size), lens)
    start = np.cumsum(lens) - lens
    shift = lens[tok] - 1 - (np.arange(total) - start[tok])
    bits = ((vals[tok] >> shift) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-total % 8, np.uint8)])
    by = np.packbits(bits)
    ff = np.nonzero(by == 0xFF)[0]
    return np.insert(by, ff + 1, 0).tobytes()


def encode_rule(rgb_u8, quality: int = 85, subsampling: str = "4:2:0") -> bytes:
    """THE definition: uint8 [H, W, 3] -> the bytes of a baseline JPEG file."""
    rgb = np.asarray(rgb_u8)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or 0 in rgb.shape:
        raise ValueError(f"the picture must be uint8 [H, W, 3], got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[:2]
    head = header(H, W, quality, subsampling)
    return head + pack_scan(*entropy_bits(*scan_blocks(rgb, quality, subsampling))) + b"\xff\xd9"


# ------------------------------------------------------------------------------------------ rows
def pack_rows(classes, scores, heat, files, max_bytes: int) -> np.ndarray:
    """The engine's row layout [n, 2 + h*w + 1 + ceil(max_bytes/4)] fp32 words."""
    return pack_overlay_jpeg(classes, scores, heat, files, max_bytes)


def unpack_rows(rows, h: int, w: int, max_bytes: int) -> tuple:
    """-> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], files: a list of n bytes objects)."""
    return unpack_overlay_jpeg(np.ascontiguousarray(rows, dtype=np.float32), h, w, max_bytes)


# ------------------------------------------------------------------------------------------ config
def resolve(path: Path, quality_flag: int | None = None) -> OverlayJpeg | None:
    """The version's ``OverlayJpeg``: its "overlay_jpeg" block over the defaults, ``--overlay_jpeg_quality``
    over that; None where neither is there. ValueError (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    if "overlay_jpeg" not in meta and quality_flag is None:
        return None
    block = meta.get("overlay_jpeg", {})
    if not isinstance(block, dict):
        raise ValueError(f"{path / name}: \"overlay_jpeg\" must be an object like {{\"quality\": 85}}")
    unknown = sorted(set(block) - {"quality", "subsampling", "max_bytes"})
    if unknown:
        raise ValueError(f"{path / name}: unknown \"overlay_jpeg\" keys {unknown}")
    try:
        spec = check(OverlayJpeg(**block))
    except ValueError as e:
        raise ValueError(f"{path / name}: {e}") from e
    if quality_flag is not None:
        if isinstance(quality_flag, bool) or not isinstance(quality_flag, int) or not 1 <= quality_flag <= 100:
            raise ValueError(f"--overlay_jpeg_quality must be an integer in 1..100, got {quality_flag!r}")
        spec = OverlayJpeg(quality_flag, spec.subsampling, spec.max_bytes)
    return spec


def add_signatures(src, path, quality_flag: int | None = None) -> None:
    """Give a loaded ModelSource that has the overlay trio and an "overlay_jpeg" block (or the flag) the three
    overlay_jpeg signatures. They are told from the overlay trio by their last output, a DT_STRING."""
    from .explain import map_outputs
    from .outputs import add_trio
    spec = resolve(path, quality_flag)
    if spec is None:
        return
    if src.overlay is None:
        raise ValueError(f"{path}: \"overlay_jpeg\" needs the overlay signatures, which this family does not have")
    from ..engine import registry
    info = registry.get(src.family)
    h, w = info.map_size
    src.overlay_jpeg = spec
    outs = map_outputs(h, w) + (("jpeg_bytes", P.DT_STRING, (-1,)),)
    add_trio(src, OVERLAY_JPEG_SIGNATURES, "classes", (-1, 1), outputs=outs, explain=(h, w),
             rollout=info.cam_oracle is None, overlay=src.input_size)
