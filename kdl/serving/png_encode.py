"""Cutouts as PNG files: the ``cutout_png`` / ``cutout_png_image`` / ``cutout_png_bytes`` signatures.

The cutout trio answers the raw RGBA picture and leaves the file to the caller. These three answer the cutout
trio's ``classes``, ``scores`` and ``coverage`` plus ``png_bytes`` DT_STRING [-1]: the cutout as a finished PNG
file, at most ``max_bytes`` long (default ceil(S*S*4 / 2)); a file that does not fit is answered as b"" and
counted in ``kdl_cutout_png_overflow_total``. Configuration (opt-in): ``"cutout_png": {"max_bytes": null}`` in
the version's ``kdl_model.json`` / ``synthetic.json``, or ``--cutout_png``; either needs the version's cutout
signatures. A result row is 2 + h*w + 1 front words (explain's front and the cutout's count), a length word,
then the file in ceil(max_bytes / 4) words, the bytes behind it 0 (``pack_rows`` / ``unpack_rows``).

A cutout is the one picture answer that has to be a PNG, because it carries alpha. Zlib's output is not
reproduced: the encoder's rule is defined HERE, once. ``png_rule`` in numpy is the definition, and the GPU
kernels (kernels/png_encode.hip, the ``png_encode`` op, ``add_png_encode`` in a captured program,
``encode_gpu`` below) reproduce it byte for byte. Its oracle is the decoder: Pillow opens the file and
``zlib.decompress`` of the IDAT gives the filtered rows.

``png_rule(pictures uint8 [n, H, W, C], max_bytes)``, C = 3 (colour type 2) or 4 (colour type 6), integers only:

1. filter   per row, the five PNG filter types with bpp = C (a = the byte C to the left, b = the byte above,
            c = the byte above a; all 0 outside the picture; Average is (a + b) >> 1; Paeth takes a, then b,
            then c on ties). The row keeps the type with the smallest sum of |residual as a signed byte|
            (v < 128 ? v : 256 - v), ties to the smaller type. The filtered stream is H rows of
            L = 1 + W*C bytes, the type byte first.
2. matches  every row is a segment of its own: no match reaches outside its row, and the type byte is an
            ordinary byte of it. The candidate distances are DISTANCES(C) = (1, C). At position j of row
            bytes f, the match length of distance d is 0 for j < d, else the number of k >= 0 with
            f[j+k] == f[j+k-d] before the first mismatch, capped at MAX_MATCH = 258 and at L - j.
3. parse    greedy from j = 0: best = the longest of the candidates, ties to the smaller distance; if
            best >= MIN_MATCH = 4 the token is the match (best, d) and j += best, else the literal f[j] and
            j += 1.
4. block    one deflate block per picture, BFINAL = 1. The literal/length histogram (symbols 0..285, with one
            end-of-block, 256) and the distance histogram are taken over all rows.
   lengths  ``code_lengths(counts, limit)``: the used symbols sorted by (count, symbol) ascending; one used
            symbol gets length 1. Otherwise a Huffman tree by the two-queue merge: the leaves in sorted order
            and the merged nodes in the order they were made; each step takes twice the smaller front, the
            leaf on equal weights. n[l] = the leaves at depth l, depths above ``limit`` counted at ``limit``.
            Kraft repair: while sum n[l] << (limit - l) exceeds 1 << limit: n[limit] -= 1; the largest
            l < limit with n[l] > 0 gives n[l] -= 1, n[l+1] += 2. Then the sorted symbols take lengths from
            ``limit`` downwards: the first n[limit] symbols get ``limit``, the next n[limit-1] get limit - 1, ...
            The literal/length code has limit 15; the code-length code has limit 7. The distance code
            needs no tree: DISTANCES has two members, so each used distance symbol gets length 1.
   codes    canonical (RFC 1951 3.2.2), sent bit-reversed as deflate packs Huffman codes.
   header   HLIT = the largest used literal/length symbol + 1 (>= 257); HDIST = the largest used distance
            symbol + 1, or 1 with a single length 0 where no match was made. The HLIT + HDIST lengths, as
            one sequence, are run-coded greedily from the left, r = the run of equal values at position i:
            value 0 and r >= 3: one 17 (n = min(r, 138) <= 10) or 18 (n > 10) for n zeros; else a value equal
            to the last value sent and r >= 3: one 16 for n = min(r, 6); else the value itself.
            HCLEN = the last used entry of the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, + 1, >= 4.
   choice   the same tokens are totalled under the fixed code (BTYPE 01); the dynamic block (BTYPE 10, header
            included) is written only where it is strictly shorter.
5. file     the PNG signature; IHDR (W, H, 8 bit, colour type 2 or 6, no interlace); one IDAT holding 78 01,
            the block and the Adler-32 of the filtered stream; IEND; CRC-32 on each chunk.
6. overflow a file longer than ``max_bytes`` is answered as b"".

The op writes one row of 32-bit words per picture: optional front words copied from the caller's rows, a
length word (0 = overflow), then the file in ceil(max_bytes / 4) words, the bytes behind it 0.
"""
from __future__ import annotations

import struct
import zlib
from pathlib import Path

import numpy as np

from ..engine.base import CutoutPng, cutout_png_cap, pack_cutout_png, unpack_cutout_png  # noqa: F401
from . import protos as P

CUTOUT_PNG_SIGNATURE = "cutout_png"
CUTOUT_PNG_IMAGE_SIGNATURE = "cutout_png_image"
CUTOUT_PNG_BYTES_SIGNATURE = "cutout_png_bytes"
CUTOUT_PNG_SIGNATURES = (CUTOUT_PNG_SIGNATURE, CUTOUT_PNG_IMAGE_SIGNATURE, CUTOUT_PNG_BYTES_SIGNATURE)
OUTPUT_KEYS = ("classes", "scores", "coverage", "png_bytes")
KEYS = ("max_bytes",)
MAX_SIDE = 1024                                # kPngEncMaxSide
MAX_CAP = 1 << 24                              # kPngEncMaxCap
MIN_MATCH = 4
MAX_MATCH = 258
FILE_OVERHEAD = 63                             # every byte of the file that is not the deflate block
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
# match length - 3 -> (length symbol, extra bits, their value); 258 is symbol 285, not 284 + 31
_LEN_SYM = np.zeros(256, np.int64)
for _s, _b in enumerate(LEN_BASE):
    _LEN_SYM[_b - 3:] = 257 + _s
_LEN_XBITS = np.asarray(LEN_EXTRA, np.int64)[_LEN_SYM - 257]
_LEN_XVAL = np.arange(3, 259) - np.asarray(LEN_BASE, np.int64)[_LEN_SYM - 257]
_FIXED_LENS = np.asarray([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, np.int64)      # 286 and 287 take codes, never sent


def distances(C: int) -> tuple:
    """The candidate distances of a picture with C bytes a pixel, smaller first."""
    return (1, C)


def default_cap(H: int, W: int, C: int = 4) -> int:
    return (H * W * C + 1) // 2


# ------------------------------------------------------------------------------------------ 1. filter
def filter_rows(pic: np.ndarray) -> np.ndarray:
    """uint8 [H, W, C] -> the filtered stream uint8 [H, 1 + W*C]."""
    H, W, C = pic.shape
    x = pic.reshape(H, W * C).astype(np.int64)
    a = np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, C:] = b[:, :-C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255          # [5, H, W*C]
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)                          # [5, H]
    kind = np.argmin(cost, axis=0)                                                  # the first minimum
    out = np.empty((H, 1 + W * C), np.uint8)
    out[:, 0] = kind
    out[:, 1:] = res[kind, np.arange(H)]
    return out


# ------------------------------------------------------------------------------------------ 2-3. tokens
def match_lengths(f: np.ndarray, d: int) -> np.ndarray:
    """f uint8 [H, L] -> the match length of distance d at every position, int64 [H, L]."""
    H, L = f.shape
    stop = np.full((H, L), L, np.int64)                     # the first mismatch at or behind j
    j = np.arange(L)
    ne = np.ones((H, L), bool)
    ne[:, d:] = f[:, d:] != f[:, :-d]
    stop[ne] = np.broadcast_to(j, (H, L))[ne]
    stop = np.minimum.accumulate(stop[:, ::-1], axis=1)[:, ::-1]
    return np.minimum(stop - j, MAX_MATCH)


def tokens(f: np.ndarray, C: int) -> tuple:
    """The greedy parse of the filtered rows -> (lit, length, dist index) int64 arrays, one entry per token in
    stream order: length 0 = the literal ``lit``, else a match of DISTANCES[dist index]."""
    H, L = f.shape
    best = np.zeros((H, L), np.int64)
    which = np.zeros((H, L), np.int64)
    for i, d in enumerate(distances(C)):
        m = match_lengths(f, d)
        which[m > best] = i
        best = np.maximum(best, m)
    step = np.where(best >= MIN_MATCH, best, 1)
    at = []
    for r in range(H):
        nxt, j, base = step[r].tolist(), 0, r * L
        while j < L:
            at.append(base + j)
            j += nxt[j]
    at = np.asarray(at, np.int64)
    length = np.where(best >= MIN_MATCH, best, 0).reshape(-1)[at]
    return f.reshape(-1).astype(np.int64)[at], length, which.reshape(-1)[at]


# ------------------------------------------------------------------------------------------ 4. block
def code_lengths(counts, limit: int) -> np.ndarray:
    """The length-limited code of the module docstring: counts [n] -> lengths int64 [n], 0 for count 0."""
    counts = [int(c) for c in counts]
    order = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    lens = np.zeros(len(counts), np.int64)
    n = len(order)
    if n == 1:
        lens[order[0][1]] = 1
    if n < 2:
        return lens
    weight = [c for c, _ in order] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    leaf, node = 0, n
    for made in range(n, 2 * n - 1):
        for _ in range(2):
            if leaf < n and (node >= made or weight[leaf] <= weight[node]):
                pick, leaf = leaf, leaf + 1
            else:
                pick, node = node, node + 1
            weight[made] += weight[pick]
            parent[pick] = made
    depth = [0] * (2 * n - 1)
    num = [0] * (limit + 1)
    for i in range(2 * n - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
        if i < n:
            num[min(depth[i], limit)] += 1
    total = sum(num[l] << (limit - l) for l in range(1, limit + 1))
    while total > 1 << limit:
        num[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if num[l]:
                num[l] -= 1
                num[l + 1] += 2
                break
        total -= 1
    i = 0
    for l in range(limit, 0, -1):
        for _ in range(num[l]):
            lens[order[i][1]] = l
            i += 1
    return lens


def canonical(lens: np.ndarray) -> np.ndarray:
    """Canonical codes of the lengths, bit-reversed: the value deflate writes from its lowest bit."""
    codes = np.zeros(len(lens), np.int64)
    code = 0
    for l in range(1, 16):
        for s in np.nonzero(lens == l)[0]:
            codes[s] = int(format(code, f"0{l}b")[::-1], 2)
            code += 1
        code <<= 1
    return codes


def header_runs(seq) -> list:
    """The HLIT + HDIST lengths -> [(code-length symbol, extra bits, their value)] by the greedy rule."""
    out, i, prev, n = [], 0, -1, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            k = min(r, 138)
            out.append((17, 3, k - 3) if k <= 10 else (18, 7, k - 11))
            i, prev = i + k, 0
        elif v == prev and r >= 3:
            k = min(r, 6)
            out.append((16, 2, k - 3))
            i += k
        else:
            out.append((int(v), 0, 0))
            i, prev = i + 1, v
    return out


def pack_bits(values, nbits) -> tuple:
    """(value, bit count) pairs -> (the bytes deflate's LSB-first packing gives, the total bits)."""
    values, nbits = np.asarray(values, np.int64), np.asarray(nbits, np.int64)
    total = int(nbits.sum())
    start = np.cumsum(nbits) - nbits
    k = np.arange(total) - np.repeat(start, nbits)
    bits = (np.repeat(values, nbits) >> k) & 1
    return np.packbits(bits.astype(np.uint8), bitorder="little").tobytes(), total


def block_code(hist: np.ndarray, dhist: np.ndarray) -> tuple:
    """The histograms of a picture (end-of-block counted) -> (the header as (value, bits) pairs, the
    literal/length lengths [288], the distance lengths [30]) of the block the rule writes: steps "lengths"
    to "choice"."""
    lens = code_lengths(hist, 15)
    dlens = (dhist > 0).astype(np.int64)
    hlit = int(np.nonzero(hist)[0][-1]) + 1
    hdist = int(np.nonzero(dhist)[0][-1]) + 1 if dhist.any() else 1
    runs = header_runs(list(lens[:hlit]) + list(dlens[:hdist]))
    chist = np.bincount([s for s, _, _ in runs], minlength=19)
    clens = code_lengths(chist, 7)
    ccodes = canonical(clens)
    hclen = max(4, max(i for i, s in enumerate(CLEN_ORDER) if clens[s]) + 1)
    head = [(1, 1), (2, 2), (hlit - 257, 5), (hdist - 1, 5), (hclen - 4, 4)] + [(int(clens[s]), 3) for s in CLEN_ORDER[:hclen]]
    for s, nb, v in runs:
        head += [(int(ccodes[s]), int(clens[s])), (v, nb)]
    extra = int((hist[257:286] * np.asarray(LEN_EXTRA)).sum())
    dyn = sum(nb for _, nb in head) + int((hist * lens).sum()) + int((dhist * dlens).sum()) + extra
    fix = 3 + int((hist * _FIXED_LENS).sum()) + 5 * int(dhist.sum()) + extra
    if dyn >= fix:
        head, lens, dlens = [(1, 1), (1, 2)], _FIXED_LENS, np.full(30, 5, np.int64)
    return head, lens, dlens


def deflate_block(f: np.ndarray, C: int) -> bytes:
    """The one final deflate block of the filtered rows."""
    lit, length, which = tokens(f, C)
    is_m = length > 0
    sym = np.where(is_m, _LEN_SYM[np.maximum(length, 3) - 3], lit)
    xbits = np.where(is_m, _LEN_XBITS[np.maximum(length, 3) - 3], 0)
    xval = np.where(is_m, _LEN_XVAL[np.maximum(length, 3) - 3], 0)
    dsym = np.asarray(distances(C), np.int64)[which] - 1       # distances 1..4 are the codes 0..3, no extra bits
    hist = np.bincount(sym, minlength=288)
    hist[256] = 1
    dhist = np.bincount(dsym[is_m], minlength=30)

    head, lens, dlens = block_code(hist, dhist)
    codes, dcodes = canonical(lens), canonical(dlens)
    # per token: the literal/length code, the length's extra bits, the distance code (0 bits for a literal)
    v = np.stack([codes[sym], xval, np.where(is_m, dcodes[dsym], 0)], axis=1).reshape(-1)
    nb = np.stack([lens[sym], xbits, np.where(is_m, dlens[dsym], 0)], axis=1).reshape(-1)
    hv, hn = zip(*head)
    data, _ = pack_bits(np.concatenate([hv, v, [codes[256]]]), np.concatenate([hn, nb, [lens[256]]]))
    return data


# ------------------------------------------------------------------------------------------ 5-6. file
def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def file_head(H: int, W: int, C: int) -> bytes:
    """The 33 bytes in front of the IDAT chunk: the signature and IHDR."""
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 6, 0, 0, 0))


def png_rule(pictures, max_bytes: int | None = None) -> list:
    """uint8 [n, H, W, C] -> one PNG file per picture (module docstring); b"" where it is longer than
    ``max_bytes`` (None: ceil(H*W*C / 2))."""
    pictures = np.asarray(pictures)
    assert pictures.dtype == np.uint8 and pictures.ndim == 4 and pictures.shape[3] in (3, 4), pictures.shape
    n, H, W, C = pictures.shape
    assert 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE, (H, W)
    cap = default_cap(H, W, C) if max_bytes is None else int(max_bytes)
    files = []
    for pic in pictures:
        f = filter_rows(pic)
        data = b"\x78\x01" + deflate_block(f, C) + struct.pack(">I", zlib.adler32(f.tobytes()))
        out = file_head(H, W, C) + _chunk(b"IDAT", data) + _chunk(b"IEND", b"")
        assert len(out) == len(data) - 6 + FILE_OVERHEAD
        files.append(out if len(out) <= cap else b"")
    return files


def idat_of(file: bytes) -> bytes:
    """The data of a file's (only) IDAT chunk."""
    n = struct.unpack(">I", file[33:37])[0]
    assert file[37:41] == b"IDAT", file[33:41]
    return file[41:41 + n]


# ------------------------------------------------------------------------------------------ rows and config
def check(spec: CutoutPng) -> CutoutPng:
    m = spec.max_bytes
    if m is not None and (isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= MAX_CAP):
        raise ValueError(f"cutout_png max_bytes must be null or an integer in 1..{MAX_CAP}, got {m!r}")
    return spec


def pack_rows(classes, scores, heat, counts, files, max_bytes: int) -> np.ndarray:
    """The engine's row layout [n, 2 + h*w + 2 + ceil(max_bytes/4)] fp32 words."""
    return pack_cutout_png(classes, scores, heat, counts, files, max_bytes)


def unpack_rows(rows, h: int, w: int, max_bytes: int) -> tuple:
    """-> (classes int32 [n], scores fp32 [n], heat fp32 [n, h, w], counts uint32 [n], files: n bytes objects)."""
    return unpack_cutout_png(np.ascontiguousarray(rows, dtype=np.float32), h, w, max_bytes)


def resolve(path: Path, flag: bool = False) -> CutoutPng | None:
    """The version's ``CutoutPng``: its "cutout_png" block, or the defaults under ``--cutout_png``; None where
    neither is there. ValueError (naming the file) fails the load."""
    from .outputs import _meta
    path = Path(path)
    meta, name = _meta(path)
    if "cutout_png" not in meta and not flag:
        return None
    block = meta.get("cutout_png", {})
    if not isinstance(block, dict):
        raise ValueError(f"{path / name}: \"cutout_png\" must be an object like {{\"max_bytes\": null}}")
    unknown = sorted(set(block) - set(KEYS))
    if unknown:
        raise ValueError(f"{path / name}: unknown \"cutout_png\" keys {unknown}")
    try:
        return check(CutoutPng(**block))
    except ValueError as e:
        raise ValueError(f"{path / name}: {e}") from e


def add_signatures(src, path, flag: bool = False) -> None:
    """Give a loaded ModelSource that has the cutout trio and a "cutout_png" block (or the flag) the three
    cutout_png signatures. They are told from the cutout trio by their last output, a DT_STRING."""
    from ..engine import registry
    from .outputs import add_trio
    spec = resolve(path, flag)
    if spec is None:
        return
    if src.cutout is None:
        raise ValueError(f"{path}: \"cutout_png\" needs the cutout signatures, which this version does not have")
    if src.input_size > MAX_SIDE:
        raise ValueError(f"{path}: cutout_png takes inputs up to {MAX_SIDE}, not {src.input_size}")
    info = registry.get(src.family)
    h, w = info.map_size
    src.cutout_png = spec
    outs = (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)), ("coverage", P.DT_FLOAT, (-1, 1)),
            ("png_bytes", P.DT_STRING, (-1,)))
    add_trio(src, CUTOUT_PNG_SIGNATURES, "classes", (-1, 1), outputs=outs, explain=(h, w),
             rollout=info.cam_oracle is None)


# ------------------------------------------------------------------------------------------ the op
def rows_of(files, cap: int) -> np.ndarray:
    """The rows the op writes for these files, without front words: uint32 [n, 1 + ceil(cap / 4)]."""
    rows = np.zeros((len(files), 1 + (cap + 3) // 4), np.uint32)
    for i, data in enumerate(files):
        rows[i, 0] = len(data)
        rows[i, 1:].view(np.uint8)[:len(data)] = np.frombuffer(data, np.uint8)
    return rows


def encode_gpu(pictures, max_bytes: int | None = None, work=None):
    """``png_rule`` on the device: uint8 [n, H, W, C] CUDA tensor (rows and pictures may be strided, pixels
    packed) -> (files, rows int32 [n, 1 + ceil(cap / 4)] as the op wrote them, the workspace for a next call)."""
    import torch

    from ..ops import _lib
    lib = _lib.lib()
    n, H, W, C = pictures.shape
    assert pictures.dtype == torch.uint8 and pictures.is_cuda and pictures.stride(3) == 1 and pictures.stride(2) == C
    cap = default_cap(H, W, C) if max_bytes is None else int(max_bytes)
    if max(H, W) > lib.PNG_ENC_MAX_SIDE or not 1 <= cap <= lib.PNG_ENC_MAX_CAP:
        raise ValueError(f"png_encode: a {H} x {W} picture in at most {cap} bytes; the kernel takes sides up to "
                         f"{lib.PNG_ENC_MAX_SIDE} and {lib.PNG_ENC_MAX_CAP} bytes")
    if work is None:
        work = torch.zeros(lib.png_encode_workspace(n, H, W, C, cap), dtype=torch.uint8, device=pictures.device)
    rows = torch.empty((n, 1 + (cap + 3) // 4), dtype=torch.int32, device=pictures.device)
    lib.png_encode(dict(inp=_lib.ptr(pictures), ldi=pictures.stride(0) if n > 1 else H * pictures.stride(1),
                        row_stride=pictures.stride(1) if H > 1 else W * C, front=None, nfront=0, ldf=0,
                        out=_lib.ptr(rows), ldo=rows.shape[1], work=_lib.ptr(work), B=n, H=H, W=W, C=C, cap=cap),
                   _lib.stream_ptr())
    host = rows.cpu().numpy()
    body = np.ascontiguousarray(host[:, 1:]).view(np.uint8).reshape(n, -1)
    return [body[i, :k].tobytes() for i, k in enumerate(host[:, 0])], rows, work
