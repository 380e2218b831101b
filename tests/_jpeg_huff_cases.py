"""Files and helpers shared by the entropy-decode tests (test_jpeg_huff_cpu.py, test_jpeg_huff_gpu.py):
the oracle is ``jpeg_parse`` into a buffer pre-filled with 0x5A5A."""
import functools

import numpy as np

from _jpeg_cases import encode, pants, smooth_noise

# the eight cases of test_jpeg_gpu.py
CASES = {
    "1x1": (1, 1, dict(subsampling=2, quality=75)),
    "3x9 4:2:0": (3, 9, dict(subsampling=2, quality=95)),
    "4x9 4:2:2": (4, 9, dict(subsampling=1, quality=95)),
    "5x9 4:2:0": (5, 9, dict(subsampling=2, quality=95)),
    "17x9 4:2:0": (17, 9, dict(subsampling=2, quality=75)),
    "33x47 4:2:2": (33, 47, dict(subsampling=1, quality=90)),
    "64x64 4:4:4": (64, 64, dict(subsampling=0, quality=30)),
    "64x64 grey": (64, 64, dict(quality=100)),
}


def _file(w, h, kw, **more):
    return encode(smooth_noise(w, h, 7 * w + h, "RGB" if "subsampling" in kw else "L"), **kw, **more)


@functools.lru_cache(maxsize=None)
def small_files() -> dict:
    """The eight cases, and the same with per-file (optimised) Huffman tables."""
    out = {c: _file(*CASES[c]) for c in CASES}
    out.update({c + " optimised": _file(*CASES[c], optimize=True) for c in CASES})
    return out


@functools.lru_cache(maxsize=None)
def pants_file() -> bytes:
    return encode(pants(534, 400), quality=90, subsampling=2)


@functools.lru_cache(maxsize=None)
def noise_file() -> bytes:
    return encode(smooth_noise(534, 400, 11), quality=75, subsampling=0)


def scan_range(data: bytes) -> tuple[int, int]:
    """[first entropy-coded byte, the EOI marker) of a single-scan file."""
    at = data.index(b"\xff\xda")
    return at + 2 + int.from_bytes(data[at + 2:at + 4], "big"), data.rindex(b"\xff\xd9")


def unstuff(data: bytes) -> bytes:
    """The entropy-coded bytes of the scan: FF 00 -> FF, fill FFs dropped, up to the first marker."""
    i, _ = scan_range(data)
    out = bytearray()
    while i < len(data):
        b = data[i]
        if b != 0xFF:
            out.append(b); i += 1
        elif i + 1 >= len(data):
            break
        elif data[i + 1] == 0x00:
            out.append(0xFF); i += 2
        elif data[i + 1] == 0xFF:
            i += 1
        else:
            break
    return bytes(out)


def oracle(rt, data: bytes):
    """(status, header, coefficients) of jpeg_parse into a dirty buffer."""
    st, hd = rt.jpeg_probe(data)
    if st != rt.JPEG_OK:
        return st, hd, None
    coef = np.full(hd.ncoef, 0x5A5A, np.int16)
    st, hd = rt.jpeg_parse(data, coef)
    return st, hd, coef


def prepare(rt, data: bytes):
    """(status, header, info, prepared buffer)."""
    out = np.zeros(rt.jpeg_prepare_bound(len(data)), np.uint8)
    st, hd, info = rt.jpeg_scan_prepare(data, out)
    return st, hd, info, out


def emulate(rt, data: bytes):
    """The kernels' procedure on the host -> (error word, rounds, violations, coefficients, info)."""
    st, hd, info, out = prepare(rt, data)
    assert st == rt.JPEG_OK, hd.why
    coef = np.full(hd.ncoef, 0x5A5A, np.int16)
    err, rounds, bad = rt.jpeg_huff_cpu(rt.jpeg_huff_desc(hd, info, 0, 0), out[:info.nbytes], coef)
    return err, rounds, bad, coef, info


def truncated_pants() -> bytes:
    data = pants_file()
    lo, hi = scan_range(data)
    return data[:(lo + hi) // 2]


def mutations(data: bytes, count: int, seed: int):
    """Fixed-seed single-byte mutations inside the scan."""
    rng = np.random.default_rng(seed)
    lo, hi = scan_range(data)
    for _ in range(count):
        d = bytearray(data)
        d[int(rng.integers(lo, hi))] = int(rng.integers(0, 256))
        yield bytes(d)


@functools.lru_cache(maxsize=None)
def corrupted_files() -> tuple:
    """The first two mutations of the 33x47 file that the host decoder rejects."""
    from kdl.ops import _lib
    rt, out = _lib.rt(), []
    for d in mutations(small_files()["33x47 4:2:2"], 200, 5):
        if oracle(rt, d)[0] == rt.JPEG_MALFORMED:
            out.append(d)
            if len(out) == 2:
                break
    assert len(out) == 2
    return tuple(out)
