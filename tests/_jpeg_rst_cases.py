"""Files and helpers shared by the restart-interval entropy-decode tests (test_jpeg_rst_cpu.py,
test_jpeg_rst_gpu.py): baseline JPEGs with a DRI segment, written by Pillow's encoder
(``restart_marker_blocks`` / ``restart_marker_rows``). The oracle is ``jpeg_parse``."""
import functools

import numpy as np

from _jpeg_cases import encode, pants, smooth_noise
from _jpeg_huff_cases import CASES, mutations, oracle, scan_range

# label -> (restart interval in MCUs, number of intervals) of the 150 x 130 4:2:0 q80 file (10 x 9 MCUs)
PREPARE = {"blocks=1": (dict(restart_marker_blocks=1), 1, 90),
           "blocks=3": (dict(restart_marker_blocks=3), 3, 30),       # the marker numbers wrap past RST7
           "rows=1": (dict(restart_marker_rows=1), 10, 9),
           "blocks=1000": (dict(restart_marker_blocks=1000), 1000, 1)}   # a DRI and no marker at all


@functools.lru_cache(maxsize=None)
def prepare_files() -> dict:
    im = smooth_noise(150, 130, 9)
    return {k: encode(im, subsampling=2, quality=80, **kw) for k, (kw, _, _) in PREPARE.items()}


@functools.lru_cache(maxsize=None)
def small_rst_files() -> dict:
    """The eight cases with blocks=2 and with rows=1, plain and with optimised tables."""
    out = {}
    for c, (w, h, kw) in CASES.items():
        im = smooth_noise(w, h, 7 * w + h, "RGB" if "subsampling" in kw else "L")
        for name, rkw in (("blocks=2", dict(restart_marker_blocks=2)), ("rows=1", dict(restart_marker_rows=1))):
            out[f"{c} {name}"] = encode(im, **kw, **rkw)
            out[f"{c} {name} optimised"] = encode(im, optimize=True, **kw, **rkw)
    return out


@functools.lru_cache(maxsize=None)
def large_rst_files() -> dict:
    return {"pants blocks=4": encode(pants(534, 400), quality=90, subsampling=2, restart_marker_blocks=4),
            "pants rows=1": encode(pants(534, 400), quality=90, subsampling=2, restart_marker_rows=1),
            # two intervals of about 40 KB: each longer than one chunk
            "noise rows=25": encode(smooth_noise(534, 400, 11), quality=75, subsampling=0, restart_marker_rows=25)}


def seed_file(label: str) -> bytes:
    """The seeds of the damage tests: '150x130 4:2:0 blocks=3', '33x47 4:2:2 blocks=2', '64x64 grey rows=1'."""
    if label.startswith("150x130"):
        return prepare_files()["blocks=3"]
    return small_rst_files()[label]


def count_intervals(rt, data: bytes) -> int:
    """What the serving path gives jpeg_prepare_bound: an upper bound of the file's intervals."""
    from kdl.serving.jpeg import _intervals
    st, hd = rt.jpeg_probe(data)
    return _intervals(data, hd) if st == rt.JPEG_OK else 0


def prepare(rt, data: bytes):
    """(status, header, info, prepared buffer), the buffer sized for the file's intervals."""
    out = np.zeros(rt.jpeg_prepare_bound(len(data), count_intervals(rt, data)), np.uint8)
    st, hd, info = rt.jpeg_scan_prepare(data, out)
    return st, hd, info, out


def tables(info, out):
    """(intervals [nint, 2] = first word, bits; groups [ngroup, 2] = first interval, count): views."""
    iv = out[info.int_off:info.int_off + 8 * info.nint].view(np.uint32).reshape(-1, 2)
    gr = out[info.grp_off:info.grp_off + 8 * info.ngroup].view(np.uint32).reshape(-1, 2)
    return iv, gr


def emulate(rt, data: bytes):
    """The kernels' procedure on the host -> (error word, rounds, violations, coefficients, info)."""
    st, hd, info, out = prepare(rt, data)
    assert st == rt.JPEG_OK and info.restart_ok and not info.device_ok, hd.why
    coef = np.full(hd.ncoef, 0x5A5A, np.int16)
    err, rounds, bad = rt.jpeg_huff_cpu(rt.jpeg_huff_desc(hd, info, 0, 0), out[:info.nbytes], coef)
    return err, rounds, bad, coef, info


def markers(data: bytes) -> list:
    """Positions of the RSTm markers: inside the scan FF Dx occurs as nothing else."""
    lo, hi = scan_range(data)
    return [i for i in range(lo, hi - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def split_scan(data: bytes) -> list:
    """The unstuffed bytes of every interval."""
    lo, hi = scan_range(data)
    at = markers(data)
    parts = []
    for a, b in zip([lo] + [m + 2 for m in at], at + [hi]):
        parts.append(data[a:b].replace(b"\xff\x00", b"\xff"))
    return parts


def marker_damage(data: bytes) -> dict:
    """label -> the file with one kind of damage to its markers."""
    at = markers(data)
    m = at[len(at) // 2]
    n = at[len(at) // 2 + 1]
    lo, hi = scan_range(data)
    swapped = bytearray(data)
    swapped[m + 1], swapped[n + 1] = data[n + 1], data[m + 1]
    renumbered = bytearray(data)
    renumbered[m + 1] = 0xD0 + ((data[m + 1] - 0xD0 + 3) & 7)
    return {"removed": data[:m] + data[m + 2:],
            "swapped": bytes(swapped),
            "duplicated": data[:m] + data[m:m + 2] + data[m:],
            "renumbered": bytes(renumbered),
            "cut": data[:(m + n) // 2],
            "fill bytes": data[:m] + b"\xff\xff" + data[m:]}


def agree(rt, data: bytes, label: str):
    """Either prepare refuses the file ('refused'), or the emulation agrees with the host decoder:
    equal coefficients when it says OK, a set error word when it says MALFORMED -> its status."""
    st, hd, want = oracle(rt, data)
    st2, hd2, info, out = prepare(rt, data)
    if st2 != rt.JPEG_OK:
        assert st != rt.JPEG_OK, label
        return "refused"
    assert not info.device_ok, label
    if not info.restart_ok:
        return "refused"
    coef = np.full(hd2.ncoef, 0x5A5A, np.int16)
    err, rounds, bad = rt.jpeg_huff_cpu(rt.jpeg_huff_desc(hd2, info, 0, 0), out[:info.nbytes], coef)
    assert bad == 0, label
    if st == rt.JPEG_OK:
        assert err == 0 and np.array_equal(coef, want), label
    else:
        assert st == rt.JPEG_MALFORMED and err != 0, label
    return st


@functools.lru_cache(maxsize=None)
def corrupted_rst_files() -> tuple:
    """The first two mutations of '33x47 4:2:2 blocks=2' that the host decoder rejects while prepare
    still answers restart_ok."""
    from kdl.ops import _lib
    rt, out = _lib.rt(), []
    for d in mutations(seed_file("33x47 4:2:2 blocks=2"), 200, 5):
        if oracle(rt, d)[0] == rt.JPEG_MALFORMED and prepare(rt, d)[2].restart_ok:
            out.append(d)
            if len(out) == 2:
                break
    assert len(out) == 2
    return tuple(out)
