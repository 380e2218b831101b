"""The device entropy decode on the host: jpeg_scan_prepare stages what the kernels read, and
jpeg_huff_cpu runs their procedure (subsequences, fixed-point rounds, block scan, write pass, DC
sums) through the shared code of csrc/runtime/jpeg_huff.h. The oracle is jpeg_parse: equal
coefficients for every file it accepts, a set error word for every scan it rejects."""
import numpy as np
import pytest

from _jpeg_cases import encode, smooth_noise
from _jpeg_huff_cases import (emulate, mutations, noise_file, oracle, pants_file, prepare, scan_range, small_files,
                              truncated_pants, unstuff)
from kdl.ops import _lib

rt = _lib.rt()


# ------------------------------------------------------------------------------ prepare
def _staged(info, out) -> bytes:
    words = out[info.scan_off:info.scan_off + info.scan_bytes].view(np.uint32)
    return words.astype(">u4").tobytes()             # the words hold the scan big-endian


def _check_prepare(data):
    st, hd, info, out = prepare(rt, data)
    assert st == rt.JPEG_OK, hd.why
    want = unstuff(data)
    assert info.nbits == 8 * len(want)
    staged = _staged(info, out)
    assert staged[:len(want)] == want
    assert len(staged) >= len(want) + 4 and not any(staged[len(want):])     # zero padded
    assert info.scan_off == 2 * hd.ncomp * rt.JPEG_HUFF_TAB_BYTES and info.nbytes == info.scan_off + info.scan_bytes
    assert info.device_ok
    return hd, info


def test_prepare_unstuffs_the_scan():
    q100 = small_files()["64x64 grey"]
    lo, hi = scan_range(q100)
    assert b"\xff\x00" in q100[lo:hi]                 # the file has stuffed bytes
    hd, info = _check_prepare(q100)
    assert info.nb == 1 and info.comp == [0] and info.nblocks == 64
    filled = q100[:hi] + b"\xff" + q100[hi:]          # a fill byte in front of EOI
    _check_prepare(filled)
    assert unstuff(filled) == unstuff(q100)
    hd, info = _check_prepare(pants_file())
    assert info.nb == 6 and info.comp == [0, 0, 0, 0, 1, 2] and info.nblocks == 34 * 25 * 6
    hd, info = _check_prepare(small_files()["33x47 4:2:2"])
    assert info.nb == 4 and info.comp == [0, 0, 1, 2]


def test_prepare_statuses_equal_jpeg_parse():
    im = smooth_noise(64, 48, 2)
    base = encode(im, quality=80)
    at = base.index(b"\xff\xc4")
    seg = 2 + int.from_bytes(base[at + 2:at + 4], "big")
    nodim = bytearray(base)
    sof = base.index(b"\xff\xc0")
    nodim[sof + 5:sof + 7] = b"\0\0"
    files = {"progressive": encode(im, quality=80, progressive=True),
             "cmyk": encode(im.convert("CMYK"), quality=80),
             "png": encode(im, "PNG"), "empty": b"",
             "missing table": base[:at] + base[at + seg:],
             "short segment": base[:at + 2] + b"\xff\xff" + base[at + 4:],
             "zero dimension": bytes(nodim), "no scan": base[:base.index(b"\xff\xda")]}
    seen = set()
    for label, data in files.items():
        coef = np.zeros(1 << 16, np.int16)
        st, hd = rt.jpeg_parse(data, coef)
        st2, hd2, info, _ = prepare(rt, data)
        assert st != rt.JPEG_OK and (st2, hd2.why) == (st, hd.why), label
        assert not info.device_ok
        seen.add(st)
    assert seen == {rt.JPEG_UNSUPPORTED, rt.JPEG_MALFORMED}
    st, hd, _, _ = prepare(rt, files["missing table"])
    assert "missing Huffman table" in hd.why
    out = np.zeros(rt.jpeg_prepare_bound(len(base)), np.uint8)
    st, hd, info = rt.jpeg_scan_prepare(base, out, 64 * 48 - 1)
    assert st == rt.JPEG_MALFORMED and "pixel limit" in hd.why


def test_restart_intervals_are_not_for_the_device():
    data = encode(smooth_noise(150, 130, 9), subsampling=2, quality=80, restart_marker_blocks=3)
    st, hd, info, _ = prepare(rt, data)
    assert st == rt.JPEG_OK and hd.restart == 3 and not info.device_ok


# ------------------------------------------------------------------------------ coefficients
def test_coefficients_equal_jpeg_parse():
    files = dict(small_files())
    files["pants 534x400 4:2:0 q90"] = pants_file()
    files["noise 534x400 4:4:4 q75"] = noise_file()
    most_rounds, longest = 0, 0
    for label, data in files.items():
        st, hd, want = oracle(rt, data)
        assert st == rt.JPEG_OK, label
        err, rounds, bad, coef, info = emulate(rt, data)
        assert err == 0 and bad == 0, label
        assert np.array_equal(coef, want), label
        most_rounds, longest = max(most_rounds, rounds), max(longest, info.nbits)
    # not trivially: the states had to synchronise over several rounds, and one scan spans more than two chunks
    assert most_rounds >= 3
    assert longest > 2 * rt.JPEG_HUFF_SUB_BITS * rt.JPEG_HUFF_CHUNK
    assert emulate(rt, files["1x1"])[4].nbits < rt.JPEG_HUFF_SUB_BITS      # shorter than one subsequence


# ------------------------------------------------------------------------------ errors
def _check_against_host(data, label):
    st, hd, want = oracle(rt, data)
    st2, hd2, info, out = prepare(rt, data)
    assert st2 == rt.JPEG_OK and info.device_ok, label       # the damage is inside the scan
    err, rounds, bad, coef, _ = emulate(rt, data)
    assert bad == 0, label
    if st == rt.JPEG_OK:
        assert err == 0 and np.array_equal(coef, want), label
    else:
        assert st == rt.JPEG_MALFORMED and err != 0, label
    return st


def test_truncated_scan_sets_the_error_word():
    assert _check_against_host(truncated_pants(), "truncated") == rt.JPEG_MALFORMED


@pytest.mark.parametrize("seed_file", ["33x47 4:2:2", "64x64 grey optimised"])
def test_mutated_scans_agree_with_the_host_decoder(seed_file):
    seen = {rt.JPEG_OK: 0, rt.JPEG_MALFORMED: 0}
    for i, d in enumerate(mutations(small_files()[seed_file], 200, 5)):
        seen[_check_against_host(d, f"{seed_file} mutation {i}")] += 1
    assert seen[rt.JPEG_OK] and seen[rt.JPEG_MALFORMED], seen      # both implications were exercised
