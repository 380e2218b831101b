"""Restart intervals in the device entropy decode, on the host: jpeg_scan_prepare carries its
unstuffing on through the RSTm markers and adds the interval and group tables, and jpeg_huff_cpu
runs the procedure of jpeg_huff_rst_decode + jpeg_dc_rst_scan (one workgroup per group of intervals,
every interval from its known entry state, DC sums that start again at every interval) through the
shared code of csrc/runtime/jpeg_huff.h. The oracle is jpeg_parse: equal coefficients for every
file it accepts, a set error word -- or a prepare that refuses the file -- for every one it rejects."""
import numpy as np
import pytest

from _jpeg_huff_cases import mutations, oracle
from _jpeg_rst_cases import (PREPARE, agree, count_intervals, emulate, large_rst_files, marker_damage, prepare,
                             prepare_files, seed_file, small_rst_files, split_scan, tables)
from kdl.ops import _lib

rt = _lib.rt()
S, T = rt.JPEG_HUFF_SUB_BITS, rt.JPEG_HUFF_CHUNK
SENTINEL = 0x5A5A


# ------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("label", list(PREPARE))
def test_prepare_stages_the_intervals(label):
    _, ri, nint = PREPARE[label]
    data = prepare_files()[label]
    assert count_intervals(rt, data) == nint
    st, hd, info, out = prepare(rt, data)
    assert st == rt.JPEG_OK and hd.restart == ri
    assert info.restart_ok and not info.device_ok
    assert (info.ri, info.nint) == (ri, nint)
    want = split_scan(data)
    assert len(want) == nint
    iv, gr = tables(info, out)
    words = out[info.scan_off:info.scan_off + info.scan_bytes].view(np.uint32)
    nxt = 0
    for (word, bits), part in zip(iv, want):
        assert bits == 8 * len(part)                                  # the padding bits in front of the marker are gone
        nwords = (len(part) + 3) // 4
        assert word == nxt                                            # every interval from a word boundary
        staged = words[word:word + nwords + 1].astype(">u4").tobytes()
        assert staged[:len(part)] == part and not any(staged[len(part):])      # big-endian words, one zero word behind
        nxt = word + nwords + 1
    assert 4 * nxt == info.scan_bytes and info.nbits == 8 * sum(len(p) for p in want)
    assert info.int_off == info.scan_off + info.scan_bytes and info.int_off % 4 == 0
    assert info.nbytes == info.grp_off + 8 * info.ngroup <= out.size
    # the groups tile the intervals, each within the rule
    assert gr[0, 0] == 0 and (gr[1:, 0] == gr[:-1, 0] + gr[:-1, 1]).all() and gr[-1].sum() == nint
    for first, count in gr:
        assert count == 1 or sum(-(-int(b) // S) for b in iv[first:first + count, 1]) <= T


def test_some_intervals_are_shorter_than_a_subsequence():
    parts = split_scan(prepare_files()["blocks=1"])
    assert min(len(p) for p in parts) * 8 < S < max(len(p) for p in parts) * 8


def test_prepare_bound_needs_the_interval_count():
    data = prepare_files()["blocks=1"]
    out = np.zeros(rt.jpeg_prepare_bound(len(data)), np.uint8)
    canary = np.full(out.size + 64, 0xA5, np.uint8)
    buf = canary[:out.size]
    st, hd, info = rt.jpeg_scan_prepare(data, buf)
    assert st == rt.JPEG_MALFORMED and hd.why == "prepare buffer too small" and not info.restart_ok
    assert (canary[out.size:] == 0xA5).all()
    # a header cannot claim more table than the file can hold markers
    assert rt.jpeg_prepare_bound(100, 1 << 40) == rt.jpeg_prepare_bound(100, 51)
    assert rt.jpeg_prepare_bound(100, 0) == rt.jpeg_prepare_bound(100)


# ------------------------------------------------------------------------------ coefficients
def test_coefficients_equal_jpeg_parse():
    files = {**prepare_files(), **small_rst_files(), **large_rst_files()}
    assert len(files) == 4 + 32 + 3
    most_rounds = most_groups = longest = 0
    for label, data in files.items():
        st, hd, want = oracle(rt, data)
        assert st == rt.JPEG_OK, label
        err, rounds, bad, coef, info = emulate(rt, data)
        assert err == 0 and bad == 0, label
        assert np.array_equal(coef, want), label
        iv, _ = tables(info, prepare(rt, data)[3])
        most_rounds, most_groups = max(most_rounds, rounds), max(most_groups, info.ngroup)
        longest = max(longest, int(iv[:, 1].max()))
    # not trivially: states had to synchronise inside an interval, one image needs several
    # workgroups, and one interval is walked in more than one chunk
    assert most_rounds >= 2 and most_groups > 1 and longest > S * T
    info = emulate(rt, large_rst_files()["pants blocks=4"])[4]
    assert info.nint == 213 and info.ngroup > 1
    info = emulate(rt, large_rst_files()["noise rows=25"])[4]
    assert info.nint == 2 and info.ngroup == 2


# ------------------------------------------------------------------------------ damage
def test_damaged_markers_are_refused_or_agree_with_the_host():
    data = seed_file("150x130 4:2:0 blocks=3")
    seen = {}
    for label, d in marker_damage(data).items():
        seen[label] = agree(rt, d, label)
    assert seen["fill bytes"] == rt.JPEG_OK                # fill bytes in front of a marker are no damage
    assert oracle(rt, marker_damage(data)["fill bytes"])[2].tobytes() == oracle(rt, data)[2].tobytes()
    assert seen["removed"] == seen["renumbered"] == seen["swapped"] == seen["duplicated"] == "refused"
    assert seen["cut"] in ("refused", rt.JPEG_MALFORMED)
    assert oracle(rt, marker_damage(data)["cut"])[0] == rt.JPEG_MALFORMED


@pytest.mark.parametrize("seed", ["150x130 4:2:0 blocks=3", "33x47 4:2:2 blocks=2", "64x64 grey rows=1"])
def test_mutated_scans_agree_with_the_host_decoder(seed):
    seen = {rt.JPEG_OK: 0, rt.JPEG_MALFORMED: 0, "refused": 0}
    for i, d in enumerate(mutations(seed_file(seed), 200, 5)):
        seen[agree(rt, d, f"{seed} mutation {i}")] += 1
    # both implications were exercised with restart_ok still true
    assert seen[rt.JPEG_OK] and seen[rt.JPEG_MALFORMED], seen


# ------------------------------------------------------------------------------ validation
def _edits(info, iv, gr):
    """label -> edit(descriptor words, stage) of a restart descriptor with several groups; the five
    restart fields are the descriptor's last words: ri, nint, ngroup, int_off, grp_off."""
    def field(at, value):
        def edit(words, stage):
            words[at] = value
        return edit

    def table(at, value):
        def edit(words, stage):
            stage[at:at + 4].view(np.uint32)[0] = value
        return edit

    def one_group(words, stage):
        words[-3] = 1
        stage[info.grp_off:info.grp_off + 8].view(np.uint32)[:] = (0, info.nint)
    return {"table offset past the staging": field(-2, info.nbytes),
            "group table past the staging": field(-1, info.nbytes - 4),
            "interval words past the scan": table(info.int_off + 8 * (info.nint - 1), info.scan_bytes // 4),
            "interval bits > 32 x words": table(info.int_off + 4, 32 * int(iv[1, 0] - iv[0, 0]) + 1),
            "Ri = 0": field(-5, 0),
            "wrong interval count": field(-4, info.nint + 1),
            "a group over the T-subsequence rule": one_group}


def test_edited_descriptors_are_refused():
    data = large_rst_files()["pants blocks=4"]
    st, hd, info, out = prepare(rt, data)
    iv, gr = tables(info, out)
    assert info.ngroup > 1 and sum(-(-int(b) // S) for b in iv[:, 1]) > T
    desc = rt.jpeg_huff_desc(hd, info, 0, 0)
    words = np.frombuffer(desc, np.uint32)
    assert list(words[-5:]) == [info.ri, info.nint, info.ngroup, info.int_off, info.grp_off]
    stage = out[:info.nbytes]
    assert rt.jpeg_huff_desc_valid(desc, stage, hd.ncoef)
    # the fields are zero for a file without restart intervals, and such a descriptor needs no tables
    from _jpeg_huff_cases import pants_file, prepare as prepare_plain
    _, phd, pinfo, pout = prepare_plain(rt, pants_file())
    assert not np.frombuffer(rt.jpeg_huff_desc(phd, pinfo, 0, 0), np.uint32)[-5:].any()
    for label, edit in _edits(info, iv.copy(), gr.copy()).items():
        w, s = words.copy(), stage.copy()
        edit(w, s)
        assert not rt.jpeg_huff_desc_valid(w.tobytes(), s, hd.ncoef), label
        coef = np.full(hd.ncoef, SENTINEL, np.int16)
        err, rounds, bad = rt.jpeg_huff_cpu(w.tobytes(), s, coef)
        assert (err, rounds, bad) == (1, 0, 0) and (coef == SENTINEL).all(), label
