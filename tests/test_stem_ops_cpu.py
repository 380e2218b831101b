"""The stem operator tests' own references and bounds, checked on the CPU: the float64 reference
equals F.conv2d on the rounded operands; a float32 emulation of a correct kernel (either order of
raw * scale + shift) fits every bound of tests/_stem_cases.py on every launch that
tests/test_stem_ops_gpu.py makes; the known-bad variants (a tap lost in the last column, padding
filled with a raw 0 pixel, the scale / shift of the wrong channel, H and W swapped in the
address, a truncating conversion of the A operand, the image boundary ignored inside a fragment)
do not; and an emulation of stem_rows_kernel's window addressing gathers exactly the reference's
bytes, at every pointer offset, without one read outside the tensor."""
import pytest
import torch
import torch.nn.functional as F

import _stem_cases as SC

GROUPS = [(k, KW) for k in ("stem", "rows") for KW in (3, 7)]


def test_the_matrix_covers_every_instance_and_edge():
    seen = {}
    for L in SC.all_launches():
        seen.setdefault(L.inst, []).append(L)
    assert set(seen) == set(SC.instances()) and len(seen) == 30
    for inst, ls in seen.items():
        assert {L.kind for L in ls} == set(SC.KINDS), inst
        assert {L.ldy_extra for L in ls} == {0, 8}, inst
        assert {L.act for L in ls} == ({0, 1, 2} if inst.cout == 64 and inst.generic else {1}), inst
        ms = {SC.case(L).M for L in ls}
        if inst.KW == 3:
            assert {1, 24, 128, 129, 480} <= ms, (inst, ms)
        if inst.generic:
            assert any(L.prob.pad > L.prob.H for L in ls) or inst.KW == 3
            assert any(L.prob.H != L.prob.W for L in ls)
    assert len(SC.unaligned_launches()) == 8


def test_both_orders_of_the_normalisation():
    """The 768 (pixel value, channel) pairs, fused and separate, in both storage types."""
    for dt in (0, 1):
        fused, sep = SC.operand_table(dt)
        n = int((fused != sep).sum())
        step = (fused - sep).abs().max().item()
        print(f"{'fp16' if dt else 'bf16'}: {n} of 768 pairs round differently with and without contraction "
              f"(largest difference {step:g})")
        assert torch.equal(fused.to(SC.DTYPES[dt]).float(), fused)
        # with the torchvision constants every pair rounds to the same value either way, so the
        # reference is the operand of both kernels and the bound's extra term is zero
        assert n == 0
        # one unit in the last place at most: the bound's extra term is |w_k| times this
        assert step <= 2.0 ** (-7 if dt == 0 else -10) * fused.abs().max().item()


@pytest.mark.parametrize("kernel,KW", GROUPS)
def test_reference_equals_conv2d(kernel, KW):
    for L in SC.launches(kernel, KW):
        c, i, p = SC.case(L), L.inst, L.prob
        a = SC.a_operand(c.img, i.generic, i.dt).double().permute(0, 3, 1, 2)
        wd = c.w.double().permute(0, 3, 1, 2)
        want = F.conv2d(a, wd, c.bias.double(), stride=p.stride, padding=p.pad).permute(0, 2, 3, 1)
        wanta = F.conv2d(a.abs(), wd.abs(), c.bias.double().abs(), stride=p.stride, padding=p.pad).permute(0, 2, 3, 1)
        assert want.shape == c.pre.shape == (p.B, c.OH, c.OW, i.cout)
        tol = 1e-13 * c.A
        assert bool(((c.pre - want).abs() <= tol).all()) and bool(((c.A - wanta).abs() <= tol).all()), SC.describe(L)
        if L.kind == "cancel" and c.OH > 2 and c.OW > 2 and p.pad == 0:
            assert float((c.A / (c.pre.abs() + 1e-30)).median()) > 20, SC.describe(L)


@pytest.mark.parametrize("kernel,KW", GROUPS)
def test_emulation_fits_the_bounds(kernel, KW):
    worst, n = 0.0, 0
    for L in SC.launches(kernel, KW):
        c = SC.case(L)
        for variant in ("", "separate") if L.inst.generic and kernel == "stem" else ("",):
            err = c.err(SC.emulate(L, variant))
            assert SC.within(err, c.bound), (SC.describe(L), variant, SC.ratio(err, c.bound))
            worst = max(worst, SC.ratio(err, c.bound))
            n += 1
    print(f"{kernel} {KW}x{KW}: {n} emulated launches, worst err / bound {worst:.3f}")
    assert worst < 1


def _misses(variant: str, applies) -> int:
    """Launches of the matrix on which the variant misses its bound; where it does not apply it
    must change nothing."""
    missed, tried = 0, 0
    for L in SC.all_launches():
        if not applies(L):
            continue
        c = SC.case(L)
        err = c.err(SC.emulate(L, variant))
        tried += 1
        if not SC.within(err, c.bound):
            missed += 1
    print(f"variant {variant}: misses the bound on {missed} of {tried} launches")
    return missed


def test_a_tap_lost_in_the_last_column_misses():
    assert _misses("lost_tap", lambda L: L.kind != "edge" and L.prob.H > 8) >= 10


def test_padding_filled_with_shift_misses():
    assert _misses("pad_shift", lambda L: L.inst.generic and L.prob.pad > 0) >= 20
    L = next(x for x in SC.all_launches() if not x.inst.generic)
    assert torch.equal(SC.emulate(L, "pad_shift").view(torch.int16), SC.emulate(L).view(torch.int16))


def test_the_wrong_channels_scale_and_shift_misses():
    assert _misses("channel", lambda L: L.inst.generic and L.kind == "benign") >= 20


def test_h_and_w_swapped_in_the_address_misses():
    assert _misses("swap_hw", lambda L: L.kind == "benign" and L.prob.H != L.prob.W and L.prob.H > 2) >= 20


def test_a_truncating_operand_conversion_misses():
    assert _misses("truncate", lambda L: L.inst.generic and L.kind == "cancel" and SC.case(L).M > 20) >= 3


def test_an_ignored_image_boundary_misses():
    assert _misses("no_boundary", lambda L: L.prob.B > 1 and L.kind == "benign" and SC.case(L).OH * SC.case(L).OW % 16) >= 5


def test_rows_window_addressing_gathers_the_reference_and_stays_inside():
    moved = [L for _, ls in SC.unaligned_launches() for L in ls]
    n_al = n_before = n_past = 0
    both_ends = False
    for L in list(SC.launches("rows", 3)) + list(SC.launches("rows", 7)) + moved:
        raw, keep, lo, hi, al, before, past = SC.rows_windows(L)
        want_raw, want_keep = SC.rows_gather_reference(L)
        total = L.prob.B * L.prob.H * L.prob.W * 3
        assert 0 <= lo and hi < total, (SC.describe(L), lo, hi, total)
        assert (keep == want_keep).all() and (raw == want_raw).all(), SC.describe(L)
        n_al, n_before, n_past = n_al + al, n_before + before, n_past + past
        if L.prob.B == 1 and before and past:
            both_ends = True
    print(f"stem_rows_kernel windows: {n_al} aligned, {n_before} byte-wise before the tensor, {n_past} past its end")
    assert n_al and n_before and n_past and both_ends
