"""The MBConv operator tests' own references and bounds, checked on the CPU: float32 emulations
of what a correct kernel does fit every bound of tests/_mbconv_cases.py on every problem that
tests/test_mbconv_ops_gpu.py launches, and the known-bad variants (a tap lost in the last
column, stride-2 padding on the wrong side, a truncating bf16 conversion, a pool of unrounded
activations, a pool part lost or counted twice, a squeeze-excite without its 1 / HW) do not.
So the GPU file can fail for those reasons; the older 2e-2-of-the-maximum check cannot."""
import pytest
import torch
import torch.nn.functional as F

import _mbconv_cases as MC


def _err(y, ref):
    return (y.double() - ref).abs()


@pytest.mark.parametrize("K,S", MC.KS)
def test_depthwise_and_pool_emulation_fit_the_bounds(K, S):
    wy, wp = 0.0, 0.0
    keys = MC.all_case_keys(K, S)
    for n, key in enumerate(keys):
        c = MC.dw_case(*key)
        for act in MC.ACTS:
            y = MC.dw_emulate(c.x, c.w, c.bias, K, S, act)
            err, bound = _err(y, c.ref(act)), c.bound(act)
            assert MC.within(err, bound), (key, act, MC.ratio(err, bound))
            wy = max(wy, MC.ratio(err, bound))
            rows = [1, 5, 64][n % 3]
            pool = MC.pool_emulate(y, c.w1, rows)
            ref, pb = MC.pool_reference(y, c.w1, pool.shape[1])
            perr = (pool.double().sum(1) - ref).abs()
            assert MC.within(perr, pb), (key, act, MC.ratio(perr, pb))
            wp = max(wp, MC.ratio(perr, pb))
    print(f"K {K} S {S}: {len(keys)} problems, fp32 emulation worst err / bound: depthwise {wy:.3f}, pool {wp:.3f}")


@pytest.mark.parametrize("K,S", MC.KS)
def test_depthwise_reference_equals_conv2d(K, S):
    for kind, (H, W) in zip(MC.KINDS, MC.MAPS):
        x, w, bias, _ = MC.dw_inputs(kind, 3, H, W, 16, K, S, 1)
        pre, A = MC.dw_reference(x, w, bias, K, S)
        wd = w.double().t().reshape(16, 1, K, K)
        xd = x.double().permute(0, 3, 1, 2)
        want = F.conv2d(xd, wd, bias.double(), stride=S, padding=(K - 1) // 2, groups=16).permute(0, 2, 3, 1)
        wanta = F.conv2d(xd.abs(), wd.abs(), bias.double().abs(), stride=S, padding=(K - 1) // 2, groups=16)
        assert pre.shape == want.shape
        tol = 1e-13 * A
        assert bool(((pre - want).abs() <= tol).all()) and bool(((A - wanta.permute(0, 2, 3, 1)).abs() <= tol).all())


VARIANT_KINDS = ["benign", "big", "cancel"]      # under SiLU 'neg' outputs are ~0 whatever the taps do


@pytest.mark.parametrize("K,S", MC.KS)
def test_a_tap_lost_in_the_last_column_misses_the_bound(K, S):
    for H, W in MC.MAPS[2:]:
        for kind in VARIANT_KINDS:
            c = MC.dw_case(kind, 3, H, W, 32, K, S, 3)
            for act in MC.ACTS:
                bad = MC.dw_emulate(c.x, c.w, c.bias, K, S, act, "lost_tap")
                err, bound = _err(bad, c.ref(act)), c.bound(act)
                assert MC.within(err[:, :, :-1], bound[:, :, :-1])            # nothing else moved
                share = MC.share_over(err[:, :, -1], bound[:, :, -1])
                print(f"lost tap K {K} S {S} {H}x{W} {kind} act {act}: {share:.3f} of the last column over the bound")
                assert share > 0.5, (H, W, kind, act, share)


@pytest.mark.parametrize("K", [3, 5])
def test_stride2_padding_on_the_wrong_side_misses_the_bound(K):
    for H, W in MC.MAPS:
        for kind in VARIANT_KINDS:
            c = MC.dw_case(kind, 3, H, W, 32, K, 2, 3)
            for act in MC.ACTS:
                bad = MC.dw_emulate(c.x, c.w, c.bias, K, 2, act, "pad_shift")
                share = MC.share_over(_err(bad, c.ref(act)), c.bound(act))
                print(f"pad shift K {K} {H}x{W} {kind} act {act}: {share:.3f} of the outputs over the bound")
                assert share > 0.5, (H, W, kind, act, share)


@pytest.mark.parametrize("K,S", MC.KS)
def test_bf16_truncation_misses_the_bound_but_passes_the_older_check(K, S):
    """The older check, max |err| / max |ref| < 2e-2 on Gaussian data, lets a truncating
    conversion (2^-7 relative) through; the per-element bound does not."""
    for H, W in MC.MAPS[1:]:
        c = MC.dw_case("benign", 3, H, W, 32, K, S, 3)
        for act in MC.ACTS:
            bad = MC.dw_emulate(c.x, c.w, c.bias, K, S, act, "truncate")
            err, bound = _err(bad, c.ref(act)), c.bound(act)
            share, old = MC.share_over(err, bound), float(err.max() / c.ref(act).abs().max())
            print(f"truncation K {K} S {S} {H}x{W} act {act}: {share:.3f} over the bound, worst {MC.ratio(err, bound):.2f}; "
                  f"older check {old:.2e} < 2e-2")
            assert not MC.within(err, bound)
            assert old < 2e-2


@pytest.mark.parametrize("K,S", MC.KS)
def test_a_pool_of_unrounded_activations_misses_the_bound(K, S):
    """w1 = identity, so a squeeze unit is a channel: the fp32 activations differ from the
    stored ones by a random walk of 132 bf16 roundings, far more than fp32 summation allows."""
    C = 64
    c = MC.dw_case("benign", 3, 12, 11, C, K, S, 3)
    eye = torch.eye(C)
    f = MC.dw_emulate(c.x, c.w, c.bias, K, S, 2, rounded=False)
    y = f.to(torch.bfloat16)
    ref, bound = MC.pool_reference(y, eye, 3)
    good = (MC.pool_emulate(y, eye, 5).double().sum(1) - ref).abs()
    assert MC.within(good, bound)
    err = (MC.pool_emulate(f, eye, 5).double().sum(1) - ref).abs()
    share = MC.share_over(err, bound)
    print(f"unrounded pool K {K} S {S}: {share:.3f} of the channels over the bound, median {float((err / bound).median()):.1f}x")
    assert share > 0.5, share


@pytest.mark.parametrize("K,S", MC.KS)
def test_a_pool_part_lost_or_counted_twice_misses_the_bound(K, S):
    for kind in ("benign", "big", "cancel"):
        c = MC.dw_case(kind, 3, 12, 11, 64, K, S, 20)
        y = MC.dw_emulate(c.x, c.w, c.bias, K, S, 2)
        pool = MC.pool_emulate(y, c.w1, 1)                      # one part per output row
        ref, bound = MC.pool_reference(y, c.w1, pool.shape[1])
        for name, bad in (("lost", pool[:, 1:]), ("twice", torch.cat([pool, pool[:, 3:4]], 1))):
            err = (bad.double().sum(1) - ref).abs()
            print(f"pool part {name} K {K} S {S} {kind}: {MC.share_over(err, bound):.3f} of the units over the bound")
            assert not MC.within(err, bound)


@pytest.mark.parametrize("Cs", MC.SE_CS)
def test_squeeze_excite_emulation_fits_and_its_variants_miss(Cs):
    worst = 0.0
    shares = {"drop": [], "twice": [], "no_hw": []}
    for nt in MC.se_ntiles(Cs):
        for C in MC.SE_C:
            for B in MC.SE_B:
                inp = MC.se_inputs(B, nt, C, Cs)
                ref, bound = MC.se_reference(*inp, 132)
                err = _err(MC.se_emulate(*inp, 132), ref)
                assert MC.within(err, bound), (Cs, nt, C, B, MC.ratio(err, bound))
                worst = max(worst, MC.ratio(err, bound))
                for v in shares:
                    bad = _err(MC.se_emulate(*inp, 132, v), ref)
                    assert not MC.within(bad, bound), (v, Cs, nt, C, B)
                    shares[v].append(MC.share_over(bad, bound))
    print(f"squeeze_excite Cs {Cs}: emulation worst err / bound {worst:.3f}; least share over the bound: "
          + ", ".join(f"{v} {min(s):.3f}" for v, s in shares.items()))


def test_squeeze_excite_extreme_logits_are_exactly_zero_or_one():
    inp = MC.se_inputs(3, 7, 264, 20, logit=100.0)
    ref, bound = MC.se_reference(*inp, 132)
    got = MC.se_emulate(*inp, 132)
    assert MC.within(_err(got, ref), bound)
    assert bool(((got == 0) | (got == 1)).all()) and bool((got == 0).any()) and bool((got == 1).any())


def test_channel_scale_expectation_stays_in_the_normal_range():
    for HW, C in MC.CHS_SHAPES:
        y, scale = MC.chscale_inputs(3, HW, C)
        want = MC.chscale_expected(y, scale).float()
        assert bool(torch.isfinite(want).all())
        assert bool(((want == 0) | (want.abs() >= 2.0 ** -126)).all())
        assert bool((want[:, :, 0] == 0).all()) and torch.equal(want[:, :, 1], y[:, :, 1].float())
        assert torch.equal(want[:, :, 2], -y[:, :, 2].float())


def test_the_matrix_holds_every_dispatched_instance():
    keys = MC.matrix_keys()
    direct = {k for k in keys if k[2] == 2}
    tiled = {k for k in keys if k[2] == 1}
    assert len(direct) == 4 * 2 * 8 * 2 * 2 and len(tiled) == 4 * 5 * 4 * 2
