"""The classifier-tail tests' own references and bounds, checked on the CPU: the float64
references equal a plain matmul on the rounded operands; float32 emulations of correct kernels,
with each kernel's summation order, fit every bound of tests/_tail_cases.py on every problem that
tests/test_tail_ops_gpu.py launches; and the known-bad variants (a K slice dropped when KT is no
multiple of 4, a missing 1 / HW, a pixel group counted twice when HW < 4, the ReLU before b1 is
added) do not."""
import torch

import _tail_cases as TC


def _err(y, ref):
    return (y.double() - ref).abs()


def test_the_lists_of_the_issue_are_all_run():
    ls = TC.fc_launches()
    for F, N in TC.FC_SMALL:
        assert {(B, r, d) for B, f, n, r, d, _ in ls if (f, n) == (F, N)} == \
            {(B, r, d) for B in TC.FC_B for r in (0, 1) for d in (0, 1)}
    for F, N in TC.FC_LARGE:
        mine = [l for l in ls if (l[1], l[2]) == (F, N)]
        assert {l[3] for l in mine} == {0, 1} and {l[4] for l in mine} == {0, 1} and {l[5] for l in mine} == {False, True}
    assert {l[0] for l in ls if l[1] > 96} == set(TC.FC_B)
    assert {l[5] for l in ls if l[1] <= 96 and l[0] % 16} == {False, True}
    for n, name in enumerate(("B", "HW", "F", "H1", "NC")):
        assert {c[n + 1] for c in TC.HEAD_CASES} == set(TC.HEAD_LISTS[name]), name
    assert {c[6] for c in TC.HEAD_CASES} == {0, 8} and {c[0] for c in TC.HEAD_CASES} == {"benign", "cancel"}


def test_fc_reference_is_a_matmul_and_the_emulation_fits():
    worst = 0.0
    for B, F, N, relu, dt, _ in TC.fc_launches():
        x, w, bias = TC.fc_inputs(B, F, N, dt)
        assert torch.equal(x.to(TC.DTYPES[dt]).float(), x) and torch.equal(w.to(TC.DTYPES[dt]).float(), w)
        ref, bound = TC.fc_reference(x, w, bias, relu)
        want = torch.nn.functional.linear(x.double(), w.double(), bias.double())
        assert bool(((ref - (torch.relu(want) if relu else want)).abs() <= 1e-13 * bound / ((F + 4) * TC.U32)).all())
        err = _err(TC.fc_emulate(x, w, bias, relu), ref)
        assert TC.within(err, bound), (B, F, N, relu, dt, TC.ratio(err, bound))
        worst = max(worst, TC.ratio(err, bound))
    print(f"fc_mfma: {len(TC.fc_launches())} problems, fp32 emulation worst err / bound {worst:.3f}")
    assert worst < 1


def test_fc_with_a_dropped_k_slice_misses():
    missed = 0
    for B, F, N, relu, dt, _ in TC.fc_launches():
        x, w, bias = TC.fc_inputs(B, F, N, dt)
        ref, bound = TC.fc_reference(x, w, bias, relu)
        bad = TC.fc_emulate(x, w, bias, relu, "drop_slice")
        if (F // 32) % 4 == 0:
            assert torch.equal(bad, TC.fc_emulate(x, w, bias, relu))
        else:
            assert not TC.within(_err(bad, ref), bound), (B, F, N, relu, dt)
            missed += 1
    print(f"fc_mfma without the last KT % 4 steps: misses on {missed} problems")
    assert missed >= 56


def test_head_reference_is_a_matmul_and_the_emulation_fits():
    worst = 0.0
    for key in TC.HEAD_CASES:
        x, w1t, b1, w2, b2 = TC.head_inputs(*key)
        F = w1t.shape[1]
        ref, bound, pre = TC.head_reference(x, w1t, b1, w2, b2)
        want = torch.relu(x[:, :, :F].double().mean(1) @ w1t.double().t() + b1.double()) @ w2.double() + b2.double()
        A = torch.relu(pre).abs() @ w2.double().abs() + b2.double().abs()
        assert bool(((ref - want).abs() <= 1e-13 * A).all())
        if key[0] == "cancel":       # near 0, and on both sides wherever there is more than one value
            assert float(pre.abs().max()) < 0.2, key
            assert pre.numel() < 8 or (bool((pre > 0).any()) and bool((pre < 0).any())), key
        err = _err(TC.head_emulate(x, w1t, b1, w2, b2), ref)
        assert TC.within(err, bound), (key, TC.ratio(err, bound))
        worst = max(worst, TC.ratio(err, bound))
    print(f"head_dense: {len(TC.HEAD_CASES)} problems, fp32 emulation worst err / bound {worst:.3f}")
    assert worst < 1


def _head_misses(variant, applies):
    missed = tried = 0
    for key in TC.HEAD_CASES:
        if not applies(key):
            continue
        inp = TC.head_inputs(*key)
        ref, bound, _ = TC.head_reference(*inp)
        tried += 1
        missed += not TC.within(_err(TC.head_emulate(*inp, variant), ref), bound)
    print(f"head_dense variant {variant}: misses on {missed} of {tried} problems")
    return missed, tried


def test_head_without_one_over_hw_misses():
    missed, tried = _head_misses("no_hw", lambda k: k[2] > 1)
    assert missed == tried >= 6


def test_head_with_a_pixel_group_counted_twice_misses():
    missed, tried = _head_misses("group_twice", lambda k: k[2] < 4)
    assert missed >= 3          # not all: one hidden unit that the ReLU zeroes either way hides it
    key = next(k for k in TC.HEAD_CASES if k[2] >= 4)
    inp = TC.head_inputs(*key)
    assert torch.equal(TC.head_emulate(*inp, "group_twice"), TC.head_emulate(*inp))


def test_head_with_the_relu_before_b1_misses():
    missed, tried = _head_misses("relu_first", lambda k: True)
    assert missed == tried


def test_gap_reference_bounds_hold_for_a_sequential_fp32_mean():
    worst = 0.0
    for dt in (0, 1):
        for F in TC.GAP_F:
            for HW in TC.GAP_HW:
                x = TC.gap_inputs(2, HW, F, F + 8, dt)
                assert bool(torch.isnan(x[:, :, F:]).all())
                ref, b32, b16 = TC.gap_reference(x, F, dt)
                parts = [TC._seq_sum(x[:, p::8, :F].float(), 1) for p in range(8)]
                s = parts[0]
                for p in parts[1:]:
                    s = s + p
                y = s * torch.tensor(1.0 / HW, dtype=torch.float32)
                assert TC.within(_err(y, ref), b32) and TC.within(_err(y.to(TC.DTYPES[dt]), ref), b16), (dt, F, HW)
                worst = max(worst, TC.ratio(_err(y, ref), b32), TC.ratio(_err(y.to(TC.DTYPES[dt]), ref), b16))
                lost = (s - x[:, HW - 1, :F].float()) * torch.tensor(1.0 / HW, dtype=torch.float32)
                assert not TC.within(_err(lost, ref), b32), ("a lost pixel fits the bound", dt, F, HW)
    print(f"gap: fp32 emulation worst err / bound {worst:.3f}")
