"""The conv-GEMM checker of tests/_conv_cases.py must have teeth (no GPU).

For every case of the table at its smallest shape: the fp32 emulation of the kernel passes
``check``; each planted fault fails it; the share of depthwise entries whose bf16 rounding could
flip (D of the error model) stays within 3 %. The first round's gate, max |y - ref| <= 2e-2 max |ref|
(tests/test_kernels_gpu.py ``_check``), is re-implemented in the helper and run on the same faulty
outputs: the faults it lets through are printed; it must let each of the first three (wrong border
tap, dropped bias, truncated depthwise output) through somewhere in the table, and on the
middle-flow layer (K = 736, n = 728) every one of them that applies there.

A dropped bias is planted only where an output can show it: on the channel with the smallest
non-zero |bias|, when that exceeds twice the smallest bound of its column (among 728 channels of
0.1 randn the smallest is about 1e-4, below the fp32 summation error at K = 736).
"""
import functools

import pytest
import torch

from _conv_cases import FAULTS, MAX_FLAGGED, check, emulate, fault_applies, make_case, old_gate_passes
from kdl.ops.conv import MODE_CONV, MODE_DW, MODE_PW

# name -> (make_case arguments, depthwise weight forms the ids of that case read)
TABLE = {
    "sep_k32_n8": (dict(mode=MODE_DW, cin=32, n=8, B=2, H=5, W=7, seed=1, relu_in=True, relu_out=1), ("fp32", "bf16")),
    "sep_k96_n120_res": (dict(mode=MODE_DW, cin=96, n=120, B=2, H=5, W=7, seed=22, relu_in=True, with_res=True),
                         ("fp32", "bf16")),
    "sep_k736_n728": (dict(mode=MODE_DW, cin=728, n=728, B=2, H=5, W=7, seed=3, relu_in=True, relu_out=1),
                      ("fp32", "bf16")),
    "sep_1x1_relu2": (dict(mode=MODE_DW, cin=160, n=8, B=1, H=1, W=1, seed=4, relu_out=2, with_res=True), ("fp32", "bf16")),
    "sep_zero_image": (dict(mode=MODE_DW, cin=64, n=120, B=2, H=5, W=7, seed=5, pattern="zero"), ("fp32", "bf16")),
    "sep_cancel": (dict(mode=MODE_DW, cin=64, n=120, B=2, H=5, W=7, seed=6, pattern="cancel", with_res=True),
                   ("fp32", "bf16")),
    "sep_wide_ld": (dict(mode=MODE_DW, cin=32, n=120, B=2, H=5, W=7, seed=7, wide=True, with_res=True, relu_out=1),
                    ("fp32", "bf16")),
    "pw_k32": (dict(mode=MODE_PW, cin=32, n=120, B=1, H=1, W=17, seed=8, with_res=True, relu_out=2), ("fp32",)),
    "pw_k64_s2_f16": (dict(mode=MODE_PW, cin=64, n=120, B=1, H=2, W=29, seed=9, stride=2, dtype=torch.float16,
                           relu_out=1), ("fp32",)),
    "pw_k2304": (dict(mode=MODE_PW, cin=2304, n=8, B=1, H=1, W=15, seed=10, with_res=True), ("fp32",)),
    "c3_k288": (dict(mode=MODE_CONV, cin=32, n=56, B=1, H=3, W=19, seed=11, relu_out=1), ("fp32",)),
    "c3_k576_s2_f16": (dict(mode=MODE_CONV, cin=64, n=120, B=1, H=4, W=31, seed=12, stride=2, dtype=torch.float16,
                            with_res=True), ("fp32",)),
}
PARAMS = [(name, form) for name, (_, forms) in TABLE.items() for form in forms]
_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = make_case(name, **TABLE[name][0])
    return _cases[name]


def _passes(case, form, fault):
    whole, body = emulate(case, form, fault)
    try:
        check(body, case, form, guards=[(whole, body.numel())], tag=f"{form} {fault}")
    except AssertionError:
        return False, old_gate_passes(body, case, form)
    return True, old_gate_passes(body, case, form)


@pytest.mark.parametrize("name,form", PARAMS)
def test_flagged_share_within_cap(name, form):
    flagged = _case(name).core(form)[2]
    print(f"{name} {form}: {100 * flagged:.2f} % of depthwise entries flagged")
    assert flagged <= MAX_FLAGGED


@pytest.mark.parametrize("name,form", PARAMS)
def test_emulation_passes(name, form):
    ok, old = _passes(_case(name), form, None)
    assert ok and old


@functools.lru_cache(maxsize=None)
def _faults(name, form):
    """fault -> (passes the check, passes the old gate), for the faults that apply to the case."""
    case = _case(name)
    return {f: _passes(case, form, f) for f in FAULTS if fault_applies(case, f)}


@pytest.mark.parametrize("name,form", PARAMS)
def test_planted_faults_are_caught(name, form):
    res = _faults(name, form)
    for fault, (ok, _) in res.items():
        assert not ok, f"{name} {form}: planted fault {fault} passes the check"
    missed_by_old = [f for f, (_, old) in res.items() if old]
    print(f"{name} {form}: the 2e-2 max|ref| gate lets through: {', '.join(missed_by_old) or 'nothing'}")
    if name == "sep_k736_n728":
        assert set(FAULTS[:3]) & set(res) <= set(missed_by_old), missed_by_old


def test_old_gate_lets_the_first_three_faults_through():
    """The gap on record: each of the first three faults passes the old gate in some case of the table."""
    for fault in FAULTS[:3]:
        assert any(_faults(*p).get(fault, (0, False))[1] for p in PARAMS), fault


def test_every_fault_is_planted_somewhere():
    for fault in FAULTS:
        assert any(fault_applies(_case(n), fault) for n in TABLE), fault
