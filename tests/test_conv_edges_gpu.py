"""Every id of the conv-GEMM family at the smallest shapes that reach its tile and image edges,
against the float64 reference and per-element bound of tests/_conv_cases.py (run on MI355X).

Only (split, id) pairs that ``lay.variants(W)`` offers are launched, through ``lay.args`` on the
direct binding. The output starts as NaN between two guard regions of at least 320 rows (the
tallest M tile); x, res, the split lowering's scratch, the split-K workspace and its counters
are guarded the same way, and the counters must read zero after every launch. Each test prints
``RATIO <kernel file> <largest error / bound>``; docs/guide.md records them.

The fused separable group runs relu_in x relu_out x residual in full (12 combinations) on every
(shape, K, n) and asserts that each launched id met all of them; the epilogues of one case share
the depthwise and GEMM part of the reference. The 2-D tiled and pointwise / 3x3 groups rotate the
combinations over their grids. Every case is built by ``make_case``, which holds the share of
flagged depthwise roundings to 3 % by reseeding.
"""
import itertools

import pytest
import torch

from _conv_cases import MAX_FLAGGED, buf_rows, check, guarded, guards_intact, make_case, out_rows
from kdl.ops import _lib
from kdl.ops.conv import (C3_BASE, MODE_CONV, MODE_DW, MODE_PW, PIPE_BASE, S2D_BASE, S2DP, S2DW, SEP_BASE, SEPW_BASE,
                          cfg_tile, is_splitk, splitk_parts)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_ROWS = 320
COMBOS = list(itertools.product((0, 1), (0, 1, 2), (0, 1)))      # relu_in, relu_out, residual


def kernel_file(cfg, split=False):
    if split:
        return "dwconv.hip"
    if is_splitk(cfg) or PIPE_BASE <= cfg < SEP_BASE:
        return "gemm_pipe.hip"
    if cfg < PIPE_BASE:
        return "conv_gemm.hip"
    return "sepconv_ws.hip" if cfg < S2D_BASE else "sepconv_2d.hip" if cfg < C3_BASE else "conv3x3_2d.hip"


class Runner:
    """One case on the device: guarded copies of x and res, one launch per id, ratios per kernel file."""

    def __init__(self, case):
        self.case, lay = case, case.lay
        assert case.flagged() <= MAX_FLAGGED, case.name
        self.xw, self.x = guarded(case.x.numel(), 512 * case.ldx, lay.dtype, 0, DEV)
        self.x.copy_(case.x.flatten())
        self.rw = self.r = None
        if case.res is not None:
            self.rw, self.r = guarded(case.res.numel(), GUARD_ROWS * case.ldr, lay.dtype, 0, DEV)
            self.r.copy_(case.res.flatten())
        self.ratios = {}

    def output(self):
        case, lay = self.case, self.case.lay
        rows = buf_rows(case)
        whole, body = guarded(rows * lay.ldy, GUARD_ROWS * lay.ldy, lay.dtype, float("nan"), DEV)
        prefill = None
        if case.opad:       # rows the op does not own: the zero border (opad 1), the class-token rows (opad 2)
            other = torch.ones(rows, dtype=torch.bool)
            other[torch.from_numpy(out_rows(case))] = False
            body.view(rows, lay.ldy)[other.to(DEV)] = 0.0 if case.opad == 1 else 1.5
            prefill = body.clone()
        return whole, body, prefill

    def run(self, cfg, x=None, mode=None, form="fp32", tag="", file=None, sk=0):
        """``sk``: run the LDS-DMA id ``cfg`` with this ksplit (16 has no id of its own: 2000 + 100 * 16
        would land in the streaming GEMM's range, so it is set on the binding's arguments)."""
        case, lay = self.case, self.case.lay
        C, s = _lib.lib(), _lib.stream_ptr()
        whole, body, prefill = self.output()
        guards = [(whole, body.numel()), (self.xw, self.x.numel())]
        if self.rw is not None:
            guards.append((self.rw, self.r.numel()))
        base = splitk_parts(cfg)[1] if is_splitk(cfg) else cfg
        args = lay.args(_lib.ptr(self.x if x is None else x), _lib.ptr(body), case.g,
                        _lib.ptr(self.r) if case.res_on else None,
                        ldx=case.ldx if x is None else lay.cin_pad, ldr=case.ldr, cfg=base, opad=case.opad)
        mode = lay.mode if mode is None else mode
        if is_splitk(cfg):
            sk = splitk_parts(cfg)[0]
        if sk:
            bm, bn = cfg_tile(base)
            tiles = -(-case.M // bm) * (lay.nf(base) * 16 // bn)
            ww, ws = guarded(sk * tiles * bm * bn, 4096, torch.float32, float("nan"), DEV)
            cw, cnt = guarded(tiles, 64, torch.int32, 0, DEV)
            args.update(ksplit=sk, ws=_lib.ptr(ws), cnt=_lib.ptr(cnt))
            guards += [(ww, ws.numel()), (cw, cnt.numel())]
            C.conv_gemm(mode, base, args, s)          # first of two launches on one workspace
            torch.cuda.synchronize()
            assert int(cnt.abs().sum()) == 0, f"{case.name} cfg {cfg}: counters not reset"
            first = body.clone()
            body.copy_(prefill if prefill is not None else torch.full_like(body, float("nan")))
        C.conv_gemm(mode, base, args, s)
        torch.cuda.synchronize()
        if sk:
            assert int(cnt.abs().sum()) == 0, f"{case.name} cfg {cfg}: counters not reset"
            assert torch.equal(body.view(torch.int16), first.view(torch.int16)), f"{case.name} cfg {cfg}: launches differ"
        ratio = check(body, case, form, guards=guards, prefill=prefill, tag=f"cfg {cfg} ksplit {sk} {tag}")
        file = file or kernel_file(cfg)
        self.ratios[file] = max(self.ratios.get(file, 0.0), ratio)
        return body


def _merge(dst, src):
    for f, r in src.items():
        dst[f] = max(dst.get(f, 0.0), r)


def _print(ratios):
    for f, r in sorted(ratios.items()):
        print(f"RATIO {f} {r:.3f}")
    assert ratios


# ------------------------------------------------------------------ fused separable, ids 0-9 and 120-158
SEP_SHAPES = [(2, 5, 7), (3, 9, 9), (1, 1, 1), (1, 1, 40)]
SEP_K = [32, 96, 160, 736]
SEP_N = [8, 128, 728]


EPILOGUES = list(itertools.product((0, 1, 2), (False, True)))     # relu_out, residual


def _fused(case, lo=0, hi=S2D_BASE, epilogues=None):
    """Every fused id of [lo, hi) the layer offers at this width, once per epilogue (default: the case's own)."""
    run = Runner(case)
    ids = [c for split, c in case.lay.variants(case.g.W) if not split and not is_splitk(c) and lo <= c < hi]
    for ro, res_on in epilogues or [(case.lay.relu_out, case.res_on and case.res is not None)]:
        case.set_epilogue(ro, res_on)
        for cfg in ids:
            run.run(cfg, form="fp32" if cfg < PIPE_BASE else "bf16", tag=f"out{ro} res{int(res_on)}")
    return ids, run.ratios


@pytest.mark.parametrize("n", SEP_N)
@pytest.mark.parametrize("K", SEP_K)
@pytest.mark.parametrize("si", range(len(SEP_SHAPES)))
def test_fused_separable(si, K, n):
    """relu_in x relu_out x residual in full: every id launched here meets all 12 combinations."""
    B, H, W = SEP_SHAPES[si]
    ratios, met = {}, {}
    for ri in (0, 1):
        case = make_case(f"sep B{B} {H}x{W} K{K} n{n} in{ri}", MODE_DW, K, n, B, H, W,
                         seed=1000 + 100 * si + K + n + 5000 * ri, relu_in=bool(ri), with_res=True, device=DEV)
        ids, r = _fused(case, epilogues=EPILOGUES)
        for c in ids:
            met.setdefault(c, set()).update((ri, ro, res) for ro, res in EPILOGUES)
        _merge(ratios, r)
    assert met and all(len(v) == len(COMBOS) for v in met.values()), met
    assert any(c < PIPE_BASE for c in met), sorted(met)
    if n == 728:            # the only n of the three at which the warp-specialized ids are candidates
        assert any(SEPW_BASE <= c < S2D_BASE for c in met), sorted(met)
    _print(ratios)


@pytest.mark.parametrize("kind", ["wide", "zero", "cancel"])
def test_fused_separable_strides_and_patterns(kind):
    """ldx = cin_pad + 32 and ldr = ldy + 32 with NaN pad columns; an all-zero image; a cancelling chunk."""
    ratios = {}
    for n, K in [(128, 96), (728, 736)]:
        case = make_case(f"{kind} sep K{K} n{n}", MODE_DW, K, n, 3, 9, 9, seed=7 + n, relu_out=1, with_res=True,
                         wide=kind == "wide", pattern=None if kind == "wide" else kind, device=DEV)
        _merge(ratios, _fused(case)[1])
    _print(ratios)


# ------------------------------------------------------------------ 2-D tiled, ids 160-204
@pytest.mark.parametrize("H", [1, 5, 9])
@pytest.mark.parametrize("W", [64, 67, 81])
def test_tiled_2d(W, H):
    ratios, seen = {}, set()
    for i, (K, n) in enumerate(itertools.product((64, 128), (120, 248))):
        ri, ro, res = COMBOS[(3 * [64, 67, 81].index(W) + [1, 5, 9].index(H) + 5 * i) % len(COMBOS)]
        case = make_case(f"2d B2 {H}x{W} K{K} n{n} in{ri} out{ro} res{res}", MODE_DW, K, n, 2, H, W,
                         seed=2000 + W + 10 * H + K + n, relu_in=bool(ri), relu_out=ro, with_res=bool(res), device=DEV)
        ids, r = _fused(case, S2D_BASE, C3_BASE)
        seen.update(ids)
        _merge(ratios, r)
    assert set(S2DP) | set(S2DW) <= seen, sorted((set(S2DP) | set(S2DW)) - seen)
    _print(ratios)


@pytest.mark.parametrize("kind", ["wide", "zero", "cancel"])
def test_tiled_2d_strides_and_patterns(kind):
    case = make_case(f"{kind} 2d", MODE_DW, 64, 120, 2, 5, 67, seed=31, relu_out=2, with_res=True,
                     wide=kind == "wide", pattern=None if kind == "wide" else kind, device=DEV)
    _print(_fused(case, S2D_BASE, C3_BASE)[1])


def test_tiled_2d_relu_after_add_without_residual():
    """relu_out 2 with no residual is still a ReLU (the DMA-wave ids 200-204 once skipped it)."""
    ratios, seen = {}, set()
    for n in (120, 248):
        case = make_case(f"2d relu2 nores n{n}", MODE_DW, 64, n, 2, 5, 67, seed=32, relu_out=2, device=DEV)
        ids, r = _fused(case, S2D_BASE, C3_BASE)
        seen.update(ids)
        _merge(ratios, r)
    assert set(S2DW) <= seen
    _print(ratios)


# ------------------------------------------------------------------ pointwise and 3x3, ids 0-9, 16-63, split-K
def _geometry(mode, M, stride, even):
    """(B, H, W) with B * OH * OW == M: one output row, H odd or even."""
    if mode == MODE_PW:
        return (1, 1, M) if stride == 1 else (1, 2, 2 * M) if even else (1, 1, 2 * M - 1)
    return (1, 3, M + 2) if stride == 1 else (1, 4, 2 * M + 2) if even else (1, 3, 2 * M + 1)


def _gemm_ids(lay, W):
    return [c for _, c in lay.variants(W) if c < SEP_BASE or is_splitk(c)]


@pytest.mark.parametrize("mode,cin", [(MODE_PW, 32), (MODE_PW, 64), (MODE_PW, 2304), (MODE_PW, 512),
                                      (MODE_CONV, 32), (MODE_CONV, 64), (MODE_CONV, 256)])
def test_pointwise_and_3x3(mode, cin):
    """M in {1, 15, 17, BM - 1, BM + 1} for every M tile height among the ids; stride, element type,
    krot, opad, relu_out and the residual rotate over the M values. n = 376 offers every N tile up
    to 384; n = 728 adds the 768-wide tiles of ids 4, 5 and 7 at their own M values.
    cin 512 (K/32 = 16) is there for ksplit 16."""
    ratios, seen = {}, set()
    probe = make_case("probe", mode, cin, 376, 1, 3, 3, seed=0, ksplit=(2, 3, 16))
    bms = sorted({cfg_tile(c)[0] for c in _gemm_ids(probe.lay, 3)})
    for n, ms in [(376, sorted({1, 15, 17} | {b + d for b in bms for d in (-1, 1)})), (728, [1, 15, 17, 31, 33, 63, 65])]:
        for i, M in enumerate(ms):
            stride, f16, krot, opad = 1 + i % 2, (i // 2) % 2, (i // 3) % 2, i % 3
            _, ro, res = COMBOS[(i + cin // 32) % len(COMBOS)]
            case = make_case(f"gemm mode{mode} cin{cin} n{n} M{M} s{stride} f16{f16} krot{krot} opad{opad} out{ro} res{res}",
                             mode, cin, n, *_geometry(mode, M, stride, i % 4 >= 2), seed=3000 + cin + M + n,
                             stride=stride, relu_out=ro, with_res=bool(res), opad=opad, krot=krot,
                             dtype=torch.float16 if f16 else torch.bfloat16, ksplit=(2, 3, 16), device=DEV)
            assert case.M == M
            run = Runner(case)
            ids = _gemm_ids(case.lay, case.g.W)
            if n == 728:
                ids = [c for c in ids if c < PIPE_BASE and cfg_tile(c)[1] == 768]
            for cfg in ids:
                run.run(cfg)
                if (case.lay.K // 32) % 16 == 0 and PIPE_BASE <= cfg < SEP_BASE and cfg_tile(cfg)[0] <= 160:
                    run.run(cfg, sk=16)
            seen.update(ids)
            _merge(ratios, run.ratios)
    sks = {splitk_parts(c)[0] for c in seen if is_splitk(c)}
    assert sks == {s for s in (2, 3) if (probe.lay.K // 32) % s == 0}, sks
    assert {4, 5, 7} <= seen
    _print(ratios)


@pytest.mark.parametrize("kind", ["wide", "zero", "cancel"])
@pytest.mark.parametrize("mode", [MODE_PW, MODE_CONV])
def test_pointwise_and_3x3_strides_and_patterns(mode, kind):
    B, H, W = (2, 3, 11) if mode == MODE_PW else (2, 5, 13)
    case = make_case(f"{kind} gemm mode{mode}", mode, 64, 376, B, H, W, seed=41, relu_out=1, with_res=True, krot=1,
                     wide=kind == "wide", pattern=None if kind == "wide" else kind, ksplit=(2,), device=DEV)
    run = Runner(case)
    for cfg in _gemm_ids(case.lay, W):
        run.run(cfg)
    _print(run.ratios)


@pytest.mark.parametrize("kind", ["randn", "wide", "zero", "cancel"])
@pytest.mark.parametrize("B,H,W", [(2, 3, 3), (1, 7, 21), (2, 11, 36)])
def test_conv3x3_tiled(B, H, W, kind):
    """ids 208-215 (cin 32, one N tile, no residual): a single pixel, partial tiles in both directions;
    also with ldx = cin_pad + 32 over NaN pad columns, an all-zero image and a cancelling chunk."""
    case = make_case(f"c3 {kind} B{B} {H}x{W}", MODE_CONV, 32, 56, B, H, W, seed=50 + H, wide=kind == "wide",
                     pattern=kind if kind in ("zero", "cancel") else None, device=DEV)
    assert case.ldx == (64 if kind == "wide" else 32)
    run = Runner(case)
    ids = [c for _, c in case.lay.variants(W) if c >= C3_BASE]
    assert len(ids) == 8, ids
    for ro in (0, 1):
        case.set_epilogue(ro, False)
        for cfg in ids:
            run.run(cfg, tag=f"out{ro}")
    _print(run.ratios)


# ------------------------------------------------------------------ split lowering: dw3x3, then the GEMM
@pytest.mark.parametrize("B,H,W,K,n", [(2, 5, 7, 32, 8), (3, 9, 9, 96, 128), (3, 9, 9, 736, 728), (1, 1, 40, 160, 128)])
def test_split_lowering(B, H, W, K, n):
    """dw3x3 algo 1 and algo 2 (partial bands and segments) into a guarded scratch buffer, then a
    register-B, an LDS-DMA and a split-K GEMM on it, end to end with the fp32-weight bound."""
    case = make_case(f"split B{B} {H}x{W} K{K} n{n}", MODE_DW, K, n, B, H, W, seed=60 + K, relu_in=True, relu_out=1,
                     with_res=True, ksplit=(2, 3), device=DEV)
    lay, run = case.lay, Runner(case)
    splits = [c for split, c in lay.variants(W) if split]
    gemms = [next(c for c in splits if c < PIPE_BASE), next(c for c in splits if PIPE_BASE <= c < SEP_BASE)]
    gemms += [c for c in splits if is_splitk(c)][:1]
    for kw in [dict(algo=1), dict(algo=2), dict(algo=2, seg=2, rb=2, pd=2), dict(algo=2, seg=3, rb=5, pd=1),
               dict(algo=2, seg=4, rb=H, pd=2)]:
        tw, tmp = guarded(case.M * lay.cin_pad, GUARD_ROWS * lay.cin_pad, lay.dtype, float("nan"), DEV)
        _lib.lib().dw3x3({**lay.dw_args(_lib.ptr(run.x), _lib.ptr(tmp), case.g), **kw}, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert guards_intact(tw, tmp.numel()), f"{case.name} {kw}: scratch guard overwritten"
        assert not torch.isnan(tmp.float()).any(), f"{case.name} {kw}: scratch element unwritten"
        for cfg in gemms:
            run.run(cfg, x=tmp, mode=MODE_PW, tag=str(kw), file="dwconv.hip")
    _print(run.ratios)
