"""Float64 reference, per-element error bound, checker and CPU emulation for the conv-GEMM
family (conv_gemm.hip, gemm_pipe.hip with split-K, sepconv_ws.hip, sepconv_2d.hip,
conv3x3_2d.hip, dwconv.hip). Shared by test_conv_bound_cpu.py and test_conv_edges_gpu.py.

Everything is float64 numpy on the CPU, from the exact operands the kernel consumes: the
bf16 / fp16 ``x`` and ``res``, ``lay.w_ref`` (the element-type-rounded weights), the fp32 bias,
and the depthwise weights in the form the id reads (``form``):

  "fp32"  ids 0-9 and the split lowering's dw3x3: the fp32 ``dww``
  "bf16"  ids >= 120: ``bf16(dww)``, as pack_dw_entries rounds them for the matrix cores

Error model, u = 2^-23, in the order the kernel rounds:

  depthwise   a64[m,k] = exact 9-tap sum (ReLU on load, zero padding), Ab = sum |x||w|,
              eta = (32 + 16) u Ab: an fp32 9-FMA chain or one 32-deep MFMA step, with the
              factor 2 the gallery tests use for the MFMA's undocumented internal rounding.
  bf16(a)     a_ref = bf16_rn(a64). Rounding is monotonic, so the kernel's value lies between
              bf16_rn(a64 - eta) and bf16_rn(a64 + eta): D[m,k] is the larger distance of
              those two from a_ref. D is zero unless a rounding midpoint lies within eta of
              a64, and then one bf16 ulp ("flagged" entries; their share is capped at 3 % by
              the CPU test, as a condition on the cases, not a measurement).
  GEMM+bias   v64 = a_ref w^T + bias,  G = (K + 16) u (|a_ref| |w|^T + |bias|) + D |w|^T;
              the + 16 covers the (at most 16) split-K partial sums. Pointwise and 3x3 modes:
              a_ref is the gathered input, D = 0.
  store       E1 = G + h(|v64| + G), h(t) = half a bf16 (fp16) ulp of t's binade,
              2^(floor(log2 t) - 8) (- 11 for fp16). ReLU is 1-Lipschitz.
              h(t) lies between 2^-9 t (top of a binade) and 2^-8 t (its bottom). A flat
              2^-9 (|v64| + G) is NOT a bound: round-to-nearest-even of a value at the bottom
              of a binade is off by up to 2^-8 of it (bf16 keeps 8 significant bits), and the
              fp32 emulation below, with torch's own cast, exceeds it on a third of its
              elements. h is the exact statement of the same rounding, never looser than the
              format's unit roundoff and equal to 2^-9 t where that figure holds.
  residual    expected v64 + res; bound E1 + h(|v64 + res| + E1) + 2^-24 (|v64 + res| + E1):
              one more rounding and the fp32 add. ReLU after the add adds nothing.

Columns n .. ldy hold zero weights and zero bias: exactly 0, or exactly res (its ReLU for
relu_out 2). SiLU / GELU epilogues (relu_out 3, 4) and ascale are not modelled here; the MBConv
and ViT edge tests own them.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from kdl.ops.conv import MODE_CONV, MODE_DW, MODE_PW, ConvGemmLayer, Geometry
from kdl.ops.pack import round_up

U = 2.0 ** -23
GUARD_BYTE = 0x5A
MAX_FLAGGED = 0.03


# ---------------------------------------------------------------- number formats
def round_to(a: np.ndarray, dt: int) -> np.ndarray:
    """float64 -> nearest bf16 (dt 0) or fp16 (dt 1) value, ties to even, kept as float64."""
    bits, emin = (8, -133) if dt == 0 else (11, -24)
    _, e = np.frexp(a)
    ulp = np.ldexp(1.0, np.maximum(e - bits, emin))
    return np.rint(a / ulp) * ulp


def half_ulp(t: np.ndarray, dt: int) -> np.ndarray:
    """Half the spacing of bf16 (dt 0) / fp16 (dt 1) values in the binade of t >= 0; 0 at t = 0."""
    bits, emin = (8, -133) if dt == 0 else (11, -24)
    _, e = np.frexp(t)
    return np.where(t > 0, np.ldexp(0.5, np.maximum(e - bits, emin)), 0.0)


def to_f64(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().double().numpy()


# ---------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    lay: ConvGemmLayer
    g: Geometry
    x: torch.Tensor                 # [B*H*W][ldx] element type, CPU; pad columns NaN when ldx > cin_pad
    res: torch.Tensor | None        # [M][ldr]
    ldx: int
    ldr: int
    opad: int = 0
    pattern: str | None = None
    res_on: bool = True             # set_epilogue: launch and reference with or without ``res``
    refs: dict = field(default_factory=dict)

    @property
    def M(self) -> int:
        return self.g.M

    @property
    def r(self) -> torch.Tensor | None:
        return self.res if self.res_on else None

    def set_epilogue(self, relu_out: int, res_on: bool) -> "Case":
        """Another epilogue on the same operands: the depthwise and GEMM part of the reference is shared."""
        assert self.res is not None or not res_on
        self.lay.relu_out, self.res_on = int(relu_out), bool(res_on)
        return self

    def core(self, form: str = "fp32"):
        form = form if self.lay.mode == MODE_DW else "fp32"
        if ("core", form) not in self.refs:
            self.refs["core", form] = _core(self, form)
        return self.refs["core", form]

    def ref(self, form: str = "fp32"):
        key = (form if self.lay.mode == MODE_DW else "fp32", self.lay.relu_out, self.r is not None)
        if key not in self.refs:
            self.refs[key] = reference(self, key[0])
        return self.refs[key]

    def flagged(self) -> float:
        """Largest share of depthwise entries flagged in D over the two weight forms (0 off MODE_DW)."""
        return max(self.core(f)[2] for f in ("fp32", "bf16")) if self.lay.mode == MODE_DW else 0.0


def make_case(name, mode, cin, n, B, H, W, *, seed, stride=1, relu_in=False, relu_out=0, with_res=False,
              dtype=torch.bfloat16, wide=False, pattern=None, opad=0, krot=0, ksplit=(), device="cpu") -> Case:
    """A layer with the weight scales of tests/test_kernels_gpu.py's ``_layer`` and randn inputs.
    ``wide``: ldx = cin_pad + 32 and ldr = ldy + 32 with NaN in the pad columns.
    ``pattern`` "zero": image 0 is all zeros; "cancel": the first 8-channel chunk holds +-64
    alternating by channel, with one weight (and depthwise filter) shared by the chunk, so its
    terms cancel exactly in v64 while sum |a||w| stays large.
    The share of depthwise entries flagged in D is a condition on the inputs (at most MAX_FLAGGED
    for both weight forms): a seed whose case exceeds it is replaced by seed + 7919, + 2 * 7919, ...,
    so every case built here meets the cap, on the CPU table and on the GPU alike."""
    kw = dict(stride=stride, relu_in=relu_in, relu_out=relu_out, with_res=with_res, dtype=dtype, wide=wide,
              pattern=pattern, opad=opad, krot=krot, ksplit=ksplit, device=device)
    for k in range(32):
        case = _build(name, mode, cin, n, B, H, W, seed + 7919 * k, **kw)
        if case.flagged() <= MAX_FLAGGED:
            return case
    raise AssertionError(f"{name}: no seed within the {MAX_FLAGGED:.0%} cap on flagged depthwise entries")


def _build(name, mode, cin, n, B, H, W, seed, *, stride, relu_in, relu_out, with_res, dtype, wide, pattern, opad, krot,
           ksplit, device) -> Case:
    gen = torch.Generator().manual_seed(seed)
    cin_pad = round_up(cin, 32)
    K = 9 * cin_pad if mode == MODE_CONV else cin_pad
    w = torch.zeros(n, K, dtype=torch.float64)
    if mode == MODE_CONV:
        w.view(n, 9, cin_pad)[:, :, :cin] = torch.randn(n, 9, cin, generator=gen, dtype=torch.float64) / (9 * cin) ** 0.5
    else:
        w[:, :cin] = torch.randn(n, cin, generator=gen, dtype=torch.float64) / cin ** 0.5
    bias = torch.randn(n, generator=gen) * 0.1
    dww = None
    if mode == MODE_DW:
        dww = torch.zeros(9, cin_pad)
        dww[:, :cin] = torch.randn(9, cin, generator=gen) / 3
    x = torch.zeros(B, H, W, cin_pad)
    x[..., :cin] = torch.randn(B, H, W, cin, generator=gen)
    if pattern == "zero":
        x[0] = 0
    elif pattern == "cancel":
        assert cin >= 8 and not relu_in
        x[..., :8] = 64.0 * torch.tensor([1, -1] * 4)
        w.view(n, -1, cin_pad)[:, :, :8] = w.view(n, -1, cin_pad)[:, :, :1]
        if dww is not None:
            dww[:, :8] = dww[:, :1]
    else:
        assert pattern is None
    if mode == MODE_DW:
        OH, OW = H, W
    elif mode == MODE_CONV:
        OH, OW = (H - 3) // stride + 1, (W - 3) // stride + 1
    else:
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = Geometry(B, H, W, OH, OW)
    lay = ConvGemmLayer(name, mode, w, bias, cin_pad=cin_pad, n=n, stride=stride, dww=dww, relu_in=relu_in,
                        relu_out=relu_out, device=device, dtype=dtype, ksplit=ksplit)
    lay.krot = krot
    ldx = cin_pad + (32 if wide else 0)
    ldr = lay.ldy + (32 if wide else 0)
    xb = torch.full((B * H * W, ldx), float("nan"))
    xb[:, :cin_pad] = x.view(-1, cin_pad)
    res = None
    if with_res:
        res = torch.full((g.M, ldr), float("nan"))
        res[:, :lay.ldy] = 0
        res[:, :n] = torch.randn(g.M, n, generator=gen)
        res = res.to(dtype)
    return Case(name, lay, g, xb.to(dtype), res, ldx, ldr, opad=opad, pattern=pattern)


# ---------------------------------------------------------------- float64 reference and bound
def _taps(xs: np.ndarray):
    """xs [B][H][W][C] -> the nine zero-padded shifted views, tap = 3 * dy + dx."""
    B, H, W, C = xs.shape
    xp = np.zeros((B, H + 2, W + 2, C), xs.dtype)
    xp[:, 1:-1, 1:-1] = xs
    return [xp[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]


def _operands(case: Case, form: str):
    lay, g = case.lay, case.g
    xs = to_f64(case.x)[:, :lay.cin_pad].reshape(g.B, g.H, g.W, lay.cin_pad)
    w = to_f64(lay.w_ref)
    bias = to_f64(lay.bias)[:lay.n]
    dww = None
    if lay.mode == MODE_DW:
        dww = lay.dww.detach().cpu()
        dww = to_f64(dww.to(torch.bfloat16) if form == "bf16" else dww)
    return xs, w, bias, dww


def gather(case: Case, xs: np.ndarray) -> np.ndarray:
    """The pointwise / 3x3 A operand [M][K] (k = tap * cin_pad + c)."""
    lay, g = case.lay, case.g
    st = lay.stride
    if lay.mode == MODE_PW:
        return xs[:, ::st, ::st][:, :g.OH, :g.OW].reshape(g.M, lay.cin_pad)
    cols = [xs[:, dy:dy + st * (g.OH - 1) + 1:st, dx:dx + st * (g.OW - 1) + 1:st] for dy in range(3) for dx in range(3)]
    return np.concatenate(cols, -1).reshape(g.M, 9 * lay.cin_pad)


def _core(case: Case, form: str):
    """-> (v64 [M][n] before any ReLU, G [M][n], share of (m, k) entries flagged in D)."""
    lay, g = case.lay, case.g
    xs, w, bias, dww = _operands(case, form)
    if lay.mode == MODE_DW:
        xin = np.maximum(xs, 0) if lay.relu_in else xs
        a64 = np.zeros_like(xin)
        ab = np.zeros_like(xin)
        for t, v in enumerate(_taps(xin)):
            a64 += v * dww[t]
            ab += np.abs(v) * np.abs(dww[t])
        eta = 48 * U * ab
        a_ref = round_to(a64, 0)
        D = np.maximum(np.abs(round_to(a64 + eta, 0) - a_ref), np.abs(round_to(a64 - eta, 0) - a_ref))
        a_ref, D = a_ref.reshape(g.M, -1), D.reshape(g.M, -1)
        flagged = float((D > 0).mean())
    else:
        a_ref = gather(case, xs)
        D, flagged = None, 0.0
    aw = np.abs(w).T
    v = a_ref @ w.T + bias
    G = (lay.K + 16) * U * (np.abs(a_ref) @ aw + np.abs(bias))
    if D is not None:
        G += D @ aw
    return v, G, flagged


def reference(case: Case, form: str = "fp32"):
    """-> (expected [M][ldy], bound [M][ldy], share of (m, k) entries flagged in D)."""
    lay, g = case.lay, case.g
    v, G, flagged = case.core(form)
    E = G + half_ulp(np.abs(v) + G, lay.dt)
    if lay.relu_out == 1:
        v = np.maximum(v, 0)
    exp = np.zeros((g.M, lay.ldy))
    bnd = np.zeros((g.M, lay.ldy))
    exp[:, :lay.n], bnd[:, :lay.n] = v, E
    if case.r is not None:
        exp = exp + to_f64(case.r)[:, :lay.ldy]
        t = np.abs(exp[:, :lay.n]) + E
        bnd[:, :lay.n] = E + half_ulp(t, lay.dt) + 2.0 ** -24 * t
    if lay.relu_out == 2:
        exp = np.maximum(exp, 0)
    return exp, bnd, flagged


def exact_rows_of_zero_image(case: Case) -> np.ndarray:
    """Rows of an all-zero image have a = 0 exactly: the output is the rounded bias (+ res), bit for bit."""
    lay = case.lay
    b = np.zeros(lay.ldy)
    b[:lay.n] = to_f64(lay.bias)[:lay.n]
    if lay.relu_out == 1:
        b = np.maximum(b, 0)
    rows = case.g.OH * case.g.OW
    e = np.broadcast_to(round_to(b, lay.dt), (rows, lay.ldy))
    if case.r is not None:
        e = round_to(e + to_f64(case.r)[:rows, :lay.ldy], lay.dt)
    return np.maximum(e, 0) if lay.relu_out == 2 else e


# ---------------------------------------------------------------- guarded buffers
def guarded(numel: int, guard: int, dtype, fill, device="cpu"):
    """-> (whole, body): ``body`` (numel elements, filled with ``fill``) between two guard regions
    of ``guard`` elements (rounded up to 64) holding GUARD_BYTE in every byte."""
    guard = round_up(max(guard, 64), 64)
    whole = torch.empty(numel + 2 * guard, dtype=dtype, device=device)
    whole.view(torch.uint8).fill_(GUARD_BYTE)
    body = whole[guard:guard + numel]
    body.fill_(fill)
    return whole, body


def guards_intact(whole: torch.Tensor, numel: int) -> bool:
    guard = (whole.numel() - numel) // 2
    b = whole.detach()                      # compared where the buffer lives: only two flags cross to the host
    lo, hi = b[:guard].view(torch.uint8), b[guard + numel:].view(torch.uint8)
    return bool((lo == GUARD_BYTE).all()) and bool((hi == GUARD_BYTE).all())


# ---------------------------------------------------------------- checker
def out_rows(case: Case) -> np.ndarray:
    """Row of the output buffer that holds output row m (epilogue.h out_offset)."""
    g = case.g
    m = np.arange(g.M)
    if case.opad == 0:
        return m
    ohw = g.OH * g.OW
    b, rem = m // ohw, m % ohw
    if case.opad == 2:
        return b * (ohw + 1) + 1 + rem
    return (b * (g.OH + 2) + rem // g.OW + 1) * (g.OW + 2) + rem % g.OW + 1


def buf_rows(case: Case) -> int:
    g = case.g
    if case.opad == 1:
        return g.B * (g.OH + 2) * (g.OW + 2)
    if case.opad == 2:
        return g.B * (g.OH * g.OW + 1)
    return g.M


def check(y: torch.Tensor, case: Case, form: str = "fp32", guards=(), prefill=None, tag: str = "") -> float:
    """``y``: the whole output buffer [buf_rows][ldy] (element type). Asserts that every stored
    element is within its bound (NaN never is), that columns n .. ldy are exact, that rows the op
    does not own (opad borders) still hold ``prefill``, and that every (whole, numel) pair of
    ``guards`` is intact. Prints and returns the largest error / bound ratio."""
    lay = case.lay
    tag = f"{case.name} {tag}"
    for i, (whole, numel) in enumerate(guards):
        assert guards_intact(whole, numel), f"{tag}: guard {i} overwritten"
    exp, bnd, _ = case.ref(form)
    yb = to_f64(y).reshape(buf_rows(case), lay.ldy)
    rows = out_rows(case)
    if case.opad:
        other = np.ones(len(yb), bool)
        other[rows] = False
        assert np.array_equal(yb[other], to_f64(prefill).reshape(yb.shape)[other]), f"{tag}: a row outside the output changed"
    yy = yb[rows]
    err = np.abs(yy[:, :lay.n] - exp[:, :lay.n])
    b = bnd[:, :lay.n]
    bad = ~(err <= b)                                # NaN compares false: an unwritten element fails
    if bad.any():
        m, c = np.argwhere(bad)[0]
        raise AssertionError(f"{tag}: {int(bad.sum())} element(s) out of bound, first y[{m},{c}] = {yy[m, c]!r}, "
                             f"expected {exp[m, c]!r} +- {b[m, c]:.3e}")
    pad_ok = yy[:, lay.n:] == exp[:, lay.n:]
    assert pad_ok.all(), f"{tag}: pad column {lay.n + int(np.argwhere(~pad_ok)[0][1])} is not exact"
    nz = b > 0
    ratio = float((err[nz] / b[nz]).max()) if nz.any() else 0.0
    assert (err[~nz] == 0).all(), f"{tag}: a zero-bound element differs"
    if case.pattern == "zero":                       # image 0 is all zeros: rounded bias (+ res), bit for bit
        e = exact_rows_of_zero_image(case)
        assert np.array_equal(yy[:len(e)], e), f"{tag}: rows of the all-zero image are not the rounded bias"
    print(f"{tag}: max err/bound {ratio:.3f}")
    return ratio


def old_gate_passes(y: torch.Tensor, case: Case, form: str = "fp32") -> bool:
    """tests/test_kernels_gpu.py's ``_check``: max |y - ref| <= 2e-2 max |ref|, pad columns exactly 0
    (it starts from zeros, so an unwritten element reads 0 there)."""
    exp, _, _ = case.ref(form)
    yy = np.nan_to_num(to_f64(y).reshape(-1, case.lay.ldy)[:case.M], nan=0.0)
    return bool(np.abs(yy - exp).max() <= 2e-2 * (np.abs(exp).max() + 1e-6))


# ---------------------------------------------------------------- CPU emulation with planted faults
FAULTS = ("tap_clamped", "bias_dropped", "dw_truncated", "res_row", "kstep_skipped", "guard_hit", "pad_unwritten")


def fault_applies(case: Case, fault: str) -> bool:
    lay = case.lay
    if fault in ("tap_clamped", "dw_truncated"):
        return lay.mode == MODE_DW
    if fault == "res_row":
        return case.r is not None and case.M > 1
    if fault == "pad_unwritten":
        return lay.n < lay.ldy
    if fault == "bias_dropped":             # an output can only show a bias that is larger than its bound:
        c = _smallest_bias(case)            # among 728 channels the smallest |bias| is ~1e-4, below any bound
        return all(abs(float(case.lay.bias[c])) > 2 * case.ref(f)[1][:, c].min() for f in ("fp32", "bf16"))
    return True


def _smallest_bias(case: Case) -> int:
    b = np.abs(to_f64(case.lay.bias)[:case.lay.n])
    return int(np.argmin(np.where(b != 0, b, np.inf)))


def _cast(a: np.ndarray, dt: int) -> np.ndarray:
    """fp32 -> element type -> fp32, round to nearest even (the kernels' pack)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float16 if dt else torch.bfloat16).float().numpy()


def emulate(case: Case, form: str = "fp32", fault: str | None = None):
    """numpy fp32 model of the kernel with its roundings: a sequential fp32 depthwise, cast to bf16,
    fp32 GEMM + bias, store rounding, residual add. Writes into a NaN-filled guarded buffer and
    returns (whole, body [M][ldy]). ``fault``: one of FAULTS, planted as the issue describes."""
    lay, g = case.lay, case.g
    assert case.opad == 0
    xs, w, bias, dww = _operands(case, form)
    xs, w, bias = xs.astype(np.float32), w.astype(np.float32), bias.astype(np.float32)
    if lay.mode == MODE_DW:
        xin = np.maximum(xs, 0) if lay.relu_in else xs
        taps = [t.copy() for t in _taps(xin)]
        if fault == "tap_clamped":          # last image, pixel (0, 0), tap (-1, -1): the clamped neighbour is the
            px = xin[-1, 0, 0]               # pixel itself; the 8-channel chunk (not the first) of median tap weight
            wt = (np.abs(px) * np.abs(dww[0])).reshape(-1, 8)[1:].sum(1)
            c8 = 8 * (int(np.argsort(wt)[len(wt) // 2]) + 1)
            taps[0][-1, 0, 0, c8:c8 + 8] = px[c8:c8 + 8]
        acc = np.zeros_like(xin)
        for t, v in enumerate(taps):
            acc = acc + v * dww[t].astype(np.float32)
        if fault == "dw_truncated":
            a = (acc.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        else:
            a = _cast(acc, 0)
        a = a.reshape(g.M, -1)
    else:
        a = gather(case, xs)
    if fault == "bias_dropped":
        bias = bias.copy()
        bias[_smallest_bias(case)] = 0
    v = a @ w.T
    if fault == "kstep_skipped":            # the last M tile (16 rows) stops one k-step early
        rows = min(16, g.M)
        v[-rows:] = a[-rows:, :lay.K - 32] @ w[:, :lay.K - 32].T
    v = v + bias
    if lay.relu_out == 1:
        v = np.maximum(v, 0)
    out = np.zeros((g.M, lay.ldy), np.float32)
    out[:, :lay.n] = v
    out = _cast(out, lay.dt)
    if case.r is not None:
        rv = case.r.float().numpy()[:, :lay.ldy].copy()
        if fault == "res_row":
            rv[g.M - 1] = rv[g.M - 2]
        out = _cast(out + rv, lay.dt)
    if lay.relu_out == 2:
        out = np.maximum(out, 0)
    whole, body = guarded(g.M * lay.ldy, 16 * lay.ldy, case.lay.dtype, float("nan"))
    body.view(g.M, lay.ldy).copy_(torch.from_numpy(out))
    if fault == "pad_unwritten":
        body.view(g.M, lay.ldy)[:, lay.n] = float("nan")
    if fault == "guard_hit":                # one 16-byte store at row M
        whole[whole.numel() - (whole.numel() - body.numel()) // 2:][:8] = 0
    return whole, body
