"""dwconv7_ln and ln_s2d (kernels/dwconv_ln.hip) at the smallest shapes that reach each of their
indices, against a float64 reference over the stored values (bf16 x; fp32 w, bias, gamma, beta), and
the ConvNeXt-Tiny engine built on them against the fp32 oracle (run on MI355X).

Per-element bound (the form of tests/_conv_cases.py), per pixel, u = 2^-24:
  d      an fp32 chain of 49 multiply-adds from the bias (fused or not: at most two roundings a tap)
         is within e_c = (2*49 + 16) u (sum |x*w| + |bias_c|) of the exact d_c.
  stats  the fp32 sum of C values adds at most (C + 16) u max_c |d_c| to the mean, so every d_c the
         statistics see is within E = max_c e_c + (C + 16) u max_c |d_c| of a consistent exact row.
  norm   with s = sqrt(var + eps), n_c = (d_c - mean) / s: a perturbation of at most E in every d_c
         moves a centred value by at most 2E and s by at most 2E (the triangle inequality on the
         row's norm), so n_c moves by at most (2E / s')(1 + |n_c|), s' >= s - 2E; to first order
         g_c = |gamma_c| (2E / s)(1 + |n_c|) + 8 u (|gamma_c n_c| + |beta_c|), the last term for the
         fp32 rsqrt, scale and shift. E <= s / 64 is asserted on every tested pixel, which keeps the
         first-order form within 1 / 32 of the exact one.
  store  |y - exact| <= g_c + half a bf16 ulp at |exact| + g_c.
ln_s2d: the same with e_c = 0 (d = x is exact). An fp32 torch emulation of the kernel's arithmetic
(sequential unfused chain, two-pass variance, one rounding) reached at most 0.97 of the bound on the
CPU: the store's half ulp is most of the bound, and a rounding can use all of it.
"""
import itertools

import numpy as np
import pytest
import torch

from _conv_cases import guarded, guards_intact, half_ulp, to_f64
from kdl.ops import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
MAPS = ((3, 5), (7, 7), (10, 19))   # under the halo on both sides / every row partly outside / interior, odd W, H > ring
_REFS: dict = {}


def make(C, H, W, seed=0, variant=""):
    """Stored operands. ``variant``: "image" scales image 1's x by 256; "chunk" scales every channel
    outside chunk 1 by 256 with gamma = 1, beta = 0; "flat" is x = 0, bias = 3."""
    gen = torch.Generator().manual_seed(seed + 31 * C + H)
    x = torch.randn(2, H, W, C, generator=gen)
    w, bias = torch.randn(49, C, generator=gen) / 7, torch.randn(C, generator=gen) * 0.1
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), torch.randn(C, generator=gen) * 0.1
    if variant == "image":
        x[1] *= 256
    elif variant == "chunk":
        x[..., :8] *= 256
        x[..., 16:] *= 256
        gamma, beta = torch.ones(C), torch.zeros(C)
    elif variant == "flat":
        x, bias = torch.zeros_like(x), torch.full((C,), 3.0)
    return dict(C=C, H=H, W=W, B=2, x=x.to(torch.bfloat16), w=w, bias=bias, gamma=gamma, beta=beta)


def norm_reference(d, e, c, eps):
    """d [..., C] exact, e its per-element error -> (exact y, bound), float64; asserts E <= s / 64."""
    C, gamma, beta = d.shape[-1], to_f64(c["gamma"]), to_f64(c["beta"])
    E = (e.max(-1) + (C + 16) * U * np.abs(d).max(-1))[..., None]
    mean = d.mean(-1, keepdims=True)
    s = np.sqrt(((d - mean) ** 2).mean(-1, keepdims=True) + eps)
    assert (E <= s / 64).all(), "the first-order bound needs E <= s / 64"
    n = (d - mean) / s
    exact = gamma * n + beta
    g = np.abs(gamma) * (2 * E / s) * (1 + np.abs(n)) + 8 * U * (np.abs(gamma * n) + np.abs(beta))
    return exact, g + half_ulp(np.abs(exact) + g, 0)


def reference(c, eps=1e-6):
    x, w, bias = to_f64(c["x"]), to_f64(c["w"]), to_f64(c["bias"])
    H, W = c["H"], c["W"]
    xp = np.zeros((c["B"], H + 6, W + 6, c["C"]))
    xp[:, 3:-3, 3:-3] = x
    d, mag = np.broadcast_to(bias, x.shape).copy(), np.broadcast_to(np.abs(bias), x.shape).copy()
    for ky, kx in itertools.product(range(7), range(7)):
        t = xp[:, ky:ky + H, kx:kx + W] * w[ky * 7 + kx]
        d += t
        mag += np.abs(t)
    return norm_reference(d, (2 * 49 + 16) * U * mag, c, eps)


def shared(C, H, W, variant=""):
    key = (C, H, W, variant)
    if key not in _REFS:
        c = make(C, H, W, variant=variant)
        _REFS[key] = (c, {k: c[k].to(DEV).contiguous() for k in ("x", "w", "bias", "gamma", "beta")}, reference(c))
    return _REFS[key]


def run(op, c, dev, ref, out_rows, ncol, pad, eps=1e-6, **over):
    """One launch into a guarded, pre-filled output of row stride ncol + pad; every element against its
    bound, pad columns and guards untouched. -> largest error / bound."""
    ldy = ncol + pad
    whole, body = guarded(out_rows * ldy, 64 * ldy, torch.bfloat16, 7.0, DEV)
    args = dict(y=body.data_ptr(), ldx=c["C"], ldy=ldy, eps=eps, **{k: c[k] for k in ("B", "H", "W", "C")},
                **{k: v.data_ptr() for k, v in dev.items()})
    args.update(over)
    getattr(_lib.lib(), op)(args, _lib.stream_ptr())
    torch.cuda.synchronize()
    y = to_f64(body).reshape(out_rows, ldy)
    exact, bnd = (a.reshape(out_rows, ncol) for a in ref)
    err = np.abs(y[:, :ncol] - exact)
    ratio = float((np.where(np.isnan(err), np.inf, err) / bnd).max())
    print(f"RATIO {op} C={c['C']} {c['H']}x{c['W']} pad={pad} {over}: {ratio:.3f}")
    assert ratio <= 1.0
    assert (y[:, ncol:] == 7.0).all(), "pad columns written"
    assert guards_intact(whole, out_rows * ldy)
    return body


@pytest.mark.parametrize("hw", MAPS)
@pytest.mark.parametrize("C", [96, 768])
def test_dwconv7_ln_within_bound(C, hw):
    """The launcher's band, bands of two rows (prologue and one ring step) and one band of the whole map;
    the launcher's strip and, on the 19-wide map, one that makes three (C = 96) or seven strips."""
    H, W = hw
    c, dev, ref = shared(C, H, W)
    tws = (0, 7 if C == 96 else 3) if W == 19 else (0,)
    for rows, tw, pad in itertools.product((0, 2, H), tws, (0, 16)):
        run("dwconv7_ln", c, dev, ref, 2 * H * W, C, pad, rows=rows, tw=tw)


@pytest.mark.parametrize("variant", ["image", "chunk"])
@pytest.mark.parametrize("C", [96, 768])
def test_dwconv7_ln_reads_no_other_image_or_channel(C, variant):
    """Image 1, or every channel outside one 8-channel chunk, is 256 times larger: a read across an
    image or channel boundary is off by orders of magnitude of the bound."""
    c, dev, ref = shared(C, 7, 7, variant)
    run("dwconv7_ln", c, dev, ref, 2 * 49, C, 0, rows=2)


@pytest.mark.parametrize("C", [96, 768])
def test_dwconv7_ln_constant_pixel(C):
    """x = 0, bias = 3: every d is 3 exactly, so are the sum and the mean, every deviation is 0 and the
    output is bf16(beta) bit for bit at the model's eps (a one-pass variance gives 9 - 9 +- an ulp of 9
    against eps = 1e-6); at eps = 1e-3 the bound's own condition holds and is asserted too."""
    c = make(C, 7, 7, variant="flat")
    dev = {k: c[k].to(DEV).contiguous() for k in ("x", "w", "bias", "gamma", "beta")}
    run("dwconv7_ln", c, dev, reference(c, 1e-3), 2 * 49, C, 0, eps=1e-3)
    beta = to_f64(c["beta"].to(torch.bfloat16)) + np.zeros((2 * 49, C))
    y = run("dwconv7_ln", c, dev, (beta, np.full_like(beta, np.inf)), 2 * 49, C, 0)
    assert np.array_equal(to_f64(y).reshape(2 * 49, C), beta)


REFUSED = {"C=12": dict(C=12, ldx=16, ldy=16), "C=1032": dict(C=1032, ldx=1032, ldy=1032), "ldy<C": dict(ldy=88),
           "y_align": {}, "eps=0": dict(eps=0.0), "ring": dict(H=10, W=19, tw=19, rows=10)}


@pytest.mark.parametrize("bad", list(REFUSED))
def test_dwconv7_ln_refuses(bad):
    """The call raises and writes nothing. "ring": at C = 768 eight rows of 19 + 6 pixels exceed the LDS."""
    C = 768 if bad == "ring" else 96
    c, dev, _ = shared(C, 10, 19)
    whole, body = guarded(2 * 190 * 1032 + 8, 4096, torch.bfloat16, 7.0, DEV)
    args = dict(y=body.data_ptr() + (2 if bad == "y_align" else 0), ldx=C, ldy=C, eps=1e-6, B=2, H=10, W=19, C=C,
                **{k: v.data_ptr() for k, v in dev.items()})
    args.update(REFUSED[bad])
    with pytest.raises(RuntimeError):
        _lib.lib().dwconv7_ln(args, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((body == 7.0).all()) and guards_intact(whole, body.numel())


@pytest.mark.parametrize("hw", [(2, 2), (6, 10)])
@pytest.mark.parametrize("C", [96, 384])
def test_ln_s2d_within_bound_and_in_order(C, hw):
    """Every pixel against the bound at column (ky*2 + kx)*C + c of row (b, oy/2, ox/2); an odd H is refused."""
    H, W = hw
    c = make(C, H, W, seed=5)
    dev = {k: c[k].to(DEV).contiguous() for k in ("x", "gamma", "beta")}
    x = to_f64(c["x"])
    s2d = lambda a: a.reshape(2, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 4 * C)  # noqa: E731
    ref = tuple(s2d(a) for a in norm_reference(x, np.zeros_like(x), c, 1e-6))
    for pad in (0, 16):
        body = run("ln_s2d", c, dev, ref, 2 * H * W // 4, 4 * C, pad)
    with pytest.raises(RuntimeError):
        _lib.lib().ln_s2d(dict(x=dev["x"].data_ptr(), gamma=dev["gamma"].data_ptr(), beta=dev["beta"].data_ptr(),
                               y=body.data_ptr(), B=2, H=H - 1, W=W, C=C, ldx=C, ldy=4 * C, eps=1e-6), _lib.stream_ptr())


# ------------------------------------------------------------------------------------------ engine
def test_convnext_engine_matches_oracle():
    """vit_b16's gate of tests/test_bench_configs_gpu.py (the family with this GEMM / LayerNorm / GELU
    mix): relative logit error <= 0.05 and cosine >= 0.995 against the fp32 oracle on the ResNeXt
    test's three images; captured replays are bit-equal to the eager forward; embed="raw" rows against
    the feature oracle. Measured on MI355X: see profiles/convnext.txt."""
    from kdl.engine import registry
    info = registry.get("convnext_tiny")
    p = info.init_params(0)
    x = torch.randint(0, 256, (3, 224, 224, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    ref = info.oracle(p, x)
    eng = info.engine(p, 2, DEV)
    assert sum(s.kind == "dwln" for s in eng.steps) == 18 and sum(s.kind == "ln_s2d" for s in eng.steps) == 3
    for lo in (0, 2):
        xs, r = x[lo:lo + 2], ref[lo:lo + 2]
        eager = eng.forward(xs.to(DEV), capture=False).cpu()
        for _ in range(3):
            assert torch.equal(eng.forward(xs.to(DEV), capture=True).cpu(), eager)
        rel = ((eager - r).abs().max() / r.abs().max()).item()
        cos = torch.nn.functional.cosine_similarity(eager, r, dim=1).min().item()
        print(f"CONVNEXT images {lo}..: rel {rel:.5f} cos {cos:.6f} top1 {(eager.argmax(1) == r.argmax(1)).tolist()}")
        assert rel <= 0.05 and cos >= 0.995
    rows = info.engine(p, 2, DEV, embed="raw").forward(x[:2].to(DEV)).cpu()
    want = info.feature_oracle(p, x[:2])
    frel = ((rows - want).abs().max() / want.abs().max()).item()
    print(f"CONVNEXT embed raw: rel {frel:.5f}")
    assert rows.shape == want.shape == (2, 768) and frel <= 0.05
