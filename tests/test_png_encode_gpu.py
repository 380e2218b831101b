"""kernels/png_encode.hip against kdl/serving/png_encode.py png_rule, byte for byte."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from _png_cases import CONTENTS, SIZES, cap_of, picture
from kdl.serving import png_encode as E

pytestmark = pytest.mark.gpu

BAND = 8                                                     # kPngBand: a row's predecessor in another workgroup
SHAPES = SIZES + ((BAND + 1, 64), (2 * BAND, 21))


def test_band_is_the_kernels():
    from kdl.ops import _lib
    assert _lib.lib().PNG_ENC_BAND == BAND


@pytest.mark.parametrize("C", (3, 4))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("H,W", SHAPES)
def test_png_encode_equals_the_rule(H, W, C, B):
    """Every content, B pictures a launch (picture b is content b, b + 1, ..: strides and the histogram's
    reset), twice on one workspace."""
    for first in range(0, len(CONTENTS), B):
        names = [CONTENTS[(first + b) % len(CONTENTS)] for b in range(B)]
        pics = np.stack([picture(n, H, W, C, seed=b) for b, n in enumerate(names)])
        cap = max(cap_of(n, H, W, C) for n in names)
        want = E.png_rule(pics, cap)
        assert all(want), names
        dev = torch.from_numpy(pics).cuda()
        files, rows, work = E.encode_gpu(dev, cap)
        again, rows2, _ = E.encode_gpu(dev, cap, work)
        assert files == want, (names, [len(f) for f in files], [len(f) for f in want])
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), E.rows_of(want, cap))      # the zeros behind the file
        assert torch.equal(rows, rows2)
        for f, p in zip(files, pics):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), p)


@pytest.mark.parametrize("S,B", ((299, 2), (600, 1)))
def test_cutout_sized_photographs_fit_the_default_cap(S, B):
    """The served sizes: rows of 1197 and 2401 bytes, every thread with a run of positions, 12 doubling rounds."""
    pics = np.stack([picture("photo", S, S, 4)] * B)
    pics[-1, S // 2:] = pics[-1, S // 2:, ::-1]
    want = E.png_rule(pics)
    files, rows, _ = E.encode_gpu(torch.from_numpy(pics).cuda())
    assert all(want) and files == want
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), E.rows_of(want, E.default_cap(S, S, 4)))


@pytest.mark.parametrize("C", (3, 4))
def test_overflow_writes_length_zero_and_nothing_past_the_row(C):
    from kdl.ops import _lib
    lib = _lib.lib()
    pics = np.stack([picture("noise", 17, 299, C), picture("zero", 17, 299, C)])
    full = E.png_rule(pics, 1 << 20)
    cap = len(full[0]) - 1                                       # one byte short for the noise, room for the other
    ldo = 1 + (cap + 3) // 4 + 2
    dev = torch.from_numpy(pics).cuda()
    rows = torch.full((3, ldo), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    work = torch.zeros(lib.png_encode_workspace(2, 17, 299, C, cap), dtype=torch.uint8, device="cuda")
    lib.png_encode(dict(inp=_lib.ptr(dev), ldi=pics[0].size, row_stride=299 * C, front=None, nfront=0, ldf=0,
                        out=_lib.ptr(rows), ldo=ldo, work=_lib.ptr(work), B=2, H=17, W=299, C=C, cap=cap),
                   _lib.stream_ptr())
    got = rows.cpu().numpy().view(np.uint32)
    want = np.full((3, ldo), 0x5A5A5A5A, np.uint32)
    want[:2, :ldo - 2] = E.rows_of(E.png_rule(pics, cap), cap)
    assert E.png_rule(pics, cap)[0] == b"" and (want[0, :ldo - 2] == 0).all()
    assert np.array_equal(got, want)
    assert E.encode_gpu(dev, cap + 1)[0] == full


def test_refusals():
    from kdl.ops import _lib
    lib = _lib.lib()
    dev = torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device="cuda")
    rows = torch.zeros((1, 64), dtype=torch.int32, device="cuda")
    work = torch.zeros(lib.png_encode_workspace(1, 4, 4, 4, 128), dtype=torch.uint8, device="cuda")
    good = dict(inp=_lib.ptr(dev), ldi=64, row_stride=16, front=None, nfront=0, ldf=0, out=_lib.ptr(rows), ldo=64,
                work=_lib.ptr(work), B=1, H=4, W=4, C=4, cap=128)
    for bad in (dict(C=2), dict(H=lib.PNG_ENC_MAX_SIDE + 1), dict(cap=lib.PNG_ENC_MAX_CAP + 1), dict(ldo=32),
                dict(row_stride=15), dict(work=None), dict(nfront=1)):
        with pytest.raises(RuntimeError):
            lib.png_encode(dict(good, **bad), _lib.stream_ptr())
    assert lib.png_encode_workspace(1, 4, 4, 2, 128) == 0


# ------------------------------------------------------------------------------------ engines
def _images(S, seed, n):
    """Noise (its file overflows the default cap) beside flat blocks (theirs fits)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8)
    blocks = torch.randint(0, 256, (n, 4, 4, 3), generator=g, dtype=torch.uint8)
    x[1::2] = blocks.repeat_interleave((S + 3) // 4, 1).repeat_interleave((S + 3) // 4, 2)[1::2, :S, :S]
    return x


@pytest.mark.parametrize("family,nb", (("xception", 3), ("vit_b16", 2)))
def test_engine_rows(family, nb, xparams):
    """The captured program with the cutout_png step, three forwards on one workspace, against the cutout engine."""
    from kdl.engine import registry
    from kdl.engine.base import Cutout, CutoutPng, cutout_png_cap, unpack_cutout, unpack_cutout_png
    info = registry.get(family)
    p = xparams if family == "xception" else info.init_params(0)
    mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
    S, (h, w) = info.input_size, info.map_size
    cap = cutout_png_cap(S)
    batches = [_images(S, 5 + i, nb) for i in range(2)]
    eng = info.engine(p, nb, "cuda", cutout=Cutout(), **mode)
    wide = [eng.forward(x.cuda()).cpu().numpy() for x in batches]
    names = [s.name for s in eng.steps]
    del eng
    eng = info.engine(p, nb, "cuda", cutout=Cutout(), cutout_png=CutoutPng(), **mode)
    assert [s.name for s in eng.steps] == names + ["cutout_png"]
    rows = [eng.forward(batches[0].cuda(), capture=True).cpu().numpy(), eng.forward(batches[1].cuda()).cpu().numpy(),
            eng.forward(batches[0].cuda()).cpu().numpy()]
    eager = eng.forward(batches[0].cuda(), capture=False).cpu().numpy()
    assert np.array_equal(eng.cutout_raw().cpu().numpy().view(np.int32), wide[0].view(np.int32))
    assert np.array_equal(rows[0].view(np.int32), rows[2].view(np.int32))
    assert np.array_equal(rows[0].view(np.int32), eager.view(np.int32))
    for got, raw in zip(rows[:2], wide):
        assert got.shape == (nb, 2 + h * w + 2 + (cap + 3) // 4)
        assert np.array_equal(got[:, :2 + h * w + 1].view(np.int32), raw[:, :2 + h * w + 1].view(np.int32))   # front and count
        pics = unpack_cutout(raw, h, w, S)[4]
        files = unpack_cutout_png(got, h, w, cap)[4]
        assert files == E.png_rule(pics, cap) and files[0] == b"" and files[1]
        assert np.array_equal(got.view(np.uint32)[:, 2 + h * w + 1:], E.rows_of(files, cap))
        for f, pic in zip(files, pics):
            assert not f or np.array_equal(np.asarray(Image.open(io.BytesIO(f))), pic)


def test_cutout_png_needs_a_cutout(xparams):
    from kdl.engine.base import CutoutPng
    from kdl.engine.xception import XceptionEngine
    with pytest.raises(ValueError, match="needs cutout"):
        XceptionEngine(xparams, 1, "cuda", explain=True, cutout_png=CutoutPng())
