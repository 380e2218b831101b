"""Filtered resize + center crop on the MI355X: the two HIP kernels (resample_h_u8, resample_v_u8)
equal the installed Pillow bit for bit from raw pixels and from JPEG sample planes, alone, batched
and cropped; the launchers refuse tables and descriptors outside the buffers; a GPU server with a
"preprocess" spec answers serving_bytes and serving_image with the logits of apply_spec_pil pixels."""
import grpc
import numpy as np
import pytest
import torch
from PIL import Image

from _jpeg_cases import encode, pants, smooth_noise
from _resample_ref import CROP_SHAPES, FILTERS, SQUASH_SHAPES, noise, pil_resize
from kdl.gateway import preprocess as pp
from kdl.gateway.client import PredictionStub, make_request
from kdl.gateway.preprocess import ResizeSpec, apply_spec_pil
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _tables(H, W, nh, nw, flt, window=None):
    from kdl.serving.resize import FilterTables
    return FilterTables(H, W, nh, nw, flt, torch.device("cuda"), window)


def _launch(tabs, descs, rows, n_rows, OH, OW, jpeg=None, n_jpeg=0, launch=True, **over):
    """resample_h_u8 (JPEG kind for the first ``n_jpeg`` descriptors, raw kind for the rest) and
    resample_v_u8 into a SENTINEL-filled [n_rows, OH, OW, 3] output; ``over`` overrides arguments."""
    from kdl.ops import _lib
    C, D = _lib.lib(), _lib.rt().RESAMPLE_DESC_BYTES
    n = len(descs)
    h_desc = np.concatenate(descs)
    d_desc = torch.from_numpy(h_desc).cuda()
    tmp_cap = sum(t.tmp_bytes for t in tabs)
    tmp = torch.empty(max(tmp_cap, 4), dtype=torch.uint8, device="cuda")
    out = torch.full((n_rows, OH, OW, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    args = dict(desc=d_desc.data_ptr(), h_desc=h_desc.ctypes.data, tmp=tmp.data_ptr(), tmp_cap=tmp_cap,
                out=out.data_ptr(), out_rows=n_rows, OH=OH, OW=OW, n=n, **(jpeg or {}))
    args.update(over)
    s = torch.cuda.current_stream().cuda_stream
    if launch:
        if n_jpeg:
            C.resample_h_u8({**args, "n": n_jpeg}, 1, s)
        if n > n_jpeg:
            C.resample_h_u8({**args, "desc": args["desc"] + n_jpeg * D, "h_desc": args["h_desc"] + n_jpeg * D,
                             "n": n - n_jpeg}, 0, s)
        C.resample_v_u8(args, s)
        torch.cuda.synchronize()
    return out.cpu().numpy(), args, (d_desc, tmp, out, h_desc)


def gpu_raw(arrs, tabs, rows, n_rows):
    """Raw kind: ``arrs[k]`` through ``tabs[k]`` into row ``rows[k]``."""
    srcs = [torch.from_numpy(a).cuda() for a in arrs]
    descs, off = [], 0
    for a, t, src, row in zip(arrs, tabs, srcs, rows):
        descs.append(t.desc(src.data_ptr(), off, row))
        off += t.tmp_bytes
    return _launch(tabs, descs, rows, n_rows, tabs[0].OH, tabs[0].OW)[0]


def gpu_jpeg(files, tabs_of, rows, n_rows, raw=()):
    """JPEG kind: jpeg_idct_u8, then the horizontal pass from the sample planes. ``tabs_of(H, W)``
    makes an image's tables; ``raw``: [H, W, 3] arrays that join the call as raw-kind images."""
    from kdl.ops import _lib
    from kdl.serving.jpeg import CallLayout
    rt, C = _lib.rt(), _lib.lib()
    heads = []
    for d in files:
        st, hd = rt.jpeg_probe(d)
        assert st == rt.JPEG_OK, hd.why
        heads.append(hd)
    lay = CallLayout([hd.ncoef for hd in heads])
    hin = np.zeros(lay.nbytes, np.uint8)
    tabs, descs, off = [], [], 0
    for k, d in enumerate(files):
        st, hd = rt.jpeg_parse(d, lay.coef(hin, k, heads[k].ncoef))
        assert st == rt.JPEG_OK, hd.why
        t = tabs_of(hd.H, hd.W)
        tabs.append(t)
        descs.append(t.desc(k, off, rows[k]))
        off += t.tmp_bytes
        lay.add(hin, k, hd, rows[k], t.dev[2], t.dev[0])
    srcs = [torch.from_numpy(a).cuda() for a in raw]
    for a, src, row in zip(raw, srcs, rows[len(files):]):
        t = tabs_of(a.shape[0], a.shape[1])
        tabs.append(t)
        descs.append(t.desc(src.data_ptr(), off, row))
        off += t.tmp_bytes
    d_in = torch.from_numpy(hin).cuda()
    planes = torch.empty(lay.ncoef, dtype=torch.uint8, device="cuda")
    OH, OW = tabs[0].OH, tabs[0].OW
    scratch = torch.empty((n_rows, OH, OW, 3), dtype=torch.uint8, device="cuda")    # jpeg_idct_u8 never writes it
    s = torch.cuda.current_stream().cuda_stream
    C.jpeg_idct_u8(lay.args(hin.ctypes.data, d_in.data_ptr(), planes.data_ptr(), lay.ncoef, scratch.data_ptr(),
                            n_rows, OH, OW), s)
    jpeg = dict(jdesc=d_in.data_ptr(), h_jdesc=hin.ctypes.data, n_jdesc=lay.n_desc, planes=planes.data_ptr(),
                plane_cap=lay.ncoef)
    return _launch(tabs, descs, rows, n_rows, OH, OW, jpeg=jpeg, n_jpeg=len(files))[0]


# ------------------------------------------------------------------------------ raw source
@pytest.mark.parametrize("flt", FILTERS)
def test_raw_squash_equals_pillow(flt):
    for H, W, oh, ow in SQUASH_SHAPES:
        a = noise(H, W)
        got = gpu_raw([a], [_tables(H, W, oh, ow, flt)], [0], 1)
        assert np.array_equal(got[0], pil_resize(a, oh, ow, flt)), (H, W, oh, ow)


@pytest.mark.parametrize("flt", FILTERS)
def test_raw_crop_equals_apply_spec_pil(flt):
    from kdl.serving.resize import FilterTables
    for H, W, R, S in CROP_SHAPES:
        a, spec = noise(H, W, 1), ResizeSpec(flt, R)
        got = gpu_raw([a], [FilterTables.for_spec(H, W, spec, S, torch.device("cuda"))], [0], 1)
        assert np.array_equal(got[0], apply_spec_pil(Image.fromarray(a), spec, S)), (H, W, R, S)


@pytest.mark.parametrize("flt", FILTERS)
def test_odd_size_into_the_middle_row(flt):
    """S = 35 into row 1 of 3: the row starts at 35 * 35 * 3 = 3675 bytes and the source rows at
    y * 53 * 3, neither a multiple of 4; rows 0 and 2 keep their sentinel bytes."""
    a = noise(37, 53, 2)
    got = gpu_raw([a], [_tables(37, 53, 35, 35, flt)], [1], 3)
    assert np.array_equal(got[1], pil_resize(a, 35, 35, flt))
    assert (got[0] == SENTINEL).all() and (got[2] == SENTINEL).all()


def test_unaligned_source_address():
    """The packed images of a request start at i * H * W * 3 bytes: every alignment of the source."""
    a = noise(41, 29, 3)
    want = pil_resize(a, 24, 24, "bicubic")
    buf = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")
    t = _tables(41, 29, 24, 24, "bicubic")
    for shift in (1, 2, 3):
        buf[shift:shift + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        got = _launch([t], [t.desc(buf.data_ptr() + shift, 0, 0)], [0], 1, 24, 24)[0]
        assert np.array_equal(got[0], want), shift


def test_lds_span_limit():
    """700 x 500 -> 64 with LANCZOS: ksize 49 across, 64 columns of it no longer fit the coefficient
    budget of a workgroup, so the launcher narrows the column groups."""
    a = noise(700, 500, 4)
    t = _tables(700, 500, 64, 64, "lanczos")
    assert t.xk.shape[1] == 49
    assert np.array_equal(gpu_raw([a], [t], [0], 1)[0], pil_resize(a, 64, 64, "lanczos"))
    # a 40x downscale. BOX: ksize 41, 64 columns fit the coefficient budget but span 2560 source
    # pixels, more than a staged row holds; LANCZOS: ksize 241, one column alone spans 240 pixels
    a = noise(8, 2600, 5)
    for flt in ("box", "lanczos"):
        assert np.array_equal(gpu_raw([a], [_tables(8, 2600, 8, 65, flt)], [0], 1)[0], pil_resize(a, 8, 65, flt)), flt


# ------------------------------------------------------------------------------ JPEG source
def _squash(flt, oh, ow):
    return lambda H, W: _tables(H, W, oh, ow, flt)


def _pil_spec(data, spec, S):
    return apply_spec_pil(pp.load_image(data), spec, S)


def test_jpeg_squash_equals_pillow():
    files = [encode(smooth_noise(33, 47, 1), subsampling=1, quality=90),
             encode(smooth_noise(17, 9, 2), subsampling=2, quality=75),
             encode(smooth_noise(64, 64, 3, "L"), quality=100)]
    for d in files:
        got = gpu_jpeg([d], _squash("bilinear", 56, 40), [0], 1)
        want = np.asarray(pp.load_image(d).resize((40, 56), Image.BILINEAR))
        assert np.array_equal(got[0], want)


def test_jpeg_restart_markers_and_crop():
    from kdl.serving.resize import FilterTables
    d = encode(smooth_noise(150, 130, 9), subsampling=2, quality=80, restart_marker_blocks=3)
    spec = ResizeSpec("bicubic", 48)
    got = gpu_jpeg([d], lambda H, W: FilterTables.for_spec(H, W, spec, 40, torch.device("cuda")), [0], 1)
    assert np.array_equal(got[0], _pil_spec(d, spec, 40))


def test_jpeg_534x400_to_299_bicubic():
    d = encode(pants(534, 400), quality=90, subsampling=2)
    got = gpu_jpeg([d], _squash("bicubic", 299, 299), [0], 1)
    assert np.array_equal(got[0], _pil_spec(d, ResizeSpec("bicubic"), 299))


def test_mixed_batch_and_untouched_row():
    """Three JPEGs of different sizes and samplings and one raw image in one call, into rows 2, 0, 1
    of five; row 3 is nobody's and keeps its sentinel bytes, the raw image goes to row 4."""
    files = [encode(smooth_noise(17, 9, 2), subsampling=2, quality=75),
             encode(smooth_noise(64, 64, 3, "L"), quality=100),
             encode(smooth_noise(150, 130, 9), subsampling=1, quality=80)]
    a = noise(23, 71, 6)
    got = gpu_jpeg(files, _squash("hamming", 56, 40), [2, 0, 1, 4], 5, raw=[a])
    for k, row in enumerate([2, 0, 1]):
        want = np.asarray(pp.load_image(files[k]).resize((40, 56), Image.HAMMING))
        assert np.array_equal(got[row], want), k
    assert np.array_equal(got[4], pil_resize(a, 56, 40, "hamming"))
    assert (got[3] == SENTINEL).all()


# ------------------------------------------------------------------------------ launcher refusals
def test_launchers_refuse_what_lies_outside_the_buffers():
    """The launch functions check the host copy of every bounds table and descriptor against the
    capacities of the call before anything reaches the device."""
    from kdl.ops import _lib
    C = _lib.lib()
    a = noise(37, 53, 7)
    src = torch.from_numpy(a).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def refused(t, **over):
        _, args, keep = _launch([t], [t.desc(src.data_ptr(), 0, 0)], [0], 1, t.OH, t.OW, launch=False)
        args.update(over)
        for fn in (lambda: C.resample_h_u8(args, 0, s), lambda: C.resample_v_u8(args, s)):
            with pytest.raises(RuntimeError):
                fn()
        del keep

    t = _tables(37, 53, 24, 24, "bilinear")
    _, args, keep = _launch([t], [t.desc(src.data_ptr(), 0, 0)], [0], 1, 24, 24)       # the good call runs
    refused(t, tmp_cap=t.tmp_bytes - 1)                     # a scratch capacity too small
    refused(t, out_rows=0)
    refused(t, n=0)
    refused(t, n=65536)
    refused(t, OW=0)
    t = _tables(37, 53, 24, 24, "bilinear")
    t.xb[-1, 0] += 1                                        # one pixel past the source row
    refused(t)
    t = _tables(37, 53, 24, 24, "bilinear")
    t.yb[-1, 1] += 1                                        # one row past the rows of the intermediate
    refused(t)
    t = _tables(37, 53, 24, 24, "bilinear")
    t.xb[0, 0] = -1
    refused(t)
    t = _tables(37, 53, 24, 24, "bilinear")
    t.xb[3, 1] = t.xk.shape[1] + 1                          # more taps than the table has
    refused(t)
    t = _tables(37, 53, 24, 24, "bilinear")
    t.rows = 38                                             # rows beyond the source
    refused(t)
    t = _tables(37, 53, 24, 24, "bilinear")
    with pytest.raises(RuntimeError):                       # a JPEG-kind call without descriptors
        C.resample_h_u8(_launch([t], [t.desc(0, 0, 0)], [0], 1, 24, 24, launch=False)[1], 1, s)
    with pytest.raises(RuntimeError):                       # an output row outside the batch
        C.resample_v_u8(_launch([t], [t.desc(src.data_ptr(), 0, 1)], [0], 1, 24, 24, launch=False)[1], s)
    torch.cuda.synchronize()
    del keep


def test_resizer_runs_the_spec_and_refuses_what_no_column_group_can_hold():
    from kdl.serving.backend import ServingError
    from kdl.serving.resize import Resizer
    dev = torch.cuda.current_device()
    x = np.stack([noise(97, 131, 9), noise(97, 131, 10)])
    for text in ("hamming", "bicubic:40", "nearest:40"):
        spec = ResizeSpec.parse(text)
        got = Resizer(35, dev, contexts=1, spec=spec)(x)
        assert np.array_equal(got, np.stack([apply_spec_pil(Image.fromarray(a), spec, 35) for a in x])), text
    # 30000 pixels across to 32 with LANCZOS: 5625 taps per output pixel, beyond a workgroup's LDS
    with pytest.raises(ServingError, match="too wide"):
        Resizer(32, dev, contexts=1, spec="lanczos")(np.zeros((1, 2, 30000, 3), np.uint8))


# ------------------------------------------------------------------------------ the GPU server
@pytest.fixture(scope="module")
def gpu_server(tmp_path_factory):
    base = tmp_path_factory.mktemp("m") / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text('{"seed": 0, "preprocess": "bilinear:320"}')
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1,
                       host="127.0.0.1", file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=8, batch_timeout_micros=1000,
                                               allowed_batch_sizes=[1, 2, 4, 8]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    yield srv
    srv.stop(0)


def _logits(resp, n):
    got = np.asarray(resp.outputs["dense_7"].float_val, np.float32)
    assert got.size == 10 * n
    return got


def test_gpu_server_applies_the_spec(gpu_server):
    """serving_bytes (decoded and resampled on the GPU), serving_image (PIL-decoded pixels, resampled
    on the GPU) and serving_uint8 fed apply_spec_pil pixels give bit-equal logits; a progressive file
    takes the PIL fallback into the same batch; a 299 x 299 input is still resized to 320 and cropped."""
    stub = PredictionStub(grpc.insecure_channel(f"127.0.0.1:{gpu_server.grpc_port}"))
    spec = ResizeSpec("bilinear", 320)
    s = gpu_server.manager.get("clothing-model", None, None)
    assert s.source.preprocess == spec
    a, b = pants(534, 400), smooth_noise(534, 400, 11)
    files = [encode(a, quality=90, subsampling=2), encode(b, quality=75, subsampling=0),
             encode(a, quality=85, subsampling=1, progressive=True)]
    want_px = np.stack([_pil_spec(d, spec, 299) for d in files])
    px = np.stack([np.asarray(pp.load_image(d), np.uint8) for d in files])
    r0 = _logits(stub.Predict(make_request(want_px, signature="serving_uint8", input_key="images"), timeout=60), 3)
    r1 = _logits(stub.Predict(make_request(files, signature="serving_bytes", input_key="image_bytes"), timeout=60), 3)
    r2 = _logits(stub.Predict(make_request(px, signature="serving_image", input_key="images"), timeout=60), 3)
    assert np.array_equal(r1, r0) and np.array_equal(r2, r0)
    r = s.runner("serving_bytes")
    assert r.gpu and r.device_path and s.runner("serving_image").device_path, \
        "the resampled images round-tripped through the host"
    assert np.array_equal(r.decode(files), want_px)            # the tensor handed to the engine, bit for bit
    # an image already at the model size: R = 320 != S, so it is resized and cropped all the same
    sq = noise(299, 299, 8)
    want = apply_spec_pil(Image.fromarray(sq), spec, 299)
    assert not np.array_equal(want, sq)
    assert np.array_equal(s.runner("serving_image").resizer(sq[None])[0], want)
    r3 = _logits(stub.Predict(make_request(sq[None], signature="serving_image", input_key="images"), timeout=60), 1)
    r4 = _logits(stub.Predict(make_request(want[None], signature="serving_uint8", input_key="images"), timeout=60), 1)
    assert np.array_equal(r3, r4)
    assert s.device_alive()
