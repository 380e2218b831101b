"""serving_bytes on the MI355X: the two HIP kernels (jpeg_idct_u8, jpeg_sample_rgb_u8) equal the
CPU pixel path and Pillow bit for bit, alone, batched and with the PIL-NEAREST resize folded in;
a GPU server answers serving_bytes with exactly the logits of serving_image."""
import io

import grpc
import numpy as np
import pytest
import torch

from _jpeg_cases import decode_cpu, encode, pants, pil_rgb, smooth_noise
from kdl.gateway import preprocess as pp
from kdl.gateway.client import PredictionStub, make_request
from kdl.gateway.preprocess import nearest_indices
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def gpu_decode(files, rows, n_rows, OH, OW):
    """One decode call: ``files[k]`` into row ``rows[k]`` of a [n_rows, OH, OW, 3] output that starts
    as SENTINEL bytes; PIL-NEAREST tables from each image's size to OH x OW."""
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
    tabs = []
    for k, d in enumerate(files):
        st, hd = rt.jpeg_parse(d, lay.coef(hin, k, heads[k].ncoef))
        assert st == rt.JPEG_OK, hd.why
        ys = torch.from_numpy(nearest_indices(hd.H, OH)).cuda()
        xs = torch.from_numpy(nearest_indices(hd.W, OW)).cuda()
        tabs += [ys, xs]
        lay.add(hin, k, hd, rows[k], ys, xs)
    d_in = torch.from_numpy(hin).cuda()
    planes = torch.empty(lay.ncoef, dtype=torch.uint8, device="cuda")
    out = torch.full((n_rows, OH, OW, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    args = lay.args(hin.ctypes.data, d_in.data_ptr(), planes.data_ptr(), lay.ncoef, out.data_ptr(), n_rows, OH, OW)
    s = torch.cuda.current_stream().cuda_stream
    C.jpeg_idct_u8(args, s)
    C.jpeg_sample_rgb_u8(args, s)
    torch.cuda.synchronize()
    return out.cpu().numpy(), args


CASES = {
    "1x1": (1, 1, dict(subsampling=2, quality=75)),
    "3x9 4:2:0": (3, 9, dict(subsampling=2, quality=95)),            # chroma 2 samples wide: replicated
    "4x9 4:2:2": (4, 9, dict(subsampling=1, quality=95)),
    "5x9 4:2:0": (5, 9, dict(subsampling=2, quality=95)),            # 3 samples wide: the triangle filter
    "17x9 4:2:0": (17, 9, dict(subsampling=2, quality=75)),          # odd dw / dh, partial MCUs on both axes
    "33x47 4:2:2": (33, 47, dict(subsampling=1, quality=90)),
    "64x64 4:4:4": (64, 64, dict(subsampling=0, quality=30)),
    "64x64 grey": (64, 64, dict(quality=100)),
}


def _file(w, h, kw):
    return encode(smooth_noise(w, h, 7 * w + h, "RGB" if "subsampling" in kw else "L"), **kw)


@pytest.mark.parametrize("case", list(CASES))
def test_kernels_equal_cpu_path_and_pillow(case):
    from kdl.ops import _lib
    w, h, kw = CASES[case]
    data = _file(w, h, kw)
    got, _ = gpu_decode([data], [0], 1, h, w)          # identity tables: OH = H, OW = W
    st, _, cpu = decode_cpu(_lib.rt(), data)
    assert st == 0
    assert np.array_equal(got[0], cpu)
    assert np.array_equal(got[0], pil_rgb(data))


def test_batch_of_different_images_and_untouched_row():
    """Three images of different sizes and samplings in one call, each resized to 40 x 56 into rows
    2, 0, 1; row 3 is nobody's and keeps its sentinel bytes."""
    from PIL import Image
    files = [_file(*CASES[c]) for c in ("17x9 4:2:0", "64x64 grey")]
    files.append(encode(smooth_noise(150, 130, 9), subsampling=2, quality=80, restart_marker_blocks=3))
    OH, OW = 56, 40
    got, _ = gpu_decode(files, [2, 0, 1], 4, OH, OW)
    for k, row in enumerate([2, 0, 1]):
        want = np.asarray(Image.open(io.BytesIO(files[k])).convert("RGB").resize((OW, OH), Image.NEAREST))
        assert np.array_equal(got[row], want), k
    assert (got[3] == SENTINEL).all()


def test_resize_534x400_to_299_equals_to_uint8():
    data = encode(pants(534, 400), quality=90, subsampling=2)
    got, _ = gpu_decode([data], [0], 1, 299, 299)
    assert np.array_equal(got[0], pp.to_uint8(pp.load_image(data), (299, 299)))


def test_launchers_reject_descriptors_outside_the_buffers():
    """The launch functions check every descriptor against the call's capacities before anything
    reaches the device: a call whose buffers are declared smaller than its planes is refused."""
    from kdl.ops import _lib
    data = _file(*CASES["33x47 4:2:2"])
    _, args = gpu_decode([data], [0], 1, 47, 33)
    s = torch.cuda.current_stream().cuda_stream
    for bad in (dict(coef_cap=args["coef_cap"] - 64), dict(plane_cap=64), dict(out_rows=0), dict(n_wg=args["n_wg"] + 1),
                dict(qt_cap=63)):
        for fn in (_lib.lib().jpeg_idct_u8, _lib.lib().jpeg_sample_rgb_u8):
            with pytest.raises(RuntimeError):
                fn({**args, **bad}, s)


# ------------------------------------------------------------------------------ the GPU server
@pytest.fixture(scope="module")
def gpu_server(tmp_path_factory):
    base = tmp_path_factory.mktemp("m") / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text('{"seed": 0}')
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1,
                       host="127.0.0.1", file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=8, batch_timeout_micros=1000,
                                               allowed_batch_sizes=[1, 2, 4, 8]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    yield srv
    srv.stop(0)


def test_gpu_serving_bytes_equals_serving_image(gpu_server):
    """Same images, same n: serving_bytes (decoded on the GPU) and serving_image (PIL-decoded pixels,
    resized on the GPU) give bit-equal logits; a progressive file in the request takes the PIL
    fallback into the same batch."""
    stub = PredictionStub(grpc.insecure_channel(f"127.0.0.1:{gpu_server.grpc_port}"))
    a, b = pants(534, 400), smooth_noise(534, 400, 11)
    for files in ([encode(a, quality=90, subsampling=2), encode(b, quality=75, subsampling=0)],
                  [encode(b, quality=85, subsampling=1), encode(a, quality=90, progressive=True)],
                  [encode(smooth_noise(299, 299, 12), quality=90)]):
        n = len(files)
        px = np.stack([np.asarray(pp.load_image(d), np.uint8) for d in files])
        r1 = stub.Predict(make_request(files, signature="serving_bytes", input_key="image_bytes"), timeout=60)
        r2 = stub.Predict(make_request(px, signature="serving_image", input_key="images"), timeout=60)
        got = np.asarray(r1.outputs["dense_7"].float_val, np.float32)
        assert got.size == 10 * n and np.array_equal(got, np.asarray(r2.outputs["dense_7"].float_val, np.float32))
    s = gpu_server.manager.get("clothing-model", None, None)
    r = s.runner("serving_bytes")
    assert r.gpu and r.device_path, "the decoded images round-tripped through the host"
    rows = r.decode(files)                      # the tensor handed to the engine, bit for bit
    assert np.array_equal(rows[0], pp.to_uint8(pp.load_image(files[0]), (299, 299)))
    assert s.device_alive()
