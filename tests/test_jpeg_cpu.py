"""serving_bytes without a GPU: the host JPEG decoder (kdl._rt.jpeg_parse + jpeg_pixels_cpu) is
bit-identical to Pillow, tells "unsupported" from "malformed", and the signature works end to end
through an in-process CPU server (gRPC string_val, REST b64, the gateway's bytes mode)."""
import base64
import json
import socket
import urllib.error
import urllib.request

import grpc
import numpy as np
import pytest
from PIL import Image

from _jpeg_cases import decode_cpu, encode, pants, pil_rgb, smooth_noise, with_segments
from kdl import _rt as rt
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request
from kdl.ingest.keras_map import to_keras_variables
from kdl.ingest.savedmodel import write_savedmodel
from kdl.models import xception as X
from kdl.serving import protos as P
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

SIZES = [(1, 1), (17, 9), (33, 47), (50, 31), (64, 64), (534, 400)]


def _source(w, h, mode="RGB"):
    return pants(w, h).convert(mode) if (w, h) == (534, 400) else smooth_noise(w, h, 3 * w + h, mode)


def _variants(w, h):
    """(label, file) for every subsampling / grey, quality and encoder option of one size."""
    for sub in (0, 1, 2, "L"):
        im = _source(w, h, "L" if sub == "L" else "RGB")
        kw = {} if sub == "L" else {"subsampling": sub}
        for q in (30, 75, 100):
            yield f"sub{sub} q{q}", encode(im, quality=q, **kw)
        yield f"sub{sub} optimize", encode(im, quality=75, optimize=True, **kw)
        yield f"sub{sub} restart_blocks", encode(im, quality=75, restart_marker_blocks=2, **kw)
        yield f"sub{sub} restart_rows", encode(im, quality=75, restart_marker_rows=1, **kw)
        yield f"sub{sub} COM+APP1", with_segments(encode(im, quality=75, **kw))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_equals_pillow(size):
    w, h = size
    for label, data in _variants(w, h):
        st, hd, got = decode_cpu(rt, data)
        assert st == rt.JPEG_OK, (label, hd.why)
        assert (hd.W, hd.H) == (w, h), label
        ref = pil_rgb(data)
        assert got.shape == ref.shape and np.array_equal(got, ref), \
            (label, int(np.abs(got.astype(int) - ref).max()))


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
def test_narrow_images_equal_pillow(w):
    """libjpeg upsamples chroma planes of at most 2 samples (images up to 4 pixels wide) by plain
    replication, vertically too, and switches to the triangle filter from 3 samples (width 5) on."""
    for h in (1, 3, 9, 20):
        for sub in (1, 2):
            im = smooth_noise(w, h, 11 * w + h)
            px = np.asarray(im).copy()
            px[..., 0] = np.random.default_rng(w + h).integers(0, 256, (h, w))   # strong chroma steps
            data = encode(Image.fromarray(px), quality=95, subsampling=sub)
            st, hd, got = decode_cpu(rt, data)
            assert st == rt.JPEG_OK, hd.why
            assert np.array_equal(got, pil_rgb(data)), (w, h, sub)


def test_header_fields():
    data = encode(smooth_noise(50, 31, 1), quality=75, subsampling=2)
    st, hd = rt.jpeg_probe(data)
    assert st == rt.JPEG_OK and (hd.W, hd.H, hd.ncomp, hd.hmax, hd.vmax) == (50, 31, 3, 2, 2)
    # (id, h, v, tq, bw, bh, dw, dh, coef_off): whole MCUs of 16x16; planes back to back, no interleave
    assert hd.comps == [(1, 2, 2, 0, 8, 4, 50, 31, 0), (2, 1, 1, 1, 4, 2, 25, 16, 2048),
                        (3, 1, 1, 1, 4, 2, 25, 16, 2560)]
    assert hd.ncoef == 3072
    st, hd = rt.jpeg_parse(data, np.zeros(hd.ncoef, np.int16))
    assert st == rt.JPEG_OK and hd.qt.shape == (4, 64) and hd.qt[0].min() >= 1 and not hd.qt[2:].any()
    st, hd = rt.jpeg_parse(data, np.zeros(hd.ncoef - 1, np.int16))       # the caller's buffer is checked
    assert st == rt.JPEG_MALFORMED


def test_statuses():
    im = smooth_noise(64, 48, 2)
    base = encode(im, quality=80)
    for label, data in [("progressive", encode(im, quality=80, progressive=True)),
                        ("cmyk", encode(im.convert("CMYK"), quality=80)),
                        ("png", encode(im, "PNG")), ("empty", b"")]:
        st, hd, _ = decode_cpu(rt, data)
        assert st == rt.JPEG_UNSUPPORTED and hd.why, label
    cut = base[:int(len(base) * 0.6)]
    at = base.index(b"\xff\xc4")
    dht = base[:at + 2] + b"\xff\xff" + base[at + 4:]                    # a DHT length past the end
    nodim = bytearray(base)
    sof = base.index(b"\xff\xc0")
    nodim[sof + 5:sof + 7] = b"\0\0"                                     # zero height
    for label, data in [("truncated", cut), ("dht length", dht), ("zero dimension", bytes(nodim))]:
        st, hd, _ = decode_cpu(rt, data)
        assert st == rt.JPEG_MALFORMED and hd.why, label
    st, hd = rt.jpeg_probe(base, 64 * 48 - 1)                            # the pixel limit comes first
    assert st == rt.JPEG_MALFORMED and "pixel limit" in hd.why


# ------------------------------------------------------------------------------ the CPU server
@pytest.fixture(scope="module")
def server(tmp_path_factory):
    repo = tmp_path_factory.mktemp("models") / "clothing-model"
    write_savedmodel(repo / "1", to_keras_variables(X.init_params(seed=5), residual_offset=2))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        rest_port = so.getsockname()[1]
    cfg = ServerConfig(port=0, rest_api_port=rest_port, model_name="clothing-model", model_base_path=str(repo),
                       device="cpu", host="127.0.0.1", file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=4, batch_timeout_micros=2000,
                                               allowed_batch_sizes=[1, 2, 4]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    yield srv
    srv.stop(0)


@pytest.fixture(scope="module")
def stub(server):
    ch = grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}")
    yield PredictionStub(ch)
    ch.close()


@pytest.fixture(scope="module")
def files():
    """Three sizes and subsamplings, the middle one progressive (the PIL fallback)."""
    return [encode(pants(534, 400), quality=90, subsampling=2),
            encode(smooth_noise(120, 77, 4), quality=85, subsampling=0, progressive=True),
            encode(smooth_noise(301, 64, 5), quality=70, subsampling=1)]


def _logits(resp, n):
    return np.asarray(resp.outputs["dense_7"].float_val, np.float32).reshape(n, 10)


def _bytes_request(images):
    return make_request(list(images), signature="serving_bytes", input_key="image_bytes")


@pytest.fixture(scope="module")
def three(stub, files):
    return _logits(stub.Predict(_bytes_request(files), timeout=60), 3)


def test_grpc_string_val_equals_the_pil_path(stub, files, three):
    # the rows handed to the engine are to_uint8(load_image(data)): same request shape, same logits
    rows = np.stack([pp.to_uint8(pp.load_image(d), (299, 299)) for d in files])
    ref = _logits(stub.Predict(make_request(rows, signature="serving_uint8", input_key="images"), timeout=60), 3)
    assert np.array_equal(three, ref)
    # request by request: each file alone equals serving_image of its PIL-decoded pixels
    for d in files:
        got = _logits(stub.Predict(_bytes_request([d]), timeout=60), 1)
        px = np.asarray(pp.load_image(d), np.uint8)[None]
        want = _logits(stub.Predict(make_request(px, signature="serving_image", input_key="images"), timeout=60), 1)
        assert np.array_equal(got, want)
    # a scalar DT_STRING tensor is one image
    one = stub.Predict(make_request(files[2], signature="serving_bytes", input_key="image_bytes"), timeout=60)
    assert np.array_equal(_logits(one, 1), got)


def test_rest_b64(server, files, three):
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model:predict"
    b64 = [{"b64": base64.b64encode(d).decode()} for d in files]
    for body, key in [({"signature_name": "serving_bytes", "instances": b64}, "predictions"),
                      ({"signature_name": "serving_bytes", "inputs": {"image_bytes": b64}}, "outputs")]:
        out = json.load(urllib.request.urlopen(urllib.request.Request(url, data=json.dumps(body).encode(),
                                                                      method="POST")))
        assert np.array_equal(np.asarray(out[key], np.float32), three)
    bad = {"signature_name": "serving_bytes", "instances": [{"b64": "***"}]}
    with pytest.raises(urllib.error.HTTPError) as e:
        urllib.request.urlopen(urllib.request.Request(url, data=json.dumps(bad).encode(), method="POST"))
    assert e.value.code == 400


def test_metadata_lists_the_signature(stub):
    req = P.GetModelMetadataRequest()
    req.model_spec.name = "clothing-model"
    req.metadata_field.append("signature_def")
    sdm = P.SignatureDefMap()
    stub.GetModelMetadata(req, timeout=5).metadata["signature_def"].Unpack(sdm)
    sd = sdm.signature_def["serving_bytes"]
    assert list(sd.inputs) == ["image_bytes"] and sd.inputs["image_bytes"].dtype == P.DT_STRING
    assert [d.size for d in sd.inputs["image_bytes"].tensor_shape.dim] == [-1]
    assert list(sd.outputs) == ["dense_7"]


def test_bad_requests(stub, files, monkeypatch):
    cut = files[0][:int(len(files[0]) * 0.6)]
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(_bytes_request([files[2], cut]), timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT and "image 1" in e.value.details()
    with pytest.raises(grpc.RpcError) as e:                              # neither a JPEG nor anything PIL reads
        stub.Predict(_bytes_request([b"not an image"]), timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT and "image 0" in e.value.details()
    # the existing dtype error texts
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(make_request(np.zeros((1, 299, 299, 3), np.uint8), signature="serving_bytes",
                                  input_key="image_bytes"), timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert e.value.details() == "Expects arg[0] to be DT_STRING but DT_UINT8 is provided"
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(make_request([files[2]], signature="serving_uint8", input_key="images"), timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert e.value.details() == "Expects arg[0] to be DT_UINT8 but DT_STRING is provided"
    # the pixel limit is on the sum over the request: 301*64 + 120*77 pixels
    import kdl.serving.jpeg as J
    monkeypatch.setattr(J, "MAX_PIXELS", 301 * 64 + 120 * 77 - 1)
    stub.Predict(_bytes_request([files[2]]), timeout=30)
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(_bytes_request([files[2], files[1]]), timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT and "pixel" in e.value.details()


def test_gateway_bytes_mode_equals_raw_mode(server, files, monkeypatch):
    """GATEWAY_MODE=bytes forwards the fetched body as it is (no PIL in the gateway) and returns
    the JSON of raw mode, which decodes with PIL there and ships the pixels."""
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: files[0])
    base = {"TF_SERVING_HOST": f"127.0.0.1:{server.grpc_port}"}
    raw = create_app(GatewayConfig({**base, "GATEWAY_MODE": "raw"})).test_client()
    byt = create_app(GatewayConfig({**base, "GATEWAY_MODE": "bytes"})).test_client()
    monkeypatch.setattr(pp, "load_image", lambda data: pytest.fail("the bytes gateway decoded an image"))
    b = byt.post("/predict", json={"url": "http://example.invalid/a.jpg"})
    bb = byt.post("/predict_batch", json={"urls": ["http://example.invalid/a.jpg"] * 2})
    monkeypatch.undo()
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: files[0])
    a = raw.post("/predict", json={"url": "http://example.invalid/a.jpg"})
    assert a.status_code == b.status_code == 200, (a.data, b.data)
    assert a.get_json() == b.get_json()
    assert bb.status_code == 200 and len(bb.get_json()) == 2
    assert all(abs(bb.get_json()[0][k] - v) < 1e-3 for k, v in b.get_json().items())


def test_device_alive_with_a_bytes_runner(server, stub, files, three):
    s = server.manager.get("clothing-model", None, None)
    assert "serving_bytes" in s.runners and not hasattr(s.runners["serving_bytes"], "batcher")
    assert s.device_alive() and server.manager.device_alive()


def test_counters(server, three):
    from kdl.serving.metrics import METRICS
    snap = METRICS.snapshot()
    assert snap["counters"].get("kdl_jpeg_decoded_total{path=cpu}", 0) >= 2
    assert snap["counters"].get("kdl_jpeg_decoded_total{path=pil}", 0) >= 1
    assert snap["histograms"]["kdl_stage_ms{stage=jpeg_entropy}"]["count"] >= 1
