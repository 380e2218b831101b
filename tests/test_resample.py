"""Filtered resize + center crop without a GPU: the spec grammar and crop geometry, the coefficient
tables of kdl._rt.resample_coeffs against the installed Pillow (bit equality on random noise), the
CPU server's serving_image / serving_bytes under a "preprocess" spec, and the gateway's
GATEWAY_PREPROCESS. apply_spec_pil -- Pillow itself -- is the definition of correct throughout."""
import grpc
import numpy as np
import pytest
from PIL import Image

from _jpeg_cases import encode, smooth_noise
from _resample_ref import (CROP_SHAPES, FILTERS, SQUASH_SHAPES, noise, pil_resize, resize_ref, spec_ref)
from kdl.gateway import app as gw_app
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request
from kdl.gateway.preprocess import ResizeSpec, apply_spec_pil
from kdl.ops import _lib
from kdl.serving.config import BatchingParams, ServerConfig, config_from_args
from kdl.serving.server import ModelServer

rt = _lib.rt()


# ------------------------------------------------------------------------------ the spec
def test_spec_parsing():
    assert ResizeSpec.parse("") == ResizeSpec.parse(None) == ResizeSpec.parse("nearest") == ResizeSpec("nearest", None)
    assert ResizeSpec.parse("nearest") == pp.NEAREST_SPEC and pp.NEAREST_SPEC.squash
    for f in ("nearest",) + FILTERS:
        assert ResizeSpec.parse(f) == ResizeSpec(f, None)
        assert ResizeSpec.parse(f"{f}:256", 224) == ResizeSpec(f, 256)
        assert str(ResizeSpec.parse(f"{f}:256")) == f"{f}:256" and str(ResizeSpec.parse(f)) == f
    assert ResizeSpec.parse("bicubic:600", 600).resize_to == 600           # R == S is allowed
    assert not ResizeSpec.parse("bilinear:256").squash
    for bad in ("cubic", "bilinear:", ":256", "bilinear:abc", "bilinear:-3", "bilinear:25.6", "bilinear:256:224",
                "bilinear 256", "BILINEAR", "bilinear:0"):
        with pytest.raises(ValueError):
            ResizeSpec.parse(bad)
    with pytest.raises(ValueError, match="smaller"):
        ResizeSpec.parse("bilinear:223", 224)                              # R < S
    with pytest.raises(ValueError):
        ResizeSpec("bilinear", 200).geometry(400, 534, 224)
    with pytest.raises(Exception):
        ResizeSpec.parse("bilinear").filter = "box"                        # frozen


def test_crop_geometry_by_hand():
    # 400 x 534 (H x W), R 256, S 224: H is the shorter side -> 256 x int(256 * 534 / 400) = 256 x 341;
    # top = round(32 / 2) = 16, left = round(117 / 2 = 58.5) = 58 (Python rounds half to even)
    assert ResizeSpec("bilinear", 256).geometry(400, 534, 224) == (256, 341, 16, 58)
    # 300 x 7: W shorter -> 16 wide, int(16 * 300 / 7) = 685 high; top = round(669 / 2 = 334.5) = 334
    assert ResizeSpec("bicubic", 16).geometry(300, 7, 16) == (685, 16, 334, 0)
    assert ResizeSpec("bicubic", 16).geometry(7, 300, 16) == (16, 685, 0, 334)
    # squash: the window is the whole S x S image
    assert ResizeSpec("lanczos").geometry(400, 534, 299) == (299, 299, 0, 0)
    # square input, R > S: top = left = round(3 / 2 = 1.5) = 2
    assert ResizeSpec("nearest", 35).geometry(50, 50, 32) == (35, 35, 2, 2)


def test_nearest_is_todays_behaviour():
    a = noise(77, 120)
    assert np.array_equal(apply_spec_pil(Image.fromarray(a), pp.NEAREST_SPEC, 40), pp.to_uint8(Image.fromarray(a), (40, 40)))
    # nearest with a crop: the existing index tables sliced by the window
    spec = ResizeSpec("nearest", 48)
    nh, nw, top, left = spec.geometry(77, 120, 40)
    ys, xs = pp.nearest_indices(77, nh)[top:top + 40], pp.nearest_indices(120, nw)[left:left + 40]
    assert np.array_equal(a[ys][:, xs], apply_spec_pil(Image.fromarray(a), spec, 40))


# ------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("flt", FILTERS)
def test_tables_equal_pillow(flt):
    for H, W, oh, ow in SQUASH_SHAPES:
        a = noise(H, W)
        assert np.array_equal(resize_ref(rt, a, oh, ow, flt), pil_resize(a, oh, ow, flt)), (H, W, oh, ow)


def test_table_shapes():
    b, k = rt.resample_coeffs(53, 224, 1)                  # upscale, bilinear: support 1 -> ksize 3
    assert b.shape == (224, 2) and k.shape == (224, 3) and b.dtype == k.dtype == np.int32
    b, k = rt.resample_coeffs(500, 64, 4)                  # lanczos, scale 7.8: ceil(23.4) * 2 + 1
    assert k.shape == (64, 49)
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 500).all() and (b[:, 1] <= 49).all()
    assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()
    b, k = rt.resample_coeffs(64, 64, 3)                   # an identity pass: coefficients exactly 1 and 0
    assert all(k[i, :b[i, 1]].sum() == 1 << 22 and (k[i] != 0).sum() == 1 for i in range(64))
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 5), (4, 4, -1)):
        with pytest.raises(ValueError):
            rt.resample_coeffs(*bad)


@pytest.mark.parametrize("flt", FILTERS)
def test_crop_equals_apply_spec_pil(flt):
    for H, W, R, S in CROP_SHAPES:
        a, spec = noise(H, W, 1), ResizeSpec(flt, R)
        assert np.array_equal(spec_ref(rt, a, spec, S), apply_spec_pil(Image.fromarray(a), spec, S)), (H, W, R, S)


# ------------------------------------------------------------------------------ the CPU server
def _server(tmp_path_factory, meta: str, **kw):
    base = tmp_path_factory.mktemp("m") / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text(meta)
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="cpu", host="127.0.0.1",
                       file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=4, batch_timeout_micros=1000, allowed_batch_sizes=[1, 2, 4]),
                       **kw)
    return ModelServer(cfg).start(block_until_loaded=True)


@pytest.fixture(scope="module")
def bilinear_server(tmp_path_factory):
    srv = _server(tmp_path_factory, '{"seed": 0, "preprocess": "bilinear"}')
    yield srv
    srv.stop(0)


@pytest.fixture(scope="module")
def plain_server(tmp_path_factory):
    srv = _server(tmp_path_factory, '{"seed": 0}')
    yield srv
    srv.stop(0)


def _logits(resp, n):
    return np.asarray(resp.outputs["dense_7"].float_val, np.float32).reshape(n, 10)


def _predict(srv, x, signature, key="images"):
    stub = PredictionStub(grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}"))
    return _logits(stub.Predict(make_request(x, signature=signature, input_key=key), timeout=120), len(x))


@pytest.fixture(scope="module")
def files():
    """A baseline and a progressive JPEG (the PIL fallback) of one size."""
    return [encode(smooth_noise(200, 150, 3), quality=90, subsampling=2),
            encode(smooth_noise(200, 150, 4), quality=85, subsampling=0, progressive=True)]


def test_cpu_server_applies_the_spec(bilinear_server, files):
    spec = bilinear_server.manager.get("clothing-model", None, None).source.preprocess
    assert spec == ResizeSpec("bilinear", None)
    imgs = [pp.load_image(d) for d in files]
    want = _predict(bilinear_server, np.stack([apply_spec_pil(im, spec, 299) for im in imgs]), "serving_uint8")
    px = np.stack([np.asarray(im, np.uint8) for im in imgs])
    assert np.array_equal(_predict(bilinear_server, px, "serving_image"), want)
    assert np.array_equal(_predict(bilinear_server, files, "serving_bytes", "image_bytes"), want)
    # bilinear is not nearest: the spec reached the pixels
    nearest = _predict(bilinear_server, np.stack([pp.to_uint8(im) for im in imgs]), "serving_uint8")
    assert not np.array_equal(want, nearest)
    from kdl.serving.metrics import METRICS
    assert METRICS.snapshot()["counters"].get("kdl_resize_total{filter=bilinear}", 0) >= 2


def test_server_without_the_key_is_nearest(plain_server, files):
    assert plain_server.manager.get("clothing-model", None, None).source.preprocess == pp.NEAREST_SPEC
    imgs = [pp.load_image(d) for d in files]
    want = _predict(plain_server, np.stack([pp.to_uint8(im) for im in imgs]), "serving_uint8")
    px = np.stack([np.asarray(im, np.uint8) for im in imgs])
    assert np.array_equal(_predict(plain_server, px, "serving_image"), want)
    assert np.array_equal(_predict(plain_server, files, "serving_bytes", "image_bytes"), want)


def test_flag_overrides_and_bad_specs(tmp_path):
    from kdl.serving.backend import load_version_dir
    (tmp_path / "synthetic.json").write_text('{"seed": 0, "preprocess": "bilinear:320"}')
    assert load_version_dir(tmp_path).preprocess == ResizeSpec("bilinear", 320)
    assert load_version_dir(tmp_path, preprocess="lanczos").preprocess == ResizeSpec("lanczos", None)
    with pytest.raises(ValueError):
        load_version_dir(tmp_path, preprocess="bilinear:298")              # R < S = 299
    assert config_from_args(["--preprocess", "bicubic:320"], env={}).preprocess == "bicubic:320"
    assert config_from_args([], env={}).preprocess == "" == ServerConfig().preprocess


# ------------------------------------------------------------------------------ the gateway
def test_gateway_preprocess(plain_server, files, monkeypatch):
    """GATEWAY_PREPROCESS=bicubic:320 in uint8 mode sends apply_spec_pil pixels."""
    spec, sent = ResizeSpec("bicubic", 320), []
    real = gw_app.make_request
    monkeypatch.setattr(gw_app, "make_request", lambda X, *a, **k: (sent.append(np.array(X)), real(X, *a, **k))[1])
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: files[0])
    env = {"TF_SERVING_HOST": f"127.0.0.1:{plain_server.grpc_port}", "GATEWAY_MODE": "uint8",
           "GATEWAY_PREPROCESS": "bicubic:320"}
    r = create_app(GatewayConfig(env)).test_client().post("/predict", json={"url": "http://example.invalid/a.jpg"})
    assert r.status_code == 200, r.data
    want = apply_spec_pil(pp.load_image(files[0]), spec, 299)
    assert len(sent) == 1 and sent[0].dtype == np.uint8 and np.array_equal(sent[0], want[None])
    assert GatewayConfig({}).preprocess == pp.NEAREST_SPEC
    with pytest.raises(ValueError):
        GatewayConfig({"GATEWAY_PREPROCESS": "bicubic:100"})               # R < 299
    # compat mode: the same pixels, normalised
    sent.clear()
    env["GATEWAY_MODE"] = "compat"
    r = create_app(GatewayConfig(env)).test_client().post("/predict", json={"url": "http://example.invalid/a.jpg"})
    assert r.status_code == 200, r.data
    assert np.array_equal(sent[0], pp.xception_preprocess(want[None]))
