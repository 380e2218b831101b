"""The overlay_jpeg signatures without a GPU: ``encode_rule`` against Pillow as whole files, the files through
Pillow's and the project's own decoder, row packing, config errors, a version without the block, a
``--device cpu`` server (gRPC and REST), a ``--device null`` server and the gateway's three formats."""
import base64
import io
import json
import socket
import urllib.error
import urllib.request
from pathlib import Path

import grpc
import numpy as np
import pytest
from PIL import Image

from _jpeg_cases import decode_cpu
from kdl.engine.base import Overlay, OverlayJpeg, overlay_jpeg_cap, pack_overlay_jpeg, unpack_overlay_jpeg
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request
from kdl.ops import _lib
from kdl.serving import jpeg_encode as J
from kdl.serving import overlay as O
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

PANTS = Path(__file__).parent / "data" / "pants.png"
SIGS = ("overlay_jpeg", "overlay_jpeg_image", "overlay_jpeg_bytes")
KEYS = ("classes", "scores", "heatmap", "jpeg_bytes")
SIZES = [(1, 1), (8, 8), (7, 30), (16, 16), (17, 17), (9, 23), (24, 24), (25, 40), (40, 24), (33, 47), (72, 56),
         (104, 120), (224, 224), (299, 299), (600, 600)]
QUALITIES = (1, 10, 49, 50, 75, 85, 95, 100)
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2}


def pictures(H, W):
    """noise; a smooth ramp; all 0; all 255; a 1-pixel 0/255 checkerboard."""
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(H + W - 2, 1)], -1)
    return {"noise": np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8),
            "ramp": ramp.astype(np.uint8), "zeros": np.zeros((H, W, 3), np.uint8),
            "ones": np.full((H, W, 3), 255, np.uint8),
            "checker": np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)}


def pillow(pic, quality, subsampling) -> bytes:
    b = io.BytesIO()
    Image.fromarray(pic).save(b, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[subsampling], optimize=False)
    return b.getvalue()


# ------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("H,W", SIZES)
def test_rule_equals_pillow_as_whole_files(H, W):
    rt = _lib.rt()
    for name, pic in pictures(H, W).items():
        for q in QUALITIES:
            for ss in J.SUBSAMPLINGS:
                got = J.encode_rule(pic, q, ss)
                assert got == pillow(pic, q, ss), (name, q, ss)
                # Pillow opens the file, and decodes it to the pixels the project's own host decoder gives
                with Image.open(io.BytesIO(got)) as im:
                    assert im.format == "JPEG" and im.size == (W, H) and im.mode == "RGB"
                    px = np.asarray(im)
                st, _, own = decode_cpu(rt, got)
                assert st == rt.JPEG_OK and np.array_equal(np.asarray(own).reshape(H, W, 3), px), (name, q, ss)


def test_header_and_refusals():
    h = J.header(299, 299, 85, "4:2:0")
    assert len(h) == J.HEADER_BYTES == 623 and h[:4] == b"\xff\xd8\xff\xe0" and h[-14:-12] == b"\xff\xda"
    pic = np.zeros((8, 8, 3), np.uint8)
    assert J.encode_rule(pic) == J.encode_rule(pic, 85, "4:2:0")           # the defaults
    for bad in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            J.encode_rule(pic, bad)
    with pytest.raises(ValueError, match="subsampling"):
        J.encode_rule(pic, 85, "4:2:2")
    for bad in (pic.astype(np.float32), pic[..., 0], np.zeros((0, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            J.encode_rule(bad)


def engine_pictures(S: int, seed: int = 0, n: int = 2) -> np.ndarray:
    """The seeded noise the GPU engine tests feed (tests/test_overlay_jpeg_gpu.py ``_images``)."""
    return np.random.default_rng(S + seed).integers(0, 256, (n, S, S, 3), dtype=np.uint8)


@pytest.mark.parametrize("S", [224, 299])
def test_the_gpu_tests_pictures_fit_the_default_cap(S):
    """Noise at the default quality and sampling stays under the default cap (about 0.8 byte a pixel against
    1.5), whatever is blended on it: no GPU engine or server test passes through the overflow path."""
    cap = overlay_jpeg_cap(S)
    assert cap == (S * S * 3 + 1) // 2
    heat = np.random.default_rng(1).random((7, 7), dtype=np.float32)
    for seed in (0, 20, 21, 22, 23):
        for img in engine_pictures(S, seed):
            for pic in (img, O.overlay_rule(img, heat, Overlay())):
                n = len(J.encode_rule(pic))
                assert 0 < n < cap and n < 1.0 * S * S, (S, seed, n, cap)
    b = io.BytesIO()
    Image.open(PANTS).convert("RGB").resize((299, 299)).save(b, "PNG")
    pants = np.asarray(Image.open(b).convert("RGB"))
    assert len(J.encode_rule(pants)) < overlay_jpeg_cap(299)


# ------------------------------------------------------------------------------ rows
def test_rows_round_trip_with_an_overflow_row():
    rng = np.random.default_rng(2)
    heat = rng.random((3, 3, 4), dtype=np.float32)
    classes, scores = np.array([4, 0, 9], np.int32), rng.random(3, dtype=np.float32)
    files = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (41, 45, 7)]
    cap = 42                                                    # the second file does not fit
    rows = pack_overlay_jpeg(classes, scores, heat, files, cap)
    assert rows.dtype == np.float32 and rows.shape == (3, 2 + 12 + 1 + 11)
    c, s, h, f = unpack_overlay_jpeg(rows, 3, 4, cap)
    assert np.array_equal(c, classes) and np.array_equal(s, scores) and np.array_equal(h, heat)
    assert f == [files[0], b"", files[2]]
    by = rows.view(np.uint8)[:, 4 * 15:]
    assert by[0, 41:].max() == 0 and by[1].max() == 0 and by[2, 7:].max() == 0      # pad bytes are 0
    assert rows.view(np.int32)[:, 14].tolist() == [41, 0, 7]
    with pytest.raises(AssertionError):
        unpack_overlay_jpeg(rows, 3, 4, 64)
    assert J.pack_rows(classes, scores, heat, files, cap).tobytes() == rows.tobytes()


# ------------------------------------------------------------------------------ config, signatures
def _version(tmp_path, meta=None):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, **(meta or {})}))
    return d


def test_config_block_flag_and_errors(tmp_path):
    assert load_version_dir(_version(tmp_path / "d", {"overlay_jpeg": {}}), synthetic=True).overlay_jpeg == OverlayJpeg(
        85, "4:2:0", None)
    d = _version(tmp_path / "c", {"overlay_jpeg": {"quality": 60, "subsampling": "4:4:4", "max_bytes": 50000}})
    assert load_version_dir(d, synthetic=True).overlay_jpeg == OverlayJpeg(60, "4:4:4", 50000)
    assert load_version_dir(d, synthetic=True, overlay_jpeg_quality=90).overlay_jpeg == OverlayJpeg(90, "4:4:4", 50000)
    src = load_version_dir(_version(tmp_path / "f"), synthetic=True, overlay_jpeg_quality=70)    # the flag turns it on
    assert src.overlay_jpeg == OverlayJpeg(70) and all(n in src.signatures for n in SIGS)
    for i, block in enumerate(({"quality": 0}, {"quality": 101}, {"quality": 85.5}, {"quality": "high"},
                               {"subsampling": "4:2:2"}, {"max_bytes": 0}, {"max_bytes": "1k"}, {"qualty": 85}, 85)):
        d = _version(tmp_path / f"bad{i}", {"overlay_jpeg": block})
        with pytest.raises(ValueError, match="synthetic.json"):
            load_version_dir(d, synthetic=True)
    for bad in (0, 101):
        with pytest.raises(ValueError, match="overlay_jpeg_quality"):
            load_version_dir(_version(tmp_path / f"g{bad}"), synthetic=True, overlay_jpeg_quality=bad)


def test_flag_reaches_the_config(monkeypatch):
    from kdl.serving.config import config_from_args as parse_args
    cfg = parse_args(["--model_name", "m", "--model_base_path", "/tmp/m", "--overlay_jpeg_quality", "70"])
    assert cfg.overlay_jpeg_quality == 70
    monkeypatch.setenv("KDL_OVERLAY_JPEG_QUALITY", "40")
    assert parse_args(["--model_name", "m", "--model_base_path", "/tmp/m"]).overlay_jpeg_quality == 40
    monkeypatch.delenv("KDL_OVERLAY_JPEG_QUALITY")
    assert parse_args(["--model_name", "m", "--model_base_path", "/tmp/m"]).overlay_jpeg_quality is None


@pytest.mark.parametrize("model,hw,S,rollout", [("xception", (10, 10), 299, False), ("resnet50", (7, 7), 224, False),
                                                ("efficientnet_b7", (19, 19), 600, False),
                                                ("vit_b16", (14, 14), 224, True)])
def test_signatures_with_and_without_the_block(tmp_path, model, hw, S, rollout):
    from kdl.serving.outputs import kind_of, out_cols
    meta = {} if model == "xception" else {"model": model}
    plain = load_version_dir(_version(tmp_path / "plain", meta), synthetic=True)
    src = load_version_dir(_version(tmp_path / "jpeg", dict(meta, overlay_jpeg={})), synthetic=True)
    # a version without the block has today's signatures, and the block adds the trio and changes nothing else
    assert plain.overlay_jpeg is None and not any(n in plain.signatures for n in SIGS)
    assert [n for n in src.signatures if n not in SIGS] == list(plain.signatures)
    for name, sig in plain.signatures.items():
        assert src.signatures[name] == sig and kind_of(sig).name != "overlay_jpeg", name
    h, w = hw
    for name in SIGS:
        sig = src.signatures[name]
        assert sig.explain == hw and sig.overlay == S and sig.rollout is rollout
        assert sig.outputs == (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)),
                               ("heatmap", P.DT_FLOAT, (-1, h, w)), ("jpeg_bytes", P.DT_STRING, (-1,)))
        assert kind_of(sig).name == "overlay_jpeg"
        assert out_cols(sig, src, True) == out_cols(sig, src, False) == 2 + h * w + 1 + (overlay_jpeg_cap(S) + 3) // 4
    assert src.signatures["overlay_jpeg"].input_shape == (-1, S, S, 3)
    assert src.signatures["overlay_jpeg_bytes"].input_key == src.signatures["serving_bytes"].input_key
    assert kind_of(src.signatures["overlay"]).name == "overlay"


# ------------------------------------------------------------------------------ servers
def _free_port() -> int:
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _server(base, device):
    cfg = ServerConfig(port=0, rest_api_port=_free_port(), model_name="clothing-model", model_base_path=str(base),
                       device=device, host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend="python",
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=500, allowed_batch_sizes=[1, 2]))
    return ModelServer(cfg).start(block_until_loaded=True)


SPEC = OverlayJpeg(60, "4:4:4", None)
OVERLAY = Overlay("hot", 0.75)


@pytest.fixture(scope="module")
def repo(tmp_path_factory):
    base = tmp_path_factory.mktemp("overlay_jpeg") / "clothing-model"
    _version(base, {"seed": 5, "overlay": {"colormap": "hot", "alpha": 0.75},
                    "overlay_jpeg": {"quality": 60, "subsampling": "4:4:4"}})
    return base


@pytest.fixture(scope="module")
def server(repo):
    srv = _server(repo, "cpu")
    yield srv
    srv.stop(0)


@pytest.fixture(scope="module")
def stub(server):
    ch = grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}")
    yield PredictionStub(ch)
    ch.close()


@pytest.fixture(scope="module")
def jpeg():
    b = io.BytesIO()
    Image.open(PANTS).convert("RGB").save(b, "JPEG", quality=90)
    return b.getvalue()


def _answer(resp, n=1):
    assert sorted(resp.outputs) == sorted(KEYS)
    t = resp.outputs["jpeg_bytes"]
    assert t.dtype == P.DT_STRING and [d.size for d in t.tensor_shape.dim] == [n] and len(t.string_val) == n
    hm = resp.outputs["heatmap"]
    return {"classes": [v.decode() for v in resp.outputs["classes"].string_val],
            "scores": np.asarray(resp.outputs["scores"].float_val, np.float32),
            "heatmap": np.asarray(hm.float_val, np.float32).reshape([d.size for d in hm.tensor_shape.dim]),
            "jpeg_bytes": [bytes(v) for v in t.string_val]}


def _inputs(jpeg):
    img = pp.load_image(jpeg)
    return {"overlay_jpeg": (pp.to_uint8(img)[None], "images"),
            "overlay_jpeg_image": (np.asarray(img, np.uint8)[None], "images"),
            "overlay_jpeg_bytes": ([jpeg], "image_bytes")}


@pytest.fixture(scope="module")
def answers(stub, jpeg):
    return {name: _answer(stub.Predict(make_request(x, signature=name, input_key=key), timeout=300))
            for name, (x, key) in _inputs(jpeg).items()}


def test_three_signatures_equal_overlay_and_the_rule(server, stub, answers, jpeg):
    from kdl.serving.metrics import METRICS
    src = server.manager.get("clothing-model", None, None).source
    assert src.overlay_jpeg == SPEC and src.overlay == OVERLAY
    fed = pp.to_uint8(pp.load_image(jpeg))
    for name, (x, key) in _inputs(jpeg).items():
        a = answers[name]
        r = stub.Predict(make_request(x, signature=name.replace("overlay_jpeg", "overlay"), input_key=key), timeout=300)
        pic = np.frombuffer(r.outputs["overlay"].tensor_content, np.uint8).reshape(299, 299, 3)
        assert a["classes"] == [r.outputs["classes"].string_val[0].decode()], name
        assert np.array_equal(a["scores"], np.asarray(r.outputs["scores"].float_val, np.float32)), name
        assert np.array_equal(a["heatmap"].reshape(-1), np.asarray(r.outputs["heatmap"].float_val, np.float32)), name
        (data,) = a["jpeg_bytes"]
        assert data == J.encode_rule(pic, 60, "4:4:4") == pillow(pic, 60, "4:4:4"), name
        assert np.array_equal(pic, O.overlay_rule(fed, a["heatmap"][0], OVERLAY)), name
    counters = METRICS.snapshot()["counters"]
    assert counters.get("kdl_overlay_jpeg_total{signature=overlay_jpeg}", 0) >= 1
    assert counters.get("kdl_overlay_jpeg_overflow_total{signature=overlay_jpeg}", 0) == 0
    r = server.manager.get("clothing-model", None, None).runner("overlay_jpeg")
    assert r.out_cols == 102 + 1 + (overlay_jpeg_cap(299) + 3) // 4 and not r.gpu and r.kind == "overlay_jpeg"
    req = make_request(_inputs(jpeg)["overlay_jpeg"][0], signature="overlay_jpeg", input_key="images")
    req.output_filter.append("jpeg_bytes")
    out = stub.Predict(req, timeout=300).outputs
    assert sorted(out) == ["jpeg_bytes"] and bytes(out["jpeg_bytes"].string_val[0]) == answers["overlay_jpeg"]["jpeg_bytes"][0]


def test_metadata(stub):
    req = P.GetModelMetadataRequest()
    req.model_spec.name = "clothing-model"
    req.metadata_field.append("signature_def")
    sdm = P.SignatureDefMap()
    stub.GetModelMetadata(req, timeout=5).metadata["signature_def"].Unpack(sdm)
    for name in SIGS:
        out = sdm.signature_def[name].outputs
        assert sorted(out) == sorted(KEYS)
        assert out["jpeg_bytes"].dtype == P.DT_STRING and [d.size for d in out["jpeg_bytes"].tensor_shape.dim] == [-1]
    assert sorted(sdm.signature_def["overlay"].outputs) == ["classes", "heatmap", "overlay", "scores"]


def _post(url, body):
    try:
        with urllib.request.urlopen(urllib.request.Request(url, data=json.dumps(body).encode(), method="POST"),
                                    timeout=300) as r:
            return r.status, json.load(r)
    except urllib.error.HTTPError as e:
        return e.code, json.load(e)


def test_rest_predict_answers_b64(server, answers, jpeg):
    a = answers["overlay_jpeg"]
    u8 = _inputs(jpeg)["overlay_jpeg"][0]
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model:predict"
    st, out = _post(url, {"signature_name": "overlay_jpeg", "instances": u8.tolist()})
    assert st == 200, out
    (one,) = out["predictions"]
    assert sorted(one) == sorted(KEYS) and one["classes"] == a["classes"]
    assert sorted(one["jpeg_bytes"]) == ["b64"] and base64.b64decode(one["jpeg_bytes"]["b64"]) == a["jpeg_bytes"][0]
    st, out = _post(url, {"signature_name": "overlay_jpeg", "inputs": {"images": u8.tolist()}})
    assert st == 200, out
    assert [base64.b64decode(e["b64"]) for e in out["outputs"]["jpeg_bytes"]] == a["jpeg_bytes"]
    st, out = _post(url, {"signature_name": "overlay_jpeg_bytes", "instances": [{"b64": base64.b64encode(jpeg).decode()}]})
    assert st == 200, out
    assert base64.b64decode(out["predictions"][0]["jpeg_bytes"]["b64"]) == answers["overlay_jpeg_bytes"]["jpeg_bytes"][0]


def test_null_server_answers_empty_strings(repo):
    px = np.random.default_rng(3).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)
    srv = _server(repo, "null")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            a = _answer(PredictionStub(ch).Predict(make_request(px, signature="overlay_jpeg", input_key="images"),
                                                   timeout=60), 2)
        src = srv.manager.get("clothing-model", None, None).source
    finally:
        srv.stop(0)
    assert a["classes"] == [src.labels[0]] * 2 and (a["scores"] == 0).all() and (a["heatmap"] == 0).all()
    assert a["jpeg_bytes"] == [b"", b""]


def test_overflow_answers_the_empty_string_and_counts(tmp_path, jpeg):
    from kdl.serving.metrics import METRICS
    base = tmp_path / "clothing-model"
    _version(base, {"seed": 5, "overlay_jpeg": {"max_bytes": 700}})
    srv = _server(base, "cpu")
    key = "kdl_overlay_jpeg_overflow_total{signature=overlay_jpeg_bytes}"
    before = METRICS.snapshot()["counters"].get(key, 0)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            a = _answer(PredictionStub(ch).Predict(make_request([jpeg], signature="overlay_jpeg_bytes",
                                                                input_key="image_bytes"), timeout=300))
            monkey = pytest.MonkeyPatch()
            monkey.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
            try:
                c = create_app(GatewayConfig({"GATEWAY_MODE": "bytes"}), channel=ch).test_client()
                r = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg", "format": "jpeg"})
            finally:
                monkey.undo()
    finally:
        srv.stop(0)
    assert a["jpeg_bytes"] == [b""] and a["classes"] != [""]
    assert METRICS.snapshot()["counters"].get(key, 0) - before == 2
    assert r.status_code == 502 and "max_bytes" in r.get_json()["error"]


# ------------------------------------------------------------------------------ gateway
@pytest.mark.parametrize("mode", ["uint8", "bytes", "raw"])
def test_gateway_three_formats(server, stub, answers, jpeg, monkeypatch, mode):
    a = answers[{"bytes": "overlay_jpeg_bytes", "raw": "overlay_jpeg_image"}.get(mode, "overlay_jpeg")]
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        c = create_app(GatewayConfig({"GATEWAY_MODE": mode}), channel=ch).test_client()
        r = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg", "format": "jpeg"})
        assert r.status_code == 200, r.data
        assert r.mimetype == "image/jpeg" and r.data == a["jpeg_bytes"][0]          # the server's bytes, untouched
        assert r.headers["X-KDL-Label"] == a["classes"][0]
        assert np.isclose(float(r.headers["X-KDL-Score"]), a["scores"][0], rtol=1e-6)
        png = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg"})
        assert png.status_code == 200 and png.mimetype == "image/png"
        pic = np.asarray(Image.open(io.BytesIO(png.data)))
        assert J.encode_rule(pic, 60, "4:4:4") == r.data                            # the same picture, as a PNG
        out = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg", "format": "json"})
        assert out.status_code == 200 and sorted(out.get_json()) == ["heatmap", "label", "png", "score"]
        assert base64.b64decode(out.get_json()["png"]) == png.data
        bad = c.post("/overlay", json={"url": "http://example.invalid/x.jpg", "format": "gif"})
        assert bad.status_code == 400 and "jpeg" in bad.get_json()["error"]


def test_gateway_jpeg_on_a_version_without_the_trio(tmp_path, jpeg, monkeypatch):
    base = tmp_path / "clothing-model"
    _version(base, {"seed": 5})
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    srv = _server(base, "null")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            c = create_app(GatewayConfig({"GATEWAY_MODE": "bytes"}), channel=ch).test_client()
            r = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg", "format": "jpeg"})
            ok = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg"})
    finally:
        srv.stop(0)
    assert r.status_code in (400, 404) and "error" in r.get_json()
    assert ok.status_code == 200 and ok.mimetype == "image/png"
