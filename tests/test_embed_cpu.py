"""The embed signatures without a GPU: the normalisation rule, its resolution from the version
directory and the flag, metadata, a ``--device cpu`` server against the fp32 ``feature_oracle``
(gRPC and REST), a ``--device null`` server, both gRPC front-ends, the gateway's /embed."""
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
import torch
from PIL import Image

from kdl.engine import registry
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request, process_embed_response
from kdl.ops import _lib
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig, config_from_args
from kdl.serving.embed import l2_rule, resolve
from kdl.serving.server import ModelServer

PANTS = Path(__file__).parent / "data" / "pants.png"
F = 2048
U = 2.0 ** -24
SIGS = ("embed", "embed_image", "embed_bytes")


# ------------------------------------------------------------------------------ the rule
def test_l2_rule():
    rows = np.array([[3, 4, 0, 0], [0, 0, 0, 0], [1e-20, 0, 0, 0]], np.float32)
    out = l2_rule(rows)
    assert out.dtype == np.float32 and np.isfinite(out).all()
    assert np.allclose(out[0], [0.6, 0.8, 0, 0], rtol=1e-7)
    assert (out[1] == 0).all()                                   # an all-zero row stays zero
    assert np.allclose(out[2], [1e-8, 0, 0, 0], rtol=1e-6)      # below 1e-12: divided by 1e-12


# ------------------------------------------------------------------------------ resolution
def _version(tmp_path, meta=None, name="synthetic.json"):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / name).write_text(json.dumps({"seed": 0, **(meta or {})}))
    return d


def test_normalize_resolution(tmp_path):
    assert resolve(_version(tmp_path / "a")) == "none"
    d = _version(tmp_path / "b", {"embedding": {"normalize": "l2"}})
    assert resolve(d) == "l2" and resolve(d, "none") == "none"               # the flag overrides the file
    assert resolve(_version(tmp_path / "c", {"embedding": {"normalize": "none"}}, "kdl_model.json"), "l2") == "l2"
    assert config_from_args(["--embedding_normalize", "l2"], env={}).embedding_normalize == "l2"
    assert config_from_args([], env={"KDL_EMBEDDING_NORMALIZE": "l2"}).embedding_normalize == "l2"
    assert config_from_args([], env={}).embedding_normalize is None
    for i, bad in enumerate(("L2", "max", 2, None, ["l2"])):
        d = _version(tmp_path / f"bad{i}", {"embedding": {"normalize": bad}})
        with pytest.raises(ValueError, match=r"synthetic\.json.*normalize"):
            resolve(d)
    with pytest.raises(ValueError, match=r"synthetic\.json.*embedding"):
        resolve(_version(tmp_path / "notdict", {"embedding": "l2"}))
    with pytest.raises(ValueError, match="embedding_normalize"):
        resolve(_version(tmp_path / "flag"), "l1")


def test_a_bad_spec_fails_the_load(tmp_path):
    with pytest.raises(ValueError, match=r"synthetic\.json.*normalize"):
        load_version_dir(_version(tmp_path / "a", {"embedding": {"normalize": "unit"}}), synthetic=True)
    src = load_version_dir(_version(tmp_path / "b", {"embedding": {"normalize": "l2"}}), synthetic=True)
    assert src.embed_normalize == "l2" and src.embed_dim == F
    for name in SIGS:
        sig = src.signatures[name]
        assert sig.embed == "l2" and sig.output_key == "embedding" and sig.output_shape == (-1, F)
        assert sig.top_k == 0 and sig.outputs == () and sig.input_dtype != P.DT_FLOAT
    assert src.signatures["embed"].input_shape == (-1, 299, 299, 3)
    assert src.signatures["serving_uint8"].embed == "" and src.signatures["classify"].embed == ""
    src = load_version_dir(_version(tmp_path / "c", {"embedding": {"normalize": "l2"}}), synthetic=True,
                           embedding_normalize="none")
    assert src.embed_normalize == "none" and src.signatures["embed_bytes"].embed == "raw"
    for family in ("resnet50", "vit_b16", "efficientnet_b7"):
        assert registry.get(family).features == {"resnet50": 2048, "vit_b16": 768, "efficientnet_b7": 2560}[family]
    src = load_version_dir(_version(tmp_path / "v", {"model": "vit_b16"}), synthetic=True)
    assert src.embed_dim == 768 and src.signatures["embed"].output_shape == (-1, 768)
    assert src.signatures["embed"].input_shape == (-1, 224, 224, 3)


# ------------------------------------------------------------------------------ servers
def _free_port() -> int:
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _server(base, device, frontend="python", **kw):
    cfg = ServerConfig(port=0, rest_api_port=_free_port(), model_name="clothing-model", model_base_path=str(base),
                       device=device, host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend=frontend,
                       grpc_io_threads=2, batching=BatchingParams(max_batch_size=4, batch_timeout_micros=500,
                                                                  allowed_batch_sizes=[1, 2, 4]), **kw)
    return ModelServer(cfg).start(block_until_loaded=True)


@pytest.fixture(scope="module")
def repo(tmp_path_factory):
    base = tmp_path_factory.mktemp("embed") / "clothing-model"
    _version(base, {"seed": 5})
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
def pixels():
    return np.random.default_rng(3).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def oracle(server, pixels):
    """feature_oracle rows of ``pixels`` under the served version's own weights, computed once."""
    params = server.manager.get("clothing-model", None, None).source.params
    return registry.get("xception").feature_oracle(params, torch.from_numpy(pixels)).numpy()


def _rows(resp, n=None, f=F):
    t = resp.outputs["embedding"]
    shape = [d.size for d in t.tensor_shape.dim]
    assert list(resp.outputs) == ["embedding"] and t.dtype == P.DT_FLOAT and shape[1] == f
    assert n is None or shape[0] == n
    return np.asarray(t.float_val, np.float32).reshape(shape)


def _post(url, body):
    data = body if isinstance(body, bytes) else json.dumps(body).encode()
    try:
        with urllib.request.urlopen(urllib.request.Request(url, data=data, method="POST"), timeout=120) as r:
            return r.status, json.load(r)
    except urllib.error.HTTPError as e:
        return e.code, json.load(e)


def _close(got, want):
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6), np.abs(np.asarray(got) - want).max()


def test_metadata(server, stub):
    req = P.GetModelMetadataRequest()
    req.model_spec.name = "clothing-model"
    req.metadata_field.append("signature_def")
    sdm = P.SignatureDefMap()
    stub.GetModelMetadata(req, timeout=5).metadata["signature_def"].Unpack(sdm)
    inputs = {"embed": ("images", P.DT_UINT8, [-1, 299, 299, 3]), "embed_image": ("images", P.DT_UINT8, [-1, -1, -1, 3]),
              "embed_bytes": ("image_bytes", P.DT_STRING, [-1])}
    for name, (key, dtype, shape) in inputs.items():
        sd = sdm.signature_def[name]
        assert sd.method_name == "tensorflow/serving/predict"
        assert list(sd.inputs) == [key] and sd.inputs[key].dtype == dtype
        assert [d.size for d in sd.inputs[key].tensor_shape.dim] == shape
        assert list(sd.outputs) == ["embedding"] and sd.outputs["embedding"].dtype == P.DT_FLOAT
        assert [d.size for d in sd.outputs["embedding"].tensor_shape.dim] == [-1, F]
    assert list(sdm.signature_def["serving_bytes"].outputs) == ["dense_7"]       # the others are as they were
    assert sorted(sdm.signature_def["classify"].outputs) == ["classes", "scores"]
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model/metadata"
    md = json.load(urllib.request.urlopen(url))["metadata"]["signature_def"]["signatureDef"]
    for name in SIGS:
        assert list(md[name]["outputs"]) == ["embedding"]
        assert [int(d["size"]) for d in md[name]["outputs"]["embedding"]["tensorShape"]["dim"]] == [-1, F]


def test_embed_equals_the_feature_oracle_over_grpc_and_rest(server, stub, pixels, oracle):
    resp = stub.Predict(make_request(pixels, signature="embed", input_key="images"), timeout=120)
    assert resp.model_spec.name == "clothing-model" and resp.model_spec.signature_name == "embed"
    assert resp.model_spec.version.value == 1
    _close(_rows(resp, 2), oracle)
    assert np.asarray(process_embed_response(resp), np.float32).shape == (2, F)
    r = server.manager.get("clothing-model", None, None).runner("embed")
    assert r.out_cols == F and r.sig.embed == "raw"
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model:predict"
    st, out = _post(url, {"signature_name": "embed", "instances": pixels[:1].tolist()})
    assert st == 200, out
    _close(np.asarray(out["predictions"], np.float32), oracle[:1])
    st, out = _post(url, {"signature_name": "embed", "inputs": {"images": pixels[:1].tolist()}})
    assert st == 200, out
    _close(np.asarray(out["outputs"], np.float32), oracle[:1])


def test_the_image_and_bytes_twins(server, stub):
    """A PNG decodes exactly, so embed_bytes of the file and embed_image of its pixels see the same
    image; embed of the pixels resized here by the same (nearest) rule is the third answer."""
    img = Image.open(PANTS).convert("RGB")
    b = io.BytesIO()
    img.save(b, "PNG")
    a = _rows(stub.Predict(make_request([b.getvalue()], signature="embed_bytes", input_key="image_bytes"), timeout=120), 1)
    px = np.asarray(img, np.uint8)[None]
    c = _rows(stub.Predict(make_request(px, signature="embed_image", input_key="images"), timeout=120), 1)
    d = _rows(stub.Predict(make_request(pp.to_uint8(img)[None], signature="embed", input_key="images"), timeout=120), 1)
    _close(a, c)
    _close(a, d)
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model:predict"
    st, out = _post(url, {"signature_name": "embed_bytes",
                          "instances": [{"b64": base64.b64encode(b.getvalue()).decode()}]})
    assert st == 200, out
    _close(np.asarray(out["predictions"], np.float32), a)


def test_output_filter_and_refusals(stub, pixels, oracle):
    req = make_request(pixels[:1], signature="embed", input_key="images")
    req.output_filter.append("embedding")
    _close(_rows(stub.Predict(req, timeout=120), 1), oracle[:1])
    req = make_request(pixels[:1], signature="embed", input_key="images")
    req.output_filter.append("dense_7")
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(req, timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert e.value.details() == "output tensor alias not found in signature: dense_7"
    f32 = pixels[:1].astype(np.float32) / 127.5 - 1.0                       # the embed signatures take no f32 input
    for key in ("images", "input_8"):
        with pytest.raises(grpc.RpcError) as e:
            stub.Predict(make_request(f32, signature="embed", input_key=key), timeout=30)
        assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT, e.value.details()


def test_counters(stub, pixels):
    from kdl.serving.metrics import METRICS
    before = METRICS.snapshot()["counters"]
    stub.Predict(make_request(pixels[:1], signature="embed", input_key="images"), timeout=120)
    after = METRICS.snapshot()["counters"]
    key = "kdl_embed_total{signature=embed}"
    assert after.get(key, 0) - before.get(key, 0) == 1


def test_l2_server(repo, pixels, oracle):
    """--embedding_normalize l2 over a version that declares nothing: unit rows of the same direction."""
    srv = _server(repo, "cpu", embedding_normalize="l2")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            got = _rows(PredictionStub(ch).Predict(make_request(pixels, signature="embed", input_key="images"),
                                                   timeout=120), 2)
        assert srv.manager.get("clothing-model", None, None).runner("embed").sig.embed == "l2"
    finally:
        srv.stop(0)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() <= (F / 2 + 8) * U
    _close(got, l2_rule(oracle))


def test_null_server_rows_are_f_wide(repo, pixels):
    """The null device's row is {first byte of the item + k}: F of them for an embed runner."""
    srv = _server(repo, "null")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            got = _rows(PredictionStub(ch).Predict(make_request(pixels, signature="embed", input_key="images"),
                                                   timeout=60), 2)
            ref = PredictionStub(ch).Predict(make_request(pixels, signature="serving_uint8", input_key="images"), timeout=60)
        assert len(ref.outputs["dense_7"].float_val) == 2 * 10                 # the logits signatures keep their width
    finally:
        srv.stop(0)
    want = pixels.reshape(2, -1)[:, :1].astype(np.float32) + np.arange(F, dtype=np.float32)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------ both front-ends
def _call(port, path, raw: bytes, timeout=120.0):
    with grpc.insecure_channel(f"127.0.0.1:{port}") as ch:
        try:
            return 0, "", ch.unary_unary(path)(raw, timeout=timeout)
        except grpc.RpcError as e:
            return e.code().value[0], e.details(), b""


def test_both_front_ends_answer_alike(repo, pixels):
    """embed has a fixed input shape and one float output: the native front-end learns its route
    (the fast path answers from the second request on), and its bytes equal grpcio's."""
    if not _lib.rt().http2_available()[0]:
        pytest.skip("libnghttp2 not loadable")
    nat, py = _server(repo, "null", "native"), _server(repo, "null", "python")
    try:
        assert nat.native is not None and py.native is None
        req = make_request(pixels, signature="embed", input_key="images").SerializeToString()
        fast0 = nat.native.stats()["fast_ok"]
        for _ in range(3):
            a, b = _call(nat.grpc_port, P.PREDICT_METHOD, req), _call(py.grpc_port, P.PREDICT_METHOD, req)
            assert a[0] == 0 and a == b
        assert nat.native.stats()["fast_ok"] >= fast0 + 2
        assert _rows(P.PredictResponse.FromString(a[2]), 2).shape == (2, F)
        f32 = make_request(pixels[:1].astype(np.float32), signature="embed", input_key="images").SerializeToString()
        a, b = _call(nat.grpc_port, P.PREDICT_METHOD, f32), _call(py.grpc_port, P.PREDICT_METHOD, f32)
        assert a[0] == grpc.StatusCode.INVALID_ARGUMENT.value[0] and a == b
    finally:
        nat.stop(0)
        py.stop(0)


# ------------------------------------------------------------------------------ gateway
@pytest.mark.parametrize("mode", ["uint8", "bytes", "raw", "compat"])
def test_gateway_embed(server, stub, monkeypatch, mode):
    data = PANTS.read_bytes()
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: data)
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        app = create_app(GatewayConfig({"GATEWAY_MODE": mode}), channel=ch)
        r = app.test_client().post("/embed", json={"url": "http://example.invalid/pants.png"})
        assert r.status_code == 200, r.data
        out = r.get_json()
        assert app.test_client().post("/embed", json={"nope": 1}).status_code == 400
    if mode == "bytes":
        req = make_request([data], signature="embed_bytes", input_key="image_bytes")
    elif mode == "raw":
        req = make_request(np.asarray(pp.load_image(data), np.uint8)[None], signature="embed_image", input_key="images")
    else:
        req = make_request(pp.to_uint8(pp.load_image(data))[None], signature="embed", input_key="images")
    want = _rows(stub.Predict(req, timeout=120), 1)
    assert list(out) == ["embedding"] and len(out["embedding"]) == F
    _close(np.asarray(out["embedding"], np.float32), want[0])
