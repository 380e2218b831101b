"""Classification outputs without a GPU: the numpy rule, the three classify signatures on a
``--device cpu`` synthetic Xception server, the Classify RPC and REST ``:classify`` on both gRPC
front-ends, labels and K resolution, the gateway's ``/classify`` and ``Servable.device_alive``
with wrapper runners. (The device kernel and the engines' top-k step: test_classify_gpu.py.)"""
import base64
import io
import json
import socket
import threading
import urllib.error
import urllib.request
from pathlib import Path

import grpc
import numpy as np
import pytest
from PIL import Image

from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request, process_classify_response
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.classify import pack_rows, resolve, topk_rule, unpack_rows
from kdl.serving.config import BatchingParams, ServerConfig, config_from_args
from kdl.serving.server import ModelServer

rt = pytest.importorskip("kdl._rt")

CLASSIFY = "/tensorflow.serving.PredictionService/Classify"
LABELS = [f"garment-{i}" for i in range(10)]
PANTS = Path(__file__).parent / "data" / "pants.png"


# ------------------------------------------------------------------------------ the rule
def test_rule_hand_written_cases():
    x = np.array([[1.0, 3.0, 2.0, 3.0, -1.0]], np.float32)            # a tie between 1 and 3
    cls, sc = topk_rule(x, 3)
    assert cls.dtype == np.int32 and sc.dtype == np.float32
    assert cls.tolist() == [[1, 3, 2]]
    e = np.exp(np.array([1.0, 3.0, 2.0, 3.0, -1.0]) - 3.0)
    assert np.allclose(sc[0], (e / e.sum())[[1, 3, 2]], rtol=1e-7)
    cls, sc = topk_rule(np.zeros((2, 7), np.float32) + 4.5, 3)        # all equal
    assert cls.tolist() == [[0, 1, 2]] * 2 and np.allclose(sc, 1 / 7, rtol=1e-7)
    x = np.array([[0.5, -2.0, 7.0, 0.5]], np.float32)                 # K = NC: a full stable sort
    cls, sc = topk_rule(x, 4)
    assert cls.tolist() == [[2, 0, 3, 1]] and abs(float(sc.sum()) - 1.0) < 1e-6
    assert sc[0, 1] == sc[0, 2]
    cls, sc = topk_rule(np.array([[1e4, 1e4 - 1.0]], np.float32), 2)  # a large offset does not overflow
    assert cls.tolist() == [[0, 1]] and np.allclose(sc[0], [1 / (1 + np.exp(-1.0)), 1 / (1 + np.exp(1.0))], rtol=1e-6)


def test_rows_round_trip():
    cls, sc = topk_rule(np.random.default_rng(0).standard_normal((3, 10)).astype(np.float32), 4)
    rows = pack_rows(cls, sc)
    assert rows.dtype == np.float32 and rows.shape == (3, 8)
    c2, s2 = unpack_rows(rows.copy())
    assert np.array_equal(c2, cls) and np.array_equal(s2, sc)


# ------------------------------------------------------------------------------ K and labels
def _version(tmp_path, meta=None, labels=None, name="synthetic.json"):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / name).write_text(json.dumps({"seed": 0, **(meta or {})}))
    if labels is not None:
        (d / "labels.txt").write_text("\n".join(labels) + "\n")
    return d


def test_k_and_labels_resolution(tmp_path):
    d = _version(tmp_path / "a")
    assert resolve(d, 10) == (5, "image/encoded", [str(i) for i in range(10)])       # defaults, index strings
    assert resolve(d, 3)[0] == 3                                                      # clipped to the classes
    d = _version(tmp_path / "b", {"classify": {"top_k": 4, "feature": "jpeg"}}, LABELS)
    assert resolve(d, 10) == (4, "jpeg", LABELS)
    assert resolve(d, 10, 3)[0] == 3                                                  # the flag overrides the file
    assert config_from_args(["--classify_top_k", "3"], env={}).classify_top_k == 3
    assert config_from_args([], env={"KDL_CLASSIFY_TOP_K": "7"}).classify_top_k == 7
    assert config_from_args([], env={}).classify_top_k is None
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="top_k"):
            resolve(d, 10, bad)
        with pytest.raises(ValueError, match="top_k"):
            resolve(_version(tmp_path / f"k{bad}", {"classify": {"top_k": bad}}), 10)
    d = _version(tmp_path / "c", labels=LABELS[:9])
    with pytest.raises(ValueError, match="9 labels.*10 classes"):
        resolve(d, 10)
    d = _version(tmp_path / "d", {"labels": LABELS}, name="kdl_model.json")
    assert resolve(d, 10)[2] == LABELS


def test_a_bad_spec_fails_the_load(tmp_path):
    with pytest.raises(ValueError, match="9 labels"):
        load_version_dir(_version(tmp_path / "a", labels=LABELS[:9]), synthetic=True)
    with pytest.raises(ValueError, match="top_k"):
        load_version_dir(_version(tmp_path / "b"), synthetic=True, classify_top_k=33)
    with pytest.raises(ValueError, match="top_k"):
        load_version_dir(_version(tmp_path / "c", {"classify": {"top_k": 0}}), synthetic=True)
    src = load_version_dir(_version(tmp_path / "d", {"classify": {"top_k": 4}}, LABELS), synthetic=True,
                           classify_top_k=3)
    assert src.classify_k == 3 and src.labels == LABELS
    for name in ("classify", "classify_image", "classify_bytes"):
        sig = src.signatures[name]
        assert sig.top_k == 3 and [o[0] for o in sig.outputs] == ["classes", "scores"]
    assert src.signatures["serving_uint8"].top_k == 0 and src.signatures["serving_uint8"].outputs == ()


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
    base = tmp_path_factory.mktemp("classify") / "clothing-model"
    _version(base, {"seed": 5}, LABELS)
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
def files():
    """tests/data/pants.png as a JPEG and as a PNG."""
    img = Image.open(PANTS).convert("RGB")
    out = []
    for fmt, kw in (("JPEG", dict(quality=90)), ("PNG", {})):
        b = io.BytesIO()
        img.save(b, fmt, **kw)
        out.append(b.getvalue())
    return out


def _logits(resp, n):
    return np.asarray(resp.outputs["dense_7"].float_val, np.float32).reshape(n, 10)


def _classes_scores(resp):
    cl, sc = resp.outputs["classes"], resp.outputs["scores"]
    shape = [d.size for d in sc.tensor_shape.dim]
    assert cl.dtype == P.DT_STRING and sc.dtype == P.DT_FLOAT
    assert [d.size for d in cl.tensor_shape.dim] == shape and len(cl.string_val) == len(sc.float_val) == shape[0] * shape[1]
    return (np.asarray([v.decode() for v in cl.string_val]).reshape(shape),
            np.asarray(sc.float_val, np.float32).reshape(shape))


def _expect(logits, k=5):
    cls, sc = topk_rule(logits, k)
    return np.asarray(LABELS)[cls], sc


def _same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.allclose(got[1], want[1], rtol=1e-6, atol=0), (got[1], want[1])


@pytest.fixture(scope="module")
def bytes_logits(stub, files):
    return _logits(stub.Predict(make_request(files, signature="serving_bytes", input_key="image_bytes"), timeout=120), 2)


def test_the_three_signatures_follow_the_logits_of_their_twins(stub, files, bytes_logits):
    u8 = np.random.default_rng(3).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)
    want = _expect(_logits(stub.Predict(make_request(u8, signature="serving_uint8", input_key="images"), timeout=120), 2))
    _same(_classes_scores(stub.Predict(make_request(u8, signature="classify", input_key="images"), timeout=120)), want)
    px = np.random.default_rng(4).integers(0, 256, (1, 120, 77, 3), dtype=np.uint8)
    want = _expect(_logits(stub.Predict(make_request(px, signature="serving_image", input_key="images"), timeout=120), 1))
    _same(_classes_scores(stub.Predict(make_request(px, signature="classify_image", input_key="images"), timeout=120)),
          want)
    got = stub.Predict(make_request(files, signature="classify_bytes", input_key="image_bytes"), timeout=120)
    _same(_classes_scores(got), _expect(bytes_logits))
    assert got.model_spec.name == "clothing-model" and got.model_spec.signature_name == "classify_bytes"
    assert got.model_spec.version.value == 1


def test_output_filter(stub, files, bytes_logits):
    want = _expect(bytes_logits)
    for names in (["classes"], ["scores"], ["scores", "classes"]):
        req = make_request(files, signature="classify_bytes", input_key="image_bytes")
        req.output_filter.extend(names)
        resp = stub.Predict(req, timeout=120)
        assert sorted(resp.outputs) == sorted(names)
        if "classes" in names:
            assert [v.decode() for v in resp.outputs["classes"].string_val] == want[0].reshape(-1).tolist()
        if "scores" in names:
            assert np.allclose(np.asarray(resp.outputs["scores"].float_val, np.float32), want[1].reshape(-1), rtol=1e-6)
    req = make_request(files, signature="classify_bytes", input_key="image_bytes")
    req.output_filter.append("dense_7")
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(req, timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert e.value.details() == "output tensor alias not found in signature: dense_7"


def test_metadata(server, stub):
    req = P.GetModelMetadataRequest()
    req.model_spec.name = "clothing-model"
    req.metadata_field.append("signature_def")
    sdm = P.SignatureDefMap()
    stub.GetModelMetadata(req, timeout=5).metadata["signature_def"].Unpack(sdm)
    inputs = {"classify": ("images", P.DT_UINT8, [-1, 299, 299, 3]), "classify_image": ("images", P.DT_UINT8, [-1, -1, -1, 3]),
              "classify_bytes": ("image_bytes", P.DT_STRING, [-1])}
    for name, (key, dtype, shape) in inputs.items():
        sd = sdm.signature_def[name]
        assert sd.method_name == "tensorflow/serving/predict"
        assert list(sd.inputs) == [key] and sd.inputs[key].dtype == dtype
        assert [d.size for d in sd.inputs[key].tensor_shape.dim] == shape
        assert sorted(sd.outputs) == ["classes", "scores"]
        assert sd.outputs["classes"].dtype == P.DT_STRING and sd.outputs["scores"].dtype == P.DT_FLOAT
        for k in ("classes", "scores"):
            assert [d.size for d in sd.outputs[k].tensor_shape.dim] == [-1, 5]
    assert list(sdm.signature_def["serving_bytes"].outputs) == ["dense_7"]       # the others are as they were
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model/metadata"
    md = json.load(urllib.request.urlopen(url))["metadata"]["signature_def"]["signatureDef"]
    assert sorted(md["classify"]["outputs"]) == ["classes", "scores"]
    assert md["classify_bytes"]["outputs"]["classes"]["dtype"] == "DT_STRING"


# ------------------------------------------------------------------------------ Classify RPC / REST
def _classify_request(images, model="clothing-model", signature="", feature="image/encoded"):
    req = P.ClassificationRequest()
    req.model_spec.name = model
    req.model_spec.signature_name = signature
    for data in images:
        req.input.example_list.examples.add().features.feature[feature].bytes_list.value.append(data)
    return req


def _call(port, path, raw: bytes, timeout=120.0):
    with grpc.insecure_channel(f"127.0.0.1:{port}") as ch:
        try:
            return 0, "", ch.unary_unary(path)(raw, timeout=timeout)
        except grpc.RpcError as e:
            return e.code().value[0], e.details(), b""


def _post(url, body):
    data = body if isinstance(body, bytes) else json.dumps(body).encode()
    try:
        with urllib.request.urlopen(urllib.request.Request(url, data=data, method="POST"), timeout=120) as r:
            return r.status, json.load(r)
    except urllib.error.HTTPError as e:
        return e.code, json.load(e)


def test_classify_rpc_and_rest_follow_serving_bytes(server, files, bytes_logits):
    want = _expect(bytes_logits)
    code, msg, raw = _call(server.grpc_port, CLASSIFY, _classify_request(files).SerializeToString())
    assert code == 0, msg
    resp = P.ClassificationResponse.FromString(raw)
    assert resp.model_spec.name == "clothing-model" and resp.model_spec.version.value == 1
    assert len(resp.result.classifications) == 2
    for i, c in enumerate(resp.result.classifications):
        assert [k.label for k in c.classes] == want[0][i].tolist()
        assert np.allclose([k.score for k in c.classes], want[1][i], rtol=1e-6)
    code, _, raw2 = _call(server.grpc_port, CLASSIFY,
                          _classify_request(files, signature="classify_bytes").SerializeToString())
    assert code == 0 and P.ClassificationResponse.FromString(raw2).result == resp.result
    base = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model"
    examples = [{"image/encoded": {"b64": base64.b64encode(d).decode()}} for d in files]
    for url in (base + ":classify", base + "/versions/1:classify", base + "/labels/stable:classify"):
        st, out = _post(url, {"examples": examples})
        assert st == 200, out
        assert [[c[0] for c in row] for row in out["results"]] == want[0].tolist()
        assert np.allclose([[c[1] for c in row] for row in out["results"]], want[1], rtol=1e-6)
    for body in ({"examples": examples, "context": {}}, {"examples": []}, {"examples": [{"other": {"b64": "AAAA"}}]},
                 {"examples": [{"image/encoded": 3}]}, {"signature_name": "serving_bytes", "examples": examples},
                 {"instances": examples}):
        st, out = _post(base + ":classify", body)
        assert st == 400 and out["error"], body
    assert _post(f"http://127.0.0.1:{server.rest_port}/v1/models/nope:classify", {"examples": examples})[0] == 404


def test_rest_predict_on_the_classify_signatures(server, files, bytes_logits):
    want = _expect(bytes_logits)
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model:predict"
    b64 = [{"b64": base64.b64encode(d).decode()} for d in files]
    st, out = _post(url, {"signature_name": "classify_bytes", "instances": b64})
    assert st == 200 and [p["classes"] for p in out["predictions"]] == want[0].tolist()
    assert np.allclose([p["scores"] for p in out["predictions"]], want[1], rtol=1e-6)
    st, out = _post(url, {"signature_name": "classify_bytes", "inputs": {"image_bytes": b64}})
    assert st == 200 and out["outputs"]["classes"] == want[0].tolist()
    assert np.allclose(out["outputs"]["scores"], want[1], rtol=1e-6)
    u8 = np.random.default_rng(3).integers(0, 256, (1, 299, 299, 3), dtype=np.uint8)
    st, out = _post(url, {"signature_name": "classify", "instances": u8.tolist()})
    assert st == 200 and len(out["predictions"]) == 1 and len(out["predictions"][0]["classes"]) == 5
    st, ref = _post(url, {"signature_name": "serving_uint8", "instances": u8.tolist()})
    e = _expect(np.asarray(ref["predictions"], np.float32))
    assert out["predictions"][0]["classes"] == e[0][0].tolist()
    assert np.allclose(out["predictions"][0]["scores"], e[1][0], rtol=1e-6)


def _bad_classify_requests(files):
    yield "empty body", b"", None
    yield "unparsable", b"\x0a\xff\xff\xff", None
    r = P.ClassificationRequest()
    r.model_spec.name = "clothing-model"
    r.input.example_list.SetInParent()
    yield "empty example list", r.SerializeToString(), None
    r = P.ClassificationRequest()
    r.model_spec.name = "clothing-model"
    r.input.example_list_with_context.examples.add().features.feature["image/encoded"].bytes_list.value.append(files[0])
    yield "with context", r.SerializeToString(), None
    r = _classify_request(files)
    r.input.example_list.examples.add().features.feature["other"].bytes_list.value.append(files[0])
    yield "missing feature", r.SerializeToString(), "example 2"
    r = _classify_request(files[:1])
    r.input.example_list.examples.add().features.feature["image/encoded"].float_list.value.append(1.0)
    yield "non-bytes feature", r.SerializeToString(), "example 1"
    r = _classify_request(files[:1])
    r.input.example_list.examples[0].features.feature["image/encoded"].bytes_list.value.append(files[0])
    yield "two values", r.SerializeToString(), "example 0"
    yield "another signature", _classify_request(files, signature="serving_bytes").SerializeToString(), None
    yield "not an image", _classify_request([files[0], b"junk"]).SerializeToString(), "image 1"


@pytest.fixture(scope="module")
def pair(repo):
    """The same repo behind the native and the grpcio front-end, on the null device (its logits
    are the item's first byte + the class index: classes 9, 8, ... for every image)."""
    if not rt.http2_available()[0]:
        pytest.skip("libnghttp2 not loadable")
    nat, py = _server(repo, "null", "native"), _server(repo, "null", "python")
    assert nat.native is not None and py.native is None
    yield nat, py
    nat.stop(0)
    py.stop(0)


def test_invalid_argument_cases(server, files):
    for name, raw, needle in _bad_classify_requests(files):
        code, msg, _ = _call(server.grpc_port, CLASSIFY, raw)
        assert code == grpc.StatusCode.INVALID_ARGUMENT.value[0], (name, code, msg)
        assert msg and (needle is None or needle in msg), (name, msg)
    code, msg, _ = _call(server.grpc_port, CLASSIFY, _classify_request(files, model="nope").SerializeToString())
    assert code == grpc.StatusCode.NOT_FOUND.value[0]
    for path in ("Regress", "MultiInference"):
        code, _, _ = _call(server.grpc_port, f"/tensorflow.serving.PredictionService/{path}", b"")
        assert code == grpc.StatusCode.UNIMPLEMENTED.value[0]


def test_both_front_ends_answer_alike(pair, files):
    nat, py = pair
    for name, raw, _ in _bad_classify_requests(files):
        if name == "not an image":       # the decoder's own message carries an object address
            continue
        a, b = _call(nat.grpc_port, CLASSIFY, raw), _call(py.grpc_port, CLASSIFY, raw)
        assert a[0] == grpc.StatusCode.INVALID_ARGUMENT.value[0] and a == b, (name, a, b)
    raw = _classify_request(files).SerializeToString()
    a, b = _call(nat.grpc_port, CLASSIFY, raw), _call(py.grpc_port, CLASSIFY, raw)
    assert a[0] == 0 and a == b
    resp = P.ClassificationResponse.FromString(a[2])
    assert [[k.label for k in c.classes] for c in resp.result.classifications] == [LABELS[:4:-1]] * 2
    # Predict on a classify signature: the slow path every time, equal bytes, never a learned route
    u8 = np.random.default_rng(1).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)
    req = make_request(u8, signature="classify", input_key="images").SerializeToString()
    fast0 = nat.native.stats()["fast_ok"]
    for _ in range(3):
        a, b = _call(nat.grpc_port, P.PREDICT_METHOD, req), _call(py.grpc_port, P.PREDICT_METHOD, req)
        assert a[0] == 0 and a == b
    assert nat.native.stats()["fast_ok"] == fast0
    got = _classes_scores(P.PredictResponse.FromString(a[2]))
    _same(got, _expect(u8.reshape(2, -1)[:, :1].astype(np.float32) + np.arange(10, dtype=np.float32)))


def test_counters(server, stub, files, bytes_logits):
    from kdl.serving.metrics import METRICS
    before = METRICS.snapshot()["counters"]
    stub.Predict(make_request(files[:1], signature="classify_bytes", input_key="image_bytes"), timeout=120)
    _call(server.grpc_port, CLASSIFY, _classify_request(files[:1]).SerializeToString())
    _call(server.grpc_port, CLASSIFY, b"")
    after = METRICS.snapshot()["counters"]

    def grew(key):
        return after.get(key, 0) - before.get(key, 0)
    assert grew("kdl_classify_total{signature=classify_bytes}") == 2
    assert grew("kdl_requests_total{code=OK,method=Classify}") == 1
    assert grew("kdl_requests_total{code=INVALID_ARGUMENT,method=Classify}") == 1


# ------------------------------------------------------------------------------ the top-K flag, index labels
def test_top_k_flag_and_index_labels(tmp_path, files):
    base = tmp_path / "clothing-model"
    _version(base, {"seed": 5, "classify": {"top_k": 4}})
    srv = _server(base, "null", classify_top_k=3)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            resp = PredictionStub(ch).Predict(make_request(files, signature="classify_bytes", input_key="image_bytes"),
                                              timeout=60)
        cl, sc = _classes_scores(resp)
        assert cl.tolist() == [["9", "8", "7"]] * 2 and sc.shape == (2, 3)
    finally:
        srv.stop(0)


# ------------------------------------------------------------------------------ gateway
@pytest.mark.parametrize("mode", ["uint8", "bytes", "raw", "compat"])
def test_gateway_classify(server, stub, files, bytes_logits, monkeypatch, mode):
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: files[0])
    app = create_app(GatewayConfig({"TF_SERVING_HOST": f"127.0.0.1:{server.grpc_port}", "GATEWAY_MODE": mode}))
    r = app.test_client().post("/classify", json={"url": "http://example.invalid/pants.jpg"})
    assert r.status_code == 200, r.data
    out = r.get_json()
    if mode == "bytes":
        logits = bytes_logits[:1]
    elif mode == "raw":
        px = np.asarray(pp.load_image(files[0]), np.uint8)[None]
        logits = _logits(stub.Predict(make_request(px, signature="serving_image", input_key="images"), timeout=120), 1)
    else:
        px = pp.to_uint8(pp.load_image(files[0]))[None]
        logits = _logits(stub.Predict(make_request(px, signature="serving_uint8", input_key="images"), timeout=120), 1)
    want = _expect(logits)
    assert [e["label"] for e in out] == want[0][0].tolist() and len(out) == 5
    assert np.allclose([e["score"] for e in out], want[1][0], rtol=1e-6)
    assert app.test_client().post("/classify", json={"nope": 1}).status_code == 400
    resp = stub.Predict(make_request(files[:1], signature="classify_bytes", input_key="image_bytes"), timeout=120)
    assert [e["label"] for e in process_classify_response(resp)[0]] == _expect(bytes_logits[:1])[0][0].tolist()


def test_smoke_classify_tool(server, stub, capsys):
    import ast
    import importlib.util
    spec = importlib.util.spec_from_file_location("smoke_classify", PANTS.parent.parent.parent / "tools" / "smoke_classify.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main(["--file", str(PANTS), "--grpc", f"127.0.0.1:{server.grpc_port}"]) == 0
    out = ast.literal_eval(capsys.readouterr().out.strip().splitlines()[-1])
    ref = _logits(stub.Predict(make_request([PANTS.read_bytes()], signature="serving_bytes", input_key="image_bytes"),
                               timeout=120), 1)
    want = _expect(ref)
    assert [e["label"] for e in out] == want[0][0].tolist()
    assert np.allclose([e["score"] for e in out], want[1][0], rtol=1e-6)


# ------------------------------------------------------------------------------ device_alive, the watch thread
def test_device_alive_with_wrapper_runners(tmp_path, files, monkeypatch):
    """A wrapper runner (no batcher of its own) speaks through its inner runner's batcher: a
    classify_bytes request that fails on every executor is evidence of a dead device, and a
    working signature beside it brings the device back."""
    from kdl.serving.model_repo import ModelManager
    monkeypatch.setenv("KDL_FAULT_INJECT", "fail=/classify:-1")
    base = tmp_path / "clothing-model"
    _version(base)
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="null", host="127.0.0.1",
                       batching=BatchingParams(max_batch_size=4, batch_timeout_micros=200, allowed_batch_sizes=[1, 4]),
                       warm_signatures=["classify_bytes", "classify_image", "serving_image"])
    m = ModelManager(cfg)
    m.load_initial()
    try:
        s = m.servables[max(m.servables)]
        for name in ("classify_bytes", "classify_image", "serving_image"):
            assert name in s.runners and not hasattr(s.runners[name], "batcher")
        assert m.device_alive() and s.device_alive()                 # nothing used yet; no AttributeError
        wrapper = s.runners["classify_bytes"]
        for _ in range(10):
            if not wrapper.healthy():
                break
            with pytest.raises(Exception):
                wrapper.predict(files[:1], 1, 0)
        assert not wrapper.healthy() and not m.device_alive()
        out = s.runner("serving_image").predict(np.full((1, 20, 30, 3), 5, np.uint8), 1, 0)
        assert np.array_equal(out[0], 5 + np.arange(10, dtype=np.float32))
        assert m.device_alive()
    finally:
        for sv in m.servables.values():
            sv.close()


def test_the_watch_thread_survives_a_failing_poll():
    from kdl.serving import server as S

    third = threading.Event()

    class Manager:
        calls = 0

        def device_alive(self):
            Manager.calls += 1
            if Manager.calls == 1:
                raise AttributeError("'ImageRunner' object has no attribute 'batcher'")
            if Manager.calls >= 3:
                third.set()
            return True

    class Srv:
        manager = Manager()
        cfg = ServerConfig(gpu_index=0)
    done, rc = threading.Event(), [0]
    t = threading.Thread(target=S._watch_devices, args=(Srv(), done, rc), daemon=True)
    t.start()
    assert third.wait(10), "the watch thread died on the failing poll"
    assert t.is_alive() and rc[0] == 0
    done.set()
    t.join(5)
    assert not t.is_alive()
