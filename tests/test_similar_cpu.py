"""The similar signatures without a GPU: the stored values (``load_gallery``), the numpy rule, K and
gallery resolution from the version directory and the flag, a ``--device cpu`` server against
``similar_rule`` over the fp32 ``feature_oracle`` (gRPC and REST), the gateway's /similar against
a stub, and ``build-gallery``."""
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
from kdl.gateway.client import PredictionStub, make_request, process_similar_response
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig, config_from_args
from kdl.serving.embed import l2_rule
from kdl.serving.server import ModelServer
from kdl.serving.similar import GALLERY_MAX_N, bf16_to_f64, load_gallery, resolve, similar_rule

PANTS = Path(__file__).parent / "data" / "pants.png"
F = 2048
SIGS = ("similar", "similar_image", "similar_bytes")


def _torch_bits(x32: np.ndarray) -> np.ndarray:
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------------------------ the stored values
def test_load_gallery_values(tmp_path):
    rng = np.random.default_rng(0)
    a = (rng.standard_normal((7, 16)) * 3).astype(np.float32)
    a[2] = 0                                                       # an all-zero row stays zero
    a[3] *= 1e-20                                                  # norm below 1e-12: divided by 1e-12
    np.save(tmp_path / "g32.npy", a)
    np.save(tmp_path / "g16.npy", a.astype(np.float16))
    dot = load_gallery(tmp_path / "g32.npy", 16, "dot")
    assert dot.dtype == np.uint16 and dot.shape == (7, 16) and dot.flags.c_contiguous
    assert np.array_equal(dot, _torch_bits(a))                     # torch's round-to-nearest-even
    cos = load_gallery(tmp_path / "g32.npy", 16, "cosine")
    x = a.astype(np.float64)
    want = (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    assert np.array_equal(cos, _torch_bits(want))
    assert (cos[2] == 0).all() and np.abs(np.linalg.norm(bf16_to_f64(cos[[0, 1, 4, 5, 6]]), axis=1) - 1).max() < 2e-3
    assert np.array_equal(bf16_to_f64(cos[3]), bf16_to_f64(_torch_bits((x[3] / 1e-12).astype(np.float32))))
    h = a.astype(np.float16)
    assert np.array_equal(load_gallery(tmp_path / "g16.npy", 16, "dot"), _torch_bits(h.astype(np.float32)))
    # a tie to even that plain truncation or round-half-up would get wrong: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    t = np.array([[1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8] + [0] * 14], np.float32)
    np.save(tmp_path / "tie.npy", t)
    assert load_gallery(tmp_path / "tie.npy", 16, "dot")[0, :2].tolist() == [0x3F80, 0x3F82]


def test_load_gallery_refusals(tmp_path):
    ok = np.ones((3, 16), np.float32)
    cases = {"wrongf": (ok[:, :8], "feature count"), "ndim": (ok[0], "feature count"),
             "nan": (np.where(np.eye(3, 16) > 0, np.nan, ok).astype(np.float32), "NaN or infinite"),
             "inf": (np.where(np.eye(3, 16) > 0, np.inf, ok).astype(np.float32), "NaN or infinite"),
             "empty": (ok[:0], "no rows"), "f64": (ok.astype(np.float64), "float32 or float16"),
             "int": (ok.astype(np.int32), "float32 or float16"), "big": (ok * 3.4e38, "too large for bf16")}
    for name, (arr, msg) in cases.items():
        np.save(tmp_path / f"{name}.npy", arr)
        with pytest.raises(ValueError, match=rf"{name}\.npy.*{msg}"):
            load_gallery(tmp_path / f"{name}.npy", 16, "dot")
    np.save(tmp_path / "obj.npy", np.array([{"a": 1}], dtype=object), allow_pickle=True)
    with pytest.raises(ValueError, match=r"obj\.npy"):               # pickled data is never loaded
        load_gallery(tmp_path / "obj.npy", 16)
    (tmp_path / "junk.npy").write_bytes(b"not a npy file")
    with pytest.raises(ValueError, match=r"junk\.npy"):
        load_gallery(tmp_path / "junk.npy", 16)
    with pytest.raises(ValueError, match="metric"):
        load_gallery(tmp_path / "wrongf.npy", 8, "l1")


def test_too_many_rows_are_refused(tmp_path, monkeypatch):
    import kdl.serving.similar as S
    assert GALLERY_MAX_N == 1 << 24
    monkeypatch.setattr(S, "GALLERY_MAX_N", 4)
    np.save(tmp_path / "many.npy", np.ones((5, 8), np.float32))
    with pytest.raises(ValueError, match=r"many\.npy.*5 rows exceed"):
        S.load_gallery(tmp_path / "many.npy", 8)


# ------------------------------------------------------------------------------ the rule
def test_similar_rule_ties_and_full_k():
    g = _torch_bits(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], np.float32))
    q = np.array([[2, 1, 0, 0], [0, 0, 0, 0]], np.float32)
    idx, sc = similar_rule(q, g, 5, "dot")                         # K = N: every row, ties by ascending index
    assert idx.dtype == np.int32 and sc.dtype == np.float32
    assert idx.tolist() == [[0, 2, 4, 1, 3], [0, 1, 2, 3, 4]]
    assert sc.tolist() == [[2, 2, 2, 1, 0], [0, 0, 0, 0, 0]]
    idx, sc = similar_rule(q, g, 2, "cosine")                      # the query goes through l2_rule first
    assert idx.tolist() == [[0, 2], [0, 1]]
    assert np.allclose(sc[0], 2 / np.sqrt(5), rtol=1e-6) and (sc[1] == 0).all()
    want = l2_rule(q).astype(np.float64) @ bf16_to_f64(g).T
    assert np.array_equal(sc, np.take_along_axis(want, idx.astype(np.int64), axis=1).astype(np.float32))


# ------------------------------------------------------------------------------ resolution
def _version(tmp_path, meta=None, gallery=None, ids=None, name="synthetic.json", gname="gallery.npy"):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / name).write_text(json.dumps({"seed": 0, **(meta or {})}))
    if gallery is not None:
        np.save(d / gname, gallery)
    if ids is not None:
        (d / "gallery_ids.txt").write_text("".join(i + "\n" for i in ids))
    return d


def _gallery(n=6, f=F, seed=1):
    return np.random.default_rng(seed).standard_normal((n, f)).astype(np.float32)


def test_k_metric_and_ids_resolution(tmp_path):
    assert resolve(_version(tmp_path / "none"), F) is None                       # no gallery: no signatures
    assert resolve(_version(tmp_path / "none2", {"similar": {"top_k": 3}}), F) is None
    k, metric, bits, ids = resolve(_version(tmp_path / "a", gallery=_gallery()), F)
    assert (k, metric, ids) == (5, "cosine", ["0", "1", "2", "3", "4", "5"])
    assert np.array_equal(bits, load_gallery(tmp_path / "a" / "1" / "gallery.npy", F, "cosine"))
    d = _version(tmp_path / "b", {"similar": {"top_k": 3, "metric": "dot"}}, _gallery(), list("abcdef"))
    k, metric, bits, ids = resolve(d, F)
    assert (k, metric, ids) == (3, "dot", list("abcdef"))
    assert np.array_equal(bits, _torch_bits(_gallery()))
    assert resolve(d, F, 2)[0] == 2 and resolve(d, F, 4)[0] == 4                 # file < flag
    assert resolve(d, F, 32)[0] == 6                                             # clipped to N
    d = _version(tmp_path / "c", {"similar": {"gallery": "items.npy"}}, _gallery(2), name="kdl_model.json",
                 gname="items.npy")
    assert resolve(d, F)[0] == 2
    assert config_from_args(["--similar_top_k", "7"], env={}).similar_top_k == 7
    assert config_from_args([], env={"KDL_SIMILAR_TOP_K": "9"}).similar_top_k == 9
    assert config_from_args(["--similar_top_k", "7"], env={"KDL_SIMILAR_TOP_K": "9"}).similar_top_k == 7
    assert config_from_args([], env={}).similar_top_k is None


def test_a_wrong_gallery_fails_the_load(tmp_path):
    bad = {"wrongf": dict(gallery=_gallery(3, 768)), "nan": dict(gallery=np.full((2, F), np.nan, np.float32)),
           "empty": dict(gallery=_gallery(0)), "ids": dict(gallery=_gallery(3), ids=["a", "b"])}
    match = {"wrongf": r"gallery\.npy.*feature count", "nan": r"gallery\.npy.*NaN", "empty": r"gallery\.npy.*no rows",
             "ids": r"gallery_ids\.txt.*2 ids for the 3 rows"}
    for name, kw in bad.items():
        with pytest.raises(ValueError, match=match[name]):
            load_version_dir(_version(tmp_path / name, **kw), synthetic=True)
    for i, spec in enumerate(({"top_k": 0}, {"top_k": 33}, {"top_k": "5"}, {"top_k": True}, {"metric": "l2"},
                              {"gallery": "../x.npy"}, "cosine")):
        with pytest.raises(ValueError, match=r"synthetic\.json.*similar"):
            load_version_dir(_version(tmp_path / f"spec{i}", {"similar": spec}, _gallery()), synthetic=True)
    with pytest.raises(ValueError, match=r"missing\.npy.*does not exist"):
        load_version_dir(_version(tmp_path / "missing", {"similar": {"gallery": "missing.npy"}}), synthetic=True)
    with pytest.raises(ValueError, match="top_k"):
        load_version_dir(_version(tmp_path / "flag", gallery=_gallery()), synthetic=True, similar_top_k=40)


def test_signatures_exist_only_with_a_gallery(tmp_path):
    plain = load_version_dir(_version(tmp_path / "plain"), synthetic=True)
    assert not any(n in plain.signatures for n in SIGS) and plain.gallery is None and plain.similar_k == 0
    assert {"serving_default", "serving_uint8", "classify", "embed", "embed_bytes"} <= set(plain.signatures)
    src = load_version_dir(_version(tmp_path / "g", {"similar": {"top_k": 4}}, _gallery(), list("abcdef")),
                           synthetic=True)
    assert set(plain.signatures) | set(SIGS) == set(src.signatures)
    for n in set(plain.signatures):                                                # the others are as they were
        assert src.signatures[n] == plain.signatures[n]
    for n in SIGS:
        sig = src.signatures[n]
        assert sig.similar and sig.top_k == 4 and sig.embed == "" and sig.input_dtype != P.DT_FLOAT
        assert sig.output_specs() == (("ids", P.DT_STRING, (-1, 4)), ("scores", P.DT_FLOAT, (-1, 4)))
    assert src.signatures["similar"].input_shape == (-1, 299, 299, 3)
    assert src.gallery.shape == (6, F) and src.gallery_ids == list("abcdef") and src.similar_metric == "cosine"
    src = load_version_dir(_version(tmp_path / "v", {"model": "vit_b16"}, _gallery(3, 768)), synthetic=True)
    assert src.similar_k == 3 and src.signatures["similar"].input_shape == (-1, 224, 224, 3)


# ------------------------------------------------------------------------------ a CPU server
def _free_port() -> int:
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _server(base, device, **kw):
    cfg = ServerConfig(port=0, rest_api_port=_free_port(), model_name="clothing-model", model_base_path=str(base),
                       device=device, host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend="python",
                       batching=BatchingParams(max_batch_size=4, batch_timeout_micros=500,
                                               allowed_batch_sizes=[1, 2, 4]), **kw)
    return ModelServer(cfg).start(block_until_loaded=True)


N_ITEMS, K = 12, 4
IDS = [f"item-{i:02d}" for i in range(N_ITEMS)]


@pytest.fixture(scope="module")
def pixels():
    img = Image.open(PANTS).convert("RGB")
    return np.stack([pp.to_uint8(img), np.random.default_rng(3).integers(0, 256, (299, 299, 3), dtype=np.uint8)])


@pytest.fixture(scope="module")
def repo(tmp_path_factory, pixels):
    """A synthetic Xception version whose gallery holds the fp32 oracle's own rows of the two test
    images at rows 7 and 2, twice each (rows 9 and 5 are copies: ties), and random rows elsewhere."""
    base = tmp_path_factory.mktemp("similar") / "clothing-model"
    info = registry.get("xception")
    rows = info.feature_oracle(info.init_params(seed=5), torch.from_numpy(pixels)).numpy()
    gal = np.abs(_gallery(N_ITEMS, F, 11))
    gal[7], gal[9], gal[2], gal[5] = rows[0], rows[0], rows[1], rows[1]
    _version(base, {"seed": 5, "similar": {"top_k": K}}, gal, IDS)
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
def expected(server, pixels):
    """similar_rule over the served version's own feature_oracle rows and stored gallery."""
    src = server.manager.get("clothing-model", None, None).source
    rows = registry.get("xception").feature_oracle(src.params, torch.from_numpy(pixels)).numpy()
    idx, sc = similar_rule(rows, src.gallery, K, "cosine")
    return [[IDS[j] for j in r] for r in idx], sc


def _answer(resp, n):
    ids, sc = resp.outputs["ids"], resp.outputs["scores"]
    assert sorted(resp.outputs) == ["ids", "scores"] and ids.dtype == P.DT_STRING and sc.dtype == P.DT_FLOAT
    for t in (ids, sc):
        assert [d.size for d in t.tensor_shape.dim] == [n, K]
    names = [v.decode() for v in ids.string_val]
    return [names[i * K:(i + 1) * K] for i in range(n)], np.asarray(sc.float_val, np.float32).reshape(n, K)


def _post(url, body):
    data = json.dumps(body).encode()
    try:
        with urllib.request.urlopen(urllib.request.Request(url, data=data, method="POST"), timeout=120) as r:
            return r.status, json.load(r)
    except urllib.error.HTTPError as e:
        return e.code, json.load(e)


def test_cpu_server_follows_the_rule(server, stub, pixels, expected):
    ids, sc = _answer(stub.Predict(make_request(pixels, signature="similar", input_key="images"), timeout=120), 2)
    assert ids == expected[0] and np.allclose(sc, expected[1], rtol=1e-5, atol=1e-6)
    assert ids[0][:2] == ["item-07", "item-09"] and ids[1][:2] == ["item-02", "item-05"]    # ties by row index
    assert sc[0, 0] == sc[0, 1] and abs(sc[0, 0] - 1) < 5e-3                                # bf16 storage
    r = server.manager.get("clothing-model", None, None).runner("similar")
    assert r.out_cols == F and not r.gpu and r.sig.top_k == K
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model:predict"
    st, out = _post(url, {"signature_name": "similar", "instances": pixels[:1].tolist()})
    assert st == 200, out
    assert out["predictions"][0]["ids"] == ids[0] and np.allclose(out["predictions"][0]["scores"], sc[0], rtol=1e-5)
    st, out = _post(url, {"signature_name": "similar", "inputs": {"images": pixels[:1].tolist()}})
    assert st == 200 and out["outputs"]["ids"] == [ids[0]], out
    md = json.load(urllib.request.urlopen(f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model/metadata"))
    outs = md["metadata"]["signature_def"]["signatureDef"]["similar_bytes"]["outputs"]
    assert sorted(outs) == ["ids", "scores"]


def test_the_three_signatures_agree(stub, pixels):
    img = Image.open(PANTS).convert("RGB")
    b = io.BytesIO()
    img.save(b, "PNG")                                              # a PNG decodes exactly
    a = _answer(stub.Predict(make_request([b.getvalue()], signature="similar_bytes", input_key="image_bytes"),
                             timeout=120), 1)
    c = _answer(stub.Predict(make_request(np.asarray(img, np.uint8)[None], signature="similar_image",
                                          input_key="images"), timeout=120), 1)
    d = _answer(stub.Predict(make_request(pixels[:1], signature="similar", input_key="images"), timeout=120), 1)
    assert a[0] == c[0] == d[0] and a[0][0][0] == "item-07"
    assert np.allclose(a[1], d[1], rtol=1e-6) and np.allclose(c[1], d[1], rtol=1e-6)


def test_output_filter_and_counter(stub, pixels):
    from kdl.serving.metrics import METRICS
    before = METRICS.snapshot()["counters"]
    req = make_request(pixels[:1], signature="similar", input_key="images")
    req.output_filter.append("scores")
    assert list(stub.Predict(req, timeout=120).outputs) == ["scores"]
    after = METRICS.snapshot()["counters"]
    key = "kdl_similar_total{signature=similar}"
    assert after.get(key, 0) - before.get(key, 0) == 1
    req = make_request(pixels[:1], signature="similar", input_key="images")
    req.output_filter.append("classes")
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(req, timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT


def test_flag_overrides_k(repo, pixels):
    srv = _server(repo, "cpu", similar_top_k=2)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            resp = PredictionStub(ch).Predict(make_request(pixels[:1], signature="similar", input_key="images"),
                                              timeout=120)
        assert [d.size for d in resp.outputs["ids"].tensor_shape.dim] == [1, 2]
        assert [v.decode() for v in resp.outputs["ids"].string_val] == ["item-07", "item-09"]
    finally:
        srv.stop(0)


def test_a_version_without_a_gallery_serves_as_before(tmp_path):
    base = tmp_path / "clothing-model"
    _version(base, {"seed": 5})
    srv = _server(base, "null")
    try:
        s = srv.manager.get("clothing-model", None, None)
        assert not any(n in s.signatures for n in SIGS)
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            x = np.zeros((1, 299, 299, 3), np.uint8)
            ok = PredictionStub(ch).Predict(make_request(x, signature="serving_uint8", input_key="images"), timeout=60)
            assert len(ok.outputs["dense_7"].float_val) == 10
            with pytest.raises(grpc.RpcError) as e:
                PredictionStub(ch).Predict(make_request(x, signature="similar", input_key="images"), timeout=30)
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    finally:
        srv.stop(0)


# ------------------------------------------------------------------------------ gateway
class _Rpc(grpc.RpcError):
    def __init__(self, code):
        self._code = code

    def code(self):
        return self._code

    def details(self):
        return "stub"


class _Channel:
    """A channel whose Predict answers with a fixed response, or raises a fixed status."""

    def __init__(self, answer):
        self.answer, self.requests = answer, []

    def unary_unary(self, method, request_serializer=None, response_deserializer=None):
        def call(req, timeout=None):
            self.requests.append(req)
            if isinstance(self.answer, grpc.StatusCode):
                raise _Rpc(self.answer)
            return self.answer
        return call


def _similar_response():
    r = P.PredictResponse()
    r.outputs["ids"].dtype = P.DT_STRING
    r.outputs["ids"].string_val.extend([b"shirt-3.jpg", b"17"])
    r.outputs["scores"].dtype = P.DT_FLOAT
    r.outputs["scores"].float_val.extend([0.9375, 0.5])
    for key in ("ids", "scores"):
        for d in (1, 2):
            r.outputs[key].tensor_shape.dim.add(size=d)
    return r


@pytest.mark.parametrize("mode,sig,key", [("uint8", "similar", "images"), ("compat", "similar", "images"),
                                          ("raw", "similar_image", "images"), ("bytes", "similar_bytes", "image_bytes")])
def test_gateway_similar_json(monkeypatch, mode, sig, key):
    data = PANTS.read_bytes()
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: data)
    ch = _Channel(_similar_response())
    client = create_app(GatewayConfig({"GATEWAY_MODE": mode}), channel=ch).test_client()
    r = client.post("/similar", json={"url": "http://example.invalid/pants.png"})
    assert r.status_code == 200, r.data
    assert r.get_json() == {"neighbors": [{"id": "shirt-3.jpg", "score": 0.9375}, {"id": "17", "score": 0.5}]}
    req = ch.requests[0]
    assert req.model_spec.signature_name == sig and list(req.inputs) == [key]
    assert req.inputs[key].dtype == (P.DT_STRING if mode == "bytes" else P.DT_UINT8)
    assert process_similar_response(_similar_response()) == [r.get_json()["neighbors"]]


def test_gateway_similar_errors_map_like_embed(monkeypatch):
    data = PANTS.read_bytes()
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: data)
    for code, http in ((grpc.StatusCode.DEADLINE_EXCEEDED, 504), (grpc.StatusCode.INTERNAL, 502),
                       (grpc.StatusCode.INVALID_ARGUMENT, 400), (grpc.StatusCode.UNAVAILABLE, 503)):
        client = create_app(GatewayConfig({"GATEWAY_MODE": "uint8"}), channel=_Channel(code)).test_client()
        got = {p: client.post(p, json={"url": "http://example.invalid/pants.png"}) for p in ("/similar", "/embed")}
        assert got["/similar"].status_code == got["/embed"].status_code == http
        assert got["/similar"].get_json() == got["/embed"].get_json()
    client = create_app(GatewayConfig({"GATEWAY_MODE": "uint8"}), channel=_Channel(_similar_response())).test_client()
    assert client.post("/similar", json={"nope": 1}).status_code == 400
    assert client.post("/similar", data=b"x").status_code == 400

    def broken(url, timeout=10.0):
        raise urllib.error.URLError("no route")
    monkeypatch.setattr(pp, "fetch", broken)
    assert client.post("/similar", json={"url": "http://example.invalid/x.png"}).status_code == 502


# ------------------------------------------------------------------------------ build-gallery
def test_build_gallery_on_the_cpu(tmp_path, capsys):
    from kdl import cli
    d = _version(tmp_path / "clothing-model", {"seed": 5})
    images = tmp_path / "images"
    images.mkdir()
    img = Image.open(PANTS).convert("RGB")
    img.resize((64, 80)).save(images / "b-pants.png")
    img.resize((50, 40)).transpose(Image.FLIP_LEFT_RIGHT).save(images / "a-mirror.png")
    assert cli.main(["build-gallery", str(d), str(images), "--device", "cpu", "--batch", "2"]) == 0
    assert (d / "gallery_ids.txt").read_text() == "a-mirror.png\nb-pants.png\n"
    raw = np.load(d / "gallery.npy", allow_pickle=False)
    assert raw.dtype == np.float32 and raw.shape == (2, F) and np.isfinite(raw).all()
    bits = load_gallery(d / "gallery.npy", F, "cosine")
    assert bits.shape == (2, F)
    src = load_version_dir(d, synthetic=True)
    assert src.gallery_ids == ["a-mirror.png", "b-pants.png"] and src.similar_k == 2
    # the rows are the version's own raw embed rows: the resized pixels through the fp32 oracle
    px = np.stack([pp.apply_spec_pil(Image.open(images / n).convert("RGB"), src.preprocess, 299)
                   for n in ("a-mirror.png", "b-pants.png")])
    want = registry.get("xception").feature_oracle(src.params, torch.from_numpy(px)).numpy()
    assert np.allclose(raw, want, rtol=1e-5, atol=1e-6)
