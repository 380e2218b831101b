"""The overlay signatures without a GPU: the integer rule against Pillow, the colour tables and
blend pins, config errors, the signatures of the four families, a ``--device cpu`` server (gRPC and
REST), a ``--device null`` server and the gateway's /overlay."""
import base64
import io
import itertools
import json
import socket
import urllib.error
import urllib.request
from pathlib import Path

import grpc
import numpy as np
import pytest
from PIL import Image

from kdl.engine.base import Overlay, overlay_words, pack_overlay, unpack_overlay
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request, png_bytes, process_overlay_response
from kdl.serving import overlay as O
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

PANTS = Path(__file__).parent / "data" / "pants.png"
SIGS = ("overlay", "overlay_image", "overlay_bytes")
KEYS = ("classes", "scores", "heatmap", "overlay")
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
SHAPES = [(10, 299), (7, 224), (14, 224), (19, 600), (19, 19), (19, 20), (3, 17)]


# ------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("flt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("n,S", SHAPES)
def test_upsample_equals_pillow(n, S, flt):
    rng = np.random.default_rng(n * 1000 + S)
    for q in (rng.integers(0, 256, (n, n), dtype=np.uint8), np.full((n, n), 255, np.uint8),
              np.eye(n, dtype=np.uint8) * 255):
        ref = np.asarray(Image.fromarray(q, "L").resize((S, S), PIL_FILTER[flt]))
        assert np.array_equal(O.upsample(q, S, flt), ref)


def test_upsample_of_a_rectangular_map_and_refusal_of_a_downscale():
    q = np.random.default_rng(1).integers(0, 256, (5, 9), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(q, "L").resize((31, 31), Image.BILINEAR))
    assert np.array_equal(O.upsample(q, 31, "bilinear"), ref)
    with pytest.raises(ValueError, match="upsample"):
        O.upsample(q, 8, "bilinear")
    with pytest.raises(ValueError, match="upsample"):
        O.overlay_rule(np.zeros((8, 8, 3), np.uint8), np.zeros((5, 9), np.float32))


def test_colour_tables():
    jet, hot, gray = (O.colormap_table(n) for n in ("jet", "hot", "gray"))
    for t in (jet, hot, gray):
        assert t.shape == (256, 3) and t.dtype == np.uint8 and t.flags.c_contiguous
    assert tuple(jet[0]) == (0, 0, 128) and tuple(jet[255]) == (128, 0, 0)
    u = np.arange(256)
    for c, k in enumerate((3, 2, 1)):
        assert np.array_equal(jet[:, c], np.clip(383 - np.abs(4 * u - 255 * k), 0, 255))
    for c, k in enumerate((0, 1, 2)):
        assert np.array_equal(hot[:, c], np.clip(3 * u - 255 * k, 0, 255))
    assert tuple(hot[0]) == (0, 0, 0) and tuple(hot[85]) == (255, 0, 0) and tuple(hot[255]) == (255, 255, 255)
    assert np.array_equal(gray, np.stack([u, u, u], 1))
    with pytest.raises(ValueError, match="colormap"):
        O.colormap_table("viridis")


def test_quantisation():
    f = np.float32
    x = np.array([np.nan, -1.0, -0.0, 0.0, 1.0, 1.5, np.inf, -np.inf, 0.5, 1e-9], f)
    assert O.quantise(x).tolist() == [0, 0, 0, 0, 255, 255, 255, 0, 128, 0]
    # products that land exactly on k + 0.5 go to the even k: x = (k + 0.5) / 255 is rarely exact in
    # fp32, so look for inputs whose fp32 product IS k + 0.5
    ties = []
    for k in range(255):
        x0 = f(k + 0.5) / f(255)
        for cand in (x0, np.nextafter(x0, f(0)), np.nextafter(x0, f(1))):
            if f(cand) * f(255) == f(k + 0.5):
                ties.append((f(cand), k))
                break
    assert len(ties) > 50
    for x1, k in ties:
        assert int(O.quantise(np.array([x1], f))[0]) == (k if k % 2 == 0 else k + 1), (x1, k)
    assert O.quantise(np.array([[0.25]], f)).dtype == np.uint8


def test_blend_endpoints_and_formula():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (17, 17, 3), dtype=np.uint8)
    heat = rng.random((3, 3), dtype=np.float32)
    u = O.upsample(O.quantise(heat), 17, "bilinear")
    for cmap, flt in itertools.product(O.COLORMAPS, ("bilinear", "bicubic")):
        tab = O.colormap_table(cmap)
        uu = O.upsample(O.quantise(heat), 17, flt)
        for blend in O.BLENDS:                                     # a = 0: the photograph
            assert np.array_equal(O.overlay_rule(img, heat, Overlay(cmap, 0.0, blend, flt)), img)
        assert np.array_equal(O.overlay_rule(img, heat, Overlay(cmap, 1.0, "flat", flt)), tab[uu])   # a = 256, flat
    for alpha, blend in itertools.product((1 / 256, 0.5, 0.3, 1.0), O.BLENDS):
        a = int(round(alpha * 256))
        ap = ((a * u.astype(np.int64) + 127) // 255 if blend == "heat" else np.full(u.shape, a))[..., None]
        want = (img.astype(np.int64) * (256 - ap) + O.colormap_table("jet")[u].astype(np.int64) * ap + 128) >> 8
        got = O.overlay_rule(img, heat, Overlay("jet", alpha, blend, "bilinear"))
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    cold = O.overlay_rule(img, np.zeros((3, 3), np.float32), Overlay("jet", 1.0, "heat"))
    assert np.array_equal(cold, img)                              # heat-weighted: a cold map leaves the photograph
    assert O.alpha_fixed(0) == 0 and O.alpha_fixed(1) == 256 and O.alpha_fixed(0.5) == 128
    for bad in (-0.01, 1.01):
        with pytest.raises(ValueError):
            O.overlay_rule(img, heat, Overlay("jet", bad))
    with pytest.raises(ValueError):
        O.overlay_rule(img, heat, Overlay(blend="multiply"))
    with pytest.raises(ValueError):
        O.overlay_rule(img, heat, Overlay(filter="lanczos"))
    with pytest.raises(ValueError):
        O.overlay_rule(img.astype(np.float32), heat)


def test_row_pack_and_unpack_round_trip():
    rng = np.random.default_rng(0)
    for S in (5, 6, 17):                                          # S*S*3 % 4 = 3, 0, 3
        classes = np.array([3, 2 ** 31 - 1], np.int32)
        scores = rng.random(2, dtype=np.float32)
        heat = rng.random((2, 3, 4), dtype=np.float32)
        pics = rng.integers(0, 256, (2, S, S, 3), dtype=np.uint8)
        pics[0, 0, 0] = (0, 0, 0x80)
        pics[0, 0, 1, 0] = 0x7F                                   # bytes 2..3: a signalling-NaN pattern among the words
        rows = pack_overlay(classes, scores, heat, pics)
        assert rows.dtype == np.float32 and rows.shape == (2, 2 + 12 + overlay_words(S))
        c, s, h, p = unpack_overlay(rows, 3, 4, S)
        assert np.array_equal(c, classes) and np.array_equal(s, scores) and np.array_equal(h, heat)
        assert p.dtype == np.uint8 and np.array_equal(p, pics)
        c, s, h, p = O.unpack_rows(rows.copy(), 3, 4, S)
        assert np.array_equal(p, pics) and np.array_equal(c, classes)
    with pytest.raises(AssertionError):
        unpack_overlay(rows, 3, 4, 16)


# ------------------------------------------------------------------------------ config, signatures
def _version(tmp_path, meta=None):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, **(meta or {})}))
    return d


def test_config_block_flags_and_errors(tmp_path):
    assert load_version_dir(_version(tmp_path / "d"), synthetic=True).overlay == Overlay("jet", 0.5, "heat", "bilinear")
    d = _version(tmp_path / "c", {"overlay": {"colormap": "hot", "alpha": 0.25, "blend": "flat", "filter": "bicubic"}})
    assert load_version_dir(d, synthetic=True).overlay == Overlay("hot", 0.25, "flat", "bicubic")
    src = load_version_dir(d, synthetic=True, overlay_colormap="gray", overlay_alpha=1.0)
    assert src.overlay == Overlay("gray", 1.0, "flat", "bicubic")
    for i, block in enumerate(({"colormap": "viridis"}, {"alpha": 1.5}, {"alpha": -0.1}, {"alpha": "half"},
                               {"blend": "multiply"}, {"filter": "lanczos"}, {"colour": "jet"}, "jet")):
        d = _version(tmp_path / f"bad{i}", {"overlay": block})
        with pytest.raises(ValueError, match="synthetic.json"):
            load_version_dir(d, synthetic=True)
    with pytest.raises(ValueError, match="overlay_alpha"):
        load_version_dir(_version(tmp_path / "f"), synthetic=True, overlay_alpha=2.0)
    with pytest.raises(ValueError, match="overlay_colormap"):
        load_version_dir(_version(tmp_path / "g"), synthetic=True, overlay_colormap="viridis")


def test_flags_reach_the_config(monkeypatch):
    from kdl.serving.config import config_from_args as parse_args
    cfg = parse_args(["--model_name", "m", "--model_base_path", "/tmp/m", "--overlay_colormap", "hot",
                      "--overlay_alpha", "0.75"])
    assert cfg.overlay_colormap == "hot" and cfg.overlay_alpha == 0.75
    monkeypatch.setenv("KDL_OVERLAY_COLORMAP", "gray")
    monkeypatch.setenv("KDL_OVERLAY_ALPHA", "0.125")
    cfg = parse_args(["--model_name", "m", "--model_base_path", "/tmp/m"])
    assert cfg.overlay_colormap == "gray" and cfg.overlay_alpha == 0.125


@pytest.mark.parametrize("model,hw,S,rollout", [("xception", (10, 10), 299, False), ("resnet50", (7, 7), 224, False),
                                                ("efficientnet_b7", (19, 19), 600, False),
                                                ("vit_b16", (14, 14), 224, True)])
def test_signatures_of_the_four_families(tmp_path, model, hw, S, rollout):
    meta = {} if model == "xception" else {"model": model}
    src = load_version_dir(_version(tmp_path, meta), synthetic=True)
    h, w = hw
    for name in SIGS:
        sig = src.signatures[name]
        assert sig.explain == hw and sig.overlay == S and sig.rollout is rollout
        assert sig.input_dtype != P.DT_FLOAT and not sig.top_k and not sig.embed
        assert sig.outputs == (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)),
                               ("heatmap", P.DT_FLOAT, (-1, h, w)), ("overlay", P.DT_UINT8, (-1, S, S, 3)))
    assert src.signatures["overlay"].input_shape == (-1, S, S, 3)
    assert src.signatures["overlay_image"].input_shape == src.signatures["serving_image"].input_shape
    assert src.signatures["overlay_bytes"].input_key == src.signatures["serving_bytes"].input_key
    # every earlier signature is what it is without the overlay code: none carries the mark, and the
    # method's own trio still has its three outputs
    method = ("attention", "attention_image", "attention_bytes") if rollout else ("explain", "explain_image",
                                                                                "explain_bytes")
    for name, sig in src.signatures.items():
        if name not in SIGS:
            assert sig.overlay == 0, name
    for name in method:
        assert [o[0] for o in src.signatures[name].outputs] == ["classes", "scores", "heatmap"]
        assert src.signatures[name].explain == hw
    for name in ("serving_default", "serving_uint8", "serving_image", "serving_bytes", "classify", "embed"):
        assert name in src.signatures and src.signatures[name].explain == ()


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


SPEC = Overlay("hot", 0.75, "heat", "bicubic")


@pytest.fixture(scope="module")
def repo(tmp_path_factory):
    base = tmp_path_factory.mktemp("overlay") / "clothing-model"
    _version(base, {"seed": 5, "overlay": {"colormap": "hot", "alpha": 0.75, "filter": "bicubic"}})
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


def _answer(resp, n=1, keys=KEYS, S=299):
    assert sorted(resp.outputs) == sorted(keys)
    out = {}
    if "classes" in keys:
        t = resp.outputs["classes"]
        assert t.dtype == P.DT_STRING and [d.size for d in t.tensor_shape.dim] == [n, 1]
        out["classes"] = [v.decode() for v in t.string_val]
    if "scores" in keys:
        t = resp.outputs["scores"]
        assert t.dtype == P.DT_FLOAT and [d.size for d in t.tensor_shape.dim] == [n, 1]
        out["scores"] = np.asarray(t.float_val, np.float32)
    if "heatmap" in keys:
        t = resp.outputs["heatmap"]
        assert t.dtype == P.DT_FLOAT and [d.size for d in t.tensor_shape.dim] == [n, 10, 10]
        out["heatmap"] = np.asarray(t.float_val, np.float32).reshape(n, 10, 10)
    if "overlay" in keys:
        t = resp.outputs["overlay"]
        assert t.dtype == P.DT_UINT8 and [d.size for d in t.tensor_shape.dim] == [n, S, S, 3]
        out["overlay"] = np.frombuffer(t.tensor_content, np.uint8).reshape(n, S, S, 3)
    return out


def _inputs(jpeg):
    img = pp.load_image(jpeg)
    return {"overlay": (pp.to_uint8(img)[None], "images"), "overlay_image": (np.asarray(img, np.uint8)[None], "images"),
            "overlay_bytes": ([jpeg], "image_bytes")}


@pytest.fixture(scope="module")
def answers(stub, jpeg):
    """One JPEG through the three overlay signatures and through the three explain signatures."""
    got, exp = {}, {}
    for name, (x, key) in _inputs(jpeg).items():
        got[name] = _answer(stub.Predict(make_request(x, signature=name, input_key=key), timeout=300))
        r = stub.Predict(make_request(x, signature=name.replace("overlay", "explain"), input_key=key), timeout=300)
        exp[name] = (r.outputs["classes"].string_val[0].decode(), np.asarray(r.outputs["scores"].float_val, np.float32),
                     np.asarray(r.outputs["heatmap"].float_val, np.float32).reshape(1, 10, 10))
    return got, exp


def test_three_signatures_equal_explain_and_the_rule(server, answers, jpeg):
    got, exp = answers
    src = server.manager.get("clothing-model", None, None).source
    assert src.overlay == SPEC
    # the served preprocess result of each signature: the gateway's own uint8 resize for the pixels
    # signature, the version's spec (NEAREST) for the other two
    img = pp.load_image(jpeg)
    fed = {"overlay": pp.to_uint8(img), "overlay_image": pp.to_uint8(img), "overlay_bytes": pp.to_uint8(img)}
    for name in SIGS:
        a, (label, score, heat) = got[name], exp[name]
        assert a["classes"] == [label], name
        assert np.array_equal(a["scores"], score) and np.array_equal(a["heatmap"], heat), name
        assert np.array_equal(a["overlay"][0], O.overlay_rule(fed[name], a["heatmap"][0], SPEC)), name
        assert not np.array_equal(a["overlay"][0], fed[name])     # the heat is on it


def test_every_output_filter_subset_and_the_counter(stub, answers, jpeg):
    from kdl.serving.metrics import METRICS
    got, _ = answers
    x, key = _inputs(jpeg)["overlay"]
    before = METRICS.snapshot()["counters"]
    n = 0
    for r in range(1, 5):
        for keys in itertools.combinations(KEYS, r):
            req = make_request(x, signature="overlay", input_key=key)
            req.output_filter.extend(keys)
            a = _answer(stub.Predict(req, timeout=300), keys=keys)
            n += 1
            for k in keys:
                assert np.array_equal(a[k], got["overlay"][k]) if k != "classes" else a[k] == got["overlay"][k]
    after = METRICS.snapshot()["counters"]
    key_m = "kdl_overlay_total{signature=overlay}"
    assert after.get(key_m, 0) - before.get(key_m, 0) == n == 15
    assert after.get("kdl_explain_total{signature=overlay}", 0) == 0
    req = make_request(x, signature="overlay", input_key=key)
    req.output_filter.append("dense_7")
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(req, timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    f32 = x.astype(np.float32) / 127.5 - 1.0                      # the overlay signatures take no f32 input
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(make_request(f32, signature="overlay", input_key="images"), timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT


def test_metadata_and_runner(server, stub):
    req = P.GetModelMetadataRequest()
    req.model_spec.name = "clothing-model"
    req.metadata_field.append("signature_def")
    sdm = P.SignatureDefMap()
    stub.GetModelMetadata(req, timeout=5).metadata["signature_def"].Unpack(sdm)
    for name in SIGS:
        out = sdm.signature_def[name].outputs
        assert sorted(out) == sorted(KEYS)
        assert out["overlay"].dtype == P.DT_UINT8 and [d.size for d in out["overlay"].tensor_shape.dim] == [-1, 299, 299, 3]
        assert out["heatmap"].dtype == P.DT_FLOAT and [d.size for d in out["heatmap"].tensor_shape.dim] == [-1, 10, 10]
        assert out["classes"].dtype == P.DT_STRING and out["scores"].dtype == P.DT_FLOAT
    assert sorted(sdm.signature_def["explain"].outputs) == ["classes", "heatmap", "scores"]
    r = server.manager.get("clothing-model", None, None).runner("overlay")
    assert r.out_cols == 102 + overlay_words(299) and r.sig.explain == (10, 10) and r.sig.overlay == 299
    assert not r.gpu and r.kind == "overlay" and not r.sig.rollout      # no engines on a CPU; Grad-CAM's family


def _post(url, body):
    try:
        with urllib.request.urlopen(urllib.request.Request(url, data=json.dumps(body).encode(), method="POST"),
                                    timeout=300) as r:
            return r.status, json.load(r)
    except urllib.error.HTTPError as e:
        return e.code, json.load(e)


def test_rest_predict_returns_the_same(server, answers, jpeg):
    got, _ = answers
    a = got["overlay"]
    u8 = _inputs(jpeg)["overlay"][0]
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model:predict"
    st, out = _post(url, {"signature_name": "overlay", "instances": u8.tolist()})
    assert st == 200, out
    (one,) = out["predictions"]
    assert sorted(one) == sorted(KEYS)
    assert one["classes"] == a["classes"] and np.allclose(one["scores"], a["scores"], rtol=1e-6)
    assert np.allclose(one["heatmap"], a["heatmap"][0], atol=1e-6)
    assert np.array_equal(np.asarray(one["overlay"]), a["overlay"][0]) and isinstance(one["overlay"][0][0][0], int)
    st, out = _post(url, {"signature_name": "overlay", "inputs": {"images": u8.tolist()}})
    assert st == 200, out
    assert out["outputs"]["classes"] == [a["classes"]] and np.allclose(out["outputs"]["heatmap"], a["heatmap"], atol=1e-6)
    assert np.array_equal(np.asarray(out["outputs"]["overlay"]), a["overlay"])
    st, out = _post(url, {"signature_name": "overlay_bytes", "instances": [{"b64": base64.b64encode(jpeg).decode()}]})
    assert st == 200, out
    assert np.array_equal(np.asarray(out["predictions"][0]["overlay"]), got["overlay_bytes"]["overlay"][0])


def test_null_server_returns_zero_rows(repo):
    px = np.random.default_rng(3).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)
    srv = _server(repo, "null")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            a = _answer(PredictionStub(ch).Predict(make_request(px, signature="overlay", input_key="images"),
                                                   timeout=60), 2)
        src = srv.manager.get("clothing-model", None, None).source
    finally:
        srv.stop(0)
    assert a["classes"] == [src.labels[0]] * 2 and (a["scores"] == 0).all() and (a["heatmap"] == 0).all()
    assert (a["overlay"] == 0).all()


# ------------------------------------------------------------------------------ gateway
@pytest.mark.parametrize("mode", ["uint8", "bytes", "raw"])
def test_gateway_overlay(server, answers, jpeg, monkeypatch, mode):
    got, _ = answers
    a = got[{"bytes": "overlay_bytes", "raw": "overlay_image"}.get(mode, "overlay")]
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        c = create_app(GatewayConfig({"GATEWAY_MODE": mode}), channel=ch).test_client()
        r = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg"})
        assert r.status_code == 200, r.data
        assert r.mimetype == "image/png" and r.data[:8] == b"\x89PNG\r\n\x1a\n"
        pic = Image.open(io.BytesIO(r.data))
        assert pic.mode == "RGB" and np.array_equal(np.asarray(pic), a["overlay"][0])
        assert r.headers["X-KDL-Label"] == a["classes"][0]
        assert np.isclose(float(r.headers["X-KDL-Score"]), a["scores"][0], rtol=1e-6)
        r = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg", "format": "json"})
        assert r.status_code == 200, r.data
        out = r.get_json()
        assert sorted(out) == ["heatmap", "label", "png", "score"]
        assert out["label"] == a["classes"][0] and np.allclose(out["heatmap"], a["heatmap"][0], atol=1e-6)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(base64.b64decode(out["png"])))), a["overlay"][0])
        assert c.post("/overlay", json={"nope": 1}).status_code == 400
        assert c.post("/overlay", json={"url": "http://example.invalid/x.jpg", "format": "gif"}).status_code == 400

        def gone(url, timeout=10.0):
            raise urllib.error.URLError("no route")
        monkeypatch.setattr(pp, "fetch", gone)
        assert c.post("/overlay", json={"url": "http://example.invalid/pants.jpg"}).status_code == 502


def test_gateway_maps_a_model_server_error_to_502(jpeg, monkeypatch):
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    with grpc.insecure_channel(f"127.0.0.1:{_free_port()}") as ch:         # nothing listens there
        c = create_app(GatewayConfig({"GATEWAY_MODE": "bytes", "GATEWAY_TIMEOUT": "2"}), channel=ch).test_client()
        r = c.post("/overlay", json={"url": "http://example.invalid/pants.jpg"})
    assert r.status_code in (502, 503, 504) and "error" in r.get_json()


def test_png_writer_and_response_parser():
    rng = np.random.default_rng(4)
    for shape in ((1, 1, 3), (5, 7, 3), (64, 33, 3)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        pic = Image.open(io.BytesIO(png_bytes(a)))
        assert pic.mode == "RGB" and pic.size == (shape[1], shape[0]) and np.array_equal(np.asarray(pic), a)
    resp = P.PredictResponse()
    resp.outputs["classes"].string_val.extend([b"a", b"b"])
    resp.outputs["scores"].float_val.extend([0.5, 0.25])
    resp.outputs["heatmap"].float_val.extend(np.arange(8, dtype=np.float32).tolist())
    for d in (2, 2, 2):
        resp.outputs["heatmap"].tensor_shape.dim.add(size=d)
    pics = rng.integers(0, 256, (2, 3, 3, 3), dtype=np.uint8)
    resp.outputs["overlay"].tensor_content = pics.tobytes()
    for d in pics.shape:
        resp.outputs["overlay"].tensor_shape.dim.add(size=d)
    out = process_overlay_response(resp)
    assert [o["label"] for o in out] == ["a", "b"] and np.array_equal(out[1]["picture"], pics[1])
    assert out[0]["heatmap"] == [[0.0, 1.0], [2.0, 3.0]]


def test_smoke_tool_writes_the_file(server, jpeg, tmp_path, monkeypatch):
    """tools/smoke_overlay.py against a gateway: here the gateway's test client stands in for HTTP."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("smoke_overlay", Path(__file__).parent.parent / "tools" / "smoke_overlay.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = tmp_path / "pants.jpg"
    src.write_bytes(jpeg)
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        c = create_app(GatewayConfig({"GATEWAY_MODE": "bytes"}), channel=ch).test_client()

        def post(url, body, timeout=60.0):
            r = c.post(url[url.index("/overlay"):], json=body)
            return r.status_code, dict(r.headers), r.data
        monkeypatch.setattr(mod, "post_json", post)
        out = tmp_path / "x.png"
        assert mod.main(["--gateway", "http://gw.invalid:9696", "--file", str(src), "--out", str(out)]) == 0
    assert np.asarray(Image.open(out)).shape == (299, 299, 3)
