"""The attention signatures without a GPU: ``rollout_oracle`` against an independent numpy loop over
the heads, its row-sum and positivity properties, which families get the signatures, the row layout
at 14 x 14, a ``--device cpu`` server (gRPC and REST), a ``--device null`` server and the gateway's
/attention."""
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
import torch.nn.functional as F
from PIL import Image

from kdl.engine import registry
from kdl.engine.base import pack_explain, unpack_explain
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request
from kdl.models import vit as V
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

PANTS = Path(__file__).parent / "data" / "pants.png"
SIGS = ("attention", "attention_image", "attention_bytes")


# ------------------------------------------------------------------------------ the rule
def numpy_rollout(p, x_u8):
    """The definition head by head in float64 numpy. The residual stream is the model's own fp32
    (``V.encoder_layer``); Q and K are formed here from its ln_1 output. -> (R [n, T, T] after the
    last layer, every layer's A^ row sums)."""
    with torch.no_grad():
        x = V.embed(p, V.preprocess(x_u8))
        n, T, D = x.shape
        dh = D // V.HEADS
        r, sums = None, []
        for i in range(V.DEPTH):
            L = f"encoder.layers.encoder_layer_{i}"
            h = F.layer_norm(x, (D,), p[f"{L}.ln_1.weight"], p[f"{L}.ln_1.bias"], V.LN_EPS).double().numpy()
            w = p[f"{L}.self_attention.in_proj_weight"].double().numpy()
            b = p[f"{L}.self_attention.in_proj_bias"].double().numpy()
            mean = np.zeros((n, T, T))
            for hd in range(V.HEADS):
                q = h @ w[hd * dh:(hd + 1) * dh].T + b[hd * dh:(hd + 1) * dh]
                k = h @ w[D + hd * dh:D + (hd + 1) * dh].T + b[D + hd * dh:D + (hd + 1) * dh]
                s = np.einsum("ntd,nud->ntu", q, k) / np.sqrt(dh)
                e = np.exp(s - s.max(axis=2, keepdims=True))
                mean += e / e.sum(axis=2, keepdims=True)
            a = (mean / V.HEADS + np.eye(T)) / 2
            sums.append(a.sum(axis=2))
            r = a if r is None else np.einsum("ntk,nku->ntu", a, r)
            x = V.encoder_layer(p, i, x)
    return r, np.stack(sums)


@pytest.fixture(scope="module")
def case():
    info = registry.get("vit_b16")
    p = info.init_params(0)
    x = torch.randint(0, 256, (2, 224, 224, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    return info, p, x


def test_oracle_equals_the_numpy_head_loop(case):
    """fp32 torch against float64 numpy from the same fp32 residual stream: the scores (|s| < 3 at
    random init) carry a few 1e-7 relative, twelve products of 197 terms with rows summing to 1 a
    few 1e-6 at most; 2e-5 absolute on values in 0..1 is ten times that."""
    info, p, x = case
    k, score, heat = info.rollout_oracle(p, x)
    r, sums = numpy_rollout(p, x)
    want = r[:, 0, 1:] / r[:, 0, 1:].max(axis=1, keepdims=True)
    assert heat.shape == (2, 14, 14) and heat.dtype == torch.float32 and k.dtype == torch.int32
    err = np.abs(heat.numpy().reshape(2, 196) - want).max()
    print(f"max |oracle - numpy| {err:.3e}")
    assert err <= 2e-5
    logits = info.oracle(p, x)
    assert np.array_equal(k.numpy(), logits.argmax(dim=1).numpy())
    assert np.allclose(score.numpy(), torch.softmax(logits, dim=1).max(dim=1).values.numpy(), rtol=1e-5)


def test_rows_sum_to_one_and_the_map_is_positive(case):
    info, p, x = case
    r, sums = numpy_rollout(p, x)
    assert np.abs(sums - 1).max() <= 1e-12                      # every A^: no renormalisation needed
    assert np.abs(r.sum(axis=2) - 1).max() <= 1e-12 and (r > 0).all()
    _, _, heat = info.rollout_oracle(p, x)
    assert (heat > 0).all() and heat.amax(dim=(1, 2)).tolist() == [1.0, 1.0]


def test_registry_sets_the_oracle_for_vit_only():
    for fam in ("vit_b16", "vit_b16_fp8"):
        info = registry.get(fam)
        assert info.rollout_oracle is not None and info.map_size == (14, 14) and info.cam_oracle is None
    for fam in ("xception", "resnet50", "resnet50_bf16", "efficientnet_b7"):
        assert registry.get(fam).rollout_oracle is None and registry.get(fam).cam_oracle is not None


def test_explain_still_refuses_and_points_to_rollout():
    from kdl.engine.vit import ViTEngine
    with pytest.raises(ValueError, match="spatial") as e:
        ViTEngine({}, max_batch=2, device="cpu", explain=True)
    assert "rollout=True" in str(e.value)


# ------------------------------------------------------------------------------ rows
def test_row_pack_and_unpack_round_trip_at_14():
    rng = np.random.default_rng(1)
    classes = np.array([0, 999, 2 ** 31 - 1], np.int32)
    scores, heat = rng.random(3, dtype=np.float32), rng.random((3, 14, 14), dtype=np.float32)
    rows = pack_explain(classes, scores, heat)
    assert rows.dtype == np.float32 and rows.shape == (3, 198)
    c, s, h = unpack_explain(rows, 14, 14)
    assert np.array_equal(c, classes) and np.array_equal(s, scores) and np.array_equal(h, heat)
    from kdl.serving import rollout as RO
    assert np.array_equal(RO.pack_rows(classes, scores, heat).view(np.int32), rows.view(np.int32))
    assert np.array_equal(RO.unpack_rows(rows, 14, 14)[2], heat)


# ------------------------------------------------------------------------------ signatures
def _version(tmp_path, meta=None):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, **(meta or {})}))
    return d


def test_signatures_for_vit_and_none_for_the_cnns(tmp_path):
    for fam in ("vit_b16", "vit_b16_fp8"):
        src = load_version_dir(_version(tmp_path / fam, {"model": fam}), synthetic=True)
        for name in SIGS:
            sig = src.signatures[name]
            assert sig.explain == (14, 14) and sig.rollout and sig.input_dtype != P.DT_FLOAT
            assert not sig.top_k and not sig.embed
            assert [(o[0], o[1], o[2]) for o in sig.outputs] == [
                ("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)), ("heatmap", P.DT_FLOAT, (-1, 14, 14))]
        assert src.signatures["attention"].input_shape == (-1, 224, 224, 3)
        assert not any(n.startswith("explain") for n in src.signatures)
        assert not src.signatures["serving_uint8"].rollout and src.signatures["embed"].explain == ()
    for fam in (None, "resnet50"):
        src = load_version_dir(_version(tmp_path / str(fam), {"model": fam} if fam else None), synthetic=True)
        assert not any(name in src.signatures for name in SIGS)
        assert "explain" in src.signatures and not src.signatures["explain"].rollout


# ------------------------------------------------------------------------------ servers
def _free_port() -> int:
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _server(base, device):
    cfg = ServerConfig(port=0, rest_api_port=_free_port(), model_name="vit", model_base_path=str(base),
                       device=device, host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend="python",
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=500, allowed_batch_sizes=[1, 2]))
    return ModelServer(cfg).start(block_until_loaded=True)


@pytest.fixture(scope="module")
def repo(tmp_path_factory):
    base = tmp_path_factory.mktemp("attention") / "vit"
    _version(base, {"seed": 5, "model": "vit_b16"})
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
    assert sorted(resp.outputs) == ["classes", "heatmap", "scores"]
    cl, sc, hm = resp.outputs["classes"], resp.outputs["scores"], resp.outputs["heatmap"]
    assert cl.dtype == P.DT_STRING and sc.dtype == P.DT_FLOAT and hm.dtype == P.DT_FLOAT
    assert [d.size for d in cl.tensor_shape.dim] == [n, 1] and [d.size for d in sc.tensor_shape.dim] == [n, 1]
    assert [d.size for d in hm.tensor_shape.dim] == [n, 14, 14]
    return ([v.decode() for v in cl.string_val], np.asarray(sc.float_val, np.float32),
            np.asarray(hm.float_val, np.float32).reshape(n, 14, 14))


@pytest.fixture(scope="module")
def answers(server, stub, jpeg):
    """One JPEG through the three signatures, and the oracle's answer for the same pixels."""
    img = pp.load_image(jpeg)
    u8 = pp.to_uint8(img, (224, 224))[None]
    got = {"attention_bytes": _answer(stub.Predict(make_request([jpeg], model_name="vit", signature="attention_bytes",
                                                                input_key="image_bytes"), timeout=300)),
           "attention_image": _answer(stub.Predict(make_request(np.asarray(img, np.uint8)[None], model_name="vit",
                                                                signature="attention_image", input_key="images"),
                                                   timeout=300)),
           "attention": _answer(stub.Predict(make_request(u8, model_name="vit", signature="attention",
                                                          input_key="images"), timeout=300))}
    src = server.manager.get("vit", None, None).source
    k, score, heat = registry.get("vit_b16").rollout_oracle(src.params, torch.from_numpy(u8.copy()))
    return got, (src.labels[int(k[0])], score.numpy(), heat.numpy()), u8


def test_three_signatures_agree_and_equal_the_oracle(answers):
    got, (label, score, heat), _ = answers
    for name in SIGS:
        labels, sc, hm = got[name]
        assert labels == [label], name
        assert np.allclose(sc, score, rtol=1e-5, atol=1e-7), name
        assert np.allclose(hm, heat, rtol=0, atol=1e-6), (name, np.abs(hm - heat).max())
        assert hm.max() == 1.0 and hm.min() > 0.0


def test_metadata_and_runner(server, stub, answers):
    req = P.GetModelMetadataRequest()
    req.model_spec.name = "vit"
    req.metadata_field.append("signature_def")
    sdm = P.SignatureDefMap()
    stub.GetModelMetadata(req, timeout=5).metadata["signature_def"].Unpack(sdm)
    for name in SIGS:
        out = sdm.signature_def[name].outputs
        assert sorted(out) == ["classes", "heatmap", "scores"]
        assert [d.size for d in out["heatmap"].tensor_shape.dim] == [-1, 14, 14]
    assert "explain" not in sdm.signature_def
    r = server.manager.get("vit", None, None).runner("attention")
    assert r.out_cols == 198 and r.sig.explain == (14, 14) and r.kind == "attention"
    assert not r.gpu                                            # no engines on a CPU


def _post(url, body):
    try:
        with urllib.request.urlopen(urllib.request.Request(url, data=json.dumps(body).encode(), method="POST"),
                                    timeout=300) as r:
            return r.status, json.load(r)
    except urllib.error.HTTPError as e:
        return e.code, json.load(e)


def test_rest_predict_returns_the_same(server, answers):
    got, _, u8 = answers
    labels, sc, hm = got["attention"]
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/vit:predict"
    st, out = _post(url, {"signature_name": "attention", "instances": u8.tolist()})
    assert st == 200, out
    (one,) = out["predictions"]
    assert one["classes"] == labels and np.allclose(one["scores"], sc, rtol=1e-5)
    assert np.asarray(one["heatmap"]).shape == (14, 14) and np.allclose(one["heatmap"], hm[0], atol=1e-6)
    st, out = _post(url, {"signature_name": "attention", "inputs": {"images": u8.tolist()}})
    assert st == 200, out
    assert out["outputs"]["classes"] == [labels] and np.allclose(out["outputs"]["heatmap"], hm, atol=1e-6)


def test_output_filter_and_counter(stub, answers):
    from kdl.serving.metrics import METRICS
    _, _, u8 = answers
    before = METRICS.snapshot()["counters"]
    req = make_request(u8, model_name="vit", signature="attention", input_key="images")
    req.output_filter.append("heatmap")
    resp = stub.Predict(req, timeout=300)
    assert list(resp.outputs) == ["heatmap"] and len(resp.outputs["heatmap"].float_val) == 196
    after = METRICS.snapshot()["counters"]
    key, other = "kdl_attention_total{signature=attention}", "kdl_explain_total{signature=attention}"
    assert after.get(key, 0) - before.get(key, 0) == 1 and after.get(other, 0) == before.get(other, 0)
    f32 = u8.astype(np.float32) / 255.0                                     # the attention signatures take no f32 input
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(make_request(f32, model_name="vit", signature="attention", input_key="images"), timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT


def test_null_server_returns_zero_rows(repo):
    px = np.random.default_rng(3).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    srv = _server(repo, "null")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            labels, sc, hm = _answer(PredictionStub(ch).Predict(make_request(px, model_name="vit", signature="attention",
                                                                             input_key="images"), timeout=60), 2)
        src = srv.manager.get("vit", None, None).source
    finally:
        srv.stop(0)
    assert labels == [src.labels[0]] * 2 and (sc == 0).all() and (hm == 0).all()


# ------------------------------------------------------------------------------ gateway
@pytest.mark.parametrize("mode", ["bytes", "raw"])
def test_gateway_attention(server, answers, jpeg, monkeypatch, mode):
    """The two modes in which the model server sizes the image itself (the gateway's own uint8
    preprocessing is Xception's 299 x 299)."""
    got, _, _ = answers
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        app = create_app(GatewayConfig({"GATEWAY_MODE": mode, "MODEL_NAME": "vit"}), channel=ch)
        r = app.test_client().post("/attention", json={"url": "http://example.invalid/pants.jpg"})
        assert r.status_code == 200, r.data
        out = r.get_json()
        assert app.test_client().post("/attention", json={"nope": 1}).status_code == 400
    labels, sc, hm = got[{"bytes": "attention_bytes", "raw": "attention_image"}[mode]]
    assert sorted(out) == ["heatmap", "label", "score"]
    assert out["label"] == labels[0] and np.isclose(out["score"], sc[0], rtol=1e-6)
    assert len(out["heatmap"]) == 14 and all(len(row) == 14 for row in out["heatmap"])
    assert np.allclose(out["heatmap"], hm[0], atol=1e-6)
