"""The palette signatures without a GPU: literal answers of the integer rule, a second implementation in
plain loops, rows and config errors, the signatures with and without the block, a ``--device cpu`` server
(gRPC and REST, by row and by column) and the gateway's /colors."""
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

from kdl.engine.base import Palette
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request, process_palette_response
from kdl.serving import overlay as O
from kdl.serving import palette as PL
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

PANTS = Path(__file__).parent / "data" / "pants.png"
GOLDEN = Path(__file__).parent / "golden" / "outputs"
SIGS = ("palette", "palette_image", "palette_bytes")
KEYS = ("classes", "scores", "colors", "fractions", "names")
UNIFORM3 = Palette(colors=3, weight="uniform")


def flat(S, rgb):
    return np.broadcast_to(np.asarray(rgb, np.uint8), (S, S, 3)).copy()


# ------------------------------------------------------------------------------ the rule: literal answers
def test_flat_picture():
    W, col, n = PL.palette_rule(flat(5, (200, 200, 200)), np.zeros((1, 1), np.float32), UNIFORM3)
    assert W == 375 and col.dtype == np.uint8 and n.dtype == np.uint32
    assert col.tolist() == [[200, 200, 200], [0, 0, 0], [0, 0, 0]] and n.tolist() == [375, 0, 0]


def test_two_tone_picture_checks_both_tie_rules():
    img = np.zeros((4, 4, 3), np.uint8)
    img[:2] = 255
    W, col, n = PL.palette_rule(img, np.zeros((2, 2), np.float32), UNIFORM3)
    assert W == 240
    assert col.tolist() == [[0, 0, 0], [255, 255, 255], [0, 0, 0]] and n.tolist() == [120, 120, 0]


def test_the_uint32_bound_at_1024_white_pixels_a_side():
    W, col, n = PL.palette_rule(flat(1024, (255, 255, 255)), np.zeros((1, 1), np.float32),
                                Palette(colors=1, weight="uniform"))
    assert W == 15728640 and col.tolist() == [[255, 255, 255]] and n.tolist() == [15728640]
    with pytest.raises(ValueError, match="1024"):
        PL.palette_rule(np.zeros((1025, 1025, 3), np.uint8), np.zeros((1, 1), np.float32), UNIFORM3)


def test_three_flat_regions():
    img = np.empty((10, 10, 3), np.uint8)
    img[:5] = (200, 30, 40)
    img[5:8] = (20, 90, 160)
    img[8:] = (250, 250, 5)
    W, col, n = PL.palette_rule(img, np.zeros((3, 3), np.float32), UNIFORM3)
    assert W == 1500
    assert col.tolist() == [[200, 30, 40], [20, 90, 160], [250, 250, 5]] and n.tolist() == [750, 450, 300]


@pytest.mark.parametrize("fill", [0.0, np.nan, -3.0])
def test_a_map_without_weight_answers_zeros(fill):
    img = np.random.default_rng(0).integers(0, 256, (9, 9, 3), dtype=np.uint8)
    W, col, n = PL.palette_rule(img, np.full((3, 3), fill, np.float32), Palette(colors=4))
    assert W == 0 and not col.any() and not n.any() and col.shape == (4, 3) and n.shape == (4,)


# ------------------------------------------------------------------------------ a second implementation
def loops_rule(img, heat, spec):
    """The issue's seven steps in plain Python over pixels and bins; shares only ``overlay.upsample``."""
    S, K, T = img.shape[0], spec.colors, spec.rounds
    if spec.weight == "map":
        u = O.upsample(O.quantise(heat), S, spec.filter)
    hist = {}
    for y in range(S):
        for x in range(S):
            w = int(u[y, x]) >> 4 if spec.weight == "map" else 15
            r, g, b = (int(v) for v in img[y, x])
            e = hist.setdefault((r >> 4) << 8 | (g >> 4) << 4 | (b >> 4), [0, 0, 0, 0])
            e[0] += w
            e[1] += w * r
            e[2] += w * g
            e[3] += w * b
    bins = [(i, e) for i, e in sorted(hist.items()) if e[0] > 0]
    W = sum(e[0] for _, e in bins)
    if W == 0:
        return 0, [[0, 0, 0]] * K, [0] * K
    mean = [tuple((e[c] + e[0] // 2) // e[0] for c in (1, 2, 3)) for _, e in bins]

    def d2(p, q):
        return sum((a - b) ** 2 for a, b in zip(p, q))
    best = 0
    for i, (_, e) in enumerate(bins):
        if e[0] > bins[best][1][0]:
            best = i
    cen = [mean[best]]
    while len(cen) < K:
        top, arg = 0, None
        for i, (_, e) in enumerate(bins):
            v = e[0] * min(d2(mean[i], c) for c in cen)
            if v > top:
                top, arg = v, i
        if arg is None:
            break
        cen.append(mean[arg])
    for _ in range(T):
        N = [0] * len(cen)
        sums = [[0, 0, 0] for _ in cen]
        for i, (_, e) in enumerate(bins):
            j = min(range(len(cen)), key=lambda j: (d2(mean[i], cen[j]), j))
            N[j] += e[0]
            for c in range(3):
                sums[j][c] += e[1 + c]
        cen = [tuple((s + n // 2) // n for s in sm) if n else c for c, sm, n in zip(cen, sums, N)]
    order = sorted(range(len(cen)), key=lambda j: (-N[j], j))
    pad = K - len(cen)
    return W, [list(cen[j]) for j in order] + [[0, 0, 0]] * pad, [N[j] for j in order] + [0] * pad


def test_second_implementation_agrees_on_200_random_cases():
    rng = np.random.default_rng(2026)
    for case in range(200):
        S = int(rng.integers(1, 41))
        h, w = (int(v) for v in rng.integers(1, min(S, 6) + 1, 2))
        spec = Palette(colors=int(rng.integers(1, 9)), weight=("map", "uniform")[case % 2],
                       filter=("bilinear", "bicubic")[(case // 2) % 2], rounds=int(rng.integers(1, 17)))
        kind = case % 5
        if kind == 0:                                             # noise
            img = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
        elif kind == 1:                                           # few colours, fewer than K at times
            pal = rng.integers(0, 256, (int(rng.integers(1, 5)), 3), dtype=np.uint8)
            img = pal[rng.integers(0, len(pal), (S, S))]
        elif kind == 2:                                           # colours that share bins
            img = (rng.integers(0, 3, (S, S, 3)) * 7 + rng.integers(0, 250, 3)).astype(np.uint8)
        elif kind == 3:                                           # smooth
            img = np.clip(np.add.outer(np.arange(S) * 5, np.arange(S) * 3)[..., None] + rng.integers(0, 40, 3),
                          0, 255).astype(np.uint8)
        else:                                                     # two tones: ties
            img = np.where((np.arange(S) < S // 2)[:, None, None], 255, 0).astype(np.uint8) * np.ones((1, S, 3), np.uint8)
        heat = rng.random((h, w), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)
        W, col, n = PL.palette_rule(img, heat, spec)
        W2, col2, n2 = loops_rule(img, heat, spec)
        assert (W, col.tolist(), n.tolist()) == (W2, col2, n2), (case, S, spec)


def test_map_weight_is_uniform_weight_under_a_mask():
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (23, 23, 3), dtype=np.uint8)
    heat = rng.random((4, 5), dtype=np.float32)
    spec = Palette(colors=4, weight="map", filter="bicubic", rounds=3)
    wgt = O.upsample(O.quantise(heat), 23, "bicubic").astype(np.int64) >> 4
    assert np.array_equal(PL.pixel_weights(heat, 23, spec), wgt) and wgt.max() <= 15 and wgt.min() >= 0
    # w copies of a pixel at weight 15 weigh what the pixel does at weight w, 15 times over
    hist = sum((PL.histogram(img, np.where(wgt > k, 15, 0)) for k in range(15)), np.zeros((4096, 4), np.int64))
    assert np.array_equal(hist, 15 * PL.histogram(img, wgt))
    W, col, n = PL.palette_rule(img, heat, spec)
    W1, col1, n1 = PL.cluster(PL.histogram(img, wgt), 4, 3)
    assert W == W1 == int(wgt.sum()) and np.array_equal(col, col1) and np.array_equal(n, n1)


# ------------------------------------------------------------------------------ helpers around the rule
def test_fractions_and_names():
    f = PL.fractions_of(np.array([[120, 120, 0], [0, 0, 0]], np.uint32), np.array([240, 0], np.uint32))
    assert f.dtype == np.float32 and f.tolist() == [[0.5, 0.5, 0.0], [0.0, 0.0, 0.0]]
    assert PL.fractions_of(np.array([1], np.uint32), np.array(3, np.uint32))[0] == np.float32(1 / 3)
    assert [n for n, _ in PL.CSS_COLORS] == "black white gray silver red maroon orange yellow olive green lime teal " \
        "aqua blue navy purple fuchsia pink brown beige".split()
    cols = np.array([[[0, 0, 0], [250, 250, 250], [130, 5, 5]], [[245, 245, 220], [64, 128, 0], [0, 200, 250]]], np.uint8)
    assert PL.names_of(cols) == [["black", "white", "maroon"], ["beige", "olive", "aqua"]]   # (64,128,0): as far from green, olive is first


def test_row_pack_and_unpack_round_trip():
    rng = np.random.default_rng(5)
    n, h, w, K = 3, 2, 3, 4
    cl, sc = rng.integers(0, 10, n).astype(np.int32), rng.random(n, dtype=np.float32)
    heat = rng.random((n, h, w), dtype=np.float32)
    tot = np.array([0, 1, 2 ** 32 - 1], np.uint32)
    col = rng.integers(0, 256, (n, K, 3), dtype=np.uint8)
    wt = np.array([[0, 1, 2 ** 31, 2 ** 32 - 1]] * n, np.uint32)
    # a weight whose bits are a NaN pattern survives: the words are never read as floats
    wt[1, 0] = 0x7FC00001
    rows = PL.pack_rows(cl, sc, heat, tot, col, wt)
    assert rows.dtype == np.float32 and rows.shape == (n, 2 + h * w + 1 + 2 * K)
    got = PL.unpack_rows(rows, h, w, K)
    for a, b in zip(got, (cl, sc, heat, tot, col, wt)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert rows.view(np.uint32)[0, 2 + h * w + 1] == int(col[0, 0, 0]) | int(col[0, 0, 1]) << 8 | int(col[0, 0, 2]) << 16


def test_check_refusals():
    assert PL.check(Palette()) == Palette(5, "map", "bilinear", 8)
    for bad in (Palette(colors=0), Palette(colors=9), Palette(colors=2.0), Palette(colors=True), Palette(rounds=0),
                Palette(rounds=17), Palette(weight="heat"), Palette(filter="lanczos"), Palette(filter="nearest")):
        with pytest.raises(ValueError, match="palette"):
            PL.check(bad)
        with pytest.raises(ValueError, match="palette"):
            PL.palette_rule(np.zeros((2, 2, 3), np.uint8), np.zeros((1, 1), np.float32), bad)
    with pytest.raises(ValueError, match="uint8"):
        PL.palette_rule(np.zeros((2, 2, 3), np.float32), np.zeros((1, 1), np.float32))
    with pytest.raises(ValueError, match="upsample"):
        PL.palette_rule(np.zeros((2, 2, 3), np.uint8), np.zeros((3, 3), np.float32))


# ------------------------------------------------------------------------------ config, signatures
def _version(tmp_path, meta=None):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, **(meta or {})}))
    return d


def test_config_block_flag_and_errors(tmp_path):
    assert load_version_dir(_version(tmp_path / "none"), synthetic=True).palette is None
    assert load_version_dir(_version(tmp_path / "d", {"palette": {}}), synthetic=True).palette == Palette()
    d = _version(tmp_path / "c", {"palette": {"colors": 3, "weight": "uniform", "filter": "bicubic", "rounds": 2}})
    assert load_version_dir(d, synthetic=True).palette == Palette(3, "uniform", "bicubic", 2)
    assert load_version_dir(d, synthetic=True, palette_colors=8).palette == Palette(8, "uniform", "bicubic", 2)
    assert load_version_dir(_version(tmp_path / "f"), synthetic=True, palette_colors=2).palette == Palette(colors=2)
    for i, block in enumerate(({"colors": 0}, {"colors": 9}, {"colors": "five"}, {"rounds": 17}, {"weight": "heat"},
                               {"filter": "lanczos"}, {"colours": 5}, 5)):
        with pytest.raises(ValueError, match="synthetic.json"):
            load_version_dir(_version(tmp_path / f"bad{i}", {"palette": block}), synthetic=True)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="palette_colors"):
            load_version_dir(_version(tmp_path / "g"), synthetic=True, palette_colors=bad)


def test_flag_reaches_the_config(monkeypatch):
    from kdl.serving.config import config_from_args as parse_args
    base = ["--model_name", "m", "--model_base_path", "/tmp/m"]
    assert parse_args(base).palette_colors is None
    assert parse_args(base + ["--palette_colors", "3"]).palette_colors == 3
    monkeypatch.setenv("KDL_PALETTE_COLORS", "6")
    assert parse_args(base).palette_colors == 6


FAMILIES = [("xception", (10, 10), 299, False), ("resnet50", (7, 7), 224, False),
            ("efficientnet_b7", (19, 19), 600, False), ("vit_b16", (14, 14), 224, True)]


@pytest.mark.parametrize("model,hw,S,rollout", FAMILIES)
def test_signatures_with_and_without_the_block(tmp_path, model, hw, S, rollout):
    from kdl.serving import outputs as OUT
    meta = {} if model == "xception" else {"model": model}
    plain = load_version_dir(_version(tmp_path / "plain", meta), synthetic=True)
    want = json.loads((GOLDEN / "metadata.json").read_text())[model]["plain"]["order"]
    assert list(plain.signatures) == want and not set(SIGS) & set(want) and plain.palette is None
    src = load_version_dir(_version(tmp_path / "with", {**meta, "palette": {"colors": 4}}), synthetic=True)
    assert list(src.signatures) == want + list(SIGS)
    for name in want:                                            # the others are what they were
        assert src.signatures[name] == plain.signatures[name]
        assert OUT.kind_of(src.signatures[name]).name != "palette"
    for name in SIGS:
        sig = src.signatures[name]
        assert sig.explain == hw and sig.overlay == 0 and sig.rollout is rollout
        assert sig.input_dtype != P.DT_FLOAT and not sig.top_k and not sig.embed
        assert sig.outputs == (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)),
                               ("colors", P.DT_UINT8, (-1, 4, 3)), ("fractions", P.DT_FLOAT, (-1, 4)),
                               ("names", P.DT_STRING, (-1, 4)))
        assert OUT.kind_of(sig).name == "palette"
        assert OUT.out_cols(sig, src, gpu=True) == OUT.out_cols(sig, src, gpu=False) == 2 + hw[0] * hw[1] + 1 + 8
        kw = OUT.engine_kwargs(sig, src, "cuda:0")
        assert kw == dict(rollout=True, palette=Palette(colors=4)) if rollout else kw == dict(
            explain=True, palette=Palette(colors=4))
    assert src.signatures["palette"].input_shape == (-1, S, S, 3)
    assert src.signatures["palette_image"].input_shape == src.signatures["serving_image"].input_shape
    assert src.signatures["palette_bytes"].input_key == src.signatures["serving_bytes"].input_key


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


SPEC = Palette(colors=4, weight="map", filter="bicubic", rounds=5)


@pytest.fixture(scope="module")
def repo(tmp_path_factory):
    base = tmp_path_factory.mktemp("palette") / "clothing-model"
    _version(base, {"seed": 5, "palette": {"colors": 4, "filter": "bicubic", "rounds": 5}})
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


def _answer(resp, n=1, K=4):
    assert sorted(resp.outputs) == sorted(KEYS)
    o = resp.outputs
    shapes = {k: [d.size for d in o[k].tensor_shape.dim] for k in KEYS}
    assert shapes == {"classes": [n, 1], "scores": [n, 1], "colors": [n, K, 3], "fractions": [n, K], "names": [n, K]}
    assert [o[k].dtype for k in KEYS] == [P.DT_STRING, P.DT_FLOAT, P.DT_UINT8, P.DT_FLOAT, P.DT_STRING]
    return {"classes": [v.decode() for v in o["classes"].string_val],
            "scores": np.asarray(o["scores"].float_val, np.float32),
            "colors": np.frombuffer(o["colors"].tensor_content, np.uint8).reshape(n, K, 3),
            "fractions": np.asarray(o["fractions"].float_val, np.float32).reshape(n, K),
            "names": np.asarray([v.decode() for v in o["names"].string_val]).reshape(n, K).tolist()}


def _inputs(jpeg):
    img = pp.load_image(jpeg)
    return {"palette": (pp.to_uint8(img)[None], "images"), "palette_image": (np.asarray(img, np.uint8)[None], "images"),
            "palette_bytes": ([jpeg], "image_bytes")}


@pytest.fixture(scope="module")
def answers(stub, jpeg):
    """One JPEG through the three palette signatures and through the three explain signatures."""
    got, exp = {}, {}
    for name, (x, key) in _inputs(jpeg).items():
        got[name] = _answer(stub.Predict(make_request(x, signature=name, input_key=key), timeout=300))
        r = stub.Predict(make_request(x, signature=name.replace("palette", "explain"), input_key=key), timeout=300)
        exp[name] = (r.outputs["classes"].string_val[0].decode(), np.asarray(r.outputs["scores"].float_val, np.float32),
                     np.asarray(r.outputs["heatmap"].float_val, np.float32).reshape(10, 10))
    return got, exp


def test_three_signatures_equal_the_rule_on_the_oracles_map(server, answers, jpeg):
    got, exp = answers
    src = server.manager.get("clothing-model", None, None).source
    assert src.palette == SPEC
    fed = pp.to_uint8(pp.load_image(jpeg))
    for name in SIGS:
        a, (label, score, heat) = got[name], exp[name]
        assert a["classes"] == [label] and np.array_equal(a["scores"], score), name
        W, col, n = PL.palette_rule(fed, heat, SPEC)
        assert W > 0 and n[0] > 0
        assert np.array_equal(a["colors"][0], col), name
        assert np.array_equal(a["fractions"][0], PL.fractions_of(n, W)), name
        assert a["names"] == [PL.names_of(col)], name


def test_output_filter_counter_metadata_and_runner(server, stub, answers, jpeg):
    from kdl.serving.metrics import METRICS
    got, _ = answers
    x, key = _inputs(jpeg)["palette"]
    before = METRICS.snapshot()["counters"]
    req = make_request(x, signature="palette", input_key=key)
    req.output_filter.extend(["colors", "names"])
    r = stub.Predict(req, timeout=300)
    assert sorted(r.outputs) == ["colors", "names"]
    assert r.outputs["colors"].tensor_content == got["palette"]["colors"].tobytes()
    after = METRICS.snapshot()["counters"]
    key_m = "kdl_palette_total{signature=palette}"
    assert after.get(key_m, 0) - before.get(key_m, 0) == 1
    assert after.get("kdl_explain_total{signature=palette}", 0) == 0
    req = make_request(x, signature="palette", input_key=key)
    req.output_filter.append("heatmap")                           # not an output of this kind
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(req, timeout=30)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT

    req = P.GetModelMetadataRequest()
    req.model_spec.name = "clothing-model"
    req.metadata_field.append("signature_def")
    sdm = P.SignatureDefMap()
    stub.GetModelMetadata(req, timeout=5).metadata["signature_def"].Unpack(sdm)
    for name in SIGS:
        out = sdm.signature_def[name].outputs
        assert sorted(out) == sorted(KEYS)
        want = {"classes": (P.DT_STRING, [-1, 1]), "scores": (P.DT_FLOAT, [-1, 1]), "colors": (P.DT_UINT8, [-1, 4, 3]),
                "fractions": (P.DT_FLOAT, [-1, 4]), "names": (P.DT_STRING, [-1, 4])}
        for k, (dt, shape) in want.items():
            assert out[k].dtype == dt and [d.size for d in out[k].tensor_shape.dim] == shape, (name, k)
    assert sorted(sdm.signature_def["explain"].outputs) == ["classes", "heatmap", "scores"]
    r = server.manager.get("clothing-model", None, None).runner("palette")
    assert r.out_cols == 102 + 1 + 8 and r.sig.explain == (10, 10) and not r.gpu and r.kind == "palette"


def _post(url, body):
    try:
        with urllib.request.urlopen(urllib.request.Request(url, data=json.dumps(body).encode(), method="POST"),
                                    timeout=300) as r:
            return r.status, json.load(r)
    except urllib.error.HTTPError as e:
        return e.code, json.load(e)


def test_rest_predict_by_row_and_by_column(server, answers, jpeg):
    got, _ = answers
    a = got["palette"]
    u8 = _inputs(jpeg)["palette"][0]
    url = f"http://127.0.0.1:{server.rest_port}/v1/models/clothing-model:predict"
    st, out = _post(url, {"signature_name": "palette", "instances": u8.tolist()})
    assert st == 200, out
    (one,) = out["predictions"]
    assert sorted(one) == sorted(KEYS)
    assert one["classes"] == a["classes"] and np.allclose(one["scores"], a["scores"], rtol=1e-6)
    assert one["colors"] == a["colors"][0].tolist() and isinstance(one["colors"][0][0], int)
    assert np.array_equal(np.asarray(one["fractions"], np.float32), a["fractions"][0]) and one["names"] == a["names"][0]
    st, out = _post(url, {"signature_name": "palette", "inputs": {"images": u8.tolist()}})
    assert st == 200, out
    o = out["outputs"]
    assert o["classes"] == [a["classes"]] and o["colors"] == a["colors"].tolist() and o["names"] == a["names"]
    assert np.array_equal(np.asarray(o["fractions"], np.float32), a["fractions"])


def test_null_server_returns_zero_rows(repo):
    px = np.random.default_rng(3).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)
    srv = _server(repo, "null")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            a = _answer(PredictionStub(ch).Predict(make_request(px, signature="palette", input_key="images"),
                                                   timeout=60), 2)
        src = srv.manager.get("clothing-model", None, None).source
    finally:
        srv.stop(0)
    assert a["classes"] == [src.labels[0]] * 2 and (a["scores"] == 0).all()
    assert (a["colors"] == 0).all() and (a["fractions"] == 0).all() and a["names"] == [["black"] * 4] * 2


# ------------------------------------------------------------------------------ gateway
@pytest.mark.parametrize("mode", ["uint8", "bytes", "raw"])
def test_gateway_colors(server, answers, jpeg, monkeypatch, mode):
    got, _ = answers
    a = got[{"bytes": "palette_bytes", "raw": "palette_image"}.get(mode, "palette")]
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        c = create_app(GatewayConfig({"GATEWAY_MODE": mode}), channel=ch).test_client()
        r = c.post("/colors", json={"url": "http://example.invalid/pants.jpg"})
        assert r.status_code == 200, r.data
        out = r.get_json()
        assert sorted(out) == ["colors", "label", "score"]
        assert out["label"] == a["classes"][0] and np.isclose(out["score"], a["scores"][0], rtol=1e-6)
        live = [j for j in range(4) if a["fractions"][0, j] > 0]
        assert len(out["colors"]) == len(live) >= 1
        for e, j in zip(out["colors"], live):
            rgb = a["colors"][0, j].tolist()
            assert sorted(e) == ["fraction", "hex", "name", "rgb"]
            assert e["rgb"] == rgb and e["hex"] == "#%02x%02x%02x" % tuple(rgb) and e["name"] == a["names"][0][j]
            assert np.float32(e["fraction"]) == a["fractions"][0, j]
        assert c.post("/colors", json={"nope": 1}).status_code == 400


def test_response_parser_drops_zero_weights():
    resp = P.PredictResponse()
    o = resp.outputs
    o["classes"].string_val.append(b"pants")
    o["scores"].float_val.append(0.75)
    o["colors"].tensor_content = np.array([[[1, 2, 255], [9, 9, 9], [0, 0, 0]]], np.uint8).tobytes()
    o["fractions"].float_val.extend([0.75, 0.25, 0.0])
    for d in (1, 3):
        o["fractions"].tensor_shape.dim.add(size=d)
    o["names"].string_val.extend([b"blue", b"black", b"black"])
    assert process_palette_response(resp) == [{"label": "pants", "score": 0.75, "colors": [
        {"rgb": [1, 2, 255], "hex": "#0102ff", "name": "blue", "fraction": 0.75},
        {"rgb": [9, 9, 9], "hex": "#090909", "name": "black", "fraction": 0.25}]}]
