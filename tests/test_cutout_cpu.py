"""The cutout signatures without a GPU: literal answers of the rule, the table form of its rounds against a
pixel-level second implementation in plain loops, rows and config errors, the signatures with and without the
block, a ``--device cpu`` server answering ``cutout_bytes`` and the gateway's /cutout."""
import io
import json
from pathlib import Path

import grpc
import numpy as np
import pytest
from PIL import Image

from kdl.engine.base import Cutout
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request, process_cutout_response
from kdl.serving import cutout as C
from kdl.serving import overlay as O
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

PANTS = Path(__file__).parent / "data" / "pants.png"
GOLDEN = Path(__file__).parent / "golden" / "outputs"
SIGS = ("cutout", "cutout_image", "cutout_bytes")
KEYS = ("classes", "scores", "cutout", "coverage")
FEATHER = [0, 28, 57, 85, 113, 142, 170, 198, 227, 255]          # (255 c + 4) // 9 for c = 0..9


def flat(S, v=200):
    return np.full((S, S, 3), v, np.uint8)


# ------------------------------------------------------------------------------ the rule: literal answers
@pytest.mark.parametrize("S", [2, 3, 5, 17, 64])
def test_flat_picture_all_ones_map(S):
    """One colour, TB = 0: the tie goes to the garment, the mask is the gate. One majority round takes the four
    corner pixels, which see 4 of 9; no round takes none."""
    ones = np.ones((2, 2), np.float32)
    count, rgba = C.cutout_rule(flat(S), ones, Cutout(feather=False))
    want = np.full((S, S), 255, np.uint8)
    want[[0, 0, -1, -1], [0, -1, 0, -1]] = 0
    assert count == S * S - 4 and rgba.dtype == np.uint8 and rgba.shape == (S, S, 4)
    assert np.array_equal(rgba[..., 3], want) and np.array_equal(rgba[..., :3], flat(S))
    count, rgba = C.cutout_rule(flat(S), ones, Cutout(smooth=0, feather=False))
    assert count == S * S and (rgba[..., 3] == 255).all()
    count, rgba = C.cutout_rule(flat(S), ones, Cutout(smooth=0))  # feathered: the 3 x 3 mean of a full mask
    assert count == S * S and rgba[0, 0, 3] == 113 and rgba[0, 1, 3] == (170 if S > 2 else 113)
    assert S < 3 or rgba[1, 1, 3] == 255


def test_one_pixel():
    assert C.cutout_rule(flat(1), np.ones((1, 1), np.float32))[0] == 0          # 1 of 9 is no majority
    count, rgba = C.cutout_rule(flat(1), np.ones((1, 1), np.float32), Cutout(smooth=0))
    assert count == 1 and rgba.tolist() == [[[200, 200, 200, 28]]]
    count, rgba = C.cutout_rule(flat(1), np.ones((1, 1), np.float32), Cutout(smooth=0, feather=False))
    assert count == 1 and rgba.tolist() == [[[200, 200, 200, 255]]]


@pytest.mark.parametrize("heat", [np.zeros((3, 2), np.float32), np.full((2, 3), np.nan, np.float32),
                                  np.full((2, 2), 25.4 / 255, np.float32)], ids=["zeros", "nan", "below-gate"])
@pytest.mark.parametrize("feather", [False, True])
def test_no_heat_no_garment(heat, feather):
    rng = np.random.default_rng(1)
    for img in (flat(9), rng.integers(0, 256, (9, 9, 3), dtype=np.uint8)):
        count, rgba = C.cutout_rule(img, heat, Cutout(feather=feather))
        assert count == 0 and not rgba[..., 3].any() and np.array_equal(rgba[..., :3], img)
    assert C.cutout_rule(flat(9), np.full((2, 2), 25.6 / 255, np.float32), Cutout(smooth=0))[0] == 81   # rint -> 26


def test_two_colours_the_hot_half_wins_its_gated_pixels():
    """S = h = w: both resample passes are the identity. The left half is red and hot, except its top row, which
    is cold; the right half is blue and lukewarm (51 >= the gate). Red's F is 255 * 28 of 255 * 32, blue's
    51 * 32 of 255 * 32: red is garment-coloured, blue is not, and the mask is exactly red's gated pixels."""
    S = 8
    img = np.zeros((S, S, 3), np.uint8)
    img[:, :4] = (220, 30, 30)
    img[:, 4:] = (30, 30, 220)
    heat = np.full((S, S), 0.2, np.float32)
    heat[:, :4] = 1.0
    heat[0, :4] = 0.0
    assert np.array_equal(O.upsample(O.quantise(heat), S, "bilinear"), np.rint(heat * 255).astype(np.uint8))
    want = np.zeros((S, S), np.uint8)
    want[1:, :4] = 255
    for rounds in (0, 1, 2, 8):
        count, rgba = C.cutout_rule(img, heat, Cutout(rounds=rounds, smooth=0, feather=False))
        assert count == 28 and np.array_equal(rgba[..., 3], want), rounds
    # heat on the blue half instead: the same picture, the other answer
    count, rgba = C.cutout_rule(img, np.ascontiguousarray(heat[:, ::-1]), Cutout(smooth=0, feather=False))
    assert count == 28 and np.array_equal(rgba[..., 3], want[:, ::-1])


def test_feather_values_on_a_hand_made_mask():
    m = np.array([[1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0]], bool)
    count, alpha = C.finish(m, Cutout(smooth=0, feather=True))
    assert count == 5 and alpha.tolist() == [[113, 113, 57, 0, 0], [113, 113, 57, 0, 0], [57, 57, 57, 28, 28],
                                             [0, 0, 28, 28, 28], [0, 0, 28, 28, 28]]
    count, alpha = C.finish(m, Cutout(smooth=0, feather=False))
    assert count == 5 and np.array_equal(alpha, 255 * m.astype(np.uint8))
    count, alpha = C.finish(m, Cutout(smooth=1, feather=False))     # no pixel sees five: the mask empties
    assert count == 0 and not alpha.any()
    full = np.ones((5, 5), bool)
    assert C.finish(full, Cutout(smooth=0))[1].tolist() == [[113, 170, 170, 170, 113]] + [[170, 255, 255, 255, 170]] * 3 + [
        [113, 170, 170, 170, 113]]
    rng = np.random.default_rng(7)
    r = rng.random((5, 5)) < 0.6
    c = C.window_counts(r)
    assert set(np.unique(c)) <= set(range(10)) and len(np.unique(c)) >= 5
    assert np.array_equal(C.finish(r, Cutout(smooth=0))[1], np.asarray(FEATHER, np.uint8)[c])
    assert [(255 * k + 4) // 9 for k in range(10)] == FEATHER


def test_smooth_rounds_against_loops():
    rng = np.random.default_rng(3)
    m = rng.random((13, 13)) < 0.55
    cur = m.copy()
    for M in range(1, 5):
        nxt = np.zeros_like(cur)
        for y in range(13):
            for x in range(13):
                c = sum(cur[yy, xx] for yy in range(max(y - 1, 0), min(y + 2, 13))
                        for xx in range(max(x - 1, 0), min(x + 2, 13)))
                nxt[y, x] = c >= 5
        cur = nxt
        count, alpha = C.finish(m, Cutout(smooth=M, feather=False))
        assert count == int(cur.sum()) and np.array_equal(alpha, 255 * cur.astype(np.uint8)), M


# ------------------------------------------------------------------------------ second implementation
def raw_mask_by_pixels(img, u, gate, rounds):
    """Step 4 the long way: every round walks the pixels again and builds both histograms from the hard mask of
    the round before."""
    S = img.shape[0]
    binof = [[(int(img[y, x, 0]) >> 4) << 8 | (int(img[y, x, 1]) >> 4) << 4 | (int(img[y, x, 2]) >> 4)
              for x in range(S)] for y in range(S)]
    weight = [[int(u[y, x]) for x in range(S)] for y in range(S)]        # the garment's share of 255 per pixel
    mask = None
    for _ in range(rounds + 1):
        fore, back = {}, {}
        for y in range(S):
            for x in range(S):
                b = binof[y][x]
                fore[b] = fore.get(b, 0) + weight[y][x]
                back[b] = back.get(b, 0) + 255 - weight[y][x]
        TF, TB = sum(fore.values()), sum(back.values())
        fg = {b for b in fore if fore[b] * TB >= back[b] * TF}
        mask = [[binof[y][x] in fg and int(u[y, x]) >= gate for x in range(S)] for y in range(S)]
        weight = [[255 if mask[y][x] else 0 for x in range(S)] for y in range(S)]
    return np.array(mask, bool)


@pytest.mark.parametrize("S", [5, 17, 33])
def test_the_table_form_equals_a_pixel_level_implementation(S):
    rng = np.random.default_rng(S)
    levels = np.array([0, 60, 130, 250], np.uint8)
    pics = [levels[rng.integers(0, 4, (S, S, 3))], levels[rng.integers(0, 2, (S, S, 3))],
            rng.integers(0, 256, (S, S, 3), dtype=np.uint8), flat(S)]
    blob = np.exp(-((np.arange(4) - 1.3) ** 2)[:, None] - ((np.arange(3) - 1.0) ** 2)[None, :]).astype(np.float32)
    heats = [rng.random((3, 3), dtype=np.float32), blob, np.ones((2, 2), np.float32)]
    seen = set()
    for pi, img in enumerate(pics):
        for hi, heat in enumerate(heats):
            u = O.upsample(O.quantise(heat), S, "bilinear")
            for gate in (1, 26, 128):
                ok = u >= gate
                bins = C.bins_of(img)
                N, G, F = C.tables_of(bins, u, ok)
                assert N.sum() == S * S and G.sum() == ok.sum() and F.sum() == u.astype(np.int64).sum()
                for rounds in (0, 1, 2, 8):
                    want = raw_mask_by_pixels(img, u, gate, rounds)
                    got = C.colour_table(N, G, F, S, rounds)[bins] & ok
                    assert np.array_equal(got, want), (pi, hi, gate, rounds)
                    count, rgba = C.cutout_rule(img, heat, Cutout(gate, rounds, 0, False))
                    assert count == want.sum() and np.array_equal(rgba[..., 3] == 255, want)
                    seen.add((pi, hi, gate, rounds, int(want.sum())))
    assert len({s[-1] for s in seen}) > 10                          # the cases are not all the same mask


def test_rule_refusals():
    with pytest.raises(ValueError, match="1024"):
        C.cutout_rule(np.zeros((1025, 1025, 3), np.uint8), np.ones((2, 2), np.float32))
    with pytest.raises(ValueError, match="uint8"):
        C.cutout_rule(np.zeros((4, 4, 3), np.float32), np.ones((2, 2), np.float32))
    with pytest.raises(ValueError, match="uint8"):
        C.cutout_rule(np.zeros((4, 5, 3), np.uint8), np.ones((2, 2), np.float32))
    with pytest.raises(ValueError, match=r"\[h, w\]"):
        C.cutout_rule(flat(4), np.ones((4,), np.float32))


# ------------------------------------------------------------------------------ rows
def test_rows_round_trip():
    rng = np.random.default_rng(5)
    n, h, w, S = 3, 2, 3, 7
    classes = np.array([4, 0, 9], np.int32)
    scores = rng.random(n, dtype=np.float32)
    heat = rng.random((n, h, w), dtype=np.float32)
    counts = np.array([0, 49, 17], np.uint32)
    pics = rng.integers(0, 256, (n, S, S, 4), dtype=np.uint8)
    pics[0, 0, 0] = (0xA5, 0xA5, 0xC5, 0x7F)                         # a NaN pattern as a word: bits, not floats
    rows = C.pack_rows(classes, scores, heat, counts, pics)
    assert rows.dtype == np.float32 and rows.shape == (n, 2 + h * w + 1 + S * S)
    assert rows.view(np.uint32)[1, 2 + h * w] == 49
    p = pics[2, 1, 3].astype(np.uint32)
    assert rows.view(np.uint32)[2, 2 + h * w + 1 + 1 * S + 3] == p[0] | p[1] << 8 | p[2] << 16 | p[3] << 24
    c, s, m, k, px = C.unpack_rows(rows, h, w, S)
    assert np.array_equal(c, classes) and np.array_equal(s, scores) and np.array_equal(m, heat)
    assert k.dtype == np.uint32 and np.array_equal(k, counts) and px.dtype == np.uint8 and np.array_equal(px, pics)
    assert C.coverage_of(counts, S).dtype == np.float32
    assert C.coverage_of(counts, S).tolist() == [0.0, 1.0, float(np.float32(17 / 49))]


# ------------------------------------------------------------------------------ config
def _version(tmp_path, meta=None):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, **(meta or {})}))
    return d


def test_config_block_flag_and_errors(tmp_path):
    assert load_version_dir(_version(tmp_path / "none"), synthetic=True).cutout is None
    assert load_version_dir(_version(tmp_path / "d", {"cutout": {}}), synthetic=True).cutout == Cutout()
    assert Cutout() == Cutout(gate=26, rounds=2, smooth=1, feather=True, filter="bilinear")
    block = {"gate": 40, "rounds": 0, "smooth": 4, "feather": False, "filter": "bicubic"}
    d = _version(tmp_path / "c", {"cutout": block})
    assert load_version_dir(d, synthetic=True).cutout == Cutout(40, 0, 4, False, "bicubic")
    assert load_version_dir(d, synthetic=True, cutout_gate=255).cutout == Cutout(255, 0, 4, False, "bicubic")
    assert load_version_dir(_version(tmp_path / "f"), synthetic=True, cutout_gate=1).cutout == Cutout(gate=1)
    for i, bad in enumerate(({"gate": 0}, {"gate": 256}, {"gate": "low"}, {"gate": 26.5}, {"gate": True}, {"rounds": -1},
                             {"rounds": 9}, {"rounds": 1.5}, {"smooth": -1}, {"smooth": 5}, {"feather": 1},
                             {"feather": "yes"}, {"filter": "lanczos"}, {"gates": 3}, {"gate": 26, "boxes": 3}, 5, [26])):
        with pytest.raises(ValueError, match="synthetic.json"):
            C.resolve(_version(tmp_path / f"bad{i}", {"cutout": bad}))         # what the load calls
        if i % 8 == 0:
            with pytest.raises(ValueError, match="synthetic.json"):
                load_version_dir(_version(tmp_path / f"bad{i}", {"cutout": bad}), synthetic=True)
    for bad in (0, 256):
        with pytest.raises(ValueError, match="cutout_gate"):
            load_version_dir(_version(tmp_path / "g"), synthetic=True, cutout_gate=bad)
    for bad in (Cutout(gate=0), Cutout(rounds=9), Cutout(smooth=5), Cutout(feather=2), Cutout(filter="nearest")):
        with pytest.raises(ValueError, match="cutout"):
            C.check(bad)


def test_a_family_without_a_heatmap_method_is_refused(tmp_path, monkeypatch):
    from dataclasses import replace

    from kdl.engine import registry
    info = registry.get("xception")
    monkeypatch.setattr(registry, "get", lambda family: replace(info, cam_oracle=None, rollout_oracle=None))
    with pytest.raises(ValueError, match="heatmap method"):
        load_version_dir(_version(tmp_path / "x", {"cutout": {}}), synthetic=True)


def test_flag_reaches_the_config(monkeypatch):
    from kdl.serving.config import config_from_args as parse_args
    base = ["--model_name", "m", "--model_base_path", "/tmp/m"]
    assert parse_args(base).cutout_gate is None
    assert parse_args(base + ["--cutout_gate", "40"]).cutout_gate == 40
    monkeypatch.setenv("KDL_CUTOUT_GATE", "60")
    assert parse_args(base).cutout_gate == 60
    assert parse_args(base + ["--cutout_gate", "2"]).cutout_gate == 2


# ------------------------------------------------------------------------------ signatures
FAMILIES = [("xception", (10, 10), 299, False), ("resnet50", (7, 7), 224, False),
            ("efficientnet_b7", (19, 19), 600, False), ("vit_b16", (14, 14), 224, True)]


@pytest.mark.parametrize("model,hw,S,rollout", FAMILIES)
def test_signatures_with_and_without_the_block(tmp_path, model, hw, S, rollout):
    from kdl.serving import outputs as OUT
    meta = {} if model == "xception" else {"model": model}
    plain = load_version_dir(_version(tmp_path / "plain", meta), synthetic=True)
    want = json.loads((GOLDEN / "metadata.json").read_text())[model]["plain"]["order"]
    assert list(plain.signatures) == want and not set(SIGS) & set(want) and plain.cutout is None
    src = load_version_dir(_version(tmp_path / "with", {**meta, "cutout": {"gate": 30}}), synthetic=True)
    assert list(src.signatures) == want + list(SIGS)
    flagged = load_version_dir(_version(tmp_path / "flag", meta), synthetic=True, cutout_gate=30)
    assert list(flagged.signatures) == want + list(SIGS) and flagged.cutout == src.cutout == Cutout(gate=30)
    for name in want:                                            # the others are what they were
        assert src.signatures[name] == plain.signatures[name]
        assert OUT.kind_of(src.signatures[name]).name != "cutout"
    for name in SIGS:
        sig = src.signatures[name]
        assert sig.explain == hw and sig.overlay == 0 and sig.rollout is rollout
        assert sig.input_dtype != P.DT_FLOAT and not sig.top_k and not sig.embed
        assert sig.outputs == (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)),
                               ("cutout", P.DT_UINT8, (-1, S, S, 4)), ("coverage", P.DT_FLOAT, (-1, 1)))
        kind = OUT.kind_of(sig)
        assert kind.name == "cutout" and kind.trio == SIGS and kind.counter == "kdl_cutout_total" and kind.null_zero
        assert OUT.out_cols(sig, src, gpu=True) == OUT.out_cols(sig, src, gpu=False) == 2 + hw[0] * hw[1] + 1 + S * S
        kw = OUT.engine_kwargs(sig, src, "cuda:0")
        assert kw == dict(rollout=True, cutout=Cutout(gate=30)) if rollout else kw == dict(
            explain=True, cutout=Cutout(gate=30))
    assert src.signatures["cutout"].input_shape == (-1, S, S, 3)
    assert src.signatures["cutout_image"].input_shape == src.signatures["serving_image"].input_shape
    assert src.signatures["cutout_bytes"].input_key == src.signatures["serving_bytes"].input_key
    assert OUT.WRAPPED["cutout_image"] == (0, "cutout") and OUT.WRAPPED["cutout_bytes"] == (1, "cutout")
    both = load_version_dir(_version(tmp_path / "both", {**meta, "cutout": {}, "locate": {}, "palette": {}}),
                            synthetic=True)
    assert [OUT.kind_of(both.signatures[n]).name for n in ("palette", "locate", "cutout")] == ["palette", "locate",
                                                                                              "cutout"]


def test_signature_info_has_no_new_field():
    from dataclasses import fields

    from kdl.serving.backend import SignatureInfo
    want = json.loads((GOLDEN / "metadata.json").read_text())
    assert "cutout" not in [f.name for f in fields(SignatureInfo)] and want


# ------------------------------------------------------------------------------ a CPU server, end to end
SPEC = Cutout(gate=40, rounds=3, smooth=2, feather=True, filter="bicubic")
BLOCK = {"gate": 40, "rounds": 3, "smooth": 2, "feather": True, "filter": "bicubic"}


@pytest.fixture(scope="module")
def jpeg():
    b = io.BytesIO()
    Image.open(PANTS).convert("RGB").save(b, "JPEG", quality=90)
    return b.getvalue()


@pytest.fixture(scope="module")
def server(tmp_path_factory):
    base = tmp_path_factory.mktemp("cutout") / "clothing-model"
    _version(base, {"seed": 5, "cutout": BLOCK})
    cfg = ServerConfig(port=0, rest_api_port=0, model_name="clothing-model", model_base_path=str(base),
                       device="cpu", host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend="python",
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=500, allowed_batch_sizes=[1, 2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    yield srv
    srv.stop(0)


@pytest.fixture(scope="module")
def answer(server, jpeg):
    """One JPEG through cutout_bytes and through explain_bytes."""
    from kdl.serving.metrics import METRICS
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        stub = PredictionStub(ch)
        before = METRICS.snapshot()["counters"]
        got = stub.Predict(make_request([jpeg], signature="cutout_bytes", input_key="image_bytes"), timeout=300)
        after = METRICS.snapshot()["counters"]
        exp = stub.Predict(make_request([jpeg], signature="explain_bytes", input_key="image_bytes"), timeout=300)
    key = "kdl_cutout_total{signature=cutout_bytes}"
    assert after.get(key, 0) - before.get(key, 0) == 1 and after.get("kdl_explain_total{signature=cutout_bytes}", 0) == 0
    return got, exp


def test_cpu_server_answers_the_rule(server, answer, jpeg):
    got, exp = answer
    o, S = got.outputs, 299
    assert sorted(o) == sorted(KEYS)
    assert {k: [d.size for d in o[k].tensor_shape.dim] for k in KEYS} == {
        "classes": [1, 1], "scores": [1, 1], "cutout": [1, S, S, 4], "coverage": [1, 1]}
    assert [o[k].dtype for k in KEYS] == [P.DT_STRING, P.DT_FLOAT, P.DT_UINT8, P.DT_FLOAT]
    u8 = pp.to_uint8(pp.load_image(jpeg))                          # what the executor saw: decode + nearest resize
    heat = np.asarray(exp.outputs["heatmap"].float_val, np.float32).reshape(10, 10)
    count, rgba = C.cutout_rule(u8, heat, SPEC)
    pic = np.frombuffer(o["cutout"].tensor_content, np.uint8).reshape(S, S, 4)
    assert np.array_equal(pic, rgba) and np.array_equal(pic[..., :3], u8)
    assert 0 < count < S * S and (pic[..., 3] > 0).any() and (pic[..., 3] == 0).any()
    assert np.array_equal(np.asarray(o["coverage"].float_val, np.float32), C.coverage_of([count], S))
    assert list(o["classes"].string_val) == list(exp.outputs["classes"].string_val)
    assert list(o["scores"].float_val) == list(exp.outputs["scores"].float_val)
    s = server.manager.get("clothing-model", None, None)
    r = s.runner("cutout")
    assert r.out_cols == 2 + 100 + 1 + S * S and not r.gpu and r.kind == "cutout" and s.source.cutout == SPEC
    (ans,) = process_cutout_response(got)
    assert ans["label"] == o["classes"].string_val[0].decode() and np.array_equal(ans["picture"], rgba)
    assert np.float32(ans["coverage"]) == C.coverage_of([count], S)[0]


@pytest.mark.parametrize("mode", ["uint8", "bytes", "raw", "compat"])
def test_gateway_cutout(server, answer, jpeg, monkeypatch, mode):
    import base64
    got, _ = answer
    (want,) = process_cutout_response(got)
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        c = create_app(GatewayConfig({"GATEWAY_MODE": mode}), channel=ch).test_client()
        r = c.post("/cutout", json={"url": "http://example.invalid/pants.jpg"})
        assert r.status_code == 200 and r.mimetype == "image/png", r.data[:200]
        im = Image.open(io.BytesIO(r.data))
        assert im.mode == "RGBA" and im.size == (299, 299)
        assert np.array_equal(np.asarray(im), want["picture"])
        assert r.headers["X-KDL-Label"] == want["label"]
        assert np.isclose(float(r.headers["X-KDL-Score"]), want["score"], rtol=1e-6)
        assert np.float32(float(r.headers["X-KDL-Coverage"])) == np.float32(want["coverage"])
        if mode == "bytes":
            j = c.post("/cutout", json={"url": "http://example.invalid/pants.jpg", "format": "json"})
            out = j.get_json()
            assert j.status_code == 200 and sorted(out) == ["coverage", "label", "png", "score"]
            assert base64.b64decode(out["png"]) == r.data and out["label"] == want["label"]
            assert c.post("/cutout", json={"url": "http://example.invalid/p.jpg", "format": "jpeg"}).status_code == 400
            assert c.post("/cutout", json={"nope": 1}).status_code == 400


def test_null_device_answers_zero_rows(tmp_path):
    base = tmp_path / "clothing-model"
    _version(base, {"seed": 5, "cutout": {}})
    cfg = ServerConfig(port=0, rest_api_port=0, model_name="clothing-model", model_base_path=str(base),
                       device="null", host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend="python",
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=500, allowed_batch_sizes=[1, 2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        u8 = np.random.default_rng(0).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            o = PredictionStub(ch).Predict(make_request(u8, signature="cutout", input_key="images"), timeout=60).outputs
    finally:
        srv.stop(0)
    assert not np.frombuffer(o["cutout"].tensor_content, np.uint8).any() and list(o["coverage"].float_val) == [0.0, 0.0]
