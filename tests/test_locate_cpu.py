"""The locate signatures without a GPU: literal answers of the rule, a second implementation (scipy's labels and
a flood fill in plain loops), rows and config errors, the signatures with and without the block, a
``--device cpu`` server of every family that has a map method (gRPC and REST, by row and by column), the
null device and the gateway's /locate."""
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
from scipy import ndimage

from kdl.engine.base import Locate, Overlay, Palette
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request, process_locate_response
from kdl.serving import locate as L
from kdl.serving import overlay as O
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

PANTS = Path(__file__).parent / "data" / "pants.png"
GOLDEN = Path(__file__).parent / "golden" / "outputs"
SIGS = ("locate", "locate_image", "locate_bytes")
KEYS = ("classes", "scores", "boxes", "areas", "num_boxes")


def rule_on_mask(mask, K=3):
    """At S = h = w both resample passes are the identity: a map of 0.0 / 1.0 values is the mask."""
    m = np.asarray(mask, bool)
    assert m.shape[0] == m.shape[1] and np.array_equal(L.mask_of(m.astype(np.float32), m.shape[0], Locate()), m)
    count, box, area = L.locate_rule(m.astype(np.float32), m.shape[0], Locate(boxes=K))
    assert box.dtype == np.int32 and area.dtype == np.uint32 and box.shape == (K, 4) and area.shape == (K,)
    return count, box.tolist(), area.tolist()


# ------------------------------------------------------------------------------ the rule: literal answers
def test_one_pixel():
    assert rule_on_mask([[1]]) == (1, [[0, 0, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]], [1, 0, 0])
    assert rule_on_mask([[0]]) == (0, [[0, 0, 0, 0]] * 3, [0, 0, 0])
    count, box, area = L.locate_rule(np.array([[0.3]], np.float32), 4, Locate(boxes=1, threshold=77))
    assert (count, box.tolist(), area.tolist()) == (0, [[0, 0, 0, 0]], [0])      # rint(0.3 * 255) = 76 < 77
    count, box, area = L.locate_rule(np.array([[0.3]], np.float32), 4, Locate(boxes=1, threshold=76))
    assert (count, box.tolist(), area.tolist()) == (1, [[0, 0, 4, 4]], [16])


def test_pixels_that_touch_at_a_corner_are_one_component():
    m = np.zeros((5, 5), bool)
    m[1, 1] = m[2, 2] = True                                      # two components under 4-connectivity
    assert rule_on_mask(m) == (1, [[1, 1, 3, 3], [0, 0, 0, 0], [0, 0, 0, 0]], [2, 0, 0])
    m[2, 2], m[2, 0] = False, True                                # the other diagonal
    assert rule_on_mask(m) == (1, [[1, 0, 3, 2], [0, 0, 0, 0], [0, 0, 0, 0]], [2, 0, 0])
    m[2, 0], m[1, 3] = False, True                                # a gap of one pixel: two
    assert rule_on_mask(m) == (2, [[1, 1, 2, 2], [1, 3, 2, 4], [0, 0, 0, 0]], [1, 1, 0])


def test_equal_areas_go_to_the_earlier_first_pixel():
    m = np.zeros((8, 8), bool)
    m[5:7, 0:3] = True                                            # first pixel (5, 0)
    m[1:4, 5:7] = True                                            # first pixel (1, 5): earlier in raster order
    m[0, 0] = True                                                # the earliest, but the smallest
    assert rule_on_mask(m) == (3, [[1, 5, 4, 7], [5, 0, 7, 3], [0, 0, 1, 1]], [6, 6, 1])
    assert rule_on_mask(m, K=1) == (3, [[1, 5, 4, 7]], [6])       # count is not clipped to K


def test_a_ring_is_one_component():
    m = np.zeros((9, 9), bool)
    m[1:8, 2:9] = True
    m[3:6, 4:7] = False
    assert rule_on_mask(m) == (1, [[1, 2, 8, 9], [0, 0, 0, 0], [0, 0, 0, 0]], [40, 0, 0])


@pytest.mark.parametrize("fill", [0.0, np.nan, -3.0, 0.19])
def test_a_map_below_the_threshold_answers_zeros(fill):
    count, box, area = L.locate_rule(np.full((3, 3), fill, np.float32), 9, Locate(boxes=4))
    assert count == 0 and not box.any() and not area.any() and box.shape == (4, 4) and area.shape == (4,)


# ------------------------------------------------------------------------------ second implementations
def scipy_rule(mask, K):
    """scipy's 8-connected labels, ranked as the rule says."""
    lab, n = ndimage.label(mask, structure=np.ones((3, 3)))
    comps = []
    for i, sl in enumerate(ndimage.find_objects(lab)):
        ys, xs = np.nonzero(lab[sl] == i + 1)
        first = (sl[0].start + int(ys[0])) * mask.shape[1] + sl[1].start + int(xs[0])
        comps.append((-len(ys), first, [sl[0].start, sl[1].start, sl[0].stop, sl[1].stop]))
    comps.sort()
    pad = K - len(comps[:K])
    return n, [c[2] for c in comps[:K]] + [[0, 0, 0, 0]] * pad, [-c[0] for c in comps[:K]] + [0] * pad


def flood_rule(mask, K):
    """A flood fill in plain loops over pixels, seeds in raster order."""
    H, W = mask.shape
    seen = np.zeros((H, W), bool)
    comps = []
    for y in range(H):
        for x in range(W):
            if not mask[y, x] or seen[y, x]:
                continue
            stack, area, box = [(y, x)], 0, [y, x, y + 1, x + 1]
            seen[y, x] = True
            while stack:
                cy, cx = stack.pop()
                area += 1
                box = [min(box[0], cy), min(box[1], cx), max(box[2], cy + 1), max(box[3], cx + 1)]
                for ny in range(max(cy - 1, 0), min(cy + 2, H)):
                    for nx in range(max(cx - 1, 0), min(cx + 2, W)):
                        if mask[ny, nx] and not seen[ny, nx]:
                            seen[ny, nx] = True
                            stack.append((ny, nx))
            comps.append((-area, y * W + x, box))
    n = len(comps)
    comps.sort()
    pad = K - len(comps[:K])
    return n, [c[2] for c in comps[:K]] + [[0, 0, 0, 0]] * pad, [-c[0] for c in comps[:K]] + [0] * pad


def spiral(n):
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = 0
        while True:
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                break
            y, x = ny, nx
            m[y, x] = True
            moved += 1
        if not moved:
            return m
        dy, dx = dx, -dy


def mask_families(n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.indices((n, n))
    comb = np.zeros((n, n), bool)
    comb[:, ::2] = True
    comb[-1] = True
    blobs = np.zeros((n, n), bool)
    blobs[2:6, n - 7:n - 2] = True
    blobs[n - 8:n - 4, 1:6] = True
    ring = np.zeros((n, n), bool)
    ring[3:n - 3, 3:n - 3] = True
    ring[6:n - 6, 6:n - 6] = False
    return {"checkerboard": (yy + xx) % 2 == 0, "dots": (yy % 2 == 0) & (xx % 2 == 0),
            "diagonals": (yy == xx) | (yy + xx == n - 1), "spiral": spiral(n), "comb": comb, "comb_up": comb[::-1].copy(),
            "blobs": blobs, "ring": ring, "ones": np.ones((n, n), bool), "zeros": np.zeros((n, n), bool),
            "noise": rng.random((n, n)) < 0.45}


def agree(mask, K, flood=True):
    got = L.select(*L.components(mask), K)
    got = (got[0], got[1].tolist(), got[2].tolist())
    assert got == scipy_rule(mask, K)
    if flood:
        assert got == flood_rule(mask, K)
    return got


@pytest.mark.parametrize("n", [33, 64])
def test_second_implementations_agree_on_every_mask_family(n):
    ms = mask_families(n, seed=n)
    for name, m in ms.items():
        for K in (1, 8):
            count, box, area = agree(m, K)
            assert (count, box, area) == rule_on_mask(m, K), name
    assert agree(ms["checkerboard"], 1) == (1, [[0, 0, n, n]], [(n * n + 1) // 2])
    assert agree(ms["dots"], 2) == (((n + 1) // 2) ** 2, [[0, 0, 1, 1], [0, 2, 1, 3]], [1, 1])
    for one in ("diagonals", "spiral", "comb", "comb_up", "ring", "ones"):
        assert agree(ms[one], 1)[0] == 1, one
    assert ndimage.label(ms["spiral"])[1] == 1                    # a genuine spiral: one component under 4-connectivity too
    assert agree(ms["blobs"], 2) == (2, [[2, n - 7, 6, n - 2], [n - 8, 1, n - 4, 6]], [20, 20])


def test_second_implementations_agree_on_upsampled_maps():
    """A 10 x 10 map at 299 with the flood fill; 7 x 7 at 224, 19 x 19 at 600 and the 64 x 64 noise map of the
    GPU test at 1024 with scipy; every threshold class and both filters."""
    rng = np.random.default_rng(12)
    for (h, S), thr, flt, flood in (((10, 299), 128, "bilinear", True), ((7, 224), 51, "bicubic", False),
                                    ((19, 600), 200, "bilinear", False), ((14, 224), 1, "bicubic", False)):
        heat = rng.random((h, h), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)
        spec = Locate(8, thr, flt)
        mask = L.mask_of(heat, S, spec)
        assert np.array_equal(mask, O.upsample(O.quantise(heat), S, flt) >= thr)
        count, box, area = L.locate_rule(heat, S, spec)
        assert (count, box.tolist(), area.tolist()) == agree(mask, 8, flood)
    noise = (np.random.default_rng(11).random((64, 64)) < 0.45).astype(np.float32)
    spec = Locate(8, 128, "bilinear")
    count, box, area = L.locate_rule(noise, 1024, spec)
    assert (count, box.tolist(), area.tolist()) == agree(L.mask_of(noise, 1024, spec), 8, flood=False) and count > 8
    yy, xx = np.indices((64, 64))
    board = ((yy + xx) % 2 == 0).astype(np.float32)
    spec = Locate(8, 128, "bicubic")                              # thousands of runs
    count, box, area = L.locate_rule(board, 299, spec)
    assert (count, box.tolist(), area.tolist()) == agree(L.mask_of(board, 299, spec), 8, flood=False)


def test_both_resample_passes_are_the_identity_at_the_maps_own_size():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 17, 64):
        q = O.quantise(rng.random((n, n), dtype=np.float32))
        for flt in O.FILTERS:
            assert np.array_equal(O.upsample(q, n, flt), q), (n, flt)


# ------------------------------------------------------------------------------ helpers around the rule
def test_boxes_and_areas_as_fractions():
    b = L.boxes_of(np.array([[[0, 1, 299, 100], [0, 0, 0, 0]]], np.int32), 299)
    assert b.dtype == np.float32 and b.shape == (1, 2, 4)
    assert b[0, 0].tolist() == [0.0, np.float32(1 / 299), 1.0, np.float32(100 / 299)] and not b[0, 1].any()
    a = L.areas_of(np.array([[299 * 299, 1, 0]], np.uint32), 299)
    assert a.dtype == np.float32 and a[0].tolist() == [1.0, np.float32(1 / 89401), 0.0]
    assert L.areas_of(np.array([1024 * 1024], np.uint32), 1024)[0] == 1.0


def test_row_pack_and_unpack_round_trip():
    rng = np.random.default_rng(5)
    n, h, w, K = 3, 2, 3, 4
    cl, sc = rng.integers(0, 10, n).astype(np.int32), rng.random(n, dtype=np.float32)
    heat = rng.random((n, h, w), dtype=np.float32)
    count = np.array([0, 1, 2 ** 19], np.uint32)
    box = rng.integers(0, 1025, (n, K, 4)).astype(np.int32)
    box[0, 0] = (0, 0, 1024, 1024)                                # x1 = y1 = 1024
    box[1, 1] = (1023, 1023, 1024, 1024)
    area = rng.integers(0, 1024 * 1024 + 1, (n, K)).astype(np.uint32)
    area[0, 0] = 1024 * 1024
    area[2, 3] = 0x7FC00001 & 0x1FFFFF
    rows = L.pack_rows(cl, sc, heat, count, box, area)
    assert rows.dtype == np.float32 and rows.shape == (n, 2 + h * w + 1 + 3 * K)
    got = L.unpack_rows(rows, h, w, K)
    for a, b in zip(got, (cl, sc, heat, count, box, area)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    tail = rows.view(np.uint32)[0, 2 + h * w:]
    assert tail[:4].tolist() == [0, 0, 1024 | 1024 << 16, 1024 * 1024]


def test_check_refusals():
    assert L.check(Locate()) == Locate(3, 51, "bilinear")
    for bad in (Locate(boxes=0), Locate(boxes=9), Locate(boxes=2.0), Locate(boxes=True), Locate(threshold=0),
                Locate(threshold=256), Locate(threshold=51.0), Locate(filter="lanczos"), Locate(filter="nearest")):
        with pytest.raises(ValueError, match="locate"):
            L.check(bad)
        with pytest.raises(ValueError, match="locate"):
            L.locate_rule(np.zeros((1, 1), np.float32), 2, bad)
    with pytest.raises(ValueError, match="upsample"):
        L.locate_rule(np.zeros((3, 3), np.float32), 2)
    with pytest.raises(ValueError, match="1024"):
        L.locate_rule(np.zeros((3, 3), np.float32), 1025)


def test_engine_arguments_are_refused_before_any_device_use():
    """No GPU here: an engine that got as far as its first device call would fail otherwise."""
    from kdl.engine.efficientnet import EfficientNetEngine
    from kdl.engine.resnet import ResNetEngine
    from kdl.engine.vit import ViTEngine
    from kdl.engine.xception import XceptionEngine
    for make in (lambda **kw: XceptionEngine({}, max_batch=2, device="cuda", **kw),
                 lambda **kw: ResNetEngine({}, max_batch=2, device="cuda", **kw),
                 lambda **kw: EfficientNetEngine({}, max_batch=2, device="cuda", **kw)):
        with pytest.raises(ValueError, match="explain=True or rollout=True"):
            make(locate=Locate())
        with pytest.raises(ValueError, match="explain=True or rollout=True"):
            make(topk=3, locate=Locate())
        with pytest.raises(ValueError, match="each extend the heatmap rows"):
            make(explain=True, overlay=Overlay(), locate=Locate())
        with pytest.raises(ValueError, match="each extend the heatmap rows"):
            make(explain=True, palette=Palette(), locate=Locate())
        with pytest.raises(ValueError, match="locate boxes"):
            make(explain=True, locate=Locate(boxes=9))
        with pytest.raises(ValueError, match="locate threshold"):
            make(explain=True, locate=Locate(threshold=0))
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        ViTEngine({}, max_batch=2, device="cuda", locate=Locate())
    with pytest.raises(ValueError, match="each extend the heatmap rows"):
        ViTEngine({}, max_batch=2, device="cuda", rollout=True, overlay=Overlay(), locate=Locate())
    with pytest.raises(ValueError, match="each extend the heatmap rows"):
        ViTEngine({}, max_batch=2, device="cuda", rollout=True, palette=Palette(), locate=Locate())


# ------------------------------------------------------------------------------ config, signatures
def _version(tmp_path, meta=None):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, **(meta or {})}))
    return d


def test_config_block_flag_and_errors(tmp_path):
    assert load_version_dir(_version(tmp_path / "none"), synthetic=True).locate is None
    assert load_version_dir(_version(tmp_path / "d", {"locate": {}}), synthetic=True).locate == Locate()
    assert Locate() == Locate(boxes=3, threshold=51, filter="bilinear")
    d = _version(tmp_path / "c", {"locate": {"boxes": 5, "threshold": 128, "filter": "bicubic"}})
    assert load_version_dir(d, synthetic=True).locate == Locate(5, 128, "bicubic")
    assert load_version_dir(d, synthetic=True, locate_boxes=8).locate == Locate(8, 128, "bicubic")
    assert load_version_dir(_version(tmp_path / "f"), synthetic=True, locate_boxes=2).locate == Locate(boxes=2)
    for i, block in enumerate(({"boxes": 0}, {"boxes": 9}, {"boxes": "three"}, {"boxes": 2.5}, {"threshold": 0},
                               {"threshold": 256}, {"threshold": 0.2}, {"filter": "lanczos"}, {"box": 3},
                               {"boxes": 3, "colors": 5}, 5, [3])):
        with pytest.raises(ValueError, match="synthetic.json"):
            load_version_dir(_version(tmp_path / f"bad{i}", {"locate": block}), synthetic=True)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="locate_boxes"):
            load_version_dir(_version(tmp_path / "g"), synthetic=True, locate_boxes=bad)


def test_flag_reaches_the_config(monkeypatch):
    from kdl.serving.config import config_from_args as parse_args
    base = ["--model_name", "m", "--model_base_path", "/tmp/m"]
    assert parse_args(base).locate_boxes is None
    assert parse_args(base + ["--locate_boxes", "3"]).locate_boxes == 3
    monkeypatch.setenv("KDL_LOCATE_BOXES", "6")
    assert parse_args(base).locate_boxes == 6
    assert parse_args(base + ["--locate_boxes", "2"]).locate_boxes == 2


FAMILIES = [("xception", (10, 10), 299, False), ("resnet50", (7, 7), 224, False),
            ("efficientnet_b7", (19, 19), 600, False), ("vit_b16", (14, 14), 224, True)]


@pytest.mark.parametrize("model,hw,S,rollout", FAMILIES)
def test_signatures_with_and_without_the_block(tmp_path, model, hw, S, rollout):
    from kdl.serving import outputs as OUT
    meta = {} if model == "xception" else {"model": model}
    plain = load_version_dir(_version(tmp_path / "plain", meta), synthetic=True)
    want = json.loads((GOLDEN / "metadata.json").read_text())[model]["plain"]["order"]
    assert list(plain.signatures) == want and not set(SIGS) & set(want) and plain.locate is None
    src = load_version_dir(_version(tmp_path / "with", {**meta, "locate": {"boxes": 4}}), synthetic=True)
    assert list(src.signatures) == want + list(SIGS)
    for name in want:                                            # the others are what they were
        assert src.signatures[name] == plain.signatures[name]
        assert OUT.kind_of(src.signatures[name]).name != "locate"
    for name in SIGS:
        sig = src.signatures[name]
        assert sig.explain == hw and sig.overlay == 0 and sig.rollout is rollout
        assert sig.input_dtype != P.DT_FLOAT and not sig.top_k and not sig.embed
        assert sig.outputs == (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)),
                               ("boxes", P.DT_FLOAT, (-1, 4, 4)), ("areas", P.DT_FLOAT, (-1, 4)),
                               ("num_boxes", P.DT_INT32, (-1, 1)))
        assert OUT.kind_of(sig).name == "locate"
        assert OUT.out_cols(sig, src, gpu=True) == OUT.out_cols(sig, src, gpu=False) == 2 + hw[0] * hw[1] + 1 + 12
        kw = OUT.engine_kwargs(sig, src, "cuda:0")
        assert kw == dict(rollout=True, locate=Locate(boxes=4)) if rollout else kw == dict(
            explain=True, locate=Locate(boxes=4))
    assert src.signatures["locate"].input_shape == (-1, S, S, 3)
    assert src.signatures["locate_image"].input_shape == src.signatures["serving_image"].input_shape
    assert src.signatures["locate_bytes"].input_key == src.signatures["serving_bytes"].input_key
    both = load_version_dir(_version(tmp_path / "both", {**meta, "locate": {}, "palette": {}}), synthetic=True)
    assert [OUT.kind_of(both.signatures[n]).name for n in ("palette", "locate")] == ["palette", "locate"]


def test_ten_kinds():
    from kdl.serving import outputs as OUT
    assert len(OUT.KINDS) == 10 and OUT.KINDS["locate"].trio == SIGS and OUT.KINDS["locate"].counter == "kdl_locate_total"
    assert "ten kinds" in OUT.__doc__


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


SPEC = Locate(boxes=4, threshold=140, filter="bicubic")
BLOCK = {"boxes": 4, "threshold": 140, "filter": "bicubic"}


@pytest.fixture(scope="module")
def jpeg():
    b = io.BytesIO()
    Image.open(PANTS).convert("RGB").save(b, "JPEG", quality=90)
    return b.getvalue()


def _answer(resp, n=1, K=4):
    assert sorted(resp.outputs) == sorted(KEYS)
    o = resp.outputs
    shapes = {k: [d.size for d in o[k].tensor_shape.dim] for k in KEYS}
    assert shapes == {"classes": [n, 1], "scores": [n, 1], "boxes": [n, K, 4], "areas": [n, K], "num_boxes": [n, 1]}
    assert [o[k].dtype for k in KEYS] == [P.DT_STRING, P.DT_FLOAT, P.DT_FLOAT, P.DT_FLOAT, P.DT_INT32]
    return {"classes": [v.decode() for v in o["classes"].string_val],
            "scores": np.asarray(o["scores"].float_val, np.float32),
            "boxes": np.asarray(o["boxes"].float_val, np.float32).reshape(n, K, 4),
            "areas": np.asarray(o["areas"].float_val, np.float32).reshape(n, K),
            "num_boxes": np.asarray(o["num_boxes"].int_val, np.int32).reshape(n, 1)}


def _post(url, body):
    try:
        with urllib.request.urlopen(urllib.request.Request(url, data=json.dumps(body).encode(), method="POST"),
                                    timeout=300) as r:
            return r.status, json.load(r)
    except urllib.error.HTTPError as e:
        return e.code, json.load(e)


@pytest.mark.parametrize("model,hw,S,rollout", FAMILIES)
def test_cpu_server_of_every_family(tmp_path, model, hw, S, rollout):
    """gRPC and REST Predict equal the rule on the map the family's own heatmap signature answers; metadata
    shapes; the counter; the null device's rows are zeros."""
    from kdl.serving.metrics import METRICS
    base = tmp_path / "clothing-model"
    _version(base, {"seed": 5, "locate": BLOCK, **({} if model == "xception" else {"model": model})})
    u8 = np.random.default_rng(S).integers(0, 256, (1, S, S, 3), dtype=np.uint8)
    srv = _server(base, "cpu")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            before = METRICS.snapshot()["counters"]
            a = _answer(stub.Predict(make_request(u8, signature="locate", input_key="images"), timeout=300))
            after = METRICS.snapshot()["counters"]
            r = stub.Predict(make_request(u8, signature="attention" if rollout else "explain", input_key="images"),
                             timeout=300).outputs
            req = P.GetModelMetadataRequest()
            req.model_spec.name = "clothing-model"
            req.metadata_field.append("signature_def")
            sdm = P.SignatureDefMap()
            stub.GetModelMetadata(req, timeout=5).metadata["signature_def"].Unpack(sdm)
        st, by_row = _post(f"http://127.0.0.1:{srv.rest_port}/v1/models/clothing-model:predict",
                           {"signature_name": "locate", "instances": u8.tolist()})
        st2, by_col = _post(f"http://127.0.0.1:{srv.rest_port}/v1/models/clothing-model:predict",
                            {"signature_name": "locate", "inputs": {"images": u8.tolist()}})
        runner = srv.manager.get("clothing-model", None, None).runner("locate")
        assert runner.out_cols == 2 + hw[0] * hw[1] + 1 + 12 and not runner.gpu and runner.kind == "locate"
        assert srv.manager.get("clothing-model", None, None).source.locate == SPEC
    finally:
        srv.stop(0)
    key_m = "kdl_locate_total{signature=locate}"
    assert after.get(key_m, 0) - before.get(key_m, 0) == 1
    assert after.get("kdl_explain_total{signature=locate}", 0) == 0
    heat = np.asarray(r["heatmap"].float_val, np.float32).reshape(hw)
    count, box, area = L.locate_rule(heat, S, SPEC)
    assert count >= 1 and area[0] > 0                               # the maps are divided by their maximum
    assert a["classes"] == [r["classes"].string_val[0].decode()]
    assert np.array_equal(a["scores"], np.asarray(r["scores"].float_val, np.float32))
    assert a["num_boxes"].tolist() == [[count]]
    assert np.array_equal(a["boxes"][0], L.boxes_of(box, S)) and np.array_equal(a["areas"][0], L.areas_of(area, S))
    for name in SIGS:
        out = sdm.signature_def[name].outputs
        want = {"classes": (P.DT_STRING, [-1, 1]), "scores": (P.DT_FLOAT, [-1, 1]), "boxes": (P.DT_FLOAT, [-1, 4, 4]),
                "areas": (P.DT_FLOAT, [-1, 4]), "num_boxes": (P.DT_INT32, [-1, 1])}
        assert sorted(out) == sorted(want)
        for k, (dt, shape) in want.items():
            assert out[k].dtype == dt and [d.size for d in out[k].tensor_shape.dim] == shape, (name, k)
    assert st == 200 and st2 == 200, (by_row, by_col)
    (one,) = by_row["predictions"]
    assert sorted(one) == sorted(KEYS) and one["classes"] == a["classes"] and one["num_boxes"] == [count]
    assert isinstance(one["num_boxes"][0], int)
    assert np.array_equal(np.asarray(one["boxes"], np.float32), a["boxes"][0])
    assert np.array_equal(np.asarray(one["areas"], np.float32), a["areas"][0])
    o = by_col["outputs"]
    assert o["classes"] == [a["classes"]] and o["num_boxes"] == [[count]]
    assert np.array_equal(np.asarray(o["boxes"], np.float32), a["boxes"])

    srv = _server(base, "null")
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            z = _answer(PredictionStub(ch).Predict(make_request(np.concatenate([u8, u8]), signature="locate",
                                                                input_key="images"), timeout=60), 2)
        labels = srv.manager.get("clothing-model", None, None).source.labels
    finally:
        srv.stop(0)
    assert z["classes"] == [labels[0]] * 2 and (z["scores"] == 0).all()
    assert not z["boxes"].any() and not z["areas"].any() and not z["num_boxes"].any()


@pytest.fixture(scope="module")
def server(tmp_path_factory):
    base = tmp_path_factory.mktemp("locate") / "clothing-model"
    _version(base, {"seed": 5, "locate": BLOCK})
    srv = _server(base, "cpu")
    yield srv
    srv.stop(0)


def _inputs(jpeg):
    img = pp.load_image(jpeg)
    return {"locate": (pp.to_uint8(img)[None], "images"), "locate_image": (np.asarray(img, np.uint8)[None], "images"),
            "locate_bytes": ([jpeg], "image_bytes")}


@pytest.fixture(scope="module")
def answers(server, jpeg):
    """One JPEG through the three locate signatures and through the three explain signatures."""
    got, exp = {}, {}
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        stub = PredictionStub(ch)
        for name, (x, key) in _inputs(jpeg).items():
            got[name] = _answer(stub.Predict(make_request(x, signature=name, input_key=key), timeout=300))
            r = stub.Predict(make_request(x, signature=name.replace("locate", "explain"), input_key=key), timeout=300)
            exp[name] = (r.outputs["classes"].string_val[0].decode(), np.asarray(r.outputs["scores"].float_val, np.float32),
                         np.asarray(r.outputs["heatmap"].float_val, np.float32).reshape(10, 10))
        req = make_request(_inputs(jpeg)["locate"][0], signature="locate", input_key="images")
        req.output_filter.extend(["boxes", "num_boxes"])
        got["filtered"] = stub.Predict(req, timeout=300)
        req = make_request(_inputs(jpeg)["locate"][0], signature="locate", input_key="images")
        req.output_filter.append("heatmap")                       # not an output of this kind
        with pytest.raises(grpc.RpcError) as e:
            stub.Predict(req, timeout=30)
        assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    return got, exp


def test_three_signatures_equal_the_rule_on_the_oracles_map(answers):
    got, exp = answers
    for name in SIGS:
        a, (label, score, heat) = got[name], exp[name]
        assert a["classes"] == [label] and np.array_equal(a["scores"], score), name
        count, box, area = L.locate_rule(heat, 299, SPEC)
        assert count >= 1 and a["num_boxes"].tolist() == [[count]], name
        assert np.array_equal(a["boxes"][0], L.boxes_of(box, 299)), name
        assert np.array_equal(a["areas"][0], L.areas_of(area, 299)), name
    f = got["filtered"]
    assert sorted(f.outputs) == ["boxes", "num_boxes"]
    assert list(f.outputs["num_boxes"].int_val) == got["locate"]["num_boxes"].reshape(-1).tolist()


# ------------------------------------------------------------------------------ gateway
@pytest.mark.parametrize("mode", ["uint8", "bytes", "raw"])
def test_gateway_locate(server, answers, jpeg, monkeypatch, mode):
    got, _ = answers
    a = got[{"bytes": "locate_bytes", "raw": "locate_image"}.get(mode, "locate")]
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    with grpc.insecure_channel(f"127.0.0.1:{server.grpc_port}") as ch:
        c = create_app(GatewayConfig({"GATEWAY_MODE": mode}), channel=ch).test_client()
        r = c.post("/locate", json={"url": "http://example.invalid/pants.jpg"})
        assert r.status_code == 200, r.data
        out = r.get_json()
        assert sorted(out) == ["boxes", "count", "label", "score"]
        assert out["label"] == a["classes"][0] and np.isclose(out["score"], a["scores"][0], rtol=1e-6)
        assert out["count"] == int(a["num_boxes"][0, 0])
        live = [j for j in range(4) if a["areas"][0, j] > 0]
        assert len(out["boxes"]) == len(live) >= 1
        for e, j in zip(out["boxes"], live):
            assert sorted(e) == ["area", "box"]
            assert np.array_equal(np.asarray(e["box"], np.float32), a["boxes"][0, j])
            assert np.float32(e["area"]) == a["areas"][0, j]
        assert c.post("/locate", json={"nope": 1}).status_code == 400


def test_response_parser_drops_empty_boxes():
    resp = P.PredictResponse()
    o = resp.outputs
    o["classes"].string_val.append(b"pants")
    o["scores"].float_val.append(0.75)
    o["boxes"].float_val.extend([0.0, 0.25, 1.0, 0.5, 0.5, 0.5, 0.75, 1.0, 0.0, 0.0, 0.0, 0.0])
    o["areas"].float_val.extend([0.25, 0.125, 0.0])
    for d in (1, 3):
        o["areas"].tensor_shape.dim.add(size=d)
    o["num_boxes"].int_val.append(2)
    assert process_locate_response(resp) == [{"label": "pants", "score": 0.75, "count": 2, "boxes": [
        {"box": [0.0, 0.25, 1.0, 0.5], "area": 0.25}, {"box": [0.5, 0.5, 0.75, 1.0], "area": 0.125}]}]
