"""kdl/serving/png_encode.py png_rule: its oracle is the decoder."""
import io
import json
import zlib

import grpc
import numpy as np
import pytest
from PIL import Image

from _jpeg_cases import encode, pants
from _png_cases import CONTENTS, SIZES, cap_of, cutout_like, picture
from kdl.engine.base import CutoutPng
from kdl.gateway import preprocess as pp
from kdl.gateway.app import GatewayConfig, create_app
from kdl.gateway.client import PredictionStub, make_request, process_cutout_png_response, process_cutout_response
from kdl.serving import png_encode as E
from kdl.serving import protos as P
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer


@pytest.mark.parametrize("C", (3, 4))
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("content", CONTENTS)
def test_round_trip(content, H, W, C):
    pic = picture(content, H, W, C)
    file = E.png_rule(pic[None], cap_of(content, H, W, C))[0]
    im = Image.open(io.BytesIO(file))
    assert im.mode == ("RGB" if C == 3 else "RGBA") and np.array_equal(np.asarray(im), pic)
    idat = E.idat_of(file)
    assert idat[:2] == b"\x78\x01" and idat[2] & 1 == 1                      # one final block
    assert zlib.decompress(idat) == E.filter_rows(pic).tobytes()
    assert len(file) == len(idat) + E.FILE_OVERHEAD - 6


def test_rows_are_segments_and_tokens_follow_the_rule():
    """A run past 258 splits, a tail shorter than the minimum match is literals, no match leaves its row."""
    f = np.zeros((2, 301), np.uint8)
    f[0, 0], f[1, 0], f[1, 298:] = 1, 1, (7, 7, 7)
    lit, length, which = E.tokens(f, 3)
    assert length.tolist() == [0, 0, 258, 41, 0, 0, 258, 38, 0, 0, 0]
    assert lit[[0, 1, 4, 5, 8, 9, 10]].tolist() == [1, 0, 1, 0, 7, 7, 7] and not which.any()


@pytest.mark.parametrize("limit,counts", [(15, [int(round(1.618 ** i)) for i in range(30)] + [1] * 40), (7, [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89]),
                                          (15, [0, 9, 0]), (15, [4, 0, 4])])
def test_code_lengths_are_limited_complete_and_ordered(limit, counts):
    lens = E.code_lengths(counts, limit)
    used = [(c, l) for c, l in zip(counts, lens) if c]
    assert all(1 <= l <= limit for _, l in used) and all(l == 0 for c, l in zip(counts, lens) if not c)
    assert sum(2.0 ** -l for _, l in used) == (1.0 if len(used) > 1 else 0.5)
    assert all(l1 >= l2 for (c1, l1) in used for (c2, l2) in used if c1 < c2)


@pytest.mark.parametrize("S", (224, 299, 600))
def test_the_photograph_fits_the_default_cap(S):
    rgba = cutout_like(np.asarray(pants(S, S)))
    file = E.png_rule(rgba[None])[0]
    assert 0 < len(file) <= E.default_cap(S, S, 4)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(file))), rgba)


def test_overflow_is_an_empty_file():
    pics = np.stack([picture("noise", 17, 299, 4), picture("zero", 17, 299, 4)])
    full = E.png_rule(pics, 1 << 20)
    assert E.png_rule(pics, len(full[0]) - 1) == [b"", full[1]]
    assert E.png_rule(pics, len(full[0])) == full
    assert E.rows_of([b"", b"abcde"], 6).tolist() == [[0, 0, 0], [5, 0x64636261, 0x65]]


# ------------------------------------------------------------------------------ loading, a CPU server, the gateway
SIGS = ("cutout_png", "cutout_png_image", "cutout_png_bytes")


def _version(tmp_path, meta=None):
    d = tmp_path / "1"
    d.mkdir(parents=True, exist_ok=True)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, **(meta or {})}))
    return d


@pytest.mark.parametrize("model,hw,S,rollout", [("xception", (10, 10), 299, False), ("vit_b16", (14, 14), 224, True)])
def test_signatures_with_and_without_the_block(tmp_path, model, hw, S, rollout):
    from kdl.serving import outputs as OUT
    meta = {"cutout": {}} if model == "xception" else {"model": model, "cutout": {}}
    plain = load_version_dir(_version(tmp_path / "plain", meta), synthetic=True)
    assert not set(SIGS) & set(plain.signatures) and plain.cutout_png is None
    src = load_version_dir(_version(tmp_path / "with", {**meta, "cutout_png": {"max_bytes": None}}), synthetic=True)
    flagged = load_version_dir(_version(tmp_path / "flag", meta), synthetic=True, cutout_png=True)
    assert list(src.signatures) == list(flagged.signatures) == list(plain.signatures) + list(SIGS)
    assert src.cutout_png == flagged.cutout_png == CutoutPng(None)
    for name, sig in plain.signatures.items():                   # the others are what they were
        assert src.signatures[name] == sig and OUT.kind_of(src.signatures[name]).name == OUT.kind_of(sig).name
    cap = E.default_cap(S, S, 4)
    for name in SIGS:
        sig = src.signatures[name]
        assert sig.outputs == (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)),
                               ("coverage", P.DT_FLOAT, (-1, 1)), ("png_bytes", P.DT_STRING, (-1,)))
        kind = OUT.kind_of(sig)
        assert kind.name == "cutout_png" and kind.trio == SIGS and kind.counter == "kdl_cutout_png_total"
        assert OUT.out_cols(sig, src, gpu=True) == OUT.out_cols(sig, src, gpu=False) == 2 + hw[0] * hw[1] + 2 + (cap + 3) // 4
        kw = OUT.engine_kwargs(sig, src, "cuda:0")
        assert kw.pop("cutout_png") == CutoutPng(None) and kw == OUT.engine_kwargs(src.signatures["cutout"], src, "cuda:0")
    assert OUT.WRAPPED["cutout_png_bytes"] == (1, "cutout_png") and len(OUT.KINDS) == 10


def test_refusals_at_load(tmp_path):
    with pytest.raises(ValueError, match="needs the cutout signatures"):
        load_version_dir(_version(tmp_path / "a", {"cutout_png": {}}), synthetic=True)
    with pytest.raises(ValueError, match="needs the cutout signatures"):
        load_version_dir(_version(tmp_path / "b"), synthetic=True, cutout_png=True)
    for i, bad in enumerate(({"max_byte": 5}, {"max_bytes": 0}, {"max_bytes": "big"}, {"max_bytes": True}, 5)):
        with pytest.raises(ValueError, match="synthetic.json"):
            load_version_dir(_version(tmp_path / f"bad{i}", {"cutout": {}, "cutout_png": bad}), synthetic=True)
    from kdl.serving.config import config_from_args
    base = ["--model_name", "m", "--model_base_path", "/tmp/m"]
    assert not config_from_args(base).cutout_png and config_from_args(base + ["--cutout_png"]).cutout_png
    assert config_from_args(base, env={"KDL_CUTOUT_PNG": "true"}).cutout_png


def test_rows_round_trip():
    heat = np.arange(12, dtype=np.float32).reshape(2, 2, 3)
    rows = E.pack_rows([3, 4], [0.5, 0.25], heat, [7, 1 << 31], [b"abcde", b"x" * 9], 8)
    k, s, h, counts, files = E.unpack_rows(rows, 2, 3, 8)
    assert rows.shape == (2, 2 + 6 + 2 + 2) and k.tolist() == [3, 4] and np.array_equal(h, heat)
    assert counts.tolist() == [7, 1 << 31] and files == [b"abcde", b""]


def _server(base, device):
    cfg = ServerConfig(port=0, rest_api_port=0, model_name="clothing-model", model_base_path=str(base),
                       device=device, host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend="python",
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=500, allowed_batch_sizes=[1, 2]))
    return ModelServer(cfg).start(block_until_loaded=True)


@pytest.mark.parametrize("device", ["cpu", "null"])
def test_a_server_and_the_gateway(tmp_path, monkeypatch, device):
    """A CPU server's cutout_png file is png_rule of its cutout picture, and png_server hands it on untouched; a
    null server's rows are zero, so its file is empty: 502."""
    base = tmp_path / "clothing-model"
    _version(base, {"seed": 5, "cutout": {"gate": 40}, "cutout_png": {}})
    jpeg = encode(pants(320, 300), quality=90)
    monkeypatch.setattr(pp, "fetch", lambda url, timeout=10.0: jpeg)
    srv = _server(base, device)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            got = stub.Predict(make_request([jpeg], signature="cutout_png_bytes", input_key="image_bytes"), timeout=300)
            raw = stub.Predict(make_request([jpeg], signature="cutout_bytes", input_key="image_bytes"), timeout=300)
            c = create_app(GatewayConfig({"GATEWAY_MODE": "bytes"}), channel=ch).test_client()
            r = c.post("/cutout", json={"url": "http://example.invalid/pants.jpg", "format": "png_server"})
            old = c.post("/cutout", json={"url": "http://example.invalid/pants.jpg"})
    finally:
        srv.stop(0)
    o = got.outputs
    assert sorted(o) == sorted(E.OUTPUT_KEYS) and o["png_bytes"].dtype == P.DT_STRING
    assert [d.size for d in o["png_bytes"].tensor_shape.dim] == [1]
    (ans,), (want,) = process_cutout_png_response(got), process_cutout_response(raw)
    assert (ans["label"], ans["score"], ans["coverage"]) == (want["label"], want["score"], want["coverage"])
    assert old.status_code == 200 and np.array_equal(np.asarray(Image.open(io.BytesIO(old.data))), want["picture"])
    if device == "null":
        assert ans["png"] == b"" and r.status_code == 502 and "max_bytes" in r.get_json()["error"]
        return
    assert ans["png"] == E.png_rule(want["picture"][None])[0] != b""
    assert r.status_code == 200 and r.mimetype == "image/png" and r.data == ans["png"]
    assert r.headers["X-KDL-Label"] == want["label"] and np.float32(float(r.headers["X-KDL-Coverage"])) == np.float32(want["coverage"])
