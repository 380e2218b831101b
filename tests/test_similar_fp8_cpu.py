"""The fp8 gallery of kdl.serving.similar without a GPU: the quantiser, the rule on codes and scales,
the "dtype" key and --similar_dtype, and a --device null server of an fp8 version."""
import json

import grpc
import numpy as np
import pytest

from kdl.gateway.client import PredictionStub, make_request
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig, config_from_args
from kdl.serving.server import ModelServer
from kdl.serving.similar import fp8_to_f64, load_gallery, quantize_fp8, resolve, resolve_stored, similar_rule

F = 2048


def _version(d, meta, gallery):
    (d / "1").mkdir(parents=True)
    (d / "1" / "synthetic.json").write_text(json.dumps({"seed": 0, **meta}))
    np.save(d / "1" / "gallery.npy", gallery)
    return d / "1"


def _gallery(n=6):
    return np.random.default_rng(1).standard_normal((n, F)).astype(np.float32)


def test_quantiser():
    x = np.random.default_rng(0).standard_normal((5, 64)) * np.array([1e-6, 1.0, 1e4, 1.0, 1.0])[:, None]
    x[3] = 0
    # row 4: max / 448 is 1.4 units of the smallest fp32 subnormal and rounds to 1 unit, so max / s_j is 628:
    # without the clip the cast gives the NaN code 0x7F (and this row cannot meet the relative bound)
    x[4] = 0
    x[4, :3] = [8.8e-43, -8.8e-43, 1.4e-45]
    codes, scale = quantize_fp8(x)
    assert codes.dtype == np.uint8 and scale.dtype == np.float32 and codes.shape == x.shape
    assert ((codes & 0x7F) != 0x7F).all()                                   # no NaN codes
    assert scale[3] == 1.0 and (codes[3] == 0).all()
    assert scale[4] == np.float32(1.4e-45) and codes[4, :3].tolist() == [0x7E, 0xFE, 0x38]      # +-448 and 1.0
    y, v = x / scale.astype(np.float64)[:, None], fp8_to_f64(codes)
    assert (np.abs(y - v) <= np.maximum(2.0 ** -4 * np.abs(y), 2.0 ** -10))[:4].all()
    assert (np.abs(v).max(axis=1)[[0, 1, 2, 4]] == 448).all()


def test_rule_on_codes_and_scales():
    rng = np.random.default_rng(2)
    codes, scale = quantize_fp8(rng.standard_normal((9, 32)))
    codes[4] = codes[1]
    scale[4] = scale[1]                                                     # a tie: by row index
    q = rng.standard_normal((3, 32)).astype(np.float32)
    idx, sc = similar_rule(q, codes, 9, "dot", scale)
    for b in range(3):
        s = [float(scale[j]) * sum(float(q[b, i]) * float(fp8_to_f64(codes[j, i])) for i in range(32)) for j in range(9)]
        assert idx[b].tolist() == sorted(range(9), key=lambda j: (-s[j], j))
        assert np.allclose(sc[b], np.array(s)[idx[b]], rtol=1e-6, atol=1e-9)


def test_dtype_key_flag_and_default(tmp_path):
    d = _version(tmp_path / "f", {"similar": {"dtype": "fp8"}}, _gallery())
    k, metric, codes, ids, dtype, scale = resolve_stored(d, F)
    assert dtype == "fp8" and codes.dtype == np.uint8 and scale.shape == (6,) and len(resolve(d, F)) == 4
    assert resolve_stored(d, F, dtype_flag="bf16")[4:] == ("bf16", None)    # the flag overrides the json
    with pytest.raises(ValueError, match=r"synthetic\.json.*dtype"):
        load_version_dir(_version(tmp_path / "bad", {"similar": {"dtype": "int8"}}, _gallery()), synthetic=True)
    assert config_from_args(["--similar_dtype", "fp8"], env={"KDL_SIMILAR_DTYPE": "bf16"}).similar_dtype == "fp8"
    assert config_from_args([], env={"KDL_SIMILAR_DTYPE": "fp8"}).similar_dtype == "fp8"
    assert config_from_args([], env={}).similar_dtype is None
    with pytest.raises(ValueError, match="KDL_SIMILAR_DTYPE"):
        config_from_args([], env={"KDL_SIMILAR_DTYPE": "int8"})
    plain = _version(tmp_path / "p", {}, _gallery())
    src = load_version_dir(plain, synthetic=True)
    assert src.similar_dtype == "bf16" and src.gallery_scale is None
    assert np.array_equal(src.gallery, load_gallery(plain / "gallery.npy", F, "cosine"))
    assert load_version_dir(plain, synthetic=True, similar_dtype="fp8").gallery.dtype == np.uint8


def test_null_server_answers_by_the_rule(tmp_path):
    base = tmp_path / "clothing-model"
    _version(base, {"similar": {"dtype": "fp8", "top_k": 3}}, _gallery())
    cfg = ServerConfig(port=0, rest_api_port=0, model_name="clothing-model", model_base_path=str(base), device="null",
                       host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend="python",
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=500, allowed_batch_sizes=[2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        src = srv.manager.get("clothing-model", None, None).source
        assert src.similar_dtype == "fp8" and src.gallery.dtype == np.uint8
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            out = PredictionStub(ch).Predict(make_request(np.zeros((1, 299, 299, 3), np.uint8), signature="similar",
                                                          input_key="images"), timeout=120).outputs
        rows = np.arange(F, dtype=np.float32)[None]                # the null device's row: first byte of the item + k
        idx, sc = similar_rule(rows, src.gallery, 3, "cosine", src.gallery_scale)
        assert [v.decode() for v in out["ids"].string_val] == [str(j) for j in idx[0]]
        assert np.array_equal(np.asarray(out["scores"].float_val, np.float32), sc[0])
    finally:
        srv.stop(0)
