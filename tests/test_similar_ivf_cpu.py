"""The gallery index without a GPU: ``ivf_rule`` against ``similar_rule``, the stored form that
``load_ivf`` gives and what it refuses, and a ``--device cpu`` server of a version indexed by ``build_ivf``."""
import json

import grpc
import numpy as np
import pytest
import torch

from kdl.engine import registry
from kdl.gateway.client import PredictionStub, make_request
from kdl.serving.backend import load_version_dir
from kdl.serving.config import BatchingParams, ServerConfig, config_from_args
from kdl.serving.server import ModelServer
from kdl.serving.similar import (GALLERY_CHUNK, build_ivf, chunk_table, ivf_rule, load_gallery, load_ivf,
                                 similar_rule)

F = 2048


def _index(tmp_path, n=40, lists=5, f=16, seed=0):
    rng = np.random.default_rng(seed)
    np.save(tmp_path / "gallery.npy", rng.standard_normal((n, f)).astype(np.float32))
    np.save(tmp_path / "c.npy", rng.standard_normal((lists, f)).astype(np.float32))
    a = rng.integers(0, lists, n).astype(np.int32)
    a[a == 3] = 2                                                  # list 3 is empty
    np.save(tmp_path / "l.npy", a)
    return a


def test_probing_every_list_is_the_dense_rule(tmp_path):
    a = _index(tmp_path)
    g = load_gallery(tmp_path / "gallery.npy", 16)
    cbits, offsets, order = load_ivf(tmp_path / "c.npy", tmp_path / "l.npy", 40, 16)
    q = np.random.default_rng(1).standard_normal((3, 16)).astype(np.float32)
    q[2] = 0                                                       # every score equal: ties by stored position
    idx, sc = ivf_rule(q, cbits, g[order], offsets, 7, 5, "cosine")
    want_idx, want_sc = similar_rule(q, g[order], 7, "cosine")
    assert idx.dtype == np.int32 and sc.dtype == np.float32
    assert np.array_equal(idx, want_idx) and np.array_equal(sc, want_sc)
    assert idx[2].tolist() == list(range(7))
    # one list probed: only its rows, and (-1, -inf) once they run out
    idx, sc = ivf_rule(np.load(tmp_path / "c.npy")[1:2], cbits, g[order], offsets, 40, 1, "cosine")   # centroid 1 itself
    n = int((a == 1).sum())
    assert 0 < n < 40 and sorted(order[idx[0, :n]].tolist()) == np.flatnonzero(a == 1).tolist()
    assert (idx[0, n:] == -1).all() and np.isneginf(sc[0, n:]).all() and np.isfinite(sc[0, :n]).all()


def test_load_ivf_stored_form_and_refusals(tmp_path):
    a = _index(tmp_path)
    cbits, offsets, order = load_ivf(tmp_path / "c.npy", tmp_path / "l.npy", 40, 16)
    assert np.array_equal(cbits, load_gallery(tmp_path / "c.npy", 16, "cosine"))     # normalised, bf16
    assert offsets.dtype == np.int32 and offsets.tolist() == np.concatenate([[0], np.cumsum(np.bincount(a, minlength=5))]).tolist()
    for l in range(5):                                             # a list: its rows in ascending original order
        assert order[offsets[l]:offsets[l + 1]].tolist() == np.flatnonzero(a == l).tolist()
    t = chunk_table(np.array([0, 0, 1, GALLERY_CHUNK + 1, 3 * GALLERY_CHUNK + 4], np.int32))
    assert t.dtype == np.int32 and t.tolist() == [[1, 0, 1], [2, 1, GALLERY_CHUNK], [3, GALLERY_CHUNK + 1, GALLERY_CHUNK],
                                                  [3, 2 * GALLERY_CHUNK + 1, GALLERY_CHUNK], [3, 3 * GALLERY_CHUNK + 1, 3]]
    c = np.load(tmp_path / "c.npy")
    bad = {"c64": (c.astype(np.float64), a, "float32"), "cshape": (c[:, :8], a, "float32"),
           "cnan": (np.where(np.eye(5, 16) > 0, np.nan, c).astype(np.float32), a, "NaN or infinite"),
           "l64": (c, a.astype(np.int64), "int32"), "lshort": (c, a[:-1], "int32"),
           "lneg": (c, np.where(np.arange(40) == 3, -1, a).astype(np.int32), "list ids"),
           "lbig": (c, np.where(np.arange(40) == 3, 5, a).astype(np.int32), "list ids")}
    for name, (cc, aa, msg) in bad.items():
        np.save(tmp_path / f"{name}.npy", cc if name[0] == "c" else aa)
        files = (tmp_path / f"{name}.npy", tmp_path / "l.npy") if name[0] == "c" else (tmp_path / "c.npy", tmp_path / f"{name}.npy")
        with pytest.raises(ValueError, match=rf"{name}\.npy.*{msg}"):
            load_ivf(*files, 40, 16)
    import kdl.serving.similar as S
    with pytest.MonkeyPatch.context() as mp:                       # L above kGalleryMaxN
        mp.setattr(S, "GALLERY_MAX_N", 4)
        with pytest.raises(ValueError, match=r"c\.npy.*exceed"):
            load_ivf(tmp_path / "c.npy", tmp_path / "l.npy", 40, 16)


def _version(base, meta, n=60, lists=6):
    d = base / "1"
    d.mkdir(parents=True)
    gal = np.random.default_rng(8).standard_normal((n, F)).astype(np.float32)
    c, a = build_ivf(gal, lists, rounds=2)
    (d / "synthetic.json").write_text(json.dumps({"seed": 5, "similar": {"top_k": 4, **meta}}))
    np.save(d / "gallery.npy", gal)
    np.save(d / "gallery_centroids.npy", c)
    np.save(d / "gallery_lists.npy", a)
    (d / "gallery_ids.txt").write_text("".join(f"item-{i:02d}\n" for i in range(n)))
    return d, a


def test_cpu_server_follows_ivf_rule(tmp_path):
    base = tmp_path / "clothing-model"
    d, _ = _version(base, {"index": "ivf", "nprobe": 1}, n=3, lists=3)            # one row per list: K = 3 runs out
    assert load_version_dir(d, synthetic=True, similar_nprobe=3).gallery_ivf.nprobe == 3     # flag > file
    assert config_from_args(["--similar_nprobe", "3"], env={"KDL_SIMILAR_NPROBE": "9"}).similar_nprobe == 3
    with pytest.raises(ValueError, match=r"synthetic\.json.*nprobe"):
        load_version_dir(d, synthetic=True, similar_nprobe=4)                     # above L = 3
    px = np.random.default_rng(3).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)
    srv = ModelServer(ServerConfig(port=0, rest_api_port=0, model_name="clothing-model", model_base_path=str(base),
                                   device="cpu", host="127.0.0.1", file_system_poll_wait_seconds=0, grpc_frontend="python",
                                   batching=BatchingParams(max_batch_size=2, batch_timeout_micros=500,
                                                           allowed_batch_sizes=[2]))).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            out = PredictionStub(ch).Predict(make_request(px, signature="similar", input_key="images"), timeout=120).outputs
        src = srv.manager.get("clothing-model", None, None).source
        rows = registry.get("xception").feature_oracle(src.params, torch.from_numpy(px)).numpy()
        ivf = src.gallery_ivf
        idx, sc = ivf_rule(rows, ivf.centroids, src.gallery, ivf.offsets, 3, 1, "cosine")
        assert (idx[:, 0] >= 0).all() and (idx[:, 1:] == -1).all()
        want = [src.gallery_ids[j] if j >= 0 else "" for j in idx.ravel()]
        assert [v.decode() for v in out["ids"].string_val] == want
        got = np.asarray(out["scores"].float_val, np.float32).reshape(2, 3)
        assert np.allclose(got[:, 0], sc[:, 0], rtol=1e-5, atol=1e-6) and np.isneginf(got[:, 1:]).all()
    finally:
        srv.stop(0)
