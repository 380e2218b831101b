"""kdl/serving/outputs.py: one description per kind of result row.

A characterisation test. The fixtures under tests/golden/outputs/ were recorded from the answer
builders and the loader as they were before the kinds were described in one table (one builder per
kind and transport, one ``add_signatures`` loop per kind): for hand-made packed rows of every kind,
the gRPC PredictResponse parsed back to a dict, the REST body by row and by column, each with and
without an ``output_filter``, and the counters bumped; and the signatures and ``signature_def`` of
the synthetic version of every family, with and without a gallery. No model runs here."""
import dataclasses
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
from google.protobuf import json_format

from kdl.serving import protos as P
from kdl.serving.backend import NATIVE_SIGNATURE, SignatureInfo, load_version_dir
from kdl.serving.metrics import METRICS

GOLDEN = Path(__file__).parent / "golden" / "outputs"
KINDS = ["logits", "classify", "embed", "similar", "explain", "attention", "overlay"]
FAMILIES = ["xception", "resnet50", "vit_b16", "efficientnet_b7"]
K, CLASSES, F, HW, S = 2, 3, 8, (2, 3), 5          # S * S * 3 = 75: the picture's last word has a pad byte
SERVABLE = SimpleNamespace(name="m", version=3, source=SimpleNamespace(
    labels=["shirt", "hat", "shoe"], gallery_ids=["a7", "b9"]))


def case(kind: str):
    """(SignatureInfo, packed rows [2, words]) of ``kind``, at the smallest sizes that have every part."""
    from kdl.serving import classify, explain, overlay
    u8 = dict(input_key="images", input_dtype=P.DT_UINT8)
    pair = lambda first: ((first, P.DT_STRING, (-1, K)), ("scores", P.DT_FLOAT, (-1, K)))   # noqa: E731
    heat = np.array([[[0.0, 0.25, 1.0], [0.5, 0.125, 0.75]], [[1.0, 0.0, 0.0], [0.0, 0.0, 0.5]]], np.float32)
    maps = (("classes", P.DT_STRING, (-1, 1)), ("scores", P.DT_FLOAT, (-1, 1)), ("heatmap", P.DT_FLOAT, (-1, *HW)))
    top = (np.array([1, 7], np.int32), np.array([0.5, 0.25], np.float32))      # class 7 has no label
    if kind == "logits":
        return (SignatureInfo(NATIVE_SIGNATURE, output_key="dense_7", output_shape=(-1, CLASSES), **u8),
                np.array([[0.5, -1.25, 2.0], [3.0, 0.0, -0.75]], np.float32))
    if kind == "classify":
        return (SignatureInfo("classify", output_key="classes", output_shape=(-1, K), outputs=pair("classes"),
                              top_k=K, **u8),
                classify.pack_rows(np.array([[2, 0], [0, 1]]), np.array([[0.75, 0.125], [0.5, 0.25]])))
    if kind == "embed":
        return (SignatureInfo("embed", output_key="embedding", output_shape=(-1, F), embed="l2", **u8),
                (np.arange(2 * F, dtype=np.float32).reshape(2, F) - 5) / 8)
    if kind == "similar":                                                       # row 5 is not in the gallery
        return (SignatureInfo("similar", output_key="ids", output_shape=(-1, K), outputs=pair("ids"), top_k=K,
                              similar=True, **u8),
                classify.pack_rows(np.array([[1, 0], [0, 5]]), np.array([[0.875, -0.5], [0.25, 0.125]])))
    if kind in ("explain", "attention"):
        return (SignatureInfo(kind, output_key="classes", output_shape=(-1, 1), outputs=maps, explain=HW,
                              rollout=kind == "attention", **u8),
                explain.pack_rows(*top, heat))
    pics = (np.arange(2 * S * S * 3) * 7 % 256).astype(np.uint8).reshape(2, S, S, 3)
    return (SignatureInfo("overlay", output_key="classes", output_shape=(-1, 1), explain=HW, overlay=S,
                          outputs=maps + (("overlay", P.DT_UINT8, (-1, S, S, 3)),), **u8),
            overlay.pack_rows(*top, heat, pics))


def bumped(fn):
    """(fn(), {counter: how much fn() added to it})."""
    before = dict(METRICS.counters)
    out = fn()
    after = dict(METRICS.counters)
    return out, {f"{name}{dict(labels)}": v - before.get((name, labels), 0)
                 for (name, labels), v in sorted(after.items()) if v != before.get((name, labels), 0)}


def answers(kind: str, grpc_answer, rest_body) -> dict:
    """Everything recorded of one kind: ``grpc_answer(s, sig, rows, output_filter) -> bytes`` and
    ``rest_body(s, sig, rows, by_row) -> dict`` are the builders under test."""
    sig, rows = case(kind)
    out = {}
    for tag, filt in (("all", []), ("one", [sig.output_specs()[-1][0]])):
        raw, counted = bumped(lambda: grpc_answer(SERVABLE, sig, rows.copy(), filt))
        out[f"grpc_{tag}"] = {"response": json_format.MessageToDict(P.PredictResponse.FromString(raw)),
                              "counters": counted}
    for tag, by_row in (("row", True), ("column", False)):
        body, counted = bumped(lambda: rest_body(SERVABLE, sig, rows.copy(), by_row))
        out[f"rest_{tag}"] = {"body": body, "counters": counted}
    return json.loads(json.dumps(out))


def version_dir(tmp: Path, family: str, gallery: bool) -> Path:
    from kdl.engine import registry
    d = tmp / f"{family}_{int(gallery)}"
    d.mkdir()
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, "model": family}))
    if gallery:
        feats = registry.get(family).features
        np.save(d / "gallery.npy", np.linspace(-1, 1, 2 * feats, dtype=np.float32).reshape(2, feats))
    return d


def metadata(src) -> dict:
    from kdl.serving.grpc_server import signature_def_map
    sdm = signature_def_map(SimpleNamespace(signatures=src.signatures))
    return json.loads(json.dumps({
        "order": list(src.signatures),
        "signatures": {n: dataclasses.asdict(s) for n, s in src.signatures.items()},
        "outputs": {n: [k for k, _, _ in s.output_specs()] for n, s in src.signatures.items()},
        "signature_def": json_format.MessageToDict(sdm)}))


@pytest.mark.parametrize("kind", KINDS)
def test_answers_are_the_recorded_ones(kind):
    from kdl.serving.grpc_server import predict_response
    from kdl.serving.rest import predict_body
    want = json.loads((GOLDEN / "answers.json").read_text())[kind]
    got = answers(kind, predict_response, predict_body)
    assert sorted(got) == sorted(want)
    for part in want:
        assert got[part] == want[part], part


@pytest.mark.parametrize("kind", KINDS)
def test_kind_of_and_row_words(kind):
    from kdl.serving import outputs as O
    sig, rows = case(kind)
    assert O.kind_of(sig).name == kind
    src = SimpleNamespace(classes=CLASSES, gallery=np.zeros((2, F), np.uint16))
    assert O.out_cols(sig, src, gpu=True) == rows.shape[1]
    host = {"classify": CLASSES, "similar": F}.get(kind, rows.shape[1])    # logits / features, ranked on the host
    assert O.out_cols(sig, src, gpu=False) == host


@pytest.mark.parametrize("family", FAMILIES)
def test_signatures_and_metadata_are_the_recorded_ones(family, tmp_path):
    want = json.loads((GOLDEN / "metadata.json").read_text())[family]
    for tag, gallery in (("plain", False), ("gallery", True)):
        got = metadata(load_version_dir(version_dir(tmp_path, family, gallery)))
        assert got["order"] == want[tag]["order"], tag
        for name in got["order"]:
            assert list(got["signatures"][name]) == list(want[tag]["signatures"][name]), (tag, name)
        assert got == want[tag], tag


def test_follower_runner_reads_the_table(tmp_path):
    """What a data-parallel follower hands to GPUExecutor has everything setup() and _build_native()
    read: plain logits rows, no engine keywords."""
    from kdl.serving import outputs as O
    from kdl.serving.backend import GPUExecutor
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.dp import _FollowerRunner
    src = load_version_dir(tmp_path, synthetic=True)
    cfg = ServerConfig(batching=BatchingParams(max_batch_size=1, allowed_batch_sizes=[1]))
    r = _FollowerRunner(src, src.signatures[NATIVE_SIGNATURE], cfg)
    assert O.engine_kwargs(r.sig, r.source, "cuda:0") == {}
    assert r.out_cols == src.classes == 10
    ex = GPUExecutor(r, 0, cfg.engine_kwargs())          # __init__ reads sig, faults and cfg
    assert ex.engine_buckets() == [1] and ex.staging_rows() == 1
    assert r.batcher is None and r.exec_group is None and r.faults.native_args(ex.name) == (0, 0)
    assert r.source is src and r.sig.input_dtype == P.DT_UINT8
