"""Reference-compatible TF-Serving gRPC client (`model_server.py:13-56`).

Builds the request exactly like the reference gateway (model_spec name,
signature_name, inputs[<input key>] = make_tensor_proto(X)) and reads
``outputs[<output key>].float_val``, using the runtime-built protos instead of
``tensorflow_serving.apis`` (not installable offline).
"""
from __future__ import annotations

import grpc
import numpy as np

from ..serving import protos as P


class PredictionStub:
    """Equivalent of prediction_service_pb2_grpc.PredictionServiceStub."""

    def __init__(self, channel: grpc.Channel):
        self.Predict = channel.unary_unary(P.PREDICT_METHOD, request_serializer=P.PredictRequest.SerializeToString,
                                           response_deserializer=P.PredictResponse.FromString)
        self.GetModelMetadata = channel.unary_unary(
            P.METADATA_METHOD, request_serializer=P.GetModelMetadataRequest.SerializeToString,
            response_deserializer=P.GetModelMetadataResponse.FromString)


class ModelStub:
    def __init__(self, channel: grpc.Channel):
        self.GetModelStatus = channel.unary_unary(
            P.STATUS_METHOD, request_serializer=P.GetModelStatusRequest.SerializeToString,
            response_deserializer=P.GetModelStatusResponse.FromString)


def np_to_protobuf(data):
    """A numeric array as ``tensor_content``; ``bytes`` or a list of them as a DT_STRING tensor
    (scalar / shape [n], one ``string_val`` each), like ``tf.make_tensor_proto``."""
    if isinstance(data, (bytes, bytearray)):
        return P.TensorProto(dtype=P.DT_STRING, string_val=[bytes(data)])
    if isinstance(data, (list, tuple)) and data and all(isinstance(b, (bytes, bytearray)) for b in data):
        t = P.TensorProto(dtype=P.DT_STRING, string_val=[bytes(b) for b in data])
        t.tensor_shape.dim.add(size=len(data))
        return t
    return P.np_to_tensor_proto(data)


def make_request(X, model_name="clothing-model", signature="serving_default", input_key="input_8"):
    pb_request = P.PredictRequest()
    pb_request.model_spec.name = model_name
    pb_request.model_spec.signature_name = signature
    pb_request.inputs[input_key].CopyFrom(np_to_protobuf(X))
    return pb_request


def process_response(pb_result, labels, output_key="dense_7") -> dict:
    pred = pb_result.outputs[output_key].float_val
    return {c: p for c, p in zip(labels, pred)}


def process_batch_response(pb_result, labels, output_key="dense_7") -> list[dict]:
    """Batched variant (the reference's process_response only handles batch=1,
    SURVEY.md §8.1)."""
    t = pb_result.outputs[output_key]
    vals = np.asarray(t.float_val, dtype=np.float32).reshape([d.size for d in t.tensor_shape.dim])
    return [{c: float(p) for c, p in zip(labels, row)} for row in vals]


def process_classify_response(pb_result) -> list[list[dict]]:
    """A classify signature's PredictResponse (``classes`` DT_STRING [n, K], ``scores`` DT_FLOAT
    [n, K]) -> per image, K ``{"label", "score"}`` entries in the server's order."""
    cl, sc = pb_result.outputs["classes"], pb_result.outputs["scores"]
    n, k = [d.size for d in sc.tensor_shape.dim]
    labels = [v.decode() for v in cl.string_val]
    return [[{"label": labels[i * k + j], "score": float(sc.float_val[i * k + j])} for j in range(k)]
            for i in range(n)]


def process_similar_response(pb_result) -> list[list[dict]]:
    """A similar signature's PredictResponse (``ids`` DT_STRING [n, K], ``scores`` DT_FLOAT [n, K])
    -> per image, K ``{"id", "score"}`` entries, nearest first."""
    ids, sc = pb_result.outputs["ids"], pb_result.outputs["scores"]
    n, k = [d.size for d in sc.tensor_shape.dim]
    names = [v.decode() for v in ids.string_val]
    return [[{"id": names[i * k + j], "score": float(sc.float_val[i * k + j])} for j in range(k)]
            for i in range(n)]


def process_embed_response(pb_result) -> list[list[float]]:
    """An embed signature's PredictResponse (``embedding`` DT_FLOAT [n, F]) -> per image, its F floats."""
    t = pb_result.outputs["embedding"]
    n, f = [d.size for d in t.tensor_shape.dim]
    vals = np.asarray(t.float_val, dtype=np.float32).reshape(n, f)
    return [[float(v) for v in row] for row in vals]


def process_explain_response(pb_result) -> list[dict]:
    """An explain signature's PredictResponse (``classes`` DT_STRING [n, 1], ``scores`` DT_FLOAT
    [n, 1], ``heatmap`` DT_FLOAT [n, h, w]) -> per image ``{"label", "score", "heatmap"}``, the map
    as h rows of w floats."""
    cl, sc, hm = pb_result.outputs["classes"], pb_result.outputs["scores"], pb_result.outputs["heatmap"]
    n, h, w = [d.size for d in hm.tensor_shape.dim]
    maps = np.asarray(hm.float_val, dtype=np.float32).reshape(n, h, w)
    return [{"label": cl.string_val[i].decode(), "score": float(sc.float_val[i]),
             "heatmap": [[float(v) for v in row] for row in maps[i]]} for i in range(n)]


def process_palette_response(pb_result) -> list[dict]:
    """A palette signature's PredictResponse (``classes`` DT_STRING [n, 1], ``scores`` DT_FLOAT [n, 1],
    ``colors`` DT_UINT8 [n, K, 3] as ``tensor_content``, ``fractions`` DT_FLOAT [n, K], ``names`` DT_STRING
    [n, K]) -> per image ``{"label", "score", "colors": [{"rgb", "hex", "name", "fraction"}, ...]}``, heaviest
    first, the colours of fraction 0 dropped."""
    o = pb_result.outputs
    cl, sc, fr, nm = o["classes"], o["scores"], o["fractions"], o["names"]
    n, K = [d.size for d in fr.tensor_shape.dim]
    rgb = np.frombuffer(o["colors"].tensor_content, dtype=np.uint8).reshape(n, K, 3)
    frac = np.asarray(fr.float_val, dtype=np.float32).reshape(n, K)
    return [{"label": cl.string_val[i].decode(), "score": float(sc.float_val[i]),
             "colors": [{"rgb": [int(v) for v in rgb[i, j]], "hex": "#%02x%02x%02x" % tuple(int(v) for v in rgb[i, j]),
                         "name": nm.string_val[i * K + j].decode(), "fraction": float(frac[i, j])}
                        for j in range(K) if frac[i, j] > 0]} for i in range(n)]


def process_locate_response(pb_result) -> list[dict]:
    """A locate signature's PredictResponse (``classes`` DT_STRING [n, 1], ``scores`` DT_FLOAT [n, 1], ``boxes``
    DT_FLOAT [n, K, 4], ``areas`` DT_FLOAT [n, K], ``num_boxes`` DT_INT32 [n, 1]) -> per image ``{"label",
    "score", "count", "boxes": [{"box": [ymin, xmin, ymax, xmax], "area"}, ...]}``, largest first, the boxes
    of area 0 dropped. The coordinates are fractions of the picture the model saw."""
    o = pb_result.outputs
    cl, sc, ar = o["classes"], o["scores"], o["areas"]
    n, K = [d.size for d in ar.tensor_shape.dim]
    box = np.asarray(o["boxes"].float_val, dtype=np.float32).reshape(n, K, 4)
    area = np.asarray(ar.float_val, dtype=np.float32).reshape(n, K)
    return [{"label": cl.string_val[i].decode(), "score": float(sc.float_val[i]), "count": int(o["num_boxes"].int_val[i]),
             "boxes": [{"box": [float(v) for v in box[i, j]], "area": float(area[i, j])}
                       for j in range(K) if area[i, j] > 0]} for i in range(n)]


def process_cutout_response(pb_result) -> list[dict]:
    """A cutout signature's PredictResponse (``classes`` DT_STRING [n, 1], ``scores`` DT_FLOAT [n, 1], ``cutout``
    DT_UINT8 [n, S, S, 4] as ``tensor_content``, ``coverage`` DT_FLOAT [n, 1]) -> per image ``{"label", "score",
    "coverage", "picture"}``, the picture a uint8 array [S, S, 4]: the picture the model saw with its alpha."""
    o = pb_result.outputs
    t = o["cutout"]
    pics = np.frombuffer(t.tensor_content, dtype=np.uint8).reshape([d.size for d in t.tensor_shape.dim])
    return [{"label": o["classes"].string_val[i].decode(), "score": float(o["scores"].float_val[i]),
             "coverage": float(o["coverage"].float_val[i]), "picture": pics[i]} for i in range(len(pics))]


def process_overlay_response(pb_result) -> list[dict]:
    """An overlay signature's PredictResponse (explain's three outputs and ``overlay`` DT_UINT8
    [n, S, S, 3] as ``tensor_content``) -> per image ``{"label", "score", "heatmap", "picture"}``, the
    picture a uint8 array [S, S, 3]."""
    out = process_explain_response(pb_result)
    t = pb_result.outputs["overlay"]
    shape = [d.size for d in t.tensor_shape.dim]
    pics = np.frombuffer(t.tensor_content, dtype=np.uint8).reshape(shape)
    for o, p in zip(out, pics):
        o["picture"] = p
    return out


def png_bytes(picture) -> bytes:
    """uint8 [H, W, 3] -> an 8-bit RGB PNG file, [H, W, 4] -> an 8-bit RGBA one, written with zlib and struct
    alone (the gateway's ``bytes`` mode needs no image library)."""
    import struct
    import zlib
    a = np.ascontiguousarray(picture, dtype=np.uint8)
    H, W, C = a.shape
    assert C in (3, 4), a.shape

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    rows = np.concatenate([np.zeros((H, 1), dtype=np.uint8), a.reshape(H, W * C)], axis=1)   # filter type 0 per row
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 6, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
