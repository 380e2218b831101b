"""Serving gateway: ``POST /predict {"url": ...}`` -> ``{label: logit}``;
``POST /classify {"url": ...}`` -> ``[{"label": ..., "score": ...}, ...]`` (the model server's
top-K classes and softmax scores, its label strings: the classify signature of the mode);
``POST /embed {"url": ...}`` -> ``{"embedding": [...]}`` (the pooled feature vector in front of the
model's head: the embed signature of the mode).
``POST /similar {"url": ...}`` -> ``{"neighbors": [{"id": ..., "score": ...}, ...]}`` (the nearest items
of the model version's gallery, nearest first: the similar signature of the mode).
``POST /explain {"url": ...}`` -> ``{"label": ..., "score": ..., "heatmap": [[...], ...]}`` (the predicted
class and its Grad-CAM map over the model's last feature map, h rows of w values in 0..1: the explain
signature of the mode; ``/overlay`` renders the map).
``POST /attention {"url": ...}`` -> the same three fields from a ViT version's attention signature of
the mode: the map is the 14 x 14 attention rollout of the class token.
``POST /overlay {"url": ...}`` -> ``image/png``: the picture the model saw with the heatmap of whatever
method the version has painted on it (the overlay signature of the mode), label and score in the headers
``X-KDL-Label`` / ``X-KDL-Score``; with ``"format": "json"`` -> ``{"label", "score", "heatmap", "png": "<base64>"}``;
with ``"format": "jpeg"`` -> ``image/jpeg``: the file the model server encoded (the overlay_jpeg signature of the
mode, on a version that has it), handed on byte for byte, the same two headers.
``POST /colors {"url": ...}`` -> ``{"label", "score", "colors": [{"rgb": [r, g, b], "hex": "#rrggbb", "name",
"fraction"}, ...]}``: the predicted class and the garment's dominant colours, heaviest first (the palette signature
of the mode, on a version that has it); colours of weight 0 are left out.
``POST /locate {"url": ...}`` -> ``{"label", "score", "count", "boxes": [{"box": [ymin, xmin, ymax, xmax], "area"},
...]}``: the predicted class and the garment's boxes, largest first, as fractions of the picture the model saw (the
locate signature of the mode, on a version that has it); ``count`` is the number of all regions, boxes of area 0 are
left out.
``POST /cutout {"url": ...}`` -> ``image/png`` with an alpha channel: the picture the model saw, the backdrop made
transparent (the cutout signature of the mode, on a version that has it), label, score and the garment's share of
the picture in the headers ``X-KDL-Label`` / ``X-KDL-Score`` / ``X-KDL-Coverage``; with ``"format": "json"`` ->
``{"label", "score", "coverage", "png": "<base64>"}``.

Same contract as the reference Flask gateway (`model_server.py:59-70`, SURVEY.md
§2.9.1): Flask app named 'clothing-model', backend address from
``TF_SERVING_HOST`` (default ``localhost:8500``), Xception preprocessing, gRPC
Predict with a 20 s deadline, ten labels in model output order. Improvements
the reference lacks (§8.1): JSON errors (400 bad body, 502 fetch/backend errors,
504 deadline) instead of bare 500s, a batch route, health probes, and a native
mode that ships uint8 pixels to the ``serving_uint8`` signature (4x fewer bytes).

Env: TF_SERVING_HOST, MODEL_NAME, SIGNATURE, INPUT_KEY, OUTPUT_KEY, LABELS,
GATEWAY_MODE=compat|uint8|raw|bytes (raw: decoded pixels at their own size to ``serving_image``,
resized on the model server's GPU -- no resize here; bytes: the fetched file as it is to
``serving_bytes``, decoded and resized on the model server -- no PIL here), GATEWAY_PREPROCESS
(``<filter>[:<R>]``, default ``nearest``: the resize of the compat and uint8 modes, through Pillow),
PREDICT_TIMEOUT, GATEWAY_CHANNELS (gRPC connections to open:
each gets its own subchannel, so a node running one model-server process per GPU on a
shared SO_REUSEPORT port -- ``--procs`` -- sees the gateway's requests spread over all
of them instead of pinned to whichever process accepted a single connection).
"""
from __future__ import annotations

import itertools
import os
import threading
import urllib.error

import grpc
import numpy as np
from flask import Flask, jsonify, request

from ..labels import LABELS as DEFAULT_LABELS
from . import preprocess as pp
from .client import (PredictionStub, make_request, process_batch_response, process_classify_response,
                     process_cutout_response,
                     process_embed_response, process_explain_response, process_locate_response,
                     process_overlay_response,
                     process_palette_response, process_response, process_similar_response, png_bytes)


class GatewayConfig:
    def __init__(self, env=None):
        env = os.environ if env is None else env
        self.server = env.get("TF_SERVING_HOST", "localhost:8500")
        self.model_name = env.get("MODEL_NAME", "clothing-model")
        self.mode = env.get("GATEWAY_MODE", "compat")
        if self.mode not in ("compat", "uint8", "raw", "bytes"):
            raise ValueError(f"GATEWAY_MODE must be compat, uint8, raw or bytes, got {self.mode!r}")
        self.signature = env.get("SIGNATURE", {"compat": "serving_default", "uint8": "serving_uint8",
                                               "raw": "serving_image", "bytes": "serving_bytes"}[self.mode])
        self.input_key = env.get("INPUT_KEY", {"compat": "input_8", "bytes": "image_bytes"}.get(self.mode, "images"))
        self.output_key = env.get("OUTPUT_KEY", "dense_7")
        labels = env.get("LABELS", "")
        self.labels = [s for s in labels.split(",") if s] or list(DEFAULT_LABELS)
        self.timeout = float(env.get("PREDICT_TIMEOUT", "20.0"))
        self.channels = max(1, int(env.get("GATEWAY_CHANNELS", "1")))
        # the resize of the compat / uint8 modes ("<filter>[:<R>]", preprocess.ResizeSpec) to the
        # 299 x 299 model input; raw and bytes leave it to the model server (its --preprocess)
        self.preprocess = pp.ResizeSpec.parse(env.get("GATEWAY_PREPROCESS", "nearest"), pp.TARGET[0])


def create_app(cfg: GatewayConfig | None = None, channel: grpc.Channel | None = None) -> Flask:
    cfg = cfg or GatewayConfig()
    opts = [("grpc.max_send_message_length", -1), ("grpc.max_receive_message_length", -1)]
    if channel is not None:
        stubs = [PredictionStub(channel)]
    else:
        # one connection per channel (a local subchannel pool each), round-robin per request
        extra = [("grpc.use_local_subchannel_pool", 1)] if cfg.channels > 1 else []
        stubs = [PredictionStub(grpc.insecure_channel(cfg.server, options=opts + extra)) for _ in range(cfg.channels)]
    rr, rr_lock = itertools.cycle(stubs), threading.Lock()

    def next_stub():
        with rr_lock:
            return next(rr)
    preprocessor = pp.create_preprocessor("xception", target_size=(299, 299))
    app = Flask("clothing-model")
    app.config["kdl_gateway"] = cfg

    def tensor_from_image(img):
        if cfg.mode == "raw":
            return np.asarray(img, dtype=np.uint8)[None]
        if cfg.preprocess != pp.NEAREST_SPEC:
            px = pp.apply_spec_pil(img, cfg.preprocess, pp.TARGET[0])[None]
            return px if cfg.mode == "uint8" else pp.xception_preprocess(px)
        if cfg.mode == "uint8":
            return pp.to_uint8(img)[None]
        return pp.image_to_tensor(img)

    def run(X):
        req = make_request(X, cfg.model_name, cfg.signature, cfg.input_key)
        return next_stub().Predict(req, timeout=cfg.timeout)

    def fail(code: int, msg: str):
        return jsonify({"error": msg}), code

    def grpc_fail(e: grpc.RpcError):
        code = e.code() if hasattr(e, "code") else None
        http = {grpc.StatusCode.DEADLINE_EXCEEDED: 504, grpc.StatusCode.INVALID_ARGUMENT: 400,
                grpc.StatusCode.NOT_FOUND: 404, grpc.StatusCode.UNAVAILABLE: 503,
                grpc.StatusCode.RESOURCE_EXHAUSTED: 429}.get(code, 502)
        details = e.details() if hasattr(e, "details") else str(e)
        return fail(http, f"model server error ({code.name if code else 'UNKNOWN'}): {details}")

    def load(url: str):
        try:
            if cfg.mode == "bytes":        # a plain proxy: the model server decodes
                return pp.fetch(url)
            return pp.load_image(pp.fetch(url))
        except (urllib.error.URLError, ValueError, OSError) as e:
            raise LookupError(f"could not fetch/decode image from {url!r}: {e}") from e

    @app.route("/predict", methods=["POST"])
    def predict():
        body = request.get_json(silent=True)
        if not isinstance(body, dict) or not isinstance(body.get("url"), str):
            return fail(400, 'request body must be JSON {"url": "<image url>"}')
        try:
            img = load(body["url"])
        except LookupError as e:
            return fail(502, str(e))
        try:
            pb_result = run([img] if cfg.mode == "bytes" else tensor_from_image(img))
        except grpc.RpcError as e:
            return grpc_fail(e)
        return jsonify(process_response(pb_result, cfg.labels, cfg.output_key))

    def trio(first: str) -> tuple:
        """(signature, input key) of a trio for the gateway's mode; compat and uint8 resize here, as for
        /predict, and both send uint8 pixels (these signatures take no f32 input)."""
        return {"bytes": (f"{first}_bytes", "image_bytes"), "raw": (f"{first}_image", "images")}.get(
            cfg.mode, (first, "images"))

    def uint8_input(img):
        if cfg.mode == "bytes":
            return [img]
        if cfg.mode == "raw":
            return np.asarray(img, dtype=np.uint8)[None]
        if cfg.preprocess != pp.NEAREST_SPEC:
            return pp.apply_spec_pil(img, cfg.preprocess, pp.TARGET[0])[None]
        return pp.to_uint8(img)[None]

    def one_image(first: str, shape, formats=None):
        """One image URL through the trio ``first`` (a name, or body -> name) -> shape(PredictResponse, body),
        or the error answer."""
        body = request.get_json(silent=True)
        ok = isinstance(body, dict) and isinstance(body.get("url"), str)
        if formats:
            if not ok or body.get("format", formats[0]) not in formats:
                return fail(400, 'request body must be JSON {"url": "<image url>", "format"?: ' +
                            " | ".join(f'"{f}"' for f in formats) + "}")
        elif not ok:
            return fail(400, 'request body must be JSON {"url": "<image url>"}')
        try:
            img = load(body["url"])
        except LookupError as e:
            return fail(502, str(e))
        try:
            req = make_request(uint8_input(img), cfg.model_name, *trio(first(body) if callable(first) else first))
            pb_result = next_stub().Predict(req, timeout=cfg.timeout)
        except grpc.RpcError as e:
            return grpc_fail(e)
        return shape(pb_result, body)

    @app.route("/classify", methods=["POST"])
    def classify():
        return one_image("classify", lambda pb, _: jsonify(process_classify_response(pb)[0]))

    @app.route("/embed", methods=["POST"])
    def embed():
        return one_image("embed", lambda pb, _: jsonify({"embedding": process_embed_response(pb)[0]}))

    @app.route("/similar", methods=["POST"])
    def similar():
        return one_image("similar", lambda pb, _: jsonify({"neighbors": process_similar_response(pb)[0]}))

    @app.route("/explain", methods=["POST"])
    def explain():
        return one_image("explain", lambda pb, _: jsonify(process_explain_response(pb)[0]))

    @app.route("/attention", methods=["POST"])
    def attention():
        return one_image("attention", lambda pb, _: jsonify(process_explain_response(pb)[0]))

    @app.route("/colors", methods=["POST"])
    def colors():
        return one_image("palette", lambda pb, _: jsonify(process_palette_response(pb)[0]))

    @app.route("/locate", methods=["POST"])
    def locate():
        return one_image("locate", lambda pb, _: jsonify(process_locate_response(pb)[0]))

    @app.route("/cutout", methods=["POST"])
    def cutout():
        """One image through the cutout signature -> the picture with its alpha as a PNG (or, with
        "format": "json", label, score, coverage and the PNG in base64)."""
        def shape(pb_result, body):
            ans = process_cutout_response(pb_result)[0]
            png = png_bytes(ans.pop("picture"))
            if body.get("format") == "json":
                import base64
                return jsonify(dict(ans, png=base64.b64encode(png).decode()))
            resp = app.response_class(png, mimetype="image/png")
            resp.headers["X-KDL-Label"] = ans["label"]
            resp.headers["X-KDL-Score"] = repr(ans["score"])
            resp.headers["X-KDL-Coverage"] = repr(ans["coverage"])
            return resp
        return one_image("cutout", shape, formats=("png", "json"))

    @app.route("/overlay", methods=["POST"])
    def overlay():
        """One image through the overlay signature -> the rendered picture as a PNG (or, with
        "format": "json", label, score, heatmap and the PNG in base64); with "format": "jpeg" through the
        overlay_jpeg signature -> the model server's file as it is."""
        def shape(pb_result, body):
            if body.get("format") == "jpeg":
                ans = process_explain_response(pb_result)[0]
                data = bytes(pb_result.outputs["jpeg_bytes"].string_val[0])
                if not data:
                    return fail(502, "the model server's file did not fit the version's overlay_jpeg max_bytes")
                resp = app.response_class(data, mimetype="image/jpeg")
                resp.headers["X-KDL-Label"] = ans["label"]
                resp.headers["X-KDL-Score"] = repr(ans["score"])
                return resp
            ans = process_overlay_response(pb_result)[0]
            png = png_bytes(ans.pop("picture"))
            if body.get("format") == "json":
                import base64
                return jsonify(dict(ans, png=base64.b64encode(png).decode()))
            resp = app.response_class(png, mimetype="image/png")
            resp.headers["X-KDL-Label"] = ans["label"]
            resp.headers["X-KDL-Score"] = repr(ans["score"])
            return resp
        return one_image(lambda body: "overlay_jpeg" if body.get("format") == "jpeg" else "overlay", shape,
                         formats=("png", "json", "jpeg"))

    @app.route("/predict_batch", methods=["POST"])
    def predict_batch():
        body = request.get_json(silent=True)
        urls = body.get("urls") if isinstance(body, dict) else None
        if not isinstance(urls, list) or not urls or not all(isinstance(u, str) for u in urls):
            return fail(400, 'request body must be JSON {"urls": ["<image url>", ...]}')
        try:
            Xs = [load(u) for u in urls]
            if cfg.mode != "bytes":
                Xs = [tensor_from_image(x) for x in Xs]
        except LookupError as e:
            return fail(502, str(e))
        try:
            if cfg.mode == "bytes":        # all bodies in one request: the sizes may differ
                return jsonify(process_batch_response(run(Xs), cfg.labels, cfg.output_key))
            if cfg.mode == "raw" and len({x.shape for x in Xs}) > 1:
                # raw pixels of different sizes cannot share one dense tensor: one request each
                return jsonify([process_response(run(x), cfg.labels, cfg.output_key) for x in Xs])
            pb_result = run(np.concatenate(Xs))
        except grpc.RpcError as e:
            return grpc_fail(e)
        return jsonify(process_batch_response(pb_result, cfg.labels, cfg.output_key))

    @app.route("/healthz", methods=["GET"])
    def healthz():
        return jsonify({"status": "alive", "backend": cfg.server})

    return app


def main():  # dev entry like the reference's app.run (model_server.py:69-70), without debug=True
    create_app().run(host="0.0.0.0", port=int(os.environ.get("PORT", "9696")))


if __name__ == "__main__":
    main()
