"""TF-Serving REST API (:8501) + Prometheus metrics + k8s probes.

Routes (TF-Serving REST semantics):
  GET  /v1/models/<name>[/versions/<v>]            -> model_version_status
  GET  /v1/models/<name>[/versions/<v>]/metadata   -> signature_def
  POST /v1/models/<name>[/versions/<v>|/labels/<l>]:predict
       {"signature_name"?, "instances": [...]}  -> {"predictions": [...]}
       {"signature_name"?, "inputs": ...}       -> {"outputs": ...}
       (serving_bytes: every value is {"b64": "<base64 of the image file>"})
       (classify signatures: {"classes": [...], "scores": [...]} per instance, or by column)
       (embed signatures: the feature rows, as "predictions" or "outputs")
       (explain and attention signatures: {"classes": [label], "scores": [score], "heatmap": [[...]]} per instance,
        or by column; overlay signatures add "overlay": the S x S x 3 picture as nested integer lists)
  POST /v1/models/<name>[/versions/<v>|/labels/<l>]:classify
       {"signature_name"?, "examples": [{"image/encoded": {"b64": ...}}, ...]}
                                                -> {"results": [[["label", score], ...], ...]}
  GET  /monitoring/prometheus/metrics, /healthz (liveness), /readyz (readiness)
"""
from __future__ import annotations

import base64
import json
import time
import re
import threading
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

import numpy as np
from google.protobuf import json_format

from ..ops import _lib
from . import protos as P
from . import outputs as O
from .backend import ServingError
from .classify import CLASSIFY_BYTES_SIGNATURE
from .grpc_server import classify_examples, route_exact_u8, signature_def_map
from .metrics import METRICS
from .model_repo import STATE_NAMES, ModelManager

_ROUTE = re.compile(r"^/v1/models/(?P<name>[^/:]+)(?:/versions/(?P<ver>\d+)|/labels/(?P<label>[^/:]+))?"
                    r"(?P<tail>:predict|:classify|/metadata)?/?$")
_HTTP = {"INVALID_ARGUMENT": 400, "NOT_FOUND": 404, "DEADLINE_EXCEEDED": 504, "UNAVAILABLE": 503,
         "RESOURCE_EXHAUSTED": 429, "UNIMPLEMENTED": 501, "INTERNAL": 500}


def predict_body(s, sig, rows, by_row: bool) -> dict:
    """The :predict answer, per instance ("predictions") or by column ("outputs"): the rows of a
    single fp32 output as they are, else an object of the kind's named outputs (serving/outputs.py)."""
    cols = O.columns(s.source, sig, rows)
    if cols is None:
        O.answered(sig)
        return {"predictions" if by_row else "outputs": rows.tolist()}
    # a list of bytes (a ``_bytes`` output) is answered as TF-Serving does: {"b64": ...} per element
    cols = [(key, [{"b64": base64.b64encode(e).decode()} if isinstance(e, bytes) else e for e in v]
             if isinstance(v, list) else v.tolist()) for key, _, v in cols]
    if by_row:
        return {"predictions": [{key: v[i] for key, v in cols} for i in range(len(rows))]}
    return {"outputs": dict(cols)}


def make_handler(manager: ModelManager, f32_exact_u8: bool = True):
    class H(BaseHTTPRequestHandler):
        protocol_version = "HTTP/1.1"

        def log_message(self, *a):  # quiet
            pass

        def _send(self, code: int, body, ctype="application/json"):
            data = body if isinstance(body, bytes) else (json.dumps(body) if not isinstance(body, str) else body).encode()
            self.send_response(code)
            self.send_header("Content-Type", ctype)
            self.send_header("Content-Length", str(len(data)))
            self.end_headers()
            self.wfile.write(data)

        def _err(self, e: ServingError):
            self._send(_HTTP.get(e.code, 500), {"error": str(e)})

        def do_GET(self):  # noqa: N802
            if self.path.startswith("/monitoring/prometheus/metrics"):
                return self._send(200, METRICS.render(), "text/plain; version=0.0.4")
            if self.path == "/healthz":
                return self._send(200, {"status": "alive"})
            if self.path == "/readyz":
                ok = manager.ready()
                return self._send(200 if ok else 503, {"ready": ok})
            m = _ROUTE.match(self.path)
            if not m or m.group("tail") in (":predict", ":classify"):
                return self._send(404, {"error": "not found"})
            try:
                ver = int(m.group("ver")) if m.group("ver") else None
                if m.group("tail") == "/metadata":
                    s = manager.get(m.group("name"), ver, m.group("label"))
                    sdm = json_format.MessageToDict(signature_def_map(s))
                    return self._send(200, {"model_spec": {"name": s.name, "signature_name": "",
                                                           "version": str(s.version)},
                                            "metadata": {"signature_def": sdm}})
                if m.group("name") != manager.name:
                    raise ServingError("NOT_FOUND", f"Could not find any versions of model {m.group('name')}")
                st = [{"version": str(v), "state": STATE_NAMES.get(state, "UNKNOWN"),
                       "status": {"error_code": "OK" if not msg else "UNKNOWN", "error_message": msg}}
                      for v, state, msg in manager.status(ver)]
                return self._send(200, {"model_version_status": st})
            except ServingError as e:
                return self._err(e)

        def do_POST(self):  # noqa: N802
            m = _ROUTE.match(self.path)
            if m and m.group("tail") == ":classify":
                return self._classify(m)
            if not m or m.group("tail") != ":predict":
                return self._send(404, {"error": "not found"})
            t0 = time.perf_counter()
            try:
                n = int(self.headers.get("Content-Length", "0"))
                body = json.loads(self.rfile.read(n) or b"{}")
                ver = int(m.group("ver")) if m.group("ver") else None
                s = manager.get(m.group("name"), ver, m.group("label"))
                runner = s.runner(body.get("signature_name") or "serving_default")
                sig = runner.sig
                dt = np.uint8 if sig.input_dtype == P.DT_UINT8 else np.float32
                if sig.input_dtype == P.DT_STRING:      # serving_bytes: {"b64": ...} per encoded image
                    return self._predict_bytes(body, s, runner, t0)
                if "instances" in body:
                    inst = body["instances"]
                    if inst and isinstance(inst[0], dict):
                        inst = [i[sig.input_key] for i in inst]
                    x, rows = np.asarray(inst, dtype=dt), True
                elif "inputs" in body:
                    inp = body["inputs"]
                    if isinstance(inp, dict):
                        inp = inp[sig.input_key]
                    x, rows = np.asarray(inp, dtype=dt), False
                else:
                    raise ServingError("INVALID_ARGUMENT", "request must contain 'instances' or 'inputs'")
                S = sig.input_shape[1]
                if S == -1:          # serving_image: any size
                    if x.ndim != 4 or x.shape[3] != 3 or min(x.shape) < 1:
                        raise ServingError("INVALID_ARGUMENT", f"expected images [-1,-1,-1,3], got {list(x.shape)}")
                elif x.ndim != 4 or x.shape[1:] != (S, S, 3):
                    raise ServingError("INVALID_ARGUMENT", f"expected images [-1,{S},{S},3], got {list(x.shape)}")
                x = np.ascontiguousarray(x)
                dl = self.headers.get("X-Deadline-Ms")
                deadline = int(_lib.rt().now_us() + float(dl) * 1e3) if dl else 0
                n_img = x.shape[0]
                if f32_exact_u8:     # same routing as gRPC (--scatter rccl serves serving_uint8 over the node)
                    runner, x = route_exact_u8(s, runner, x, n_img)
                t1 = time.perf_counter()
                out = predict_body(s, sig, runner.predict(x, n_img, deadline), rows)
                t2 = time.perf_counter()
                r = self._send(200, out)
                # same per-request stage trace as the gRPC path (SURVEY.md §5 tracing)
                METRICS.observe("kdl_stage_ms", (t1 - t0) * 1e3, stage="parse")
                METRICS.observe("kdl_stage_ms", (t2 - t1) * 1e3, stage="batch_and_run")
                METRICS.observe("kdl_stage_ms", (time.perf_counter() - t2) * 1e3, stage="respond")
                METRICS.inc("kdl_requests_total", code="OK", method="RestPredict")
                METRICS.observe("kdl_request_latency_ms", (time.perf_counter() - t0) * 1e3, method="RestPredict")
                return r
            except ServingError as e:
                METRICS.inc("kdl_requests_total", code=e.code, method="RestPredict")
                return self._err(e)
            except (ValueError, KeyError, TypeError) as e:
                return self._err(ServingError("INVALID_ARGUMENT", str(e)))

        def _classify(self, m):
            t0 = time.perf_counter()
            try:
                n = int(self.headers.get("Content-Length", "0"))
                try:
                    body = json.loads(self.rfile.read(n) or b"{}")
                except ValueError as e:
                    raise ServingError("INVALID_ARGUMENT", f"malformed JSON body: {e}") from e
                if not isinstance(body, dict):
                    raise ServingError("INVALID_ARGUMENT", "the body must be a JSON object with \"examples\"")
                ver = int(m.group("ver")) if m.group("ver") else None
                s = manager.get(m.group("name"), ver, m.group("label"))
                if "context" in body:
                    raise ServingError("INVALID_ARGUMENT", "\"context\" is not supported: send \"examples\" only")
                items = body.get("examples")
                if not isinstance(items, list):
                    raise ServingError("INVALID_ARGUMENT", "request must contain a list \"examples\"")
                examples = []
                for i, it in enumerate(items):
                    ex = P.Example()
                    if not isinstance(it, dict):
                        raise ServingError("INVALID_ARGUMENT", f"example {i}: expected an object of features")
                    for key, v in it.items():
                        f = ex.features.feature[key]
                        for one in v if isinstance(v, list) else [v]:
                            if isinstance(one, dict) and isinstance(one.get("b64"), str):
                                try:
                                    f.bytes_list.value.append(base64.b64decode(one["b64"], validate=True))
                                except ValueError as e:
                                    raise ServingError("INVALID_ARGUMENT",
                                                       f"example {i}: feature '{key}': bad base64: {e}") from e
                            elif isinstance(one, str):
                                f.bytes_list.value.append(one.encode())
                            elif isinstance(one, bool) or not isinstance(one, (int, float)):
                                raise ServingError("INVALID_ARGUMENT", f"example {i}: feature '{key}': unsupported value")
                            elif isinstance(one, int):
                                f.int64_list.value.append(one)
                            else:
                                f.float_list.value.append(one)
                    examples.append(ex)
                dl = self.headers.get("X-Deadline-Ms")
                deadline = int(_lib.rt().now_us() + float(dl) * 1e3) if dl else 0
                labels, scores = classify_examples(s, body.get("signature_name") or "", "example_list", examples,
                                                   deadline)
                r = self._send(200, {"results": [[[name, v] for name, v in zip(lab, sc)]
                                                 for lab, sc in zip(labels, scores.tolist())]})
                METRICS.inc("kdl_requests_total", code="OK", method="RestClassify")
                METRICS.observe("kdl_request_latency_ms", (time.perf_counter() - t0) * 1e3, method="RestClassify")
                return r
            except ServingError as e:
                METRICS.inc("kdl_requests_total", code=e.code, method="RestClassify")
                return self._err(e)
            except (ValueError, KeyError, TypeError) as e:
                return self._err(ServingError("INVALID_ARGUMENT", str(e)))

        def _predict_bytes(self, body, s, runner, t0):
            sig = runner.sig
            rows = "instances" in body
            if not rows and "inputs" not in body:
                raise ServingError("INVALID_ARGUMENT", "request must contain 'instances' or 'inputs'")
            items = body["instances"] if rows else body["inputs"]
            if isinstance(items, dict) and "b64" not in items:
                items = items[sig.input_key]
            if isinstance(items, dict):                 # a scalar
                items = [items]
            images = []
            for it in items:
                if isinstance(it, dict) and "b64" not in it:
                    it = it[sig.input_key]
                if not isinstance(it, dict) or not isinstance(it.get("b64"), str):
                    raise ServingError("INVALID_ARGUMENT", f"input '{sig.input_key}' takes {{\"b64\": ...}} values")
                try:
                    images.append(base64.b64decode(it["b64"], validate=True))
                except ValueError as e:
                    raise ServingError("INVALID_ARGUMENT", f"input '{sig.input_key}': bad base64: {e}") from e
            if not images:
                raise ServingError("INVALID_ARGUMENT", f"input '{sig.input_key}' is empty")
            dl = self.headers.get("X-Deadline-Ms")
            deadline = int(_lib.rt().now_us() + float(dl) * 1e3) if dl else 0
            t1 = time.perf_counter()
            out = predict_body(s, sig, runner.predict(images, len(images), deadline), rows)
            t2 = time.perf_counter()
            r = self._send(200, out)
            METRICS.observe("kdl_stage_ms", (t1 - t0) * 1e3, stage="parse")
            METRICS.observe("kdl_stage_ms", (t2 - t1) * 1e3, stage="batch_and_run")
            METRICS.observe("kdl_stage_ms", (time.perf_counter() - t2) * 1e3, stage="respond")
            METRICS.inc("kdl_requests_total", code="OK", method="RestPredict")
            METRICS.observe("kdl_request_latency_ms", (time.perf_counter() - t0) * 1e3, method="RestPredict")
            return r

    return H


class _ReusePortHTTPServer(ThreadingHTTPServer):
    """SO_REUSEPORT listener: the per-GPU server processes of one node (``--procs``) all bind
    the same REST port and the kernel spreads connections over them."""

    def server_bind(self):
        import socket
        if hasattr(socket, "SO_REUSEPORT"):
            self.socket.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEPORT, 1)
        super().server_bind()


def start_rest_server(manager: ModelManager, host: str, port: int, reuse_port: bool = False,
                      f32_exact_u8: bool = True):
    srv = (_ReusePortHTTPServer if reuse_port else ThreadingHTTPServer)((host, port), make_handler(manager, f32_exact_u8))
    srv.daemon_threads = True
    t = threading.Thread(target=srv.serve_forever, name="rest", daemon=True)
    t.start()
    return srv
