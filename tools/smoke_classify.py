#!/usr/bin/env python
"""Smoke client for the classification outputs: prints the top-K ``[{"label", "score"}, ...]`` list
of one image, through the gateway's ``/classify`` or, with --grpc, straight from the model
server's ``classify_bytes`` signature. The counterpart of tools/smoke_test.py (``/predict``), whose
--url / --file arguments it shares.

  python tools/smoke_classify.py --file tests/data/pants.png --gateway http://localhost:9696/classify
  python tools/smoke_classify.py --file tests/data/pants.png --grpc localhost:8500
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import urllib.request

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from smoke_test import serve_file  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--url", default="http://bit.ly/mlbookcamp-pants")
    ap.add_argument("--file", default=None)
    ap.add_argument("--gateway", default="http://localhost:9696/classify")
    ap.add_argument("--grpc", default=None, help="host:port of the model server (bypass the gateway)")
    a = ap.parse_args(argv)
    if a.grpc:
        import grpc
        from kdl.gateway import preprocess as pp
        from kdl.gateway.client import PredictionStub, make_request, process_classify_response
        data = open(a.file, "rb").read() if a.file else pp.fetch(a.url)
        res = PredictionStub(grpc.insecure_channel(a.grpc)).Predict(
            make_request([data], signature="classify_bytes", input_key="image_bytes"), timeout=20.0)
        print(process_classify_response(res)[0])
        return 0
    url = serve_file(a.file) if a.file else a.url
    req = urllib.request.Request(a.gateway, data=json.dumps({"url": url}).encode(),
                                 headers={"Content-Type": "application/json"}, method="POST")
    with urllib.request.urlopen(req, timeout=30) as r:
        print(json.loads(r.read()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
