#!/usr/bin/env python
"""Smoke client for the rendered heatmap overlays: sends one image through the gateway's ``/overlay``
and writes the PNG it answers: the picture the model saw with the heat on it. Prints the label and
score from the ``X-KDL-Label`` / ``X-KDL-Score`` headers. Shares --url / --file with tools/smoke_test.py.

  python tools/smoke_overlay.py --gateway http://localhost:9696 --file tests/data/pants.png --out x.png
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


def post_json(url: str, body: dict, timeout: float = 60.0) -> tuple:
    """-> (status, headers, body bytes)."""
    req = urllib.request.Request(url, data=json.dumps(body).encode(), headers={"Content-Type": "application/json"},
                                 method="POST")
    with urllib.request.urlopen(req, timeout=timeout) as r:
        return r.status, dict(r.headers), r.read()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--url", default="http://bit.ly/mlbookcamp-pants")
    ap.add_argument("--file", default=None)
    ap.add_argument("--gateway", default="http://localhost:9696", help="the gateway, with or without /overlay")
    ap.add_argument("--out", default="overlay.png")
    a = ap.parse_args(argv)
    gw = a.gateway.rstrip("/")
    if not gw.endswith("/overlay"):
        gw += "/overlay"
    url = serve_file(a.file) if a.file else a.url
    status, headers, data = post_json(gw, {"url": url})
    if status != 200 or data[:8] != b"\x89PNG\r\n\x1a\n":
        print(f"{gw}: HTTP {status}: {data[:200]!r}", file=sys.stderr)
        return 1
    with open(a.out, "wb") as f:
        f.write(data)
    print(json.dumps({"label": headers.get("X-KDL-Label"), "score": headers.get("X-KDL-Score"), "out": a.out,
                      "bytes": len(data)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
