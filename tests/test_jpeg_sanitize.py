"""Memory safety of the host JPEG decoder on untrusted input: a stand-alone program
(kdl/csrc/tests/jpeg_fuzz.cpp) built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer
decodes Pillow-encoded seed files and fixed-seed mutations of them. Host code only: nothing is
loaded into Python under a sanitizer."""
import shutil
import subprocess
from pathlib import Path

import pytest

from _jpeg_cases import encode, smooth_noise

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kdl" / "csrc"

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_jpeg_decoder_fuzz_under_asan_ubsan(tmp_path):
    exe = tmp_path / "jpeg_fuzz"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", str(CSRC / "tests" / "jpeg_fuzz.cpp"), str(CSRC / "runtime" / "jpeg.cpp"),
           "-I", str(CSRC), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    seeds = []
    for i, (w, h, kw) in enumerate([(33, 47, dict(subsampling=2, quality=75)),
                                    (50, 31, dict(subsampling=1, quality=90, optimize=True)),
                                    (64, 64, dict(subsampling=0, quality=40, restart_marker_blocks=2)),
                                    (17, 9, dict(quality=85))]):
        im = smooth_noise(w, h, i, "L" if "subsampling" not in kw else "RGB")
        p = tmp_path / f"seed{i}.jpg"
        p.write_bytes(encode(im, **kw))
        seeds.append(str(p))
    r = subprocess.run([str(exe), "4000", *seeds], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    ok, unsupported, malformed = (int(x) for x in r.stdout.split()[1::2])
    assert ok + unsupported + malformed == 4000 * len(seeds)
    assert ok and unsupported and malformed, r.stdout       # the mutations reach all three answers
