"""Memory safety of the restart-interval entropy decode's host side on untrusted input: a stand-alone
program (kdl/csrc/tests/jpeg_rst_fuzz.cpp) built with g++ under AddressSanitizer +
UndefinedBehaviorSanitizer runs jpeg_scan_prepare -- the walk through the RSTm markers, the interval
and group tables -- and jpeg_huff_cpu, the emulation that shares its step code with the HIP kernels
(csrc/runtime/jpeg_huff.h), over Pillow-encoded files with restart markers and fixed-seed mutations of
the whole file (headers, markers, scan), and checks each against the host decoder. Host code only:
nothing is loaded into Python under a sanitizer."""
import shutil
import subprocess
from pathlib import Path

import pytest

from _jpeg_cases import encode, smooth_noise

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kdl" / "csrc"

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

PER_SEED = 1000


def test_jpeg_rst_fuzz_under_asan_ubsan(tmp_path):
    exe = tmp_path / "jpeg_rst_fuzz"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", str(CSRC / "tests" / "jpeg_rst_fuzz.cpp"),
           str(CSRC / "runtime" / "jpeg.cpp"), "-I", str(CSRC), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    seeds = []
    for i, (w, h, kw) in enumerate([(33, 47, dict(subsampling=2, quality=75, restart_marker_blocks=2)),
                                    (50, 31, dict(subsampling=1, quality=90, optimize=True, restart_marker_rows=1)),
                                    (40, 40, dict(subsampling=0, quality=100, restart_marker_blocks=1)),
                                    (64, 48, dict(quality=85, restart_marker_blocks=5))]):
        im = smooth_noise(w, h, i, "L" if "subsampling" not in kw else "RGB")
        p = tmp_path / f"seed{i}.jpg"
        p.write_bytes(encode(im, **kw))
        seeds.append(str(p))
    r = subprocess.run([str(exe), str(PER_SEED), *seeds], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    equal, rejected, unprepared = (int(x) for x in r.stdout.split()[1::2])
    assert equal + rejected + unprepared == PER_SEED * len(seeds)
    assert equal and rejected and unprepared, r.stdout      # both implications and the refusals were reached
