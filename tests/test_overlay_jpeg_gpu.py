"""jpeg_encode (kernels/jpeg_encode.hip) alone, inside the Xception, ViT-B/16 and ResNet-50 engines, through the
stage pipeline and behind the server.

The oracle of the kernel and engine tests is Pillow itself: ``Image.save(.., "JPEG", quality, subsampling,
optimize=False)`` of the same pixels. Every comparison is for equality of bytes, and the kernel tests compare
the WHOLE output buffer (length word, file, zero pad bytes, the canary behind a row and the row behind the
batch). The shipped ``encode_rule`` is checked against Pillow in tests/test_overlay_jpeg_cpu.py, where the
pictures used here are also shown to stay under the default cap.
"""
import io

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5      # a NaN pattern, as int32
SAMPLINGS = ("4:4:4", "4:2:0")
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2}
# (H, W, B): (8, 8) one Y block and three dummies; (24, 24) and (40, 24) the chroma bottom rule; (25, 40) a dummy
# column; (299, 299, 5) packed pictures at all four byte residues; (600, 600) a dummy row and column
SHAPES = [(8, 8, 1), (16, 16, 2), (17, 17, 1), (9, 23, 3), (24, 24, 1), (40, 24, 1), (25, 40, 1), (33, 47, 1),
          (299, 299, 5), (224, 224, 2), (600, 600, 2)]


def pillow(pic, quality, sampling) -> bytes:
    b = io.BytesIO()
    Image.fromarray(pic).save(b, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[sampling], optimize=False)
    return b.getvalue()


def noise(B, H, W, seed=0):
    return np.random.default_rng(1000 * H + W + seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def checker(B, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    one = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    return np.stack([one if b % 2 == 0 else 255 - one for b in range(B)])


def encode(pics, quality, sampling, cap, nfront=0, extra_words=3, extra_rows=1, ldi=None, override=None):
    """One launch on canary-filled buffers -> (the whole int32 output buffer [B + extra_rows, ldo], the front
    words given). The workspace is filled with 0xA5: what the kernels rely on being zero they clear."""
    from kdl.ops import _lib
    from kdl.serving import jpeg_encode as J
    lib = _lib.lib()
    B, H, W, _ = pics.shape
    ldi = ldi or H * W * 3
    inp = np.full(B * ldi + 8, 0xEE, np.uint8)
    for b in range(B):
        inp[b * ldi:b * ldi + H * W * 3] = pics[b].reshape(-1)
    ldo = nfront + 1 + (cap + 3) // 4 + extra_words
    out = torch.full((B + extra_rows, ldo), CANARY, dtype=torch.int32, device="cuda")
    front = np.random.default_rng(7).integers(-2**31, 2**31, (B, nfront + 2), dtype=np.int64).astype(np.int32)
    d_front = torch.from_numpy(front).cuda()
    hdr = np.frombuffer(J.header(H, W, quality, sampling), np.uint8).copy()
    d_hdr, d_inp = torch.from_numpy(hdr).cuda(), torch.from_numpy(inp).cuda()
    si = SAMPLINGS.index(sampling)
    work = torch.full((lib.jpeg_encode_workspace(B, H, W, si, cap),), 0xA5, dtype=torch.uint8, device="cuda")
    d = dict(inp=d_inp.data_ptr(), ldi=ldi, hdr=d_hdr.data_ptr(), h_hdr=hdr.ctypes.data,
             front=d_front.data_ptr() if nfront else None, ldf=nfront + 2 if nfront else 0, nfront=nfront,
             out=out.data_ptr(), ldo=ldo, work=work.data_ptr(), B=B, H=H, W=W, quality=quality, sampling=si, cap=cap)
    d.update(override or {})
    lib.jpeg_encode(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), front


def expected(files, cap, ldo, nfront=0, front=None, extra_rows=1):
    """The whole buffer as it must be: canary, then per row the front words, the length and the file with zero
    bytes up to ceil(cap / 4) words; a file that does not fit: length 0, the canary behind it."""
    want = np.full((len(files) + extra_rows, ldo), CANARY, np.int32)
    by = want.view(np.uint8)
    for b, f in enumerate(files):
        if nfront:
            want[b, :nfront] = front[b, :nfront]
        if len(f) > cap:
            want[b, nfront] = 0
            continue
        want[b, nfront] = len(f)
        lo = 4 * (nfront + 1)
        by[b, lo:lo + 4 * ((cap + 3) // 4)] = 0
        by[b, lo:lo + len(f)] = np.frombuffer(f, np.uint8)
    return want


# ------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("H,W,B", SHAPES)
def test_kernel_equals_pillow_whole_buffer(H, W, B):
    for name, pics in (("noise", noise(B, H, W)), ("checker", checker(B, H, W))):
        for q in (10, 85, 100):
            for ss in SAMPLINGS:
                files = [pillow(p, q, ss) for p in pics]
                cap = max(map(len, files)) + 5
                got, _ = encode(pics, q, ss, cap)
                want = expected(files, cap, got.shape[1])
                assert np.array_equal(got, want), (name, q, ss, np.argwhere(got != want)[:4].tolist())
                assert (got[:B, 0] > 0).all()
    again, _ = encode(pics, q, ss, cap)                     # a second launch into a fresh buffer: the same bytes
    assert np.array_equal(again, got)


def test_kernel_front_words_row_stride_and_picture_stride():
    pics = noise(3, 33, 47)
    files = [pillow(p, 75, "4:2:0") for p in pics]
    cap = max(map(len, files))
    got, front = encode(pics, 75, "4:2:0", cap, nfront=5, extra_words=6, extra_rows=2, ldi=33 * 47 * 3 + 13)
    assert np.array_equal(got, expected(files, cap, got.shape[1], 5, front, extra_rows=2))


def test_kernel_overflow_rows():
    H, W = 33, 47
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([xx * 5, yy * 7, xx + yy], -1).astype(np.uint8)
    pics = np.stack([ramp, noise(1, H, W)[0], ramp[::-1].copy()])
    files = [pillow(p, 85, "4:2:0") for p in pics]
    n = [len(f) for f in files]
    assert n[1] > max(n[0], n[2]) + 8
    for cap, lost in ((n[1] - 1, [1]), (n[1], []), (max(n[0], n[2]), [1]), (min(n[0], n[2]) - 1, [0, 1, 2]), (1, [0, 1, 2])):
        got, front = encode(pics, 85, "4:2:0", cap, nfront=2)
        want = expected(files, cap, got.shape[1], 2, front)
        assert np.array_equal(got, want), cap
        for b in range(3):                                  # that row has length 0 and keeps the canary behind it
            assert (got[b, 2] == 0 and (got[b, 3:] == CANARY).all()) == (b in lost), (cap, b)
            assert b in lost or got[b, 2] == n[b]


def test_kernel_refusals_leave_the_buffer_alone():
    pics = noise(2, 16, 24)
    cap = 4000
    ok, _ = encode(pics, 85, "4:2:0", cap)
    assert (ok[:2, 0] > 0).all()
    other = np.zeros(623, np.uint8)
    bad = [dict(inp=None), dict(hdr=None), dict(h_hdr=None), dict(out=None), dict(work=None), dict(B=0), dict(B=65536),
           dict(H=0), dict(W=0), dict(H=1025), dict(W=1025), dict(quality=0), dict(quality=101), dict(sampling=2),
           dict(sampling=-1), dict(cap=0), dict(cap=(1 << 24) + 1), dict(ldo=(cap + 3) // 4), dict(ldi=16 * 24 * 3 - 1),
           dict(nfront=-1), dict(nfront=2), dict(nfront=2, front=None, ldf=2), dict(quality=84), dict(sampling=0),
           dict(H=24, W=16), dict(h_hdr=other.ctypes.data)]
    for o in bad:
        with pytest.raises(RuntimeError):
            encode(pics, 85, "4:2:0", cap, override=o)
    for key in ("out", "work"):                             # misaligned pointers
        buf = torch.full((4096,), CANARY, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError):
            encode(pics, 85, "4:2:0", cap, override={key: buf.data_ptr() + (1 if key == "out" else 4)})
        assert (buf == CANARY).all()
    # a refused launch writes nothing: the canary buffer of a call that raises is never touched
    out = torch.full((3, 1 + 1000 + 3), CANARY, dtype=torch.int32, device="cuda")
    for o in bad:
        if "out" in o:
            continue
        with pytest.raises(RuntimeError):
            encode(pics, 85, "4:2:0", cap, override=dict(o, out=out.data_ptr(), ldo=o.get("ldo", out.shape[1])))
    assert (out == CANARY).all()


# ------------------------------------------------------------------------------------ engines
def _images(S, seed=0, n=2):
    """The seeded noise tests/test_overlay_jpeg_cpu.py shows to fit the default cap."""
    return torch.from_numpy(np.random.default_rng(S + seed).integers(0, 256, (n, S, S, 3), dtype=np.uint8))


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


SPECS = {"xception": ("jet", 0.5, "heat", "bilinear"), "resnet50": ("hot", 0.75, "flat", "bicubic"),
         "vit_b16": ("gray", 1.0, "heat", "bicubic")}


@pytest.fixture(scope="module")
def runs(xparams):
    """Per family, computed once at max_batch 2: a plain engine's logits, an overlay engine's rows, an
    overlay_jpeg engine's graph and eager rows, logits and steps, and four different batches through a stage
    pipeline on two slots with the joined engine's rows for each."""
    from kdl.engine import registry
    from kdl.engine.base import Overlay, OverlayJpeg
    from kdl.engine.stages import StagePipe
    done = {}

    def get(family):
        if family in done:
            return done[family]
        info = registry.get(family)
        p = xparams if family == "xception" else info.init_params(0)
        mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
        ov, oj = Overlay(*SPECS[family]), OverlayJpeg()
        S = info.input_size
        x = _images(S)
        e = info.engine(p, 2, "cuda")
        r = dict(S=S, hw=tuple(info.map_size), plain_logits=e.forward(x.cuda()))
        del e
        e = info.engine(p, 2, "cuda", overlay=ov, **mode)
        r["overlay"] = e.forward(x.cuda()).cpu().numpy()
        r["overlay_names"] = [s.name for s in e.steps]
        batches = [_images(S, 20 + i) for i in range(4)]
        r["overlay_batches"] = [e.forward(b.cuda()).cpu().numpy() for b in batches]
        del e
        eng = info.engine(p, 2, "cuda", overlay=ov, overlay_jpeg=oj, **mode)
        r["steps"] = [(s.kind, s.name) for s in eng.steps]
        r["graph"] = eng.forward(x.cuda(), capture=True).cpu().numpy()
        r["raw"] = eng.overlay_raw(0)[:2].cpu().numpy()
        r["logits"] = eng.last_logits(0)[:2].clone()
        r["eager"] = eng.forward(x.cuda(), capture=False).cpu().numpy()
        r["joined"] = [eng.forward(b.cuda()).cpu().numpy() for b in batches]
        del eng
        pipe = StagePipe(info.engine(p, 2, "cuda", overlay=ov, overlay_jpeg=oj, **mode), info.stage_cut)
        r["ranges"] = list(pipe.ranges)
        slots = pipe.add_input_slots(2)
        outs, ev = [], [torch.cuda.Event() for _ in range(2)]
        for i, im in enumerate(batches):
            j = i % 2
            if i >= 2:                                           # the slot's rows are drained before it is refilled
                ev[j].synchronize()
                outs.append(pipe.slot_logits(j).cpu().numpy())
            slots[j].copy_(im)
            ready = torch.cuda.Event()
            ready.record()
            pipe.launch_async(2, [ready], [ev[j]], slot=j)
        for i in (2, 3):
            ev[i % 2].synchronize()
            outs.append(pipe.slot_logits(i % 2).cpu().numpy())
        r["pipe"] = outs
        del pipe
        done[family] = r
        return r
    return get


FAMILIES = ["xception", "vit_b16", "resnet50"]


def check_rows(rows, overlay_rows, hw, S):
    """overlay_jpeg rows against the overlay engine's rows: the front words bit for bit, and each file Pillow's
    encoding of the picture the overlay engine returned."""
    from kdl.engine.base import overlay_jpeg_cap, unpack_overlay, unpack_overlay_jpeg
    h, w = hw
    cap = overlay_jpeg_cap(S)
    assert rows.shape == (len(overlay_rows), 2 + h * w + 1 + (cap + 3) // 4)
    assert np.array_equal(_bits(rows[:, :2 + h * w]), _bits(overlay_rows[:, :2 + h * w]))
    *_, pics = unpack_overlay(overlay_rows, h, w, S)
    *_, files = unpack_overlay_jpeg(rows, h, w, cap)
    body = np.ascontiguousarray(rows[:, 2 + h * w + 1:]).view(np.uint8).reshape(len(rows), -1)
    for b, f in enumerate(files):
        assert len(f) > 0 and f == pillow(pics[b], 85, "4:2:0"), b
        assert (body[b, len(f):] == 0).all()                          # pad bytes are 0


@pytest.mark.parametrize("family", FAMILIES)
def test_engine_rows(family, runs):
    r = runs(family)
    assert torch.equal(r["logits"], r["plain_logits"])               # the head is untouched, bit for bit
    assert np.array_equal(_bits(r["graph"]), _bits(r["eager"]))
    assert np.array_equal(_bits(r["raw"]), _bits(r["overlay"]))       # the raw rows, now device-only
    check_rows(r["graph"], r["overlay"], r["hw"], r["S"])
    assert [s[1] for s in r["steps"]] == r["overlay_names"] + ["overlay_jpeg"]
    assert r["steps"][-1] == ("overlay_jpeg", "overlay_jpeg")


@pytest.mark.parametrize("family", FAMILIES)
def test_stage_pipeline_files_are_each_batch_s_own(family, runs):
    r = runs(family)
    assert len(r["ranges"]) >= 2 and r["ranges"][-1][1] == len(r["steps"])
    for i, (got, want) in enumerate(zip(r["pipe"], r["joined"])):
        assert np.array_equal(_bits(got), _bits(want)), f"batch {i}"
    for i in range(1, 4):
        assert not np.array_equal(_bits(r["joined"][i]), _bits(r["joined"][0]))
    for got, ov in zip(r["pipe"], r["overlay_batches"]):
        check_rows(got, ov, r["hw"], r["S"])


def test_overlay_jpeg_needs_an_overlay_and_a_valid_spec(xparams):
    from kdl.engine.base import Overlay, OverlayJpeg
    from kdl.engine.xception import XceptionEngine
    with pytest.raises(ValueError, match="overlay=Overlay"):
        XceptionEngine(xparams, max_batch=2, device="cuda", explain=True, overlay_jpeg=OverlayJpeg())
    for bad in (OverlayJpeg(quality=0), OverlayJpeg(quality=101), OverlayJpeg(subsampling="4:2:2"), OverlayJpeg(max_bytes=0)):
        with pytest.raises(ValueError):
            XceptionEngine(xparams, max_batch=2, device="cuda", explain=True, overlay=Overlay(), overlay_jpeg=bad)


# ------------------------------------------------------------------------------------ server
def test_server_overlay_jpeg_bytes(tmp_path):
    """One overlay_jpeg_bytes request of two JPEGs over gRPC: each file is the shipped rule on the shipped overlay
    rule of the served preprocess result and the returned map; map, class and score are explain_bytes' answer."""
    from pathlib import Path

    import grpc

    from kdl.engine.base import Overlay, OverlayJpeg, overlay_jpeg_cap
    from kdl.gateway import preprocess as pp
    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.jpeg_encode import encode_rule
    from kdl.serving.overlay import overlay_rule
    from kdl.serving.server import ModelServer

    img = Image.open(Path(__file__).parent / "data" / "pants.png").convert("RGB")
    files = []
    for q in (90, 75):
        b = io.BytesIO()
        img.save(b, "JPEG", quality=q)
        files.append(b.getvalue())
    u8 = np.stack([pp.to_uint8(pp.load_image(f)) for f in files])
    base = tmp_path / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text(
        '{"seed": 0, "overlay": {"colormap": "hot", "alpha": 0.625}, "overlay_jpeg": {"quality": 70, "subsampling": "4:4:4"}}')
    spec, jspec = Overlay("hot", 0.625), OverlayJpeg(70, "4:4:4")
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                       file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000, allowed_batch_sizes=[2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            out = stub.Predict(make_request(files, signature="overlay_jpeg_bytes", input_key="image_bytes"), timeout=120).outputs
            exp = stub.Predict(make_request(files, signature="explain_bytes", input_key="image_bytes"), timeout=120).outputs
        assert sorted(out) == ["classes", "heatmap", "jpeg_bytes", "scores"]
        assert out["jpeg_bytes"].dtype == 7 and [d.size for d in out["jpeg_bytes"].tensor_shape.dim] == [2]
        heat = np.asarray(out["heatmap"].float_val, np.float32).reshape(2, 10, 10)
        assert list(out["classes"].string_val) == list(exp["classes"].string_val)
        assert np.array_equal(_bits(np.asarray(out["scores"].float_val, np.float32)),
                              _bits(np.asarray(exp["scores"].float_val, np.float32)))
        assert np.array_equal(_bits(heat), _bits(np.asarray(exp["heatmap"].float_val, np.float32).reshape(2, 10, 10)))
        for b in range(2):
            want = encode_rule(overlay_rule(u8[b], heat[b], spec), 70, "4:4:4")
            assert len(want) > 0 and bytes(out["jpeg_bytes"].string_val[b]) == want, b
        s = srv.manager.get("clothing-model", None, None)
        r = s.runner("overlay_jpeg")
        assert r.out_cols == 102 + 1 + (overlay_jpeg_cap(299) + 3) // 4 and r.executors
        assert all(ex.engine.overlay == spec and ex.engine.overlay_jpeg == jspec for ex in r.executors)
        assert s.device_alive()
    finally:
        srv.stop(0)
