"""heat_overlay (kernels/overlay.hip) alone, inside the Xception, ResNet-50 and ViT engines, through the
stage pipeline and behind the server.

The oracle of the kernel tests is written HERE, not imported: the quantisation, colour tables and
blend in a few numpy lines and the upsampling by Pillow itself (``Image.resize`` on an ``L`` image).
Everything is integer arithmetic, so every comparison is for equality of bytes; the shipped
``overlay_rule`` (kdl/serving/overlay.py) is checked against Pillow in tests/test_overlay_cpu.py, so
the two rules check each other.
"""
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5      # a NaN pattern, as int32
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
FILTER_ID = {"bilinear": 1, "bicubic": 3}
# (S, h = w, B): S = 299 with five images puts the packed input images at all four residues mod 4
# (299 * 299 * 3 = 268203 = 3 mod 4); 19 -> 19 is the identity, 19 -> 20 and 3 -> 17 the smallest upscales
SHAPES = [(299, 10, 5), (224, 14, 2), (224, 7, 2), (600, 19, 2), (19, 19, 1), (20, 19, 1), (17, 3, 1)]
ALPHAS = [0, 1, 128, 256]


# ------------------------------------------------------------------------------------ the oracle
def tables():
    u = np.arange(256, dtype=np.int64)
    jet = np.stack([np.clip(383 - np.abs(4 * u - 255 * k), 0, 255) for k in (3, 2, 1)], 1)
    hot = np.stack([np.clip(3 * u - 255 * k, 0, 255) for k in (0, 1, 2)], 1)
    return {"jet": jet.astype(np.uint8), "hot": hot.astype(np.uint8), "gray": np.stack([u, u, u], 1).astype(np.uint8)}


TABLES = tables()


def upsampled(heat, S, flt):
    """fp32 [h, w] -> int64 [S, S]: quantise (one fp32 multiply, round-half-even, NaN -> 0), then Pillow."""
    x = np.asarray(heat, np.float32)
    x = np.where(np.isnan(x), np.float32(0), np.minimum(np.maximum(x, np.float32(0)), np.float32(1)))
    q = np.rint(x.astype(np.float32) * np.float32(255)).astype(np.uint8)
    return np.asarray(Image.fromarray(q, "L").resize((S, S), PIL_FILTER[flt])).astype(np.int64)


def blend_rule(img, u, tab, a, blend):
    ap = ((a * u + 127) // 255 if blend else np.full_like(u, a))[..., None]
    return ((img.astype(np.int64) * (256 - ap) + tab[u].astype(np.int64) * ap + 128) >> 8).astype(np.uint8)


def heat_fields(h, w, seed):
    """name -> fp32 [h, w]: random, all zeros, all ones, NaN and out-of-range entries, one hot cell per corner."""
    rng = np.random.default_rng(seed)
    odd = rng.random((h, w), dtype=np.float32) * 3 - 1            # -1 .. 2
    odd.reshape(-1)[::3] = np.nan
    odd.reshape(-1)[1::7] = np.inf
    odd.reshape(-1)[2::11] = -np.inf
    out = {"random": rng.random((h, w), dtype=np.float32), "zeros": np.zeros((h, w), np.float32),
           "ones": np.ones((h, w), np.float32), "odd": odd}
    for name, (y, x) in {"tl": (0, 0), "tr": (0, w - 1), "bl": (h - 1, 0), "br": (h - 1, w - 1)}.items():
        f = np.zeros((h, w), np.float32)
        f[y, x] = 1.0
        out[name] = f
    return out


# ------------------------------------------------------------------------------------ launching
_TAB_CACHE = {}


def device_tables(h, w, S, flt):
    """Pillow's bounds and coefficients of the two axes: host arrays and their device copies."""
    key = (h, w, S, flt)
    if key not in _TAB_CACHE:
        from kdl.ops import _lib
        rt = _lib.rt()
        xb, xk = rt.resample_coeffs(w, S, FILTER_ID[flt])
        yb, yk = rt.resample_coeffs(h, S, FILTER_ID[flt])
        host = {k: np.ascontiguousarray(v, np.int32) for k, v in dict(xb=xb, xk=xk, yb=yb, yk=yk).items()}
        _TAB_CACHE[key] = (host, {k: torch.from_numpy(v).cuda() for k, v in host.items()})
    return _TAB_CACHE[key]


_DEV_TAB = {}


def device_colours(name):
    if name not in _DEV_TAB:
        _DEV_TAB[name] = torch.from_numpy(TABLES[name].copy()).cuda()
    return _DEV_TAB[name]


def words(S):
    return (S * S * 3 + 3) // 4


def make_rows(B, h, w, S, fields, extra_rows=1, ldo=None):
    """int32 host buffer [B + extra_rows, ldo], the canary everywhere, then class, score and the heat
    field of every image < B in front. ldo defaults to an odd number above the need, so the rows
    (and the pictures in them) start at all four residues mod 16 bytes."""
    need = 2 + h * w + words(S)
    if ldo is None:
        ldo = need + 5
        ldo += 1 - ldo % 2
    buf = np.full((B + extra_rows, ldo), CANARY, np.int32)
    for b in range(B):
        buf[b, 0] = 7 + b
        buf[b, 1:2] = np.float32(0.25 + b).view(np.int32)
        buf[b, 2:2 + h * w] = np.ascontiguousarray(fields[b % len(fields)], np.float32).reshape(-1).view(np.int32)
    return buf


def args(inp, rows, B, S, h, w, flt, tab, a, blend):
    host, dev = device_tables(h, w, S, flt)
    return dict(inp=inp.data_ptr(), out=rows.data_ptr(), tab=device_colours(tab).data_ptr(),
                xb=dev["xb"].data_ptr(), xk=dev["xk"].data_ptr(), yb=dev["yb"].data_ptr(), yk=dev["yk"].data_ptr(),
                h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=B, S=S, h=h, w=w, ldo=rows.shape[1],
                xks=host["xk"].shape[1], yks=host["yk"].shape[1], a=a, blend=blend)


def launch(d):
    from kdl.ops import _lib
    _lib.lib().heat_overlay(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def expected(before, imgs, fields, B, S, h, w, flt, tab, a, blend, ups=None):
    """The whole buffer after a launch: ``before`` with the S*S*3 picture bytes of rows < B replaced."""
    want = before.copy()
    by = want.view(np.uint8).reshape(want.shape[0], -1)
    o = 4 * (2 + h * w)
    for b in range(B):
        f = fields[b % len(fields)]
        u = ups[b % len(fields)] if ups is not None else upsampled(f, S, flt)
        by[b, o:o + S * S * 3] = blend_rule(imgs[b], u, TABLES[tab], a, blend).reshape(-1)
    return want


def images(B, S, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, S, S, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("S,n,B", SHAPES)
def test_kernel_is_bit_exact_and_writes_nothing_else(S, n, B):
    """Both filters, both blends, a in {0, 1, 128, 256} and the three tables over random heat; every
    heat field with both filters and both blends. The WHOLE buffer is compared: words 0 .. 2 + hw of
    every row, the pad bytes of the picture's last word, the words past it and the row behind the
    batch keep the canary (or what was in front); a second launch gives the same bytes."""
    imgs = images(B, S, seed=S + n)
    inp = torch.from_numpy(imgs).cuda()
    fields = heat_fields(n, n, seed=S * 31 + n)
    rnd = [fields["random"], fields["odd"]]
    cases = 0
    for flt in PIL_FILTER:
        ups = [upsampled(f, S, flt) for f in rnd]
        for blend, a, tab in itertools.product((0, 1), ALPHAS, TABLES):
            before = make_rows(B, n, n, S, rnd)
            rows = torch.from_numpy(before).cuda()
            launch(args(inp, rows, B, S, n, n, flt, tab, a, blend))
            got = rows.cpu().numpy()
            want = expected(before, imgs, rnd, B, S, n, n, flt, tab, a, blend, ups)
            assert np.array_equal(got, want), (S, n, flt, blend, a, tab, int((got != want).sum()))
            cases += 1
        names = list(fields)
        for i in range(0, len(names), B):                            # every field, B at a time
            fs = [fields[k] for k in names[i:i + B]]
            for blend in (0, 1):
                before = make_rows(B, n, n, S, fs)
                rows = torch.from_numpy(before).cuda()
                d = args(inp, rows, B, S, n, n, flt, "jet", 128, blend)
                launch(d)
                got = rows.cpu().numpy()
                want = expected(before, imgs, fs, B, S, n, n, flt, "jet", 128, blend)
                assert np.array_equal(got, want), (S, n, flt, blend, names[i:i + B])
                again = torch.from_numpy(before).cuda()              # determinism: the same bytes again
                launch(dict(d, out=again.data_ptr()))
                assert np.array_equal(again.cpu().numpy(), got)
    assert cases == 48


def test_endpoints_photograph_and_colour_table():
    """a = 0 gives the photograph back, a = 256 flat the colour table of the upsampled map."""
    S, n, B = 299, 10, 5
    imgs = images(B, S, 1)
    inp = torch.from_numpy(imgs).cuda()
    f = [heat_fields(n, n, 9)["random"]]
    o = 4 * (2 + n * n)
    for a, blend in ((0, 0), (0, 1), (256, 0)):
        rows = torch.from_numpy(make_rows(B, n, n, S, f)).cuda()
        launch(args(inp, rows, B, S, n, n, "bilinear", "jet", a, blend))
        pics = rows.cpu().numpy().view(np.uint8).reshape(B + 1, -1)[:B, o:o + S * S * 3].reshape(B, S, S, 3)
        want = imgs if a == 0 else np.broadcast_to(TABLES["jet"][upsampled(f[0], S, "bilinear")], imgs.shape)
        assert np.array_equal(pics, want), (a, blend)


def test_exact_row_length_rectangular_map_and_full_grid():
    """ldo at its minimum (the row behind the batch starts right after the last picture word); a
    5 x 9 map; a map as large as the picture's side in one axis only."""
    for S, h, w, B in ((31, 5, 9, 3), (24, 24, 3, 2), (9, 1, 1, 2)):
        imgs = images(B, S, S)
        inp = torch.from_numpy(imgs).cuda()
        f = [np.random.default_rng(S).random((h, w), dtype=np.float32)]
        before = make_rows(B, h, w, S, f, ldo=2 + h * w + words(S))
        rows = torch.from_numpy(before).cuda()
        launch(args(inp, rows, B, S, h, w, "bicubic", "hot", 200, 1))
        want = expected(before, imgs, f, B, S, h, w, "bicubic", "hot", 200, 1)
        assert np.array_equal(rows.cpu().numpy(), want), (S, h, w)


def test_refusals_leave_the_buffer_alone():
    n = 19
    S2, n2 = 224, 14
    imgs = images(2, S2, 3)
    inp = torch.from_numpy(imgs).cuda()
    f = [heat_fields(n2, n2, 4)["random"]]
    before = make_rows(2, n2, n2, S2, f)
    rows = torch.from_numpy(before).cuda()
    good = args(inp, rows, 2, S2, n2, n2, "bilinear", "jet", 128, 1)
    host, _ = device_tables(n2, n2, S2, "bilinear")
    need = 2 + n2 * n2 + words(S2)

    def broken(name, fn):
        t = host[name].copy()
        fn(t)
        return t

    keep = [broken("xb", lambda t: t.__setitem__((S2 - 1, 1), 3)),           # taps past the map's last column
            broken("xb", lambda t: t.__setitem__((5, 0), -1)),               # a negative first sample
            broken("yb", lambda t: t.__setitem__((100, 0), 0)),              # steps back
            broken("yb", lambda t: t.__setitem__((S2 - 1, 1), 9))]           # more taps than the table has
    bad = [dict(inp=None), dict(out=None), dict(tab=None), dict(xb=None), dict(xk=None), dict(yb=None),
           dict(yk=None), dict(h_xb=None), dict(h_yb=None),
           dict(out=good["out"] + 4, ldo=good["ldo"] - 1), dict(tab=good["tab"] + 4), dict(xb=good["xb"] + 8),
           dict(xk=good["xk"] + 4), dict(yb=good["yb"] + 8), dict(yk=good["yk"] + 4),
           dict(B=0), dict(B=-1), dict(B=65536), dict(h=0), dict(w=0), dict(h=65, w=64), dict(S=n2 - 1),
           dict(S=1025), dict(ldo=need - 1), dict(a=257), dict(a=-1), dict(blend=2), dict(blend=-1),
           dict(xks=0), dict(xks=9), dict(yks=0), dict(yks=9),
           dict(h_xb=keep[0].ctypes.data), dict(h_xb=keep[1].ctypes.data), dict(h_yb=keep[2].ctypes.data),
           dict(h_yb=keep[3].ctypes.data)]
    for over in bad:
        with pytest.raises(RuntimeError):
            launch(dict(good, **over))
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy(), before), over
    # a band that needs more map rows than a workgroup stages: a 19-row map whose rows 1.. all start at row 17
    hostS, _ = device_tables(n, n, 600, "bilinear")
    yb = hostS["yb"].copy()
    yb[0] = (0, 2)
    yb[1:, 0], yb[1:, 1] = 17, 2
    imgs6 = images(1, 600, 5)
    inp6 = torch.from_numpy(imgs6).cuda()
    before6 = make_rows(1, n, n, 600, [heat_fields(n, n, 6)["random"]])
    rows6 = torch.from_numpy(before6).cuda()
    with pytest.raises(RuntimeError):
        launch(dict(args(inp6, rows6, 1, 600, n, n, "bilinear", "jet", 128, 1), h_yb=yb.ctypes.data))
    assert np.array_equal(rows6.cpu().numpy(), before6)
    launch(good)                                                     # the same arguments, unbroken, do write
    want = expected(before, imgs, f, 2, S2, n2, n2, "bilinear", "jet", 128, 1)
    assert np.array_equal(rows.cpu().numpy(), want)


# ------------------------------------------------------------------------------------ engines
def _images(S, seed=5, n=2):
    return torch.randint(0, 256, (n, S, S, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


SPECS = {"xception": ("jet", 0.5, "heat", "bilinear"), "resnet50": ("hot", 0.75, "flat", "bicubic"),
         "vit_b16": ("gray", 1.0, "heat", "bicubic")}


def check_rows(rows, base_rows, imgs, hw, S, spec):
    """Overlay rows against the heatmap engine's rows and the oracle applied to the engine's own map."""
    from kdl.engine.base import unpack_explain, unpack_overlay
    h, w = hw
    cmap, alpha, blend, flt = spec
    assert rows.shape == (len(imgs), 2 + h * w + words(S))
    assert np.array_equal(_bits(rows[:, :2 + h * w]), _bits(base_rows))       # class, score and map: bit for bit
    c, s, heat, pics = unpack_overlay(rows, h, w, S)
    c0, s0, heat0 = unpack_explain(base_rows, h, w)
    assert np.array_equal(c, c0) and np.array_equal(_bits(heat), _bits(heat0))
    for b in range(len(imgs)):
        want = blend_rule(imgs[b], upsampled(heat[b], S, flt), TABLES[cmap], int(round(alpha * 256)), blend == "heat")
        assert np.array_equal(pics[b], want), b
    pad = rows.view(np.uint8).reshape(len(imgs), -1)[:, 4 * (2 + h * w) + S * S * 3:]
    assert (pad == 0).all()                                          # the buffer was zeros: the pad bytes still are
    return pics


@pytest.fixture(scope="module")
def runs(xparams):
    """Per family, computed once at max_batch 2: a plain engine's logits, a heatmap (explain / rollout)
    engine's rows, an overlay engine's graph and eager rows, logits and steps, and four different
    batches through a stage pipeline on two slots with the joined engine's rows for each."""
    from kdl.engine import registry
    from kdl.engine.base import Overlay
    from kdl.engine.stages import StagePipe
    done = {}

    def get(family):
        if family in done:
            return done[family]
        info = registry.get(family)
        p = xparams if family == "xception" else info.init_params(0)
        mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
        ov = Overlay(*SPECS[family])
        S = info.input_size
        x = _images(S)
        e = info.engine(p, 2, "cuda")
        r = dict(S=S, hw=tuple(info.map_size), x=x.numpy(), plain_logits=e.forward(x.cuda()),
                 plain_names=[s.name for s in e.steps])
        del e
        e = info.engine(p, 2, "cuda", **mode)
        r["base"] = e.forward(x.cuda()).cpu().numpy()
        r["base_names"] = [s.name for s in e.steps]
        del e
        eng = info.engine(p, 2, "cuda", overlay=ov, **mode)
        r["steps"] = [(s.kind, s.name, s.src) for s in eng.steps]
        r["graph"] = eng.forward(x.cuda(), capture=True).cpu().numpy()
        r["logits"] = eng.last_logits(0)[:2].clone()
        r["eager"] = eng.forward(x.cuda(), capture=False).cpu().numpy()
        batches = [_images(S, 20 + i) for i in range(4)]
        r["batches"] = [b.numpy() for b in batches]
        r["joined"] = [eng.forward(b.cuda()).cpu().numpy() for b in batches]
        del eng
        pipe = StagePipe(info.engine(p, 2, "cuda", overlay=ov, **mode), info.stage_cut)
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


@pytest.mark.parametrize("family", FAMILIES)
def test_engine_rows(family, runs):
    r = runs(family)
    assert torch.equal(r["logits"], r["plain_logits"])               # the head is untouched, bit for bit
    assert np.array_equal(_bits(r["graph"]), _bits(r["eager"]))
    pics = check_rows(r["graph"], r["base"], r["x"], r["hw"], r["S"], SPECS[family])
    assert not np.array_equal(pics, r["x"])                           # the heat is on the picture
    assert [s[1] for s in r["steps"]] == r["base_names"] + ["overlay"] and r["steps"][-1] == ("overlay", "overlay", "input")
    assert [n for n in r["base_names"] if n in r["plain_names"]] == r["plain_names"]


@pytest.mark.parametrize("family", FAMILIES)
def test_stage_pipeline_pictures_are_each_batch_s_own(family, runs):
    r = runs(family)
    assert len(r["ranges"]) >= 2 and r["ranges"][-1][1] == len(r["steps"])    # the overlay step: the last stage
    for i, (got, want) in enumerate(zip(r["pipe"], r["joined"])):
        assert np.array_equal(_bits(got), _bits(want)), f"batch {i}"
    for i in range(1, 4):                                            # and the four batches do differ
        assert not np.array_equal(_bits(r["joined"][i]), _bits(r["joined"][0]))
    h, w = r["hw"]
    from kdl.engine.base import unpack_overlay
    for got, imgs in zip(r["pipe"], r["batches"]):
        _, _, heat, pics = unpack_overlay(got, h, w, r["S"])
        cmap, alpha, blend, flt = SPECS[family]
        for b in range(2):
            want = blend_rule(imgs[b], upsampled(heat[b], r["S"], flt), TABLES[cmap], int(round(alpha * 256)),
                              blend == "heat")
            assert np.array_equal(pics[b], want)


def test_overlay_needs_a_heatmap_and_a_uint8_input(xparams):
    from kdl.engine.base import Overlay
    from kdl.engine.vit import ViTEngine
    from kdl.engine.xception import XceptionEngine
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        XceptionEngine(xparams, max_batch=2, device="cuda", overlay=Overlay())
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        ViTEngine({}, max_batch=2, device="cuda", overlay=Overlay())
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        XceptionEngine(xparams, max_batch=2, device="cuda", topk=3, overlay=Overlay())
    with pytest.raises(ValueError, match="uint8"):
        XceptionEngine(xparams, max_batch=2, device="cuda", in_kind="f32", explain=True, overlay=Overlay())
    for bad in (Overlay(colormap="viridis"), Overlay(alpha=1.5), Overlay(blend="multiply"), Overlay(filter="lanczos")):
        with pytest.raises(ValueError):
            XceptionEngine(xparams, max_batch=2, device="cuda", explain=True, overlay=bad)


# ------------------------------------------------------------------------------------ server
def test_server_overlay_bytes(tmp_path):
    """One overlay_bytes request of two JPEGs over gRPC: the pictures are the shipped rule applied to
    the served preprocess result (decode + nearest resize) and the returned map; the map, class and
    score are explain_bytes' answer for the same files."""
    import io
    from pathlib import Path

    import grpc

    from kdl.engine.base import Overlay
    from kdl.gateway import preprocess as pp
    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving.config import BatchingParams, ServerConfig
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
    (base / "1" / "synthetic.json").write_text('{"seed": 0, "overlay": {"colormap": "hot", "alpha": 0.625}}')
    spec = Overlay("hot", 0.625)
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                       file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000, allowed_batch_sizes=[2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            out = stub.Predict(make_request(files, signature="overlay_bytes", input_key="image_bytes"), timeout=120).outputs
            exp = stub.Predict(make_request(files, signature="explain_bytes", input_key="image_bytes"), timeout=120).outputs
        assert sorted(out) == ["classes", "heatmap", "overlay", "scores"]
        assert [d.size for d in out["overlay"].tensor_shape.dim] == [2, 299, 299, 3]
        assert [d.size for d in out["heatmap"].tensor_shape.dim] == [2, 10, 10]
        heat = np.asarray(out["heatmap"].float_val, np.float32).reshape(2, 10, 10)
        pics = np.frombuffer(out["overlay"].tensor_content, np.uint8).reshape(2, 299, 299, 3)
        assert list(out["classes"].string_val) == list(exp["classes"].string_val)
        assert np.array_equal(_bits(np.asarray(out["scores"].float_val, np.float32)),
                              _bits(np.asarray(exp["scores"].float_val, np.float32)))
        assert np.array_equal(_bits(heat), _bits(np.asarray(exp["heatmap"].float_val, np.float32).reshape(2, 10, 10)))
        for b in range(2):
            assert np.array_equal(pics[b], overlay_rule(u8[b], heat[b], spec)), b
        s = srv.manager.get("clothing-model", None, None)
        r = s.runner("overlay")
        assert r.out_cols == 102 + words(299) and r.executors
        assert all(ex.engine.explain and ex.engine.overlay == spec for ex in r.executors)
        assert s.device_alive()
    finally:
        srv.stop(0)
