"""palette (kernels/palette.hip) alone, inside the Xception and ViT engines, through the stage pipeline
and behind the server.

The rule is integer arithmetic, so every comparison is for equality of bits against ``palette_rule``
(kdl/serving/palette.py) applied to the row's own map and the input; tests/test_palette_cpu.py checks that
rule against literal answers and a second implementation in plain loops.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5      # a NaN pattern, as int32
FILTER_ID = {"bilinear": 1, "bicubic": 3}
WEIGHTS = ("uniform", "map")
# (S, h, w, B): one pixel; S*S*3 no multiple of 4; two staged bands of 8 rows and one row more; one
# workgroup's 64 rows exactly (and the two-tone tie: 32 white rows, 32 black ones); five workgroups per image
# with a ragged last one. 1024, sixteen workgroups at the uint32 bound, has a test of its own
SHAPES = [(1, 1, 1, 1), (5, 2, 3, 2), (17, 3, 2, 3), (64, 7, 7, 2), (299, 10, 10, 2)]


# ------------------------------------------------------------------------------------ inputs
def pictures(S, seed):
    """name -> uint8 [S, S, 3]: noise, flat, the two-tone tie, two colours (fewer than K = 3 or 8), colours
    that crowd a few bins, a smooth ramp."""
    rng = np.random.default_rng(seed)
    two = np.zeros((S, S, 3), np.uint8)
    two[:(S + 1) // 2] = 255
    few = np.empty((S, S, 3), np.uint8)
    few[...] = (200, 30, 40)
    few[:, S // 3:] = (20, 90, 160)
    crowd = (rng.integers(0, 3, (S, S, 3)) * 7 + np.array([10, 120, 236])).astype(np.uint8)
    ramp = np.clip(np.add.outer(np.arange(S) * 3, np.arange(S))[..., None] // max(S // 64, 1) + np.array([0, 40, 90]),
                   0, 255).astype(np.uint8)
    return {"noise": rng.integers(0, 256, (S, S, 3), dtype=np.uint8), "flat": np.full((S, S, 3), 200, np.uint8),
            "two": two, "few": few, "crowd": crowd, "ramp": ramp}


def heat_fields(h, w, seed):
    """name -> fp32 [h, w]: random, random with NaN and out-of-range entries, all zeros, all NaN, all ones."""
    rng = np.random.default_rng(seed)
    odd = rng.random((h, w), dtype=np.float32) * 3 - 1
    odd.reshape(-1)[::3] = np.nan
    odd.reshape(-1)[1::7] = np.inf
    return {"random": rng.random((h, w), dtype=np.float32), "odd": odd, "zeros": np.zeros((h, w), np.float32),
            "nan": np.full((h, w), np.nan, np.float32), "ones": np.ones((h, w), np.float32)}


_TAB_CACHE = {}


def device_tables(h, w, S, flt):
    key = (h, w, S, flt)
    if key not in _TAB_CACHE:
        from kdl.ops import _lib
        rt = _lib.rt()
        xb, xk = rt.resample_coeffs(w, S, FILTER_ID[flt])
        yb, yk = rt.resample_coeffs(h, S, FILTER_ID[flt])
        host = {k: np.ascontiguousarray(v, np.int32) for k, v in dict(xb=xb, xk=xk, yb=yb, yk=yk).items()}
        _TAB_CACHE[key] = (host, {k: torch.from_numpy(v).cuda() for k, v in host.items()})
    return _TAB_CACHE[key]


def workspace(B):
    from kdl.ops import _lib
    return torch.zeros(_lib.lib().palette_workspace(B), dtype=torch.uint8, device="cuda")


def make_rows(B, h, w, K, fields, extra_rows=1, ldo=None):
    """int32 host buffer [B + extra_rows, ldo], the canary everywhere, then class, score and the heat field
    of every image < B in front. ldo defaults to five words above the need (odd or even with K's parity, so
    the rows start at every residue mod 16 bytes)."""
    need = 2 + h * w + 1 + 2 * K
    ldo = need + 5 if ldo is None else ldo
    buf = np.full((B + extra_rows, ldo), CANARY, np.int32)
    for b in range(B):
        buf[b, 0] = 7 + b
        buf[b, 1:2] = np.float32(0.25 + b).view(np.int32)
        buf[b, 2:2 + h * w] = np.ascontiguousarray(fields[b], np.float32).reshape(-1).view(np.int32)
    return buf


def args(inp, rows, work, B, S, h, w, flt, K, T, weight):
    host, dev = device_tables(h, w, S, flt)
    return dict(inp=inp.data_ptr(), out=rows.data_ptr(), work=work.data_ptr(),
                xb=dev["xb"].data_ptr(), xk=dev["xk"].data_ptr(), yb=dev["yb"].data_ptr(), yk=dev["yk"].data_ptr(),
                h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=B, S=S, h=h, w=w, ldo=rows.shape[1],
                xks=host["xk"].shape[1], yks=host["yk"].shape[1], K=K, T=T, weight=WEIGHTS.index(weight))


def launch(d):
    from kdl.ops import _lib
    _lib.lib().palette(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def words_of(img, heat, spec):
    """The 1 + 2K words the rule gives, as int32 bits."""
    from kdl.serving.palette import palette_rule
    W, col, n = palette_rule(img, heat, spec)
    c = col.astype(np.uint32)
    out = np.empty(1 + 2 * spec.colors, np.uint32)
    out[0] = W
    out[1::2] = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)
    out[2::2] = n
    return out.view(np.int32)


def expected(before, imgs, fields, B, h, w, spec):
    want = before.copy()
    o = 2 + h * w
    for b in range(B):
        want[b, o:o + 1 + 2 * spec.colors] = words_of(imgs[b], fields[b], spec)
    return want


# ------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("S,h,w,B", SHAPES)
def test_kernels_are_bit_exact_and_write_nothing_else(S, h, w, B):
    """K in {1, 3, 8} x T in {1, 8} x both filters x both weights, the pictures and heat fields rotating
    through the batch. The WHOLE buffer is compared: the row fronts, the words behind the answer and the
    row behind the batch keep what they had; the workspace is all zero again; a second launch into a
    fresh buffer gives the same bits."""
    from kdl.engine.base import Palette
    pics, fields = pictures(S, seed=S), heat_fields(h, w, seed=S * 31 + h)
    pn, fn = list(pics), list(fields)
    work = workspace(B)
    cases = 0
    for i, (K, T, flt, weight) in enumerate(itertools.product((1, 3, 8), (1, 8), FILTER_ID, WEIGHTS)):
        spec = Palette(K, weight, flt, T)
        imgs = np.stack([pics[pn[(i + b) % len(pn)]] for b in range(B)])
        fs = [fields[fn[(i // 2 + b) % len(fn)]] for b in range(B)]
        inp = torch.from_numpy(imgs).cuda()
        before = make_rows(B, h, w, K, fs)
        rows = torch.from_numpy(before).cuda()
        d = args(inp, rows, work, B, S, h, w, flt, K, T, weight)
        launch(d)
        got, want = rows.cpu().numpy(), expected(before, imgs, fs, B, h, w, spec)
        assert np.array_equal(got, want), (spec, [pn[(i + b) % len(pn)] for b in range(B)],
                                           np.argwhere(got != want)[:4].tolist())
        assert not work.any(), spec
        if i % 6 == 0:
            again = torch.from_numpy(before).cuda()
            launch(dict(d, out=again.data_ptr()))
            assert np.array_equal(again.cpu().numpy(), got)
        cases += 1
    assert cases == 24


def test_every_picture_with_every_heat_field():
    """17 pixels a side, every picture against every heat field, both weights, K = 3 (two tones, two
    colours only, an all-zero and an all-NaN map among them), at the minimal row length."""
    from kdl.engine.base import Palette
    S, h, w, K = 17, 3, 2, 3
    pics, fields = pictures(S, seed=3), heat_fields(h, w, seed=4)
    combos = list(itertools.product(pics, fields))
    B = len(combos)
    imgs = np.stack([pics[p] for p, _ in combos])
    fs = [fields[f] for _, f in combos]
    inp, work = torch.from_numpy(imgs).cuda(), workspace(B)
    for weight in WEIGHTS:
        spec = Palette(K, weight, "bilinear", 4)
        before = make_rows(B, h, w, K, fs, ldo=2 + h * w + 1 + 2 * K)
        rows = torch.from_numpy(before).cuda()
        launch(args(inp, rows, work, B, S, h, w, "bilinear", K, 4, weight))
        got, want = rows.cpu().numpy(), expected(before, imgs, fs, B, h, w, spec)
        assert np.array_equal(got, want), (weight, [combos[b] for b in np.unique(np.argwhere(got != want)[:, 0])][:6])
        assert not work.any()
    o = 2 + h * w
    zero = [b for b, (_, f) in enumerate(combos) if f in ("zeros", "nan")]
    assert zero and not got[zero, o:o + 1 + 2 * K].any()         # map weight, no heat: W = 0 and zeros
    two = combos.index(("two", "ones"))                          # nine white rows, eight black ones, every weight 15
    assert got[two, o:o + 7].tolist() == [15 * 17 * 17, 0xFFFFFF, 15 * 9 * 17, 0, 15 * 8 * 17, 0, 0]


def test_the_uint32_bound_and_sixteen_workgroups_an_image():
    """1024 x 1024 all white at uniform weight: the largest sums the rule allows; then noise under a 19 x 19
    map."""
    from kdl.engine.base import Palette
    S, n = 1024, 19
    fields = [heat_fields(n, n, 8)["random"]]
    work = workspace(1)
    white = np.full((1, S, S, 3), 255, np.uint8)
    before = make_rows(1, n, n, 1, fields)
    rows = torch.from_numpy(before).cuda()
    launch(args(torch.from_numpy(white).cuda(), rows, work, 1, S, n, n, "bilinear", 1, 8, "uniform"))
    got = rows.cpu().numpy()
    o = 2 + n * n
    assert got[0, o:o + 3].view(np.uint32).tolist() == [15728640, 0xFFFFFF, 15728640]
    assert np.array_equal(got, expected(before, white, fields, 1, n, n, Palette(1, "uniform", "bilinear", 8)))
    assert not work.any()
    noise = pictures(S, 9)["noise"][None]
    before = make_rows(1, n, n, 8, fields)
    rows = torch.from_numpy(before).cuda()
    launch(args(torch.from_numpy(noise).cuda(), rows, work, 1, S, n, n, "bicubic", 8, 2, "map"))
    assert np.array_equal(rows.cpu().numpy(), expected(before, noise, fields, 1, n, n, Palette(8, "map", "bicubic", 2)))
    assert not work.any()


def test_refusals_leave_the_buffer_alone():
    S, n, B, K = 64, 7, 2, 3
    pics = pictures(S, 1)
    imgs = np.stack([pics["noise"], pics["few"]])
    inp = torch.from_numpy(imgs).cuda()
    fs = [heat_fields(n, n, 2)["random"]] * 2
    before = make_rows(B, n, n, K, fs)
    rows = torch.from_numpy(before).cuda()
    work = workspace(B)
    good = args(inp, rows, work, B, S, n, n, "bilinear", K, 8, "map")
    host, _ = device_tables(n, n, S, "bilinear")
    need = 2 + n * n + 1 + 2 * K

    def broken(name, fn):
        t = host[name].copy()
        fn(t)
        return t

    keep = [broken("xb", lambda t: t.__setitem__((S - 1, 1), 3)),            # taps past the map's last column
            broken("xb", lambda t: t.__setitem__((5, 0), -1)),               # a negative first sample
            broken("yb", lambda t: t.__setitem__((40, 0), 0)),               # steps back
            broken("yb", lambda t: t.__setitem__((S - 1, 1), 9))]            # more taps than the table has
    bad = [dict(inp=None), dict(out=None), dict(work=None), dict(xb=None), dict(xk=None), dict(yb=None),
           dict(yk=None), dict(h_xb=None), dict(h_yb=None),
           dict(out=good["out"] + 4), dict(work=good["work"] + 4), dict(xb=good["xb"] + 8), dict(xk=good["xk"] + 4),
           dict(yb=good["yb"] + 8), dict(yk=good["yk"] + 4),
           dict(B=0), dict(B=-1), dict(B=65536), dict(h=0), dict(w=0), dict(h=65, w=64), dict(S=n - 1),
           dict(S=1025), dict(K=0), dict(K=9), dict(K=-1), dict(T=0), dict(T=17), dict(weight=2), dict(weight=-1),
           dict(ldo=need - 1), dict(K=8), dict(xks=0), dict(xks=9), dict(yks=0), dict(yks=9),
           dict(h_xb=keep[0].ctypes.data), dict(h_xb=keep[1].ctypes.data), dict(h_yb=keep[2].ctypes.data),
           dict(h_yb=keep[3].ctypes.data)]
    assert rows.shape[1] < 2 + n * n + 1 + 2 * 8                 # K = 8 does not fit these rows
    for over in bad:
        with pytest.raises(RuntimeError):
            launch(dict(good, **over))
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy(), before), over
        assert not work.any(), over
    # more map rows than a workgroup stages for eight output rows: rows 0..7 of a 21-row map span all of it
    tall = np.zeros((S, 2), np.int32)
    tall[:, 1] = 1
    tall[7:, 0] = 20
    before21 = make_rows(B, 21, n, K, [np.zeros((21, n), np.float32)] * 2)
    rows21 = torch.from_numpy(before21).cuda()
    with pytest.raises(RuntimeError):
        launch(dict(good, out=rows21.data_ptr(), ldo=rows21.shape[1], h=21, h_yb=tall.ctypes.data))
    tall[7:, 0] = 15                                             # sixteen rows: taken (the device tables are the 7-row ones)
    assert np.array_equal(rows21.cpu().numpy(), before21) and not work.any()
    launch(good)                                                     # the same arguments, unbroken, do write
    from kdl.engine.base import Palette
    assert np.array_equal(rows.cpu().numpy(), expected(before, imgs, fs, B, n, n, Palette(K, "map", "bilinear", 8)))


# ------------------------------------------------------------------------------------ engines
def _images(S, seed, n):
    """Half noise, half flat blocks: a picture with a few thousand live bins beside one with a handful."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8)
    blocks = torch.randint(0, 256, (n, 4, 4, 3), generator=g, dtype=torch.uint8)
    blocks = blocks.repeat_interleave((S + 3) // 4, 1).repeat_interleave((S + 3) // 4, 2)[:, :S, :S]
    x[1::2] = blocks[1::2]
    return x


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def check_rows(rows, imgs, hw, spec, base_rows=None):
    """Palette rows: the front against the heatmap engine's, the tail against the rule on the row's own map."""
    from kdl.engine.base import unpack_palette
    h, w = hw
    K = spec.colors
    assert rows.shape == (len(imgs), 2 + h * w + 1 + 2 * K)
    if base_rows is not None:
        assert np.array_equal(_bits(rows[:, :2 + h * w]), _bits(base_rows))   # class, score and map: bit for bit
    _, _, heat, tot, col, wt = unpack_palette(rows, h, w, K)
    for b in range(len(imgs)):
        assert np.array_equal(_bits(rows[b, 2 + h * w:]), words_of(imgs[b], heat[b], spec)), b
    assert (tot > 0).all() and (wt[:, 0] > 0).all() and (wt.sum(axis=1) == tot).all()
    return col


SPECS = {"xception": (3, ("map", "bilinear", 5, 8)), "vit_b16": (2, ("map", "bicubic", 8, 3))}


@pytest.fixture(scope="module")
def runs(xparams):
    """Per family, computed once: a heatmap (explain / rollout) engine's rows, a palette engine's graph and
    eager rows, a second forward of the same captured program on other pictures, and four different batches
    through a stage pipeline on two slots with the joined engine's rows for each."""
    from kdl.engine import registry
    from kdl.engine.base import Palette
    from kdl.engine.stages import StagePipe
    done = {}

    def get(family):
        if family in done:
            return done[family]
        info = registry.get(family)
        nb, (weight, flt, K, T) = SPECS[family]
        spec = Palette(K, weight, flt, T)
        p = xparams if family == "xception" else info.init_params(0)
        mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
        S = info.input_size
        x = _images(S, 5, nb)
        e = info.engine(p, nb, "cuda", **mode)
        r = dict(S=S, hw=tuple(info.map_size), x=x.numpy(), spec=spec, base=e.forward(x.cuda()).cpu().numpy(),
                 base_names=[s.name for s in e.steps])
        del e
        eng = info.engine(p, nb, "cuda", palette=spec, **mode)
        r["steps"] = [(s.kind, s.name, s.src) for s in eng.steps]
        r["graph"] = eng.forward(x.cuda(), capture=True).cpu().numpy()
        r["eager"] = eng.forward(x.cuda(), capture=False).cpu().numpy()
        batches = [_images(S, 20 + i, nb) for i in range(4)]
        r["batches"] = [b.numpy() for b in batches]
        r["joined"] = [eng.forward(b.cuda()).cpu().numpy() for b in batches]   # the captured program, again and again
        r["work_zero"] = not any(bool(w.any()) for w in eng._palette_tabs["work"])
        del eng
        pipe = StagePipe(info.engine(p, nb, "cuda", palette=spec, **mode), info.stage_cut)
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
            pipe.launch_async(nb, [ready], [ev[j]], slot=j)
        for i in (2, 3):
            ev[i % 2].synchronize()
            outs.append(pipe.slot_logits(i % 2).cpu().numpy())
        r["pipe"] = outs
        del pipe
        done[family] = r
        return r
    return get


@pytest.mark.parametrize("family", list(SPECS))
def test_engine_rows(family, runs):
    r = runs(family)
    assert np.array_equal(_bits(r["graph"]), _bits(r["eager"]))
    check_rows(r["graph"], r["x"], r["hw"], r["spec"], r["base"])
    assert [s[1] for s in r["steps"]] == r["base_names"] + ["palette"] and r["steps"][-1] == ("palette", "palette", "input")


@pytest.mark.parametrize("family", list(SPECS))
def test_later_forwards_of_the_captured_program_start_from_an_empty_histogram(family, runs):
    r = runs(family)
    cols = [check_rows(rows, imgs, r["hw"], r["spec"]) for rows, imgs in zip(r["joined"], r["batches"])]
    assert r["work_zero"]
    assert any(not np.array_equal(cols[0], c) for c in cols[1:])     # other pictures, other colours


@pytest.mark.parametrize("family", list(SPECS))
def test_stage_pipeline_colours_are_each_batch_s_own(family, runs):
    r = runs(family)
    assert len(r["ranges"]) >= 2 and r["ranges"][-1][1] == len(r["steps"])    # the palette step: the last stage
    for i, (got, want) in enumerate(zip(r["pipe"], r["joined"])):
        assert np.array_equal(_bits(got), _bits(want)), f"batch {i}"
    for got, imgs in zip(r["pipe"], r["batches"]):
        check_rows(got, imgs, r["hw"], r["spec"])


def test_palette_needs_a_heatmap_no_overlay_and_a_uint8_input(xparams):
    from kdl.engine.base import Overlay, Palette
    from kdl.engine.vit import ViTEngine
    from kdl.engine.xception import XceptionEngine
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        XceptionEngine(xparams, max_batch=2, device="cuda", palette=Palette())
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        ViTEngine({}, max_batch=2, device="cuda", palette=Palette())
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        XceptionEngine(xparams, max_batch=2, device="cuda", topk=3, palette=Palette())
    with pytest.raises(ValueError, match="overlay"):
        XceptionEngine(xparams, max_batch=2, device="cuda", explain=True, overlay=Overlay(), palette=Palette())
    with pytest.raises(ValueError, match="uint8"):
        XceptionEngine(xparams, max_batch=2, device="cuda", in_kind="f32", explain=True, palette=Palette())
    for bad in (Palette(colors=0), Palette(colors=9), Palette(rounds=0), Palette(rounds=17), Palette(weight="heat"),
                Palette(filter="lanczos")):
        with pytest.raises(ValueError):
            XceptionEngine(xparams, max_batch=2, device="cuda", explain=True, palette=bad)


# ------------------------------------------------------------------------------------ server
def test_server_palette_bytes(tmp_path):
    """One palette_bytes request of two JPEGs over gRPC: the colours are the rule applied to the served
    preprocess result (decode + nearest resize) and the map explain_bytes answers for the same files; class
    and score are explain_bytes' too."""
    import io
    from pathlib import Path

    import grpc
    from PIL import Image

    from kdl.engine.base import Palette
    from kdl.gateway import preprocess as pp
    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving import palette as PL
    from kdl.serving.config import BatchingParams, ServerConfig
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
    (base / "1" / "synthetic.json").write_text('{"seed": 0, "palette": {"colors": 4, "rounds": 6}}')
    spec = Palette(colors=4, rounds=6)
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                       file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000, allowed_batch_sizes=[2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            out = stub.Predict(make_request(files, signature="palette_bytes", input_key="image_bytes"), timeout=120).outputs
            exp = stub.Predict(make_request(files, signature="explain_bytes", input_key="image_bytes"), timeout=120).outputs
        assert sorted(out) == ["classes", "colors", "fractions", "names", "scores"]
        assert [d.size for d in out["colors"].tensor_shape.dim] == [2, 4, 3]
        assert [d.size for d in out["fractions"].tensor_shape.dim] == [2, 4]
        heat = np.asarray(exp["heatmap"].float_val, np.float32).reshape(2, 10, 10)
        cols = np.frombuffer(out["colors"].tensor_content, np.uint8).reshape(2, 4, 3)
        frac = np.asarray(out["fractions"].float_val, np.float32).reshape(2, 4)
        names = np.asarray([v.decode() for v in out["names"].string_val]).reshape(2, 4).tolist()
        assert list(out["classes"].string_val) == list(exp["classes"].string_val)
        assert np.array_equal(_bits(np.asarray(out["scores"].float_val, np.float32)),
                              _bits(np.asarray(exp["scores"].float_val, np.float32)))
        for b in range(2):
            W, col, n = PL.palette_rule(u8[b], heat[b], spec)
            assert W > 0 and np.array_equal(cols[b], col), b
            assert np.array_equal(frac[b], PL.fractions_of(n, W)) and names[b] == PL.names_of(col), b
        s = srv.manager.get("clothing-model", None, None)
        r = s.runner("palette")
        assert r.out_cols == 102 + 1 + 8 and r.executors
        assert all(ex.engine.explain and ex.engine.palette == spec for ex in r.executors)
        assert s.device_alive()
    finally:
        srv.stop(0)
