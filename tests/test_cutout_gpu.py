"""cutout (kernels/cutout.hip) alone, inside the Xception and ViT engines, through the stage pipeline and
behind the server.

The rule is integer arithmetic, so every comparison is for equality of bits against ``cutout_rule``
(kdl/serving/cutout.py) applied to the row's own map and the input; tests/test_cutout_cpu.py checks that
rule against literal answers and a second implementation in plain loops.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5      # a NaN pattern, as int32
FILTER_ID = {"bilinear": 1, "bicubic": 3}

# (S, h, w, B): one pixel; a small non-square map; a small odd size; a mask row that crosses one 32-bit word;
# exactly two mask words; a band exactly full, then one row and one column more; several workgroups per image
# with a ragged last one. 1024, at the uint32 bound, has a test of its own
SHAPES = [(1, 1, 1, 1), (5, 2, 3, 2), (17, 3, 2, 3), (33, 3, 3, 2), (64, 7, 7, 2), (65, 7, 7, 2), (299, 10, 10, 2)]
TABLE_BYTES = 3 * 4096 * 4


# ------------------------------------------------------------------------------------ inputs
def pictures(S, seed):
    """tests/test_palette_gpu.py's pictures. name -> uint8 [S, S, 3]: noise, flat, the two-tone tie, two colours,
    colours that crowd a few bins, a smooth ramp."""
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
    """tests/test_palette_gpu.py's heat fields. name -> fp32 [h, w]: random, random with NaN and out-of-range
    entries, all zeros, all NaN, all ones."""
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


def workspace(B, S):
    from kdl.ops import _lib
    return torch.zeros(_lib.lib().cutout_workspace(B, S), dtype=torch.uint8, device="cuda")


def tables_zero(work, B, S):
    """The three colour tables of every image (the front of its part of the workspace) are all zero."""
    from kdl.ops import _lib
    stride = _lib.lib().cutout_workspace(1, S)
    assert stride % 16 == 0 and work.numel() == B * stride
    return not bool(work.view(B, stride)[:, :TABLE_BYTES].any())


def make_rows(B, h, w, S, fields, extra_rows=1, ldo=None):
    """int32 host buffer [B + extra_rows, ldo], the canary everywhere, then class, score and the heat field of
    every image < B in front. ldo defaults to five words above the need, so the rows start at every residue
    mod 16 bytes."""
    need = 2 + h * w + 1 + S * S
    ldo = need + 5 if ldo is None else ldo
    buf = np.full((B + extra_rows, ldo), CANARY, np.int32)
    for b in range(B):
        buf[b, 0] = 7 + b
        buf[b, 1:2] = np.float32(0.25 + b).view(np.int32)
        buf[b, 2:2 + h * w] = np.ascontiguousarray(fields[b], np.float32).reshape(-1).view(np.int32)
    return buf


def args(inp, rows, work, B, S, h, w, spec):
    host, dev = device_tables(h, w, S, spec.filter)
    return dict(inp=inp.data_ptr(), out=rows.data_ptr(), work=work.data_ptr(),
                xb=dev["xb"].data_ptr(), xk=dev["xk"].data_ptr(), yb=dev["yb"].data_ptr(), yk=dev["yk"].data_ptr(),
                h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=B, S=S, h=h, w=w, ldo=rows.shape[1],
                xks=host["xk"].shape[1], yks=host["yk"].shape[1], gate=spec.gate, rounds=spec.rounds,
                smooth=spec.smooth, feather=int(spec.feather))


def launch(d):
    from kdl.ops import _lib
    _lib.lib().cutout(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def words_of(img, heat, spec):
    """The 1 + S*S words the rule gives, as int32 bits."""
    from kdl.serving.cutout import cutout_rule
    count, rgba = cutout_rule(img, heat, spec)
    out = np.empty(1 + rgba.shape[0] * rgba.shape[1], np.uint32)
    out[0] = count
    out[1:] = np.ascontiguousarray(rgba).view(np.uint32).reshape(-1)
    return out.view(np.int32)


def expected(before, imgs, fields, B, h, w, spec):
    want = before.copy()
    o, S = 2 + h * w, imgs.shape[1]
    for b in range(B):
        want[b, o:o + 1 + S * S] = words_of(imgs[b], fields[b], spec)
    return want


# ------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("S,h,w,B", SHAPES)
def test_kernels_are_bit_exact_and_write_nothing_else(S, h, w, B):
    """rounds in {0, 2, 8} x smooth in {0, 1, 4} x feather x both filters x gate in {1, 26, 255}, the pictures
    and heat fields rotating through the batch. The WHOLE buffer is compared: the row fronts, the words behind
    the answer and the row behind the batch keep what they had; the colour tables are all zero again; a
    second launch into a fresh buffer gives the same bits."""
    from kdl.engine.base import Cutout
    pics, fields = pictures(S, seed=S), heat_fields(h, w, seed=S * 31 + h)
    pn, fn = list(pics), list(fields)
    work = workspace(B, S)
    cases = 0
    for i, (R, M, fe, flt, gate) in enumerate(itertools.product((0, 2, 8), (0, 1, 4), (False, True), FILTER_ID,
                                                                (1, 26, 255))):
        spec = Cutout(gate, R, M, fe, flt)
        imgs = np.stack([pics[pn[(i + b) % len(pn)]] for b in range(B)])
        fs = [fields[fn[(i // 2 + b) % len(fn)]] for b in range(B)]
        inp = torch.from_numpy(imgs).cuda()
        before = make_rows(B, h, w, S, fs)
        rows = torch.from_numpy(before).cuda()
        d = args(inp, rows, work, B, S, h, w, spec)
        launch(d)
        got, want = rows.cpu().numpy(), expected(before, imgs, fs, B, h, w, spec)
        assert np.array_equal(got, want), (spec, [pn[(i + b) % len(pn)] for b in range(B)],
                                           [fn[(i // 2 + b) % len(fn)] for b in range(B)],
                                           np.argwhere(got != want)[:4].tolist())
        assert tables_zero(work, B, S), spec
        if i % 12 == 0:
            again = torch.from_numpy(before).cuda()
            launch(dict(d, out=again.data_ptr()))
            assert np.array_equal(again.cpu().numpy(), got)
        cases += 1
    assert cases == 108


def test_every_picture_with_every_heat_field():
    """33 pixels a side, every picture against every heat field at the minimal row length, the default spec
    and one with no smoothing (an all-zero and an all-NaN map, a flat picture under an all-ones map and the
    two-tone picture among them)."""
    from kdl.engine.base import Cutout
    S, h, w = 33, 3, 2
    pics, fields = pictures(S, seed=3), heat_fields(h, w, seed=4)
    combos = list(itertools.product(pics, fields))
    B = len(combos)
    imgs = np.stack([pics[p] for p, _ in combos])
    fs = [fields[f] for _, f in combos]
    inp, work = torch.from_numpy(imgs).cuda(), workspace(B, S)
    o = 2 + h * w
    for spec in (Cutout(), Cutout(smooth=0, feather=False)):
        before = make_rows(B, h, w, S, fs, ldo=o + 1 + S * S)
        rows = torch.from_numpy(before).cuda()
        launch(args(inp, rows, work, B, S, h, w, spec))
        got, want = rows.cpu().numpy(), expected(before, imgs, fs, B, h, w, spec)
        assert np.array_equal(got, want), (spec, [combos[b] for b in np.unique(np.argwhere(got != want)[:, 0])][:6])
        assert tables_zero(work, B, S)
        zero = [b for b, (_, f) in enumerate(combos) if f in ("zeros", "nan")]
        assert zero and not got[zero, o].any() and not (got[zero, o + 1:].view(np.uint32) >> 24).any()
        full = got[combos.index(("flat", "ones")), o]                # one colour, TB = 0: the mask is the gate
        assert full == (S * S - 4 if spec.smooth else S * S)


def test_the_uint32_bound_and_the_largest_products():
    """1024 x 1024 all white under an all-ones map: N, G and F of one bin are 2^20, 2^20 and 255 * 2^20, the
    largest sums the rule allows, and TF = 255 S^2; then noise under a 19 x 19 map."""
    from kdl.engine.base import Cutout
    S, n = 1024, 19
    work = workspace(1, S)
    white = np.full((1, S, S, 3), 255, np.uint8)
    ones = [np.ones((n, n), np.float32)]
    before = make_rows(1, n, n, S, ones)
    rows = torch.from_numpy(before).cuda()
    launch(args(torch.from_numpy(white).cuda(), rows, work, 1, S, n, n, Cutout(feather=False)))
    got = rows.cpu().numpy()
    o = 2 + n * n
    assert got[0, o] == S * S - 4
    px = got[0, o + 1:o + 1 + S * S].view(np.uint32).reshape(S, S)
    assert px[0, 0] == 0x00FFFFFF and px[0, 1] == 0xFFFFFFFF and px[S - 1, S - 1] == 0x00FFFFFF
    assert int((px == 0xFFFFFFFF).sum()) == S * S - 4
    assert np.array_equal(got, expected(before, white, ones, 1, n, n, Cutout(feather=False)))
    assert tables_zero(work, 1, S)
    noise = pictures(S, 9)["noise"][None]
    fields = [heat_fields(n, n, 8)["random"]]
    spec = Cutout(26, 8, 4, True, "bicubic")
    before = make_rows(1, n, n, S, fields)
    rows = torch.from_numpy(before).cuda()
    launch(args(torch.from_numpy(noise).cuda(), rows, work, 1, S, n, n, spec))
    assert np.array_equal(rows.cpu().numpy(), expected(before, noise, fields, 1, n, n, spec))
    assert tables_zero(work, 1, S)


def test_refusals_leave_the_buffer_alone():
    from kdl.engine.base import Cutout
    S, n, B = 64, 7, 2
    pics = pictures(S, 1)
    imgs = np.stack([pics["noise"], pics["few"]])
    inp = torch.from_numpy(imgs).cuda()
    fs = [heat_fields(n, n, 2)["random"]] * 2
    before = make_rows(B, n, n, S, fs)
    rows = torch.from_numpy(before).cuda()
    work = workspace(B, S)
    spec = Cutout()
    good = args(inp, rows, work, B, S, n, n, spec)
    host, _ = device_tables(n, n, S, "bilinear")
    need = 2 + n * n + 1 + S * S

    def broken(name, fn):
        t = host[name].copy()
        fn(t)
        return t

    keep = [broken("xb", lambda t: t.__setitem__((S - 1, 1), 3)),            # taps past the map's last column
            broken("xb", lambda t: t.__setitem__((5, 0), -1)),               # a negative first sample
            broken("yb", lambda t: t.__setitem__((40, 0), 0)),               # steps back
            broken("yb", lambda t: t.__setitem__((S - 1, 1), 9))]            # more taps than the table has
    bad = [dict(S=1025), dict(S=n - 1), dict(h=65, w=64), dict(ldo=need - 1), dict(out=good["out"] + 4),
           dict(out=good["out"] + 8), dict(work=good["work"] + 4),
           dict(inp=None), dict(out=None), dict(work=None), dict(xb=None), dict(xk=None), dict(yb=None),
           dict(yk=None), dict(h_xb=None), dict(h_yb=None),
           dict(xb=good["xb"] + 8), dict(xk=good["xk"] + 4), dict(yb=good["yb"] + 8), dict(yk=good["yk"] + 4),
           dict(B=0), dict(B=-1), dict(B=65536), dict(h=0), dict(w=0),
           dict(gate=0), dict(gate=256), dict(rounds=-1), dict(rounds=9), dict(smooth=-1), dict(smooth=5),
           dict(feather=2), dict(feather=-1), dict(S=S + 1), dict(xks=0), dict(xks=9), dict(yks=0), dict(yks=9),
           dict(h_xb=keep[0].ctypes.data), dict(h_xb=keep[1].ctypes.data), dict(h_yb=keep[2].ctypes.data),
           dict(h_yb=keep[3].ctypes.data)]
    assert rows.shape[1] < 2 + n * n + 1 + (S + 1) ** 2            # S + 1 does not fit these rows
    for over in bad:
        with pytest.raises(RuntimeError):
            launch(dict(good, **over))
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy(), before), over
        assert not work.any(), over
    launch(good)                                                     # the same arguments, unbroken, do write
    assert np.array_equal(rows.cpu().numpy(), expected(before, imgs, fs, B, n, n, spec))


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
    """Cutout rows: the front against the heatmap engine's, the tail against the rule on the row's own map."""
    from kdl.engine.base import unpack_cutout
    h, w = hw
    S = imgs.shape[1]
    assert rows.shape == (len(imgs), 2 + h * w + 1 + S * S)
    if base_rows is not None:
        assert np.array_equal(_bits(rows[:, :2 + h * w]), _bits(base_rows))   # class, score and map: bit for bit
    _, _, heat, counts, pics = unpack_cutout(rows, h, w, S)
    for b in range(len(imgs)):
        assert np.array_equal(_bits(rows[b, 2 + h * w:]), words_of(imgs[b], heat[b], spec)), b
    assert np.array_equal(pics[..., :3], imgs)
    return pics[..., 3]


SPECS = {"xception": (3, (26, 2, 1, True, "bilinear")), "vit_b16": (2, (40, 8, 4, False, "bicubic"))}


@pytest.fixture(scope="module")
def runs(xparams):
    """Per family, computed once: a heatmap (explain / rollout) engine's rows, a cutout engine's graph and
    eager rows, later forwards of the same captured program on other pictures, and four different batches
    through a stage pipeline on two slots with the joined engine's rows for each."""
    from kdl.engine import registry
    from kdl.engine.base import Cutout
    from kdl.engine.stages import StagePipe
    done = {}

    def get(family):
        if family in done:
            return done[family]
        info = registry.get(family)
        nb, fields = SPECS[family]
        spec = Cutout(*fields)
        p = xparams if family == "xception" else info.init_params(0)
        mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
        S = info.input_size
        x = _images(S, 5, nb)
        e = info.engine(p, nb, "cuda", **mode)
        r = dict(S=S, hw=tuple(info.map_size), x=x.numpy(), spec=spec, base=e.forward(x.cuda()).cpu().numpy(),
                 base_names=[s.name for s in e.steps])
        del e
        eng = info.engine(p, nb, "cuda", cutout=spec, **mode)
        r["steps"] = [(s.kind, s.name, s.src) for s in eng.steps]
        r["graph"] = eng.forward(x.cuda(), capture=True).cpu().numpy()
        r["eager"] = eng.forward(x.cuda(), capture=False).cpu().numpy()
        batches = [_images(S, 20 + i, nb) for i in range(4)]
        r["batches"] = [b.numpy() for b in batches]
        r["joined"] = [eng.forward(b.cuda()).cpu().numpy() for b in batches]   # the captured program, again and again
        r["work_zero"] = all(tables_zero(w, nb, S) for w in eng._cutout_tabs["work"])
        del eng
        pipe = StagePipe(info.engine(p, nb, "cuda", cutout=spec, **mode), info.stage_cut)
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
    assert [s[1] for s in r["steps"]] == r["base_names"] + ["cutout"] and r["steps"][-1] == ("cutout", "cutout", "input")


@pytest.mark.parametrize("family", list(SPECS))
def test_later_forwards_of_the_captured_program_start_from_empty_tables_and_a_zero_count(family, runs):
    r = runs(family)
    alphas = [check_rows(rows, imgs, r["hw"], r["spec"]) for rows, imgs in zip(r["joined"], r["batches"])]
    assert r["work_zero"]
    assert any(not np.array_equal(alphas[0], a) for a in alphas[1:])     # other pictures, other masks


@pytest.mark.parametrize("family", list(SPECS))
def test_stage_pipeline_cutouts_are_each_batch_s_own(family, runs):
    r = runs(family)
    assert len(r["ranges"]) >= 2 and r["ranges"][-1][1] == len(r["steps"])    # the cutout step: the last stage
    for i, (got, want) in enumerate(zip(r["pipe"], r["joined"])):
        assert np.array_equal(_bits(got), _bits(want)), f"batch {i}"
    for got, imgs in zip(r["pipe"], r["batches"]):
        check_rows(got, imgs, r["hw"], r["spec"])


def test_cutout_needs_a_heatmap_no_other_row_extension_and_a_uint8_input(xparams):
    from kdl.engine.base import Cutout, Locate, Overlay, Palette
    from kdl.engine.vit import ViTEngine
    from kdl.engine.xception import XceptionEngine
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        XceptionEngine(xparams, max_batch=2, device="cuda", cutout=Cutout())
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        ViTEngine({}, max_batch=2, device="cuda", cutout=Cutout())
    with pytest.raises(ValueError, match="explain=True or rollout=True"):
        XceptionEngine(xparams, max_batch=2, device="cuda", topk=3, cutout=Cutout())
    for other in (dict(overlay=Overlay()), dict(palette=Palette()), dict(locate=Locate())):
        with pytest.raises(ValueError, match="set one of them"):
            XceptionEngine(xparams, max_batch=2, device="cuda", explain=True, cutout=Cutout(), **other)
    with pytest.raises(ValueError, match="uint8"):
        XceptionEngine(xparams, max_batch=2, device="cuda", in_kind="f32", explain=True, cutout=Cutout())
    for bad in (Cutout(gate=0), Cutout(gate=256), Cutout(rounds=-1), Cutout(rounds=9), Cutout(smooth=5),
                Cutout(feather=2), Cutout(filter="lanczos")):
        with pytest.raises(ValueError):
            XceptionEngine(xparams, max_batch=2, device="cuda", explain=True, cutout=bad)


# ------------------------------------------------------------------------------------ server
def test_server_cutout_bytes(tmp_path):
    """One cutout_bytes request of two JPEGs over gRPC: the pictures are the rule applied to the served
    preprocess result (decode + nearest resize) and the map explain_bytes answers for the same files; class
    and score are explain_bytes' too."""
    import io
    from pathlib import Path

    import grpc
    from PIL import Image

    from kdl.engine.base import Cutout
    from kdl.gateway import preprocess as pp
    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving import cutout as CU
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
    (base / "1" / "synthetic.json").write_text('{"seed": 0, "cutout": {"gate": 40, "rounds": 3, "smooth": 2}}')
    spec = Cutout(gate=40, rounds=3, smooth=2)
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                       file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000, allowed_batch_sizes=[2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            out = stub.Predict(make_request(files, signature="cutout_bytes", input_key="image_bytes"), timeout=120).outputs
            exp = stub.Predict(make_request(files, signature="explain_bytes", input_key="image_bytes"), timeout=120).outputs
        assert sorted(out) == ["classes", "coverage", "cutout", "scores"]
        assert [d.size for d in out["cutout"].tensor_shape.dim] == [2, 299, 299, 4]
        assert [d.size for d in out["coverage"].tensor_shape.dim] == [2, 1]
        heat = np.asarray(exp["heatmap"].float_val, np.float32).reshape(2, 10, 10)
        pics = np.frombuffer(out["cutout"].tensor_content, np.uint8).reshape(2, 299, 299, 4)
        cov = np.asarray(out["coverage"].float_val, np.float32)
        assert list(out["classes"].string_val) == list(exp["classes"].string_val)
        assert np.array_equal(_bits(np.asarray(out["scores"].float_val, np.float32)),
                              _bits(np.asarray(exp["scores"].float_val, np.float32)))
        for b in range(2):
            count, rgba = CU.cutout_rule(u8[b], heat[b], spec)
            assert np.array_equal(pics[b], rgba), b
            assert cov[b] == CU.coverage_of([count], 299)[0], b
        s = srv.manager.get("clothing-model", None, None)
        r = s.runner("cutout")
        assert r.out_cols == 102 + 1 + 299 * 299 and r.executors
        assert all(ex.engine.explain and ex.engine.cutout == spec for ex in r.executors)
        assert s.device_alive()
    finally:
        srv.stop(0)
