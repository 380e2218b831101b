"""locate (kernels/locate.hip) alone, inside the Xception and ViT engines, through the stage pipeline and
behind the server.

The rule is integer arithmetic, so every comparison is for equality of bits against ``locate_rule``
(kdl/serving/locate.py) applied to the row's own map; tests/test_locate_cpu.py checks that rule against
literal answers and a second implementation.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5      # a NaN pattern, as int32
FILTER_ID = {"bilinear": 1, "bicubic": 3}
# kLocateLdsRuns (kernels/launch.h): an image with more runs keeps its run tables in the workspace, not in LDS
LDS_RUNS = 1920
# (S, h, w, B): one pixel; smaller than any word; h != w and an odd S; one pixel past a 32-bit word; exactly
# one 64-bit ballot word per row; one past it and past eight bands of rows; the served shape;
# EfficientNet-B7's. 1024 has a test of its own
SHAPES = [(1, 1, 1, 1), (5, 2, 3, 2), (17, 3, 2, 3), (33, 33, 33, 2), (64, 64, 64, 2), (65, 13, 13, 2),
          (299, 10, 10, 2), (600, 19, 19, 1)]


# ------------------------------------------------------------------------------------ inputs
def heat_fields(h, w, seed):
    """name -> fp32 [h, w]: random, random with NaN and out-of-range entries, a smooth peak, all zeros, all
    NaN, all ones."""
    rng = np.random.default_rng(seed)
    odd = rng.random((h, w), dtype=np.float32) * 3 - 1
    odd.reshape(-1)[::3] = np.nan
    odd.reshape(-1)[1::7] = np.inf
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    peak = np.exp(-((yy - 0.4 * h) ** 2 + (xx - 0.6 * w) ** 2) / np.float32(max(h * w / 8, 1))).astype(np.float32)
    return {"random": rng.random((h, w), dtype=np.float32), "odd": odd, "peak": peak,
            "zeros": np.zeros((h, w), np.float32), "nan": np.full((h, w), np.nan, np.float32),
            "ones": np.ones((h, w), np.float32)}


def spiral(n):
    """A one-pixel-wide square spiral with a one-pixel gap between its arms: one component."""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = 0
        while True:
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx                              # the cell behind the next one must be free too
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx]:
                break
            if 0 <= ay < n and 0 <= ax < n and m[ay, ax]:
                break
            y, x = ny, nx
            m[y, x] = True
            moved += 1
        if not moved:
            return m
        dy, dx = dx, -dy


def masks(n, seed=0):
    """name -> bool [n, n]: the mask families at S = h = w, where both resample passes are the identity, so
    a map of 0.0 / 1.0 values IS the mask."""
    rng = np.random.default_rng(seed)
    yy, xx = np.indices((n, n))
    comb = np.zeros((n, n), bool)
    comb[:, ::2] = True
    comb[-1] = True                                              # teeth two columns apart, joined by the last row only
    blobs = np.zeros((n, n), bool)
    blobs[2:6, n - 7:n - 2] = True
    blobs[n - 8:n - 4, 1:6] = True
    ring = np.zeros((n, n), bool)
    ring[3:n - 3, 3:n - 3] = True
    ring[6:n - 6, 6:n - 6] = False
    return {"checkerboard": (yy + xx) % 2 == 0, "dots": (yy % 2 == 0) & (xx % 2 == 0),
            "diagonals": (yy == xx) | (yy + xx == n - 1), "spiral": spiral(n), "comb": comb, "comb_up": comb[::-1].copy(),
            "blobs": blobs, "ring": ring, "ones": np.ones((n, n), bool), "zeros": np.zeros((n, n), bool),
            "noise": rng.random((n, n)) < 0.45}


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
    return torch.zeros(_lib.lib().locate_workspace(B, S), dtype=torch.uint8, device="cuda")


def make_rows(B, h, w, K, fields, extra_rows=1, ldo=None):
    """int32 host buffer [B + extra_rows, ldo], the canary everywhere, then class, score and the heat field
    of every image < B in front. ldo defaults to five words above the need."""
    need = 2 + h * w + 1 + 3 * K
    ldo = need + 5 if ldo is None else ldo
    buf = np.full((B + extra_rows, ldo), CANARY, np.int32)
    for b in range(B):
        buf[b, 0] = 7 + b
        buf[b, 1:2] = np.float32(0.25 + b).view(np.int32)
        buf[b, 2:2 + h * w] = np.ascontiguousarray(fields[b], np.float32).reshape(-1).view(np.int32)
    return buf


def args(rows, work, B, S, h, w, flt, K, threshold):
    host, dev = device_tables(h, w, S, flt)
    return dict(out=rows.data_ptr(), work=work.data_ptr(),
                xb=dev["xb"].data_ptr(), xk=dev["xk"].data_ptr(), yb=dev["yb"].data_ptr(), yk=dev["yk"].data_ptr(),
                h_xb=host["xb"].ctypes.data, h_yb=host["yb"].ctypes.data, B=B, S=S, h=h, w=w, ldo=rows.shape[1],
                xks=host["xk"].shape[1], yks=host["yk"].shape[1], K=K, threshold=threshold)


def launch(d):
    from kdl.ops import _lib
    _lib.lib().locate(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


_RULE_CACHE = {}


def words_of(heat, S, spec):
    """The 1 + 3K words the rule gives, as int32 bits (computed once per map and spec)."""
    from kdl.serving.locate import locate_rule
    key = (np.ascontiguousarray(heat, np.float32).tobytes(), heat.shape, S, spec)
    if key not in _RULE_CACHE:
        count, box, area = locate_rule(heat, S, spec)
        bx = box.astype(np.uint32)
        out = np.empty(1 + 3 * spec.boxes, np.uint32)
        out[0] = count
        out[1::3] = bx[:, 0] | (bx[:, 1] << 16)
        out[2::3] = bx[:, 2] | (bx[:, 3] << 16)
        out[3::3] = area
        _RULE_CACHE[key] = out.view(np.int32)
    return _RULE_CACHE[key]


def expected(before, fields, B, S, h, w, spec):
    want = before.copy()
    o = 2 + h * w
    for b in range(B):
        want[b, o:o + 1 + 3 * spec.boxes] = words_of(fields[b], S, spec)
    return want


def run_exact(fields, S, h, w, spec, work=None, ldo=None):
    """One launch on a canary buffer; the WHOLE buffer equals the rule's. -> the buffer."""
    B = len(fields)
    work = workspace(B, S) if work is None else work
    before = make_rows(B, h, w, spec.boxes, fields, ldo=ldo)
    rows = torch.from_numpy(before).cuda()
    launch(args(rows, work, B, S, h, w, spec.filter, spec.boxes, spec.threshold))
    got, want = rows.cpu().numpy(), expected(before, fields, B, S, h, w, spec)
    assert np.array_equal(got, want), (spec, S, h, w, np.argwhere(got != want)[:6].tolist(),
                                       got[got != want][:6].tolist(), want[got != want][:6].tolist())
    return got


def run_count(mask):
    from kdl.serving.locate import runs_of
    return len(runs_of(mask)[0])


# ------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("S,h,w,B", SHAPES)
def test_kernels_are_bit_exact_and_write_nothing_else(S, h, w, B):
    """K in {1, 3, 8} x threshold in {1, 51, 255} x both filters, the heat fields rotating through the batch.
    The WHOLE buffer is compared: the row fronts, the words behind the answer and the row behind the
    batch keep what they had. One workspace serves all eighteen launches."""
    from kdl.engine.base import Locate
    fields = heat_fields(h, w, seed=S * 31 + h)
    fn = list(fields)
    work = workspace(B, S)
    cases = 0
    for i, (K, thr, flt) in enumerate(itertools.product((1, 3, 8), (1, 51, 255), FILTER_ID)):
        fs = [fields[fn[(i + b) % len(fn)]] for b in range(B)]
        run_exact(fs, S, h, w, Locate(K, thr, flt), work)
        cases += 1
    assert cases == 18


@pytest.mark.parametrize("n", [33, 64])
def test_arbitrary_masks(n):
    """At S = h = w the map of 0.0 / 1.0 values is the mask: every family in one batch, K = 1, 3 and 8, at
    the minimal row length."""
    from kdl.engine.base import Locate
    from kdl.serving.locate import mask_of
    ms = masks(n)
    fields = [m.astype(np.float32) for m in ms.values()] + [np.full((n, n), np.nan, np.float32)]
    for m, f in zip(ms.values(), fields):
        assert np.array_equal(mask_of(f, n, Locate()), m)            # both passes are the identity
    work = workspace(len(fields), n)
    for K, thr, flt in ((1, 51, "bilinear"), (3, 255, "bicubic"), (8, 1, "bilinear")):
        got = run_exact(fields, n, n, n, Locate(K, thr, flt), work, ldo=2 + n * n + 1 + 3 * K)
    o = 2 + n * n
    names = list(ms)
    tail = got[:, o:].view(np.uint32)                                # K = 8
    assert tail[names.index("checkerboard"), [0, 3]].tolist() == [1, (n * n + 1) // 2]
    assert tail[names.index("dots"), 0] == ((n + 1) // 2) ** 2 and (tail[names.index("dots"), 3::3] == 1).all()
    assert tail[names.index("dots"), 1:3].tolist() == [0, 1 | 1 << 16]
    assert tail[names.index("dots"), 4:6].tolist() == [2 << 16, 1 | 3 << 16]      # the tie: raster order
    for one in ("diagonals", "spiral", "comb", "comb_up", "ring", "ones"):
        assert tail[names.index(one), 0] == 1, one
    assert tail[names.index("spiral"), 3] == ms["spiral"].sum() > 4 * n
    assert tail[names.index("blobs"), [0, 3, 6]].tolist() == [2, 20, 20]
    assert tail[names.index("blobs"), 1] == 2 | (n - 7) << 16        # equal areas: the earlier first pixel
    assert not tail[names.index("zeros")].any() and not tail[len(fields) - 1].any()   # the all-NaN map: the last image


def test_replays_need_nothing_from_the_host():
    """One workspace from torch.zeros, three launches in a row with different inputs and no host write
    between them: the checkerboard, a single dot, noise. Each is exact; the first input again, into a
    fresh buffer, gives the same bits."""
    from kdl.engine.base import Locate
    n, spec = 64, Locate(8, 51, "bilinear")
    ms = masks(n, seed=3)
    dot = np.zeros((n, n), np.float32)
    dot[40, 23] = 1
    work = workspace(2, n)
    first = run_exact([ms["checkerboard"].astype(np.float32)] * 2, n, n, n, spec, work)
    run_exact([dot, dot], n, n, n, spec, work)
    run_exact([ms["noise"].astype(np.float32), dot], n, n, n, spec, work)
    again = run_exact([ms["checkerboard"].astype(np.float32)] * 2, n, n, n, spec, work)
    assert np.array_equal(first, again)


def test_run_tables_in_lds_and_in_the_workspace():
    """The path switch at kLocateLdsRuns runs: a 64 x 64 checkerboard of 60 rows has exactly LDS_RUNS runs
    (the tables in LDS), one more dot makes LDS_RUNS + 1 (the tables in the workspace); and a 64 x 64
    checkerboard upsampled with bicubic to 299, thousands of runs."""
    from kdl.engine.base import Locate
    from kdl.ops import _lib
    from kdl.serving.locate import mask_of
    assert _lib.lib().LOCATE_LDS_RUNS == LDS_RUNS
    n = 64
    yy, xx = np.indices((n, n))
    under = ((yy + xx) % 2 == 0) & (yy < 60)
    over = under.copy()
    over[62, 5] = True
    assert run_count(under) == LDS_RUNS and run_count(over) == LDS_RUNS + 1
    spec = Locate(3, 51, "bilinear")
    work = workspace(2, n)
    got = run_exact([under.astype(np.float32), over.astype(np.float32)], n, n, n, spec, work)
    tail = got[:2, 2 + n * n:].view(np.uint32)
    assert tail[0, [0, 3]].tolist() == [1, LDS_RUNS] and tail[1, [0, 3, 6]].tolist() == [2, LDS_RUNS, 1]
    got = run_exact([over.astype(np.float32), under.astype(np.float32)], n, n, n, spec, work)   # swapped: the same workspace
    board = ((yy + xx) % 2 == 0).astype(np.float32)
    spec = Locate(8, 128, "bicubic")
    assert run_count(mask_of(board, 299, spec)) > 2 * LDS_RUNS
    run_exact([board, over.astype(np.float32)[:, ::-1].copy()], 299, n, n, spec)


def test_1024_pixels_a_side():
    from kdl.engine.base import Locate
    from kdl.serving.locate import mask_of
    n, S = 64, 1024
    noise = (np.random.default_rng(11).random((n, n)) < 0.45).astype(np.float32)
    spec = Locate(8, 128, "bilinear")
    assert run_count(mask_of(noise, S, spec)) > LDS_RUNS
    got = run_exact([noise], S, n, n, spec)
    assert got[0, 2 + n * n] > 8                                     # more regions than K


def test_refusals_leave_the_buffer_alone():
    S, n, B, K = 64, 7, 2, 3
    fs = [heat_fields(n, n, 2)["random"]] * 2
    before = make_rows(B, n, n, K, fs)
    rows = torch.from_numpy(before).cuda()
    work = workspace(B, S)
    good = args(rows, work, B, S, n, n, "bilinear", K, 51)
    host, _ = device_tables(n, n, S, "bilinear")
    need = 2 + n * n + 1 + 3 * K
    back = host["yb"].copy()
    back[40, 0] = 0                                                  # steps back
    past = host["xb"].copy()
    past[S - 1, 1] = 3                                               # taps past the map's last column
    bad = [dict(out=None), dict(work=None), dict(xb=None), dict(xk=None), dict(yb=None), dict(yk=None),
           dict(h_xb=None), dict(h_yb=None),
           dict(out=good["out"] + 4), dict(work=good["work"] + 4), dict(xb=good["xb"] + 8), dict(xk=good["xk"] + 4),
           dict(yb=good["yb"] + 8), dict(yk=good["yk"] + 4),
           dict(B=0), dict(B=65536), dict(h=0), dict(w=0), dict(h=65, w=64), dict(S=n - 1), dict(S=1025),
           dict(K=0), dict(K=9), dict(threshold=0), dict(threshold=256), dict(ldo=need - 1), dict(K=8),
           dict(xks=0), dict(xks=9), dict(yks=0), dict(yks=9),
           dict(h_xb=past.ctypes.data), dict(h_yb=back.ctypes.data)]
    assert rows.shape[1] < 2 + n * n + 1 + 3 * 8                 # K = 8 does not fit these rows
    for over in bad:
        with pytest.raises(RuntimeError):
            launch(dict(good, **over))
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy(), before), over
    launch(good)                                                     # the same arguments, unbroken, do write
    from kdl.engine.base import Locate
    assert np.array_equal(rows.cpu().numpy(), expected(before, fs, B, S, n, n, Locate(K, 51, "bilinear")))


# ------------------------------------------------------------------------------------ engines
def _images(S, seed, n):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def check_rows(rows, S, hw, spec, base_rows=None):
    """Locate rows: the front against the heatmap engine's, the tail against the rule on the row's own map."""
    from kdl.engine.base import unpack_locate
    h, w = hw
    K = spec.boxes
    assert rows.shape[1] == 2 + h * w + 1 + 3 * K
    if base_rows is not None:
        assert np.array_equal(_bits(rows[:, :2 + h * w]), _bits(base_rows))   # class, score and map: bit for bit
    _, _, heat, count, box, area = unpack_locate(rows, h, w, K)
    for b in range(len(rows)):
        assert np.array_equal(_bits(rows[b, 2 + h * w:]), words_of(heat[b], S, spec)), b
    assert (count > 0).all() and (area[:, 0] > 0).all()
    return box


SPECS = {"xception": ("bilinear", 3, 128), "vit_b16": ("bicubic", 8, 51)}


@pytest.fixture(scope="module")
def runs(xparams):
    """Per family, computed once: a heatmap (explain / rollout) engine's rows at batch 3 and 1, a locate
    engine's graph and eager rows, replays of the captured program on other pictures, and four batches
    through a stage pipeline on two slots with the joined engine's rows for each."""
    from kdl.engine import registry
    from kdl.engine.base import Locate
    from kdl.engine.stages import StagePipe
    done = {}

    def get(family):
        if family in done:
            return done[family]
        info = registry.get(family)
        nb = 3
        flt, K, thr = SPECS[family]
        spec = Locate(K, thr, flt)
        p = xparams if family == "xception" else info.init_params(0)
        mode = dict(rollout=True) if info.cam_oracle is None else dict(explain=True)
        S = info.input_size
        x = _images(S, 5, nb)
        e = info.engine(p, nb, "cuda", buckets=[1, nb], **mode)
        r = dict(S=S, hw=tuple(info.map_size), spec=spec, base=e.forward(x.cuda()).cpu().numpy(),
                 base1=e.forward(x[:1].cuda()).cpu().numpy(), base_names=[s.name for s in e.steps])
        del e
        eng = info.engine(p, nb, "cuda", buckets=[1, nb], locate=spec, **mode)
        r["steps"] = [(s.kind, s.name) for s in eng.steps]
        r["graph"] = eng.forward(x.cuda(), capture=True).cpu().numpy()
        r["eager"] = eng.forward(x.cuda(), capture=False).cpu().numpy()
        r["one"] = eng.forward(x[:1].cuda()).cpu().numpy()
        batches = [_images(S, 20 + i, nb) for i in range(4)]
        r["joined"] = [eng.forward(b.cuda()).cpu().numpy() for b in batches]   # the captured program, again and again
        r["replay"] = eng.forward(x.cuda()).cpu().numpy()
        del eng
        pipe = StagePipe(info.engine(p, nb, "cuda", locate=spec, **mode), info.stage_cut)
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
    check_rows(r["graph"], r["S"], r["hw"], r["spec"], r["base"])
    check_rows(r["one"], r["S"], r["hw"], r["spec"], r["base1"])
    assert [s[1] for s in r["steps"]] == r["base_names"] + ["locate"] and r["steps"][-1] == ("locate", "locate")


@pytest.mark.parametrize("family", list(SPECS))
def test_replays_of_the_captured_program(family, runs):
    r = runs(family)
    for rows in r["joined"]:
        check_rows(rows, r["S"], r["hw"], r["spec"])
    assert np.array_equal(_bits(r["replay"]), _bits(r["graph"]))     # the first pictures again: the same bits


@pytest.mark.parametrize("family", list(SPECS))
def test_stage_pipeline_boxes_are_each_batch_s_own(family, runs):
    r = runs(family)
    assert len(r["ranges"]) >= 2 and r["ranges"][-1][1] == len(r["steps"])    # the locate step: the last stage
    for i, (got, want) in enumerate(zip(r["pipe"], r["joined"])):
        assert np.array_equal(_bits(got), _bits(want)), f"batch {i}"
        check_rows(got, r["S"], r["hw"], r["spec"])


# ------------------------------------------------------------------------------------ server
def test_server_locate_trio(tmp_path):
    """locate, locate_image (a 534 x 400 picture) and locate_bytes (pants.png as JPEG) over gRPC: the boxes
    are the rule applied to the map the matching explain signature answers; class and score are its too."""
    import io
    from pathlib import Path

    import grpc
    from PIL import Image

    from kdl.engine.base import Locate
    from kdl.gateway import preprocess as pp
    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving import locate as L
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.server import ModelServer

    img = Image.open(Path(__file__).parent / "data" / "pants.png").convert("RGB")
    b = io.BytesIO()
    img.save(b, "JPEG", quality=90)
    jpeg = b.getvalue()
    big = np.asarray(img.resize((400, 534)), np.uint8)              # 534 rows x 400 columns
    assert big.shape == (534, 400, 3)
    inputs = {"locate": (pp.to_uint8(pp.load_image(jpeg))[None], "images"), "locate_image": (big[None], "images"),
              "locate_bytes": ([jpeg], "image_bytes")}
    base = tmp_path / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text('{"seed": 0, "locate": {"boxes": 4, "threshold": 128}}')
    spec = Locate(boxes=4, threshold=128)
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                       file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000, allowed_batch_sizes=[1, 2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            for name, (x, key) in inputs.items():
                out = stub.Predict(make_request(x, signature=name, input_key=key), timeout=120).outputs
                exp = stub.Predict(make_request(x, signature=name.replace("locate", "explain"), input_key=key),
                                   timeout=120).outputs
                assert sorted(out) == ["areas", "boxes", "classes", "num_boxes", "scores"]
                assert [d.size for d in out["boxes"].tensor_shape.dim] == [1, 4, 4]
                assert [d.size for d in out["areas"].tensor_shape.dim] == [1, 4]
                assert [d.size for d in out["num_boxes"].tensor_shape.dim] == [1, 1]
                heat = np.asarray(exp["heatmap"].float_val, np.float32).reshape(10, 10)
                count, box, area = L.locate_rule(heat, 299, spec)
                assert count > 0 and list(out["num_boxes"].int_val) == [count], name
                assert np.array_equal(np.asarray(out["boxes"].float_val, np.float32).reshape(4, 4), L.boxes_of(box, 299)), name
                assert np.array_equal(np.asarray(out["areas"].float_val, np.float32), L.areas_of(area, 299)), name
                assert list(out["classes"].string_val) == list(exp["classes"].string_val)
                assert np.array_equal(_bits(np.asarray(out["scores"].float_val, np.float32)),
                                      _bits(np.asarray(exp["scores"].float_val, np.float32)))
        s = srv.manager.get("clothing-model", None, None)
        r = s.runner("locate")
        assert r.out_cols == 102 + 1 + 12 and r.executors
        assert all(ex.engine.explain and ex.engine.locate == spec for ex in r.executors)
        assert s.device_alive()
    finally:
        srv.stop(0)
