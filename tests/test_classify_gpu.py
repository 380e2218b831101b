"""softmax_topk (kernels/classify.hip) alone, as the engines' last step, and behind the server.

Reference everywhere: numpy float64 softmax plus ``np.argsort(-x, kind="stable")`` on the same
fp32 logits. Classes are compared exactly. Scores are compared at rtol = (NC + 128) * 2^-24:
NC * 2^-24 bounds any summation order of NC positive fp32 terms, 128 * 2^-24 covers the rounding
of x - max (|x - max| <= 60 in every input set, so no compared score is subnormal) through the
exponential; the float64 reference is inside that bound by construction."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NCS = [1, 2, 10, 63, 64, 65, 1000, 1001]
BS = [1, 3, 32, 33]


def rtol(nc: int) -> float:
    return (nc + 128) * 2.0 ** -24


def reference(x: np.ndarray):
    """x fp32 [B, NC] -> (stable descending order int64 [B, NC], float64 softmax [B, NC])."""
    x64 = x.astype(np.float64)
    order = np.argsort(-x64, axis=1, kind="stable")
    e = np.exp(x64 - x64.max(axis=1, keepdims=True))
    return order, e / e.sum(axis=1, keepdims=True)


def input_sets(B: int, nc: int) -> dict:
    """Every set has max - min <= 60."""
    rng = np.random.default_rng(1000 * nc + B)
    sets = {f"normal{i}": np.clip(rng.standard_normal((B, nc)) * 6.0, -30, 30).astype(np.float32) for i in range(4)}
    sets["ties"] = (np.round(np.clip(rng.standard_normal((B, nc)) * 2.0, -8, 8) * 2) / 2).astype(np.float32)
    sets["equal"] = np.full((B, nc), 1.25, np.float32)
    sets["offset"] = (np.clip(rng.standard_normal((B, nc)) * 6.0, -30, 30) + 1e4).astype(np.float32)
    for v in sets.values():
        assert float(v.max() - v.min()) <= 60.0
    return sets


def run_kernel(x: np.ndarray, K: int, ldx: int) -> np.ndarray:
    """One launch through the direct binding; returns the raw rows int32 [B, 2K]."""
    from kdl.ops import _lib
    B, nc = x.shape
    buf = torch.full((B, ldx), float("nan"), dtype=torch.float32)     # the pad columns are never read
    buf[:, :nc] = torch.from_numpy(x)
    d = buf.cuda()
    out = torch.full((B, 2 * K), -1, dtype=torch.int32, device="cuda")
    _lib.lib().softmax_topk(dict(x=d.data_ptr(), out=out.data_ptr(), B=B, NC=nc, K=K, ldx=ldx),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_rows(rows: np.ndarray, x: np.ndarray, K: int, ref=None) -> None:
    order, p = ref if ref is not None else reference(x)
    nc = x.shape[1]
    cls = rows[:, :K].view(np.int32)
    sc = np.ascontiguousarray(rows[:, K:]).view(np.float32)
    assert np.array_equal(cls, order[:, :K]), (cls, order[:, :K])
    want = np.take_along_axis(p, order[:, :K], axis=1)
    err = np.abs(sc.astype(np.float64) - want) / want
    print(f"NC={nc} K={K} B={x.shape[0]}: max score rel err {err.max():.3e} (bound {rtol(nc):.3e})")
    assert err.max() <= rtol(nc), (err.max(), rtol(nc))


@pytest.mark.parametrize("nc", NCS)
def test_kernel_matches_float64_rule(nc):
    ks = sorted({k for k in (1, 3, 5, min(nc, 32)) if k <= nc})
    for B in BS:
        for name, x in input_sets(B, nc).items():
            ref = reference(x)
            for ldx in (nc, nc + 3):
                for K in ks:
                    rows = run_kernel(x, K, ldx)
                    check_rows(rows, x, K, ref)
                    if name == "equal":
                        assert np.array_equal(rows[:, :K], np.tile(np.arange(K, dtype=np.int32), (B, 1)))


@pytest.mark.parametrize("nc,K,B", [(10, 5, 3), (1001, 32, 33)])
def test_two_launches_are_bit_equal(nc, K, B):
    x = input_sets(B, nc)["normal1"]
    a, b = run_kernel(x, K, nc), run_kernel(x, K, nc)
    assert np.array_equal(a, b)


def test_launcher_refusals_launch_nothing():
    from kdl.ops import _lib
    C = _lib.lib()
    assert C.TOPK_MAX_NC >= 1001 and C.TOPK_MAX_K == 32
    x = torch.zeros((4, 2048), dtype=torch.float32, device="cuda")
    out = torch.full((4, 64), -7, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    bad = [dict(B=4, NC=10, K=0), dict(B=4, NC=10, K=11), dict(B=4, NC=100, K=33), dict(B=0, NC=10, K=3),
           dict(B=4, NC=0, K=1), dict(B=4, NC=C.TOPK_MAX_NC + 1, K=5), dict(B=-1, NC=10, K=3)]
    for a in bad:
        with pytest.raises(RuntimeError):
            C.softmax_topk(dict(x=x.data_ptr(), out=out.data_ptr(), ldx=2048, **a), s)
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    C.softmax_topk(dict(x=x.data_ptr(), out=out.data_ptr(), ldx=2048, B=4, NC=10, K=3), s)   # still usable
    torch.cuda.synchronize()
    rows = out.view(-1)[:4 * 6].view(4, 6).cpu()                 # the kernel's rows are 2K words, packed
    assert rows[:, :3].tolist() == [[0, 1, 2]] * 4
    assert bool((out.view(-1)[4 * 6:] == -7).all())


# ------------------------------------------------------------------------------------ engine
def _engine(family: str, topk: int, params):
    from kdl.engine import registry
    return registry.get(family).engine(params, 2, "cuda", topk=topk)


@pytest.fixture(scope="module")
def family_params(xparams):
    from kdl.engine import registry
    cache = {"xception": xparams}

    def get(family):
        if family not in cache:
            cache[family] = registry.get(family).init_params(0)
        return cache[family]
    return get


def _images(family: str, seed: int) -> torch.Tensor:
    from kdl.engine import registry
    S = registry.get(family).input_size
    return torch.randint(0, 256, (2, S, S, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _check_engine_rows(eng, rows: torch.Tensor, K: int, classes: int) -> None:
    from kdl.engine.base import unpack_topk
    torch.cuda.synchronize()
    logits = eng.last_logits(0)[:2].cpu().numpy()
    assert rows.shape == (2, 2 * K) and logits.shape == (2, classes)
    order, p = reference(logits)
    cls, sc = unpack_topk(rows)
    assert np.array_equal(cls, order[:, :K]), (cls, order[:, :K])
    want = np.take_along_axis(p, order[:, :K], axis=1)
    err = np.abs(sc.astype(np.float64) - want) / want
    print(f"{eng.model_name} K={K}: max score rel err {err.max():.3e} (bound {rtol(classes):.3e})")
    assert err.max() <= rtol(classes)


@pytest.mark.parametrize("family,classes", [("xception", 10), ("resnet50", 1000)])
@pytest.mark.parametrize("topk", [3, 5])
def test_engine_rows_follow_its_own_logits(family, classes, topk, family_params):
    from kdl.engine import registry
    from kdl.engine.stages import StagePipe
    p = family_params(family)
    eng = _engine(family, topk, p)
    assert eng.topk == topk and eng.steps[-1].kind == "topk"
    x = _images(family, 5).cuda()
    for capture in (True, False):
        _check_engine_rows(eng, eng.forward(x, capture=capture), topk, classes)
    pipe = StagePipe(_engine(family, topk, p), registry.get(family).stage_cut)
    _check_engine_rows(pipe.engine, pipe.forward(x), topk, classes)


def test_engine_topk_is_clipped_and_zero_changes_nothing(family_params, xparams):
    x = _images("xception", 6).cuda()
    plain = _engine("xception", 0, xparams)
    assert plain.topk == 0 and all(s.kind != "topk" for s in plain.steps) and not plain.logit_slots
    packed = _engine("xception", 5, xparams)
    ref = plain.forward(x)
    packed.forward(x)
    torch.cuda.synchronize()
    assert ref.shape == (2, 10)
    assert torch.equal(ref, packed.last_logits(0)[:2])          # the head's logits are untouched, bit for bit
    assert torch.equal(ref, plain.last_logits(0)[:2])
    clipped = _engine("xception", 32, xparams)
    assert clipped.topk == 10 and clipped.logits.shape == (2, 20)
    _check_engine_rows(clipped, clipped.forward(x), 10, 10)


def test_engine_topk_with_input_slots(xparams):
    """Slot 1 has its own logits and packed rows; slot 0 stays untouched."""
    eng = _engine("xception", 3, xparams)
    slots = eng.add_input_slots(2)
    slots[1].copy_(_images("xception", 7).cuda())
    torch.cuda.synchronize()
    eng.launch(2, eng.stream, slot=1)
    eng.stream.synchronize()
    from kdl.engine.base import unpack_topk
    cls, sc = unpack_topk(eng.slot_logits(1))
    order, p = reference(eng.last_logits(1).cpu().numpy())
    assert np.array_equal(cls, order[:, :3])
    assert eng.slot_logits(0).abs().sum().item() == 0.0 and eng.last_logits(0).abs().sum().item() == 0.0


# ------------------------------------------------------------------------------------ server
def test_server_classify_bytes_and_classify_rpc_follow_serving_bytes(tmp_path):
    """One classify_bytes Predict of two JPEGs and one Classify RPC of the same files against the
    rule applied to serving_bytes' logits for them. The classify runner's engines run the same
    kernels and tuning on the same pixels and every sum of the engine is in a fixed order, so the
    logits are expected to be equal; classes are compared exactly."""
    import io
    from pathlib import Path

    import grpc
    from PIL import Image

    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving import protos as P
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.server import ModelServer

    img = Image.open(Path(__file__).parent / "data" / "pants.png").convert("RGB")
    files = []
    for size, q in ((534, 400), 90), ((301, 240), 75):
        b = io.BytesIO()
        img.resize(size).save(b, "JPEG", quality=q)
        files.append(b.getvalue())
    base = tmp_path / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text('{"seed": 0}')
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                       file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000, allowed_batch_sizes=[2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            ref = stub.Predict(make_request(files, signature="serving_bytes", input_key="image_bytes"), timeout=120)
            logits = np.asarray(ref.outputs["dense_7"].float_val, np.float32).reshape(2, 10)
            got = stub.Predict(make_request(files, signature="classify_bytes", input_key="image_bytes"), timeout=120)
            req = P.ClassificationRequest()
            req.model_spec.name = "clothing-model"
            for d in files:
                req.input.example_list.examples.add().features.feature["image/encoded"].bytes_list.value.append(d)
            raw = ch.unary_unary(P.CLASSIFY_METHOD)(req.SerializeToString(), timeout=120)
        s = srv.manager.get("clothing-model", None, None)
        r = s.runner("classify")
        assert r.gpu and r.sig.top_k == 5 and r.out_cols == 10 and all(ex.engine.topk == 5 for ex in r.executors)
        order, p = reference(logits)
        want_cls = [[str(c) for c in row] for row in order[:, :5]]
        want = np.take_along_axis(p, order[:, :5], axis=1)
        cl, sc = got.outputs["classes"], got.outputs["scores"]
        assert [d.size for d in sc.tensor_shape.dim] == [2, 5]
        assert np.asarray([v.decode() for v in cl.string_val]).reshape(2, 5).tolist() == want_cls
        err = np.abs(np.asarray(sc.float_val, np.float64).reshape(2, 5) - want) / want
        print(f"server classify_bytes: max score rel err {err.max():.3e} (bound {rtol(10):.3e})")
        assert err.max() <= rtol(10)
        resp = P.ClassificationResponse.FromString(raw)
        assert [[k.label for k in c.classes] for c in resp.result.classifications] == want_cls
        rpc = np.asarray([[k.score for k in c.classes] for c in resp.result.classifications], np.float32)
        assert np.array_equal(rpc, np.asarray(sc.float_val, np.float32).reshape(2, 5))     # the same runner, the same rows
        assert s.device_alive()
    finally:
        srv.stop(0)
