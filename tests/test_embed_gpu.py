"""embed_rows (kernels/embed.hip) alone, as the engines' last step, against the fp32 oracle, and
behind the server.

Reference for the kernel and the engines: float64 numpy pooling of the same bf16 / fp16 values.
With u = 2^-24, v_c the float64 mean of channel c and a_c the float64 mean of |x| over its pixels:

  raw   |got - v_c| <= E_c = (HW + 2) * u * a_c     (an fp32 sum of HW terms in any order, the
                                                     reciprocal and the scaling are inside that)
  l2    |got - v_c / n| <= E_c / n + |v_c / n| * (||E||_2 / n + (F / 2 + 8) * u),
        n = max(||v||_2, 1e-12)                      (the error of the means, of their norm, and
                                                     of an fp32 sum of F squares, root and division)

Both are computed in float64 here; each check prints its largest error / bound ratio."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
HWS = [1, 7, 49, 100, 361]
FS = [8, 72, 768, 2048, 2560]
BS = [1, 3, 33]
SENTINEL = 777.0


def bounds(x64: np.ndarray, norm: bool):
    """x64 float64 [B, HW, F] -> (reference [B, F], bound [B, F])."""
    hw, F = x64.shape[1], x64.shape[2]
    v = x64.mean(axis=1)
    E = (hw + 2) * U * np.abs(x64).mean(axis=1)
    if not norm:
        return v, E
    n = np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    w = v / n
    return w, E / n + np.abs(w) * (np.linalg.norm(E, axis=1, keepdims=True) / n + (F / 2 + 8) * U)


def check(got: np.ndarray, want: np.ndarray, bound: np.ndarray, what: str) -> float:
    assert np.isfinite(got).all(), f"{what}: NaN or inf in the rows"
    err = np.abs(got.astype(np.float64) - want)
    exact = bound == 0
    assert (err[exact] == 0).all(), f"{what}: a zero-bound element is off"
    ratio = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(f"{what}: max error / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    return ratio


def launch(x: torch.Tensor, F: int, ldo: int, dt: int, norm: int) -> torch.Tensor:
    """One call through the direct binding into sentinel-filled rows; x [B, HW, ldx] on the device."""
    from kdl.ops import _lib
    B, hw, ldx = x.shape
    out = torch.full((B, ldo), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.lib().embed_rows(dict(x=x.data_ptr(), out=out.data_ptr(), B=B, HW=hw, F=F, ldx=ldx, ldo=ldo, dt=dt,
                               norm=norm), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def base_input(B: int, hw: int, F: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(100000 * hw + 10 * F + B)
    return torch.randn((B, hw, F + 8), generator=g, dtype=torch.float32)


def make_input(base: torch.Tensor, dtype, kind: str) -> torch.Tensor:
    """[B, HW, F + 8] in ``dtype`` on the host: signed normal values, or their magnitudes (a
    post-ReLU map). From three images on, image 1 is all zero and (bf16 only: fp16 has no
    values that small) image 2 has a norm below 1e-12."""
    B = base.shape[0]
    x = base.abs() if kind == "relu" else base.clone()
    if B >= 3:
        x[1] = 0
        if dtype == torch.bfloat16:
            x[2] *= 1e-17
    return x.to(dtype)


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("hw", HWS)
def test_kernel_is_inside_the_derived_bounds(hw, F):
    worst = 0.0
    for B in BS:
        base = base_input(B, hw, F)
        for dt, dtype in ((0, torch.bfloat16), (1, torch.float16)):
            for kind in ("normal", "relu"):
                xh = make_input(base, dtype, kind)
                x64 = xh[:, :, :F].to(torch.float64).numpy()
                ref = {n: bounds(x64, bool(n)) for n in (0, 1)}
                if B >= 3 and dt == 0:
                    assert 0 < np.linalg.norm(ref[0][0][2]) < 1e-12
                wide = xh.cuda()
                tight = wide[:, :, :F].contiguous()
                for x in (tight, wide):
                    for ldo in (F, F + 3):
                        for n in (0, 1):
                            out = launch(x, F, ldo, dt, n).cpu().numpy()
                            assert (out[:, F:] == SENTINEL).all(), "pad columns were written"
                            what = f"HW={hw} F={F} B={B} dt={dt} {kind} ldx={x.shape[2]} ldo={ldo} norm={n}"
                            worst = max(worst, check(out[:, :F], *ref[n], what))
                            if B >= 3:
                                assert (out[1, :F] == 0).all(), "the all-zero image must stay zero"
    print(f"HW={hw} F={F}: largest error / bound over all cases {worst:.3f}")


def test_two_launches_are_bit_equal():
    x = make_input(base_input(33, 100, 2048), torch.bfloat16, "normal")[:, :, :2048].contiguous().cuda()
    a, b = launch(x, 2048, 2048, 0, 1), launch(x, 2048, 2048, 0, 1)
    assert torch.equal(a, b)


def test_launcher_refusals_launch_nothing():
    from kdl.ops import _lib
    C = _lib.lib()
    assert C.EMBED_MAX_F == 4096
    x = torch.ones((4, 2, 4104), dtype=torch.bfloat16, device="cuda")
    out = torch.full((4, 4104), SENTINEL, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(B=4, HW=2, F=64, ldx=4104, ldo=4104, dt=0, norm=1)
    bad = [dict(F=60), dict(F=4104), dict(F=4096, ldx=4088), dict(ldx=4100), dict(B=0), dict(HW=0), dict(dt=2),
           dict(dt=-1), dict(ldo=56), dict(F=0), dict(norm=2)]
    for a in bad:
        with pytest.raises(RuntimeError):
            C.embed_rows(dict(x=x.data_ptr(), out=out.data_ptr(), **{**ok, **a}), s)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    C.embed_rows(dict(x=x.data_ptr(), out=out.data_ptr(), **ok), s)          # still usable
    torch.cuda.synchronize()
    assert torch.equal(out[:, :64], torch.full((4, 64), 0.125, device="cuda"))   # 1 / sqrt(64)
    assert bool((out[:, 64:] == SENTINEL).all())


# ------------------------------------------------------------------------------------ engines
FAMILIES = ["xception", "resnet50", "vit_b16", "efficientnet_b7"]
MODES = ["raw", "l2"]


def _images(family: str, seed: int = 5) -> torch.Tensor:
    from kdl.engine import registry
    S = registry.get(family).input_size
    return torch.randint(0, 256, (2, S, S, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _source64(eng) -> np.ndarray:
    """The engine's own source buffer after a forward, as float64 [2, HW, F]."""
    src, hw, ldx, F, _ = eng.embed_source()
    buf = eng.bufs[src].reshape(-1)[:2 * hw * ldx].view(2, hw, ldx)[:, :, :F]
    return buf.to(torch.float64).cpu().numpy()


@pytest.fixture(scope="module")
def runs(xparams):
    """Per (family, mode), computed once: the rows of a graph and of an eager forward of an embed
    engine at max_batch 2, the derived reference of its source buffer, its logits, and the rows of
    a stage pipeline over a second such engine. Per family: the logits of a plain engine."""
    from kdl.engine import registry
    from kdl.engine.stages import StagePipe
    params, plain, done = {"xception": xparams}, {}, {}

    def get(family: str, mode: str) -> dict:
        if (family, mode) in done:
            return done[family, mode]
        info = registry.get(family)
        if family not in params:
            params[family] = info.init_params(0)
        p, x = params[family], _images(family).cuda()
        if family not in plain:
            e = info.engine(p, 2, "cuda")
            plain[family] = dict(logits=e.forward(x), steps=len(e.steps), names=[s.name for s in e.steps],
                                 slots=len(e.logit_slots), logits_shape=tuple(e.logits.shape))
            del e
        eng = info.engine(p, 2, "cuda", embed=mode)
        r = dict(plain=plain[family], params=p, F=eng.embed_dim, embed=eng.embed, last=eng.steps[-1], nsteps=len(eng.steps))
        r["graph"] = eng.forward(x, capture=True).cpu().numpy()
        torch.cuda.synchronize()
        r["ref"] = bounds(_source64(eng), mode == "l2")
        r["logits"] = eng.last_logits(0)[:2].clone()
        r["eager"] = eng.forward(x, capture=False).cpu().numpy()
        del eng
        pipe = StagePipe(info.engine(p, 2, "cuda", embed=mode), info.stage_cut)
        r["pipe"] = pipe.forward(x).cpu().numpy()
        del pipe
        done[family, mode] = r
        return r
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", FAMILIES)
def test_engine_rows_follow_its_own_source_buffer(family, mode, runs):
    from kdl.engine import registry
    r = runs(family, mode)
    F = registry.get(family).features
    assert r["F"] == F and r["embed"] == mode
    assert r["last"].kind == "embed" and r["last"].src and r["nsteps"] == r["plain"]["steps"] + 1
    for k in ("graph", "eager"):
        assert r[k].shape == (2, F)
        check(r[k], *r["ref"], f"{family} {mode} {k}")
    assert np.array_equal(r["graph"], r["eager"])
    if mode == "l2":
        assert np.abs(np.linalg.norm(r["graph"].astype(np.float64), axis=1) - 1).max() <= (F / 2 + 8) * U


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", FAMILIES)
def test_engine_logits_are_the_plain_engines(family, mode, runs):
    r = runs(family, mode)
    assert r["logits"].shape == r["plain"]["logits"].shape
    assert torch.equal(r["logits"], r["plain"]["logits"])        # the head is untouched, bit for bit


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", FAMILIES)
def test_stage_pipeline_rows_are_bit_equal(family, mode, runs):
    r = runs(family, mode)
    assert np.array_equal(r["pipe"], r["graph"])


def test_embed_off_changes_nothing(runs):
    pl = runs("xception", "raw")["plain"]
    assert "embed_rows" not in pl["names"] and pl["slots"] == 0 and pl["logits_shape"] == (2, 10)


def test_embed_with_input_slots(xparams):
    """Slot 1 has its own rows and logits; slot 0 stays zero."""
    from kdl.engine import registry
    eng = registry.get("xception").engine(xparams, 2, "cuda", embed="l2")
    slots = eng.add_input_slots(2)
    slots[1].copy_(_images("xception", 7).cuda())
    torch.cuda.synchronize()
    eng.launch(2, eng.stream, slot=1)
    eng.stream.synchronize()
    assert eng.slot_logits(1).shape == (2, 2048) and eng.last_logits(1).shape == (2, 10)
    check(eng.slot_logits(1).cpu().numpy(), *bounds(_source64(eng), True), "xception l2 slot 1")
    assert eng.last_logits(1).abs().sum().item() > 0
    assert eng.slot_logits(0).abs().sum().item() == 0.0 and eng.last_logits(0).abs().sum().item() == 0.0


def test_bad_embed_values_raise(xparams):
    from kdl.engine import registry
    mk = registry.get("xception").engine
    with pytest.raises(ValueError):
        mk(xparams, 2, "cuda", embed="l1")
    with pytest.raises(ValueError):
        mk(xparams, 2, "cuda", embed="raw", topk=3)


# ------------------------------------------------------------------------------------ fp32 oracle
# ||row - feature_oracle||_2 / ||feature_oracle||_2 of the raw rows. bf16 / fp16 activations
# against an fp32 model: the figure cannot be derived, so each family is gated at twice the largest
# value measured on the device over seeds 0..3, two images each (profiles/embed.txt). The run is
# deterministic; the margin is for other inputs.
ORACLE_GATE = {"xception": 0.0368, "resnet50": 0.0416, "vit_b16": 0.0210, "efficientnet_b7": 0.4042}


def _oracle_error(rows: np.ndarray, ref: np.ndarray) -> float:
    rows, ref = rows.astype(np.float64), ref.astype(np.float64)
    return float((np.linalg.norm(rows - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())


@pytest.mark.parametrize("family", FAMILIES)
def test_rows_against_the_fp32_oracle(family, runs):
    """Gate = 2 x the largest of 8 measured values (4 seeds x 2 images):

      family            measured max   gate
      xception          0.018360       0.0368
      resnet50          0.020751       0.0416
      vit_b16           0.010493       0.0210
      efficientnet_b7   0.202041       0.4042
    """
    from kdl.engine import registry
    r = runs(family, "raw")
    ref = registry.get(family).feature_oracle(r["params"], _images(family)).numpy()
    err = _oracle_error(r["graph"], ref)
    print(f"{family}: relative L2 error against the fp32 oracle {err:.6f} (gate {ORACLE_GATE[family]})")
    assert err <= ORACLE_GATE[family]


# ------------------------------------------------------------------------------------ server
def test_server_three_signatures_agree(tmp_path, xparams):
    """Two JPEGs through embed_bytes, their PIL-decoded pixels through embed_image, and the
    gateway-preprocessed uint8 pixels through embed: the first two decode and resize on the device
    what the third receives, so the three answers are bit-equal."""
    import io
    from pathlib import Path

    import grpc
    from PIL import Image

    from kdl.engine import registry
    from kdl.gateway import preprocess as pp
    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.server import ModelServer

    img = Image.open(Path(__file__).parent / "data" / "pants.png").convert("RGB")
    files = []
    for q in (90, 75):
        b = io.BytesIO()
        img.save(b, "JPEG", quality=q)
        files.append(b.getvalue())
    decoded = [pp.load_image(f) for f in files]
    px = np.stack([np.asarray(d, np.uint8) for d in decoded])
    u8 = np.stack([pp.to_uint8(d) for d in decoded])
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
            got = {}
            for sig, key, X in (("embed_bytes", "image_bytes", files), ("embed_image", "images", px),
                                ("embed", "images", u8)):
                t = stub.Predict(make_request(X, signature=sig, input_key=key), timeout=120).outputs["embedding"]
                assert [d.size for d in t.tensor_shape.dim] == [2, 2048]
                got[sig] = np.asarray(t.float_val, np.float32).reshape(2, 2048)
        s = srv.manager.get("clothing-model", None, None)
        r = s.runner("embed")
        assert r.out_cols == 2048 and r.executors and all(ex.engine.embed == "raw" for ex in r.executors)
        assert np.array_equal(got["embed_bytes"], got["embed"]) and np.array_equal(got["embed_image"], got["embed"])
        ref = registry.get("xception").feature_oracle(xparams, torch.from_numpy(u8)).numpy()
        err = _oracle_error(got["embed"], ref)
        print(f"server embed: relative L2 error against the fp32 oracle {err:.6f} (gate {ORACLE_GATE['xception']})")
        assert err <= ORACLE_GATE["xception"]
        assert s.device_alive()
    finally:
        srv.stop(0)
