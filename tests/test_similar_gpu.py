"""gallery_topk (kernels/similar.hip) alone, as the engines' last step, and behind the server.

Reference: float64 numpy on the same fp32 queries and the same bf16 gallery values,
S = q64 @ g64.T. With u = 2^-23 every returned score must satisfy

  |got - S[b, j]| <= E[b, j] = (F + 16) * u * sum_i |q_bi| * |g_ji|

the bound of an fp32 sum of F products in any order, doubled because the MFMA's internal
accumulation is not documented as round-to-nearest, with room for a query that reaches the matrix
cores as several bf16 terms. Every case checks four things (``check_rows``): the indices are
distinct and in range; each score is within E of the reference; the returned fp32 scores are
non-increasing with equal scores in ascending index order (exactly); and no row that was left
out could have belonged: S[b, j] - E[b, j] <= S[b, last] + E[b, last]. Near-ties are covered by
those inequalities, nothing is skipped. Each check prints its largest error / bound ratio."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
SENTINEL = 0x5A5A5A5A
NAN_BF16 = 0x7FC1


def C():
    from kdl.ops import _lib
    return _lib.lib()


def R() -> int:
    return C().GALLERY_CHUNK


def bf16_bits(x: torch.Tensor) -> np.ndarray:
    """fp32 tensor -> uint16 patterns of its round-to-nearest-even bf16 values."""
    return x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def bits64(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def reference(q32: np.ndarray, gbits: np.ndarray):
    """(S, E) float64 [B, N] of fp32 queries [B, F] and bf16 patterns [N, F]."""
    q64, g64 = q32.astype(np.float64), bits64(gbits)
    return q64 @ g64.T, (q32.shape[1] + 16) * U * (np.abs(q64) @ np.abs(g64).T)


def launch(q32: np.ndarray, gbits: np.ndarray, K: int, padded: bool = False, B: int | None = None):
    """One call through the direct binding -> (indices [B, K] int32, scores [B, K] fp32).
    ``padded``: ldq = F + 3 and ldg = F + 8 with NaN in the pad columns. The output has one row
    more than the launch writes and the workspace 256 bytes more than its size; both tails, filled
    with a sentinel, must come back intact."""
    lib = C()
    B = q32.shape[0] if B is None else B
    N, F = gbits.shape
    if padded:
        qp = np.full((q32.shape[0], F + 3), np.nan, np.float32)
        qp[:, :F] = q32
        gp = np.full((N, F + 8), NAN_BF16, np.uint16)
        gp[:, :F] = gbits
    else:
        qp, gp = q32, gbits
    q = torch.from_numpy(np.ascontiguousarray(qp)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(gp).view(np.int16)).cuda()
    out = torch.full((B + 1, 2 * K), SENTINEL, dtype=torch.int32, device="cuda")
    nw = lib.gallery_topk_workspace(B, N, K)
    assert nw > 0
    work = torch.full((nw + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    lib.gallery_topk(dict(q=q.data_ptr(), g=g.data_ptr(), out=out.data_ptr(), work=work.data_ptr(), B=B, N=N, F=F,
                          K=K, ldq=q.shape[1], ldg=g.shape[1]), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[B] == SENTINEL).all(), "words past 2K per row were written"
    assert bool((work[nw:] == 0xA5).all()), "bytes past the workspace were written"
    return o[:B, :K].copy(), o[:B, K:].copy().view(np.float32)


def check_rows(idx: np.ndarray, sc: np.ndarray, S: np.ndarray, E: np.ndarray, what: str) -> float:
    B, N = S.shape
    K = idx.shape[1]
    assert idx.shape == sc.shape == (B, K)
    worst = 0.0
    for b in range(B):
        i, s = idx[b].astype(np.int64), sc[b]
        assert ((i >= 0) & (i < N)).all() and len(set(i.tolist())) == K, (what, b, i)
        assert np.isfinite(s).all(), (what, b, s)
        err, bound = np.abs(s.astype(np.float64) - S[b, i]), E[b, i]
        assert (err[bound == 0] == 0).all(), (what, b, "a zero-bound score is off")
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert (err <= bound).all(), (what, b, err, bound)
        for k in range(K - 1):
            assert s[k] > s[k + 1] or (s[k] == s[k + 1] and i[k] < i[k + 1]), (what, b, k, s, i)
        rest = np.ones(N, bool)
        rest[i] = False
        assert (S[b, rest] - E[b, rest] <= S[b, i[-1]] + E[b, i[-1]]).all(), (what, b, "a better row was left out")
    print(f"{what}: max error / bound {worst:.3f}")
    return worst


def random_case(N: int, F: int, B: int, seed: int = 0):
    g = torch.Generator().manual_seed(1000003 * N + 101 * F + B + seed)
    q32 = torch.randn((B, F), generator=g, dtype=torch.float32).numpy()
    gbits = bf16_bits(torch.randn((N, F), generator=g, dtype=torch.float32))
    return q32, gbits


def run_case(N: int, F: int, B: int, K: int) -> float:
    q32, gbits = random_case(N, F, B)
    S, E = reference(q32, gbits)
    worst = 0.0
    for padded in (False, True):
        idx, sc = launch(q32, gbits, K, padded)
        worst = max(worst, check_rows(idx, sc, S, E, f"N={N} F={F} B={B} K={K} padded={int(padded)}"))
    return worst


BS = [1, 3, 16, 17, 33]


def n_values() -> list:
    r = R()
    return [1, 15, 16, 17, r - 1, r, r + 1, 2 * r + 3, 64 * r + 5]      # the last: 65 chunks in the merge


@pytest.mark.parametrize("ni", range(9))
def test_full_cross_of_rows_and_queries(ni):
    N = n_values()[ni]
    worst = max(run_case(N, 40, B, min(5, N)) for B in BS)
    print(f"N={N} F=40: largest error / bound over all cases {worst:.3f}")


@pytest.mark.parametrize("F", [8, 24, 768, 2048, 2560])
def test_other_feature_counts(F):
    r = R()
    worst = max(run_case(N, F, B, min(5, N)) for N, B in ((1, 1), (17, 3), (r - 1, 16), (r + 1, 17), (2 * r + 3, 33)))
    print(f"F={F}: largest error / bound over all cases {worst:.3f}")


@pytest.mark.parametrize("K", [1, 32])
def test_other_k(K):
    r = R()
    cases = [(r, 16), (2 * r + 3, 17), (64 * r + 5, 33)] + ([(1, 3), (15, 1)] if K == 1 else [(32, 3), (33, 1)])
    worst = max(run_case(N, 40, B, K) for N, B in cases)
    print(f"K={K}: largest error / bound over all cases {worst:.3f}")


# ------------------------------------------------------------------------------------ planted
PLANTED_K = 8
COSINES = [0.90 - 0.03 * k for k in range(PLANTED_K)]


def planted_case(F: int, N: int, B: int = 5):
    """Unit-norm queries; per query K rows at cosines 0.90, 0.87, ..., 0.69, every other row a
    random unit vector; the gallery rounded to bf16."""
    rng = np.random.default_rng(7 * F + N)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    q = unit(rng.standard_normal((B, F)))
    g = unit(rng.standard_normal((N, F)))
    where = rng.permutation(N)[:B * PLANTED_K].reshape(B, PLANTED_K)
    for b in range(B):
        for k, c in enumerate(COSINES):
            r = rng.standard_normal(F)
            r = unit(r - (r @ q[b]) * q[b])
            g[where[b, k]] = c * q[b] + np.sqrt(1 - c * c) * r
    return q.astype(np.float32), bf16_bits(torch.from_numpy(g.astype(np.float32)))


@pytest.mark.parametrize("F,N", [(32, 40), (64, 1000), (72, 1025), (768, 3000), (2048, 2500)])
def test_planted_neighbours_come_back_exactly(F, N):
    q32, gbits = planted_case(F, N)
    S, E = reference(q32, gbits)
    order = np.argsort(-S, axis=1, kind="stable")
    top = np.take_along_axis(S, order[:, :PLANTED_K + 1], axis=1)
    gap = float((top[:, :-1] - top[:, 1:]).min())
    print(f"F={F} N={N}: smallest gap among the top {PLANTED_K + 1} {gap:.4f}, 2 * max E {2 * E.max():.2e}")
    assert gap > 2 * E.max()                       # the reference alone decides the order
    for padded in (False, True):
        idx, sc = launch(q32, gbits, PLANTED_K, padded)
        assert np.array_equal(idx, order[:, :PLANTED_K])
        check_rows(idx, sc, S, E, f"planted F={F} N={N} padded={int(padded)}")


# ------------------------------------------------------------------------------------ ties
def test_equal_rows_rank_by_index_with_bit_equal_scores():
    r = R()
    N, F = 2 * r + 3, 72
    q32, gbits = random_case(N, F, 3)
    row = bf16_bits(torch.randn(F, generator=torch.Generator().manual_seed(9)))
    gbits[[3, r + 1, N - 1]] = row
    q32[1] = 4.0 * bits64(row).astype(np.float32)              # the three copies are query 1's best match
    S, E = reference(q32, gbits)
    assert np.argsort(-S[1], kind="stable")[:3].tolist() == [3, r + 1, N - 1]
    assert S[1, 3] - E[1, 3] > np.sort(S[1])[-4] + E[1].max()   # and nothing else comes near
    for padded in (False, True):
        idx, sc = launch(q32, gbits, 5, padded)
        assert idx[1, :3].tolist() == [3, r + 1, N - 1]
        assert len(set(sc[1, :3].view(np.uint32).tolist())) == 1
        check_rows(idx, sc, S, E, f"ties padded={int(padded)}")


def test_zero_query_returns_the_first_rows():
    q32, gbits = random_case(2 * R() + 3, 40, 3)
    q32[1] = 0
    for K in (1, 5, 32):
        idx, sc = launch(q32, gbits, K)
        assert idx[1].tolist() == list(range(K)) and (sc[1] == 0).all()


def test_two_launches_are_bit_equal():
    q32, gbits = random_case(2 * R() + 3, 2048, 33)
    a, b = launch(q32, gbits, 5), launch(q32, gbits, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_launcher_refusals_launch_nothing():
    lib = C()
    assert lib.GALLERY_MAX_N == 1 << 24 and lib.GALLERY_CHUNK > 0
    N, F, B, K = 40, 64, 4, 5
    q = torch.ones((B, 4104), dtype=torch.float32, device="cuda")
    g = torch.ones((N, 4104), dtype=torch.bfloat16, device="cuda")
    out = torch.full((B, 2 * K), SENTINEL, dtype=torch.int32, device="cuda")
    nw = lib.gallery_topk_workspace(B, N, K)
    assert nw > 0 and lib.gallery_topk_workspace(1024, 1 << 24, 32) > 0
    work = torch.zeros(nw, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(q=q.data_ptr(), g=g.data_ptr(), out=out.data_ptr(), work=work.data_ptr(), B=B, N=N, F=F, K=K,
              ldq=4104, ldg=4104)
    bad = [dict(F=60), dict(F=0), dict(F=4104), dict(F=4096, ldg=4088), dict(F=4096, ldq=4095), dict(ldg=4100),
           dict(ldg=56), dict(ldq=63), dict(K=0), dict(K=33), dict(N=3), dict(N=0), dict(N=(1 << 24) + 1),
           dict(B=0), dict(B=1025), dict(g=g.data_ptr() + 8), dict(work=None), dict(work=0)]
    for a in bad:
        with pytest.raises(RuntimeError):
            lib.gallery_topk({**ok, **a}, s)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    lib.gallery_topk(ok, s)                                      # still usable
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, :K] == np.arange(K)).all() and (o[:, K:].view(np.float32) == 64.0).all()


# ------------------------------------------------------------------------------------ engines
CASES = [("xception", "cosine"), ("xception", "dot"), ("resnet50", "cosine"), ("vit_b16", "cosine"),
         ("efficientnet_b7", "cosine")]
GALLERY_ROWS, ENGINE_K = 300, 5


def _images(family: str, seed: int = 5) -> torch.Tensor:
    from kdl.engine import registry
    S = registry.get(family).input_size
    return torch.randint(0, 256, (2, S, S, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _gallery(F: int) -> torch.Tensor:
    g = torch.randn((GALLERY_ROWS, F), generator=torch.Generator().manual_seed(F), dtype=torch.float32)
    return torch.nn.functional.normalize(g, dim=1).to(torch.bfloat16)


def _gbits(g: torch.Tensor) -> np.ndarray:
    return g.cpu().view(torch.int16).numpy().view(np.uint16)


@pytest.fixture(scope="module")
def runs(xparams):
    """Per (family, metric), computed once: the rows of a graph and of an eager forward of a similar
    engine at max_batch 2, its own feature buffer, its logits, and the rows of a stage pipeline over
    a second such engine built from the same gallery tensor. Per family: a plain engine's logits."""
    from kdl.engine import registry
    from kdl.engine.base import Similar
    from kdl.engine.stages import StagePipe
    params, plain, done = {"xception": xparams}, {}, {}

    def get(family: str, metric: str) -> dict:
        if (family, metric) in done:
            return done[family, metric]
        info = registry.get(family)
        if family not in params:
            params[family] = info.init_params(0)
        p, x = params[family], _images(family).cuda()
        if family not in plain:
            e = info.engine(p, 2, "cuda")
            plain[family] = dict(logits=e.forward(x), names=[s.name for s in e.steps], slots=len(e.logit_slots),
                                 logits_shape=tuple(e.logits.shape), features=len(e.feature_slots))
            del e
        gal = _gallery(info.features).cuda()
        sim = Similar(gal, ENGINE_K, metric)
        eng = info.engine(p, 2, "cuda", similar=sim)
        r = dict(plain=plain[family], names=[s.name for s in eng.steps], kinds=[s.kind for s in eng.steps],
                 srcs=[s.src for s in eng.steps[-2:]], gbits=_gbits(gal))
        r["graph"] = eng.forward(x, capture=True).cpu().numpy()
        torch.cuda.synchronize()
        r["features"] = eng.feature_slot(0)[:2].cpu().numpy()
        r["logits"] = eng.last_logits(0)[:2].clone()
        r["eager"] = eng.forward(x, capture=False).cpu().numpy()
        eng2 = info.engine(p, 2, "cuda", similar=sim)
        r["same_gallery"] = (eng.similar.gallery.data_ptr() == eng2.similar.gallery.data_ptr() == gal.data_ptr())
        del eng
        pipe = StagePipe(eng2, info.stage_cut)
        r["pipe"] = pipe.forward(x).cpu().numpy()
        del pipe, eng2
        done[family, metric] = r
        return r
    return get


@pytest.mark.parametrize("family,metric", CASES)
def test_engine_rows_follow_its_own_features(family, metric, runs):
    from kdl.engine.base import unpack_topk
    r = runs(family, metric)
    assert r["names"] == r["plain"]["names"] + ["embed_rows", "similar"] and r["kinds"][-2:] == ["embed", "similar"]
    assert all(r["srcs"])
    q32 = r["features"]
    if metric == "cosine":
        assert np.abs(np.linalg.norm(q32.astype(np.float64), axis=1) - 1).max() <= (q32.shape[1] / 2 + 8) * 2.0 ** -24
    S, E = reference(q32, r["gbits"])
    for k in ("graph", "eager", "pipe"):
        assert r[k].shape == (2, 2 * ENGINE_K)
        check_rows(*unpack_topk(r[k]), S, E, f"{family} {metric} {k}")
    assert np.array_equal(r["graph"].view(np.uint32), r["eager"].view(np.uint32))
    assert np.array_equal(r["graph"].view(np.uint32), r["pipe"].view(np.uint32))
    assert r["same_gallery"]


@pytest.mark.parametrize("family,metric", CASES)
def test_engine_logits_are_the_plain_engines(family, metric, runs):
    r = runs(family, metric)
    assert r["logits"].shape == r["plain"]["logits"].shape
    assert torch.equal(r["logits"], r["plain"]["logits"])        # the head is untouched, bit for bit


def test_similar_off_changes_nothing(runs):
    pl = runs("xception", "cosine")["plain"]
    assert "similar" not in pl["names"] and "embed_rows" not in pl["names"]
    assert pl["slots"] == 0 and pl["features"] == 0 and pl["logits_shape"] == (2, 10)


def test_similar_with_input_slots(xparams):
    """Slot 1 has its own rows, features and logits; slot 0 stays zero."""
    from kdl.engine import registry
    from kdl.engine.base import Similar, unpack_topk
    gal = _gallery(2048).cuda()
    eng = registry.get("xception").engine(xparams, 2, "cuda", similar=Similar(gal, ENGINE_K, "cosine"))
    slots = eng.add_input_slots(2)
    slots[1].copy_(_images("xception", 7).cuda())
    torch.cuda.synchronize()
    eng.launch(2, eng.stream, slot=1)
    eng.stream.synchronize()
    assert eng.slot_logits(1).shape == (2, 2 * ENGINE_K) and eng.last_logits(1).shape == (2, 10)
    S, E = reference(eng.feature_slot(1).cpu().numpy(), _gbits(gal))
    check_rows(*unpack_topk(eng.slot_logits(1)), S, E, "xception cosine slot 1")
    assert eng.last_logits(1).abs().sum().item() > 0
    assert eng.slot_logits(0).abs().sum().item() == 0.0 and eng.last_logits(0).abs().sum().item() == 0.0
    assert eng.feature_slot(0).abs().sum().item() == 0.0


def test_similar_k_is_clipped_to_the_gallery(xparams):
    from kdl.engine import registry
    from kdl.engine.base import Similar
    eng = registry.get("xception").engine(xparams, 2, "cuda", similar=Similar(_gallery(2048)[:3].cuda(), 5, "dot"))
    assert eng.similar_k == 3 and eng.logits.shape == (2, 6)


def test_bad_similar_values_raise(xparams):
    from kdl.engine import registry
    from kdl.engine.base import Similar
    mk = registry.get("xception").engine
    gal = _gallery(2048).cuda()
    with pytest.raises(ValueError):
        mk(xparams, 2, "cuda", similar=Similar(gal, 5, "cosine"), topk=3)
    with pytest.raises(ValueError):
        mk(xparams, 2, "cuda", similar=Similar(gal, 5, "cosine"), embed="l2")
    with pytest.raises(ValueError):
        mk(xparams, 2, "cuda", similar=Similar(gal, 5, "l1"))
    with pytest.raises(ValueError):
        mk(xparams, 2, "cuda", similar=Similar(gal[:, :768].contiguous(), 5, "cosine"))
    with pytest.raises(ValueError):
        mk(xparams, 2, "cuda", similar=Similar(gal.float(), 5, "cosine"))
    with pytest.raises(ValueError):
        mk(xparams, 2, "cuda", similar=Similar(gal, 0, "cosine"))


# ------------------------------------------------------------------------------------ server
def test_server_three_signatures_agree(tmp_path):
    """A synthetic Xception version with a 40-row gallery: 38 random rows, and at rows 11 and 29 the
    server's own raw embed rows of two JPEGs, fetched first from the same weights. Then the JPEGs
    through similar_bytes, their PIL-decoded pixels through similar_image and the
    gateway-preprocessed uint8 pixels through similar: the first two decode and resize on the
    device what the third receives, so the three answers are equal, and each image names its own
    row first with a score within E of 1 (the stored row is the image's own direction in bf16)."""
    import io
    import json
    from pathlib import Path

    import grpc
    from PIL import Image, ImageOps

    from kdl.gateway import preprocess as pp
    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.embed import l2_rule
    from kdl.serving.server import ModelServer
    from kdl.serving.similar import bf16_to_f64

    img = Image.open(Path(__file__).parent / "data" / "pants.png").convert("RGB")
    files = []
    for im, q in ((img, 90), (ImageOps.invert(img), 75)):
        b = io.BytesIO()
        im.save(b, "JPEG", quality=q)
        files.append(b.getvalue())
    decoded = [pp.load_image(f) for f in files]
    px = np.stack([np.asarray(d, np.uint8) for d in decoded])
    u8 = np.stack([pp.to_uint8(d) for d in decoded])
    F, N, K, planted = 2048, 40, 5, (11, 29)
    ids = [f"sku-{i:03d}" for i in range(N)]

    def serve(base):
        cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
                           file_system_poll_wait_seconds=0,
                           batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000, allowed_batch_sizes=[2]))
        return ModelServer(cfg).start(block_until_loaded=True)

    first = tmp_path / "first" / "clothing-model"
    (first / "1").mkdir(parents=True)
    (first / "1" / "synthetic.json").write_text('{"seed": 0}')
    srv = serve(first)
    try:
        assert "similar" not in srv.manager.get("clothing-model", None, None).signatures
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            t = PredictionStub(ch).Predict(make_request(files, signature="embed_bytes", input_key="image_bytes"),
                                           timeout=120).outputs["embedding"]
        own = np.asarray(t.float_val, np.float32).reshape(2, F)
    finally:
        srv.stop(0)
    gal = np.abs(np.random.default_rng(40).standard_normal((N, F))).astype(np.float32)
    gal[planted[0]], gal[planted[1]] = own[0], own[1]
    base = tmp_path / "second" / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text(json.dumps({"seed": 0, "similar": {"top_k": K, "metric": "cosine"}}))
    np.save(base / "1" / "gallery.npy", gal)
    (base / "1" / "gallery_ids.txt").write_text("".join(i + "\n" for i in ids))
    srv = serve(base)
    try:
        got = {}
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            for sig, key, X in (("similar_bytes", "image_bytes", files), ("similar_image", "images", px),
                                ("similar", "images", u8)):
                out = stub.Predict(make_request(X, signature=sig, input_key=key), timeout=120).outputs
                assert sorted(out) == ["ids", "scores"]
                for name in ("ids", "scores"):
                    assert [d.size for d in out[name].tensor_shape.dim] == [2, K]
                got[sig] = ([v.decode() for v in out["ids"].string_val], np.asarray(out["scores"].float_val, np.float32))
        s = srv.manager.get("clothing-model", None, None)
        r = s.runner("similar")
        assert r.out_cols == 2 * K and r.executors
        ptrs = {ex.engine.similar.gallery.data_ptr() for ex in r.executors}
        ptrs |= {ex.pipe.engine.similar.gallery.data_ptr() for ex in r.executors if ex.pipe is not None}
        assert len(ptrs) == 1                                   # one device copy for every engine
        for sig in ("similar_bytes", "similar_image"):
            assert got[sig][0] == got["similar"][0]
            assert np.array_equal(got[sig][1].view(np.uint32), got["similar"][1].view(np.uint32))
        names, scores = got["similar"][0], got["similar"][1].reshape(2, K)
        g64 = bf16_to_f64(s.source.gallery)
        q64 = l2_rule(own).astype(np.float64)
        for i in range(2):
            assert names[i * K] == ids[planted[i]]
            E = (F + 16) * U * float(np.abs(q64[i]) @ np.abs(g64[planted[i]]))
            print(f"image {i}: own score {scores[i, 0]:.7f}, |score - 1| / E {abs(float(scores[i, 0]) - 1) / E:.3f}")
            assert abs(float(scores[i, 0]) - 1) <= E
        assert s.device_alive()
    finally:
        srv.stop(0)
