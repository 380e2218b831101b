"""gallery_topk over an fp8 gallery (kernels/similar_f8.hip): alone, in an engine, behind the server.

Reference: float64 numpy on the same fp32 queries, e4m3 codes and fp32 scales,
S[b, j] = s_j * sum_i q_bi * val(e_ji), and the bound of tests/test_similar_gpu.py with one more
rounding for the scale multiply: E[b, j] = (F + 17) * 2^-23 * s_j * sum_i |q_bi| * |val(e_ji)|.
Every case goes through that file's four checks (``check_rows``)."""
import json

import numpy as np
import pytest
import torch

from kdl.serving.similar import fp8_to_f64, quantize_fp8, similar_rule
from test_similar_gpu import SENTINEL, C, R, U, check_rows

pytestmark = pytest.mark.gpu
FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)       # the 254 finite codes


def reference(q32, codes, scale):
    q64, g64, s64 = q32.astype(np.float64), fp8_to_f64(codes), scale.astype(np.float64)
    return (q64 @ g64.T) * s64, (q32.shape[1] + 17) * U * (np.abs(q64) @ np.abs(g64).T) * s64


def launch(q32, codes, scale, K, padded=False, bad=None):
    """One call through the direct binding, with the sentinel row and workspace tail of
    test_similar_gpu.launch. ``padded``: ldq = F + 3 with NaN pads, ldg = F + 16 with NaN-code pads.
    ``bad`` overrides arguments: the call must then be refused and write nothing."""
    lib, (B, F), N = C(), q32.shape, codes.shape[0]
    if padded:
        q32 = np.concatenate([q32, np.full((B, 3), np.nan, np.float32)], axis=1)
        codes = np.concatenate([codes, np.full((N, 16), 0x7F, np.uint8)], axis=1)
    q, g, s = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q32, codes, scale))
    out = torch.full((B + 1, 2 * K), SENTINEL, dtype=torch.int32, device="cuda")
    nw = lib.gallery_topk_workspace(B, N, K)
    work = torch.full((nw + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    args = dict(q=q.data_ptr(), g8=g.data_ptr(), scale=s.data_ptr(), out=out.data_ptr(), work=work.data_ptr(), B=B, N=N,
                F=F, K=K, ldq=q.shape[1], ldg=g.shape[1])
    args.update({k: (args[k] + v[1] if isinstance(v, tuple) else v) for k, v in (bad or {}).items()})
    stream = torch.cuda.current_stream().cuda_stream
    if bad:
        with pytest.raises(RuntimeError):
            lib.gallery_topk(args, stream)
    else:
        lib.gallery_topk(args, stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[B if not bad else 0:] == SENTINEL).all() and bool((work[nw:] == 0xA5).all())
    return o[:B, :K].copy(), o[:B, K:].copy().view(np.float32)


def random_case(N, F, B):
    rng = np.random.default_rng(1000003 * N + 101 * F + B)
    scale = (2.0 ** rng.integers(-12, -1, N) * rng.uniform(1, 2, N)).astype(np.float32)
    return rng.standard_normal((B, F)).astype(np.float32), FINITE[rng.integers(0, 254, (N, F))], scale


def run_case(N, F, B, K):
    q32, codes, scale = random_case(N, F, B)
    S, E = reference(q32, codes, scale)
    for padded in (False, True):
        check_rows(*launch(q32, codes, scale, K, padded), S, E, f"fp8 N={N} F={F} B={B} K={K} padded={int(padded)}")


@pytest.mark.parametrize("B", [1, 17, 33])
@pytest.mark.parametrize("ni", range(5))
def test_rows_and_queries(ni, B):
    N = [1, 17, R() - 1, R() + 1, 2 * R() + 3][ni]
    run_case(N, 48, B, min(5, N))


@pytest.mark.parametrize("F", [16, 144, 768, 2048, 2560])
def test_feature_counts(F):
    run_case(300, F, 3, 32 if F == 144 else 5)


def test_every_code_converts_exactly():
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    codes[(codes & 0x7F) == 0x7F] = 0
    scale = (2.0 ** (np.arange(16) - 8.0)).astype(np.float32)
    q32 = np.eye(16, dtype=np.float32)
    idx, sc = launch(q32, codes, scale, 16)
    want_i, want_s = similar_rule(q32, codes, 16, "dot", scale)
    assert np.array_equal(idx, want_i) and np.array_equal(sc.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(np.take_along_axis(sc, np.argsort(idx, axis=1), axis=1).T.astype(np.float64),
                          fp8_to_f64(codes) * scale.astype(np.float64)[:, None])


def test_ties_and_two_launches():
    r = R()
    q32, codes, scale = random_case(2 * r + 3, 144, 3)
    where = [163, r + 81, 2 * r + 2]                                 # waves 2, 1, 0 and tiles 2, 1, 0 of chunks 0, 1, 2
    codes[where], scale[where] = codes[163], 2.0 ** -1
    q32[1] = fp8_to_f64(codes[163]).astype(np.float32)                # the three copies are query 1's best match
    S, E = reference(q32, codes, scale)
    a, b = launch(q32, codes, scale, 5), launch(q32, codes, scale, 5)
    assert a[0][1, :3].tolist() == where and len(set(a[1][1, :3].view(np.uint32).tolist())) == 1
    check_rows(*a, S, E, "fp8 ties")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("bad", [dict(F=24), dict(g8=("+", 8)), dict(ldg=56), dict(scale=None)])
def test_refusals_launch_nothing(bad):
    q32, codes, scale = random_case(40, 48, 4)
    launch(q32, np.concatenate([codes, codes], axis=1)[:, :64], scale, 5, bad=bad)


# ------------------------------------------------------------------------------------ engine, server
def test_engine_rows_follow_its_own_features(xparams):
    from kdl.engine import registry
    from kdl.engine.base import Similar, unpack_topk
    info = registry.get("xception")
    x = torch.randint(0, 256, (2, 299, 299, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    codes, scale = quantize_fp8(np.random.default_rng(3).standard_normal((1000, info.features)))
    sim = Similar(torch.from_numpy(codes).cuda(), 5, "cosine", torch.from_numpy(scale).cuda())
    eng = info.engine(xparams, 2, "cuda", similar=sim)
    rows = eng.forward(x).cpu().numpy()
    S, E = reference(eng.feature_slot(0)[:2].cpu().numpy(), codes, scale)
    check_rows(*unpack_topk(rows), S, E, "fp8 engine")
    assert torch.equal(eng.last_logits(0)[:2], info.engine(xparams, 2, "cuda", similar=None).forward(x))
    with pytest.raises(ValueError):
        info.engine(xparams, 2, "cuda", similar=Similar(sim.gallery, 5, "cosine", sim.scale[:-1].contiguous()))


def test_server_three_signatures_agree(tmp_path):
    """A synthetic "dtype": "fp8" version: 299 x 299 pixels (nothing to resize) through similar and similar_image and
    as PNG files through similar_bytes give one answer; its ids are the rule's on the server's own embed rows at
    every rank that the reference decides by more than E[b, j] on either side."""
    import io

    import grpc
    from PIL import Image

    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.embed import l2_rule
    from kdl.serving.server import ModelServer
    F, K = 2048, 5
    base = tmp_path / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text(json.dumps({"seed": 0, "similar": {"top_k": K, "dtype": "fp8"}}))
    np.save(base / "1" / "gallery.npy", np.random.default_rng(40).standard_normal((40, F)).astype(np.float32))
    u8, png = np.random.default_rng(2).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8), [io.BytesIO(), io.BytesIO()]
    for im, b in zip(u8, png):
        Image.fromarray(im).save(b, "PNG")
    srv = ModelServer(ServerConfig(
        port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1, host="127.0.0.1",
        file_system_poll_wait_seconds=0, batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000,
                                                                 allowed_batch_sizes=[2]))).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            ask = lambda X, sig, key="images": PredictionStub(ch).Predict(
                make_request(X, signature=sig, input_key=key), timeout=120).outputs
            got = {sig: ask(u8, sig) for sig in ("similar", "similar_image", "embed")}
            got["similar_bytes"] = ask([b.getvalue() for b in png], "similar_bytes", "image_bytes")
        for sig in ("similar_image", "similar_bytes"):
            assert got[sig]["ids"].string_val == got["similar"]["ids"].string_val
            assert list(got[sig]["scores"].float_val) == list(got["similar"]["scores"].float_val)
        src = srv.manager.get("clothing-model", None, None).source
        assert src.similar_dtype == "fp8" and src.gallery.dtype == np.uint8
        rows = np.asarray(got["embed"]["embedding"].float_val, np.float32).reshape(2, F)
        S, E = reference(l2_rule(rows), src.gallery, src.gallery_scale)
        order = similar_rule(rows, src.gallery, K + 1, "cosine", src.gallery_scale)[0].astype(np.int64)
        s, e = np.take_along_axis(S, order, axis=1), np.take_along_axis(E, order, axis=1)
        gap = s[:, :-1] - e[:, :-1] > s[:, 1:] + e[:, 1:]               # rank k lies clear of rank k + 1
        sure = gap & np.concatenate([gap[:, :1] | True, gap[:, :-1]], axis=1)
        ids = np.array([int(v) for v in got["similar"]["ids"].string_val]).reshape(2, K)
        assert sure.any() and np.array_equal(ids[sure], order[:, :K][sure])
    finally:
        srv.stop(0)
