"""gallery_ivf_topk (kernels/similar_ivf.hip) alone with the probes given, as an engine's last step
behind the coarse gallery_topk, and behind the server. The reference is test_similar_gpu's float64
(S, E) with every row outside the probed lists set to S = -inf, E = 0, through its ``check_rows``
unchanged: the bound is launch.h's (F + 16) * 2^-23 * sum |q||g|, a returned non-candidate fails it,
and places past the candidates must be exactly (-1, -inf)."""
import json

import numpy as np
import pytest
import torch

from kdl.serving.similar import chunk_table, ivf_rule, load_gallery, load_ivf
from test_similar_gpu import NAN_BF16, SENTINEL, C, R, bf16_bits, bits64, check_rows, reference

pytestmark = pytest.mark.gpu


def case(F: int, B: int, seed: int = 0):
    """fp32 queries, bf16 rows stored list by list (list 4 is 64 times larger: it wins wherever it is
    wrongly scanned) and the list offsets."""
    g, r = torch.Generator().manual_seed(7 * F + B + seed), R()
    offsets = np.concatenate([[0], np.cumsum([0, 1, 15, 17, r - 1, r, r + 1, 2 * r + 3])]).astype(np.int32)   # empty .. three chunks
    rows = torch.randn((int(offsets[-1]), F), generator=g)
    rows[offsets[4]:offsets[5]] *= 64
    return torch.randn((B, F), generator=g).numpy(), bf16_bits(rows), offsets


def probes(pattern: str, B: int, P: int) -> np.ndarray:
    b = np.arange(B)[:, None]
    if pattern == "same":                                          # a full mask: the two-tile path
        return np.broadcast_to(np.array([7, 4, 0])[:P], (B, P)).astype(np.int32)
    if pattern == "own":                                           # masks of few bits; lists nobody probes
        return ((b + np.array([0, 3, 5])[:P]) % 8).astype(np.int32)
    assert pattern == "tile" and P == 3                            # list 5: 16 queries of a pass, list 6: 17
    return np.concatenate([np.where(b % 32 < 16, 5, 1), np.where((b % 32 >= 10) & (b % 32 < 27), 6, 2), 0 * b], axis=1).astype(np.int32)


def launch(q32, gbits, offsets, probe, K, padded=False, bad=None):
    """One call through the direct binding -> (positions [B, K], scores [B, K]); tails as in test_similar_gpu.launch.
    With ``bad`` the call must be refused and nothing written."""
    lib, (B, F), N, L, P = C(), q32.shape, gbits.shape[0], len(offsets) - 1, probe.shape[1]
    qp, gp = q32, gbits
    if padded:
        qp, gp = np.full((B, F + 3), np.nan, np.float32), np.full((N, F + 8), NAN_BF16, np.uint16)
        qp[:, :F], gp[:, :F] = q32, gbits
    q, g = torch.from_numpy(np.ascontiguousarray(qp)).cuda(), torch.from_numpy(np.ascontiguousarray(gp).view(np.int16)).cuda()
    pr = torch.full((B, P + 2), -7, dtype=torch.int32).cuda()     # ldp > P; ids out of range past P
    pr[:, :P] = torch.from_numpy(probe).cuda()
    tab = torch.from_numpy(chunk_table(offsets)).cuda()
    out = torch.full((B + 1, 2 * K), SENTINEL, dtype=torch.int32, device="cuda")
    nw = lib.gallery_ivf_workspace(B, K, L, tab.shape[0])
    assert nw > 0
    work = torch.full((nw + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    a = dict(q=q.data_ptr(), g=g.data_ptr(), out=out.data_ptr(), work=work.data_ptr(), B=B, N=N, F=F, K=K, ldq=q.shape[1],
             ldg=g.shape[1], probe=pr.data_ptr(), table=tab.data_ptr(), L=L, P=P, C=tab.shape[0], ldp=P + 2)
    if bad:
        with pytest.raises(RuntimeError):
            lib.gallery_ivf_topk({**a, **{k: a[k] + v[1] if isinstance(v, tuple) else v for k, v in bad.items()}},
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((work == 0xA5).all())
        return None
    lib.gallery_ivf_topk(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[B] == SENTINEL).all() and bool((work[nw:] == 0xA5).all()), "words past the output or the workspace were written"
    return o[:B, :K].copy(), o[:B, K:].copy().view(np.float32)


def check(idx, sc, q32, gbits, offsets, probe, what) -> None:
    S, E = reference(q32, gbits)
    list_of = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    for b in range(len(q32)):
        cand = np.isin(list_of, probe[b])
        n = min(idx.shape[1], int(cand.sum()))
        assert (idx[b, n:] == -1).all() and np.isneginf(sc[b, n:]).all(), (what, b, idx[b], sc[b])
        if n:
            check_rows(idx[b:b + 1, :n], sc[b:b + 1, :n], np.where(cand, S[b:b + 1], -np.inf), np.where(cand, E[b:b + 1], 0), what)


@pytest.mark.parametrize("pattern,B,P,F,K", [("same", 33, 1, 48, 5), ("same", 17, 3, 8, 32), ("same", 1, 3, 2048, 1),
                                             ("own", 33, 3, 2048, 5), ("own", 17, 1, 8, 5), ("own", 1, 1, 48, 1),
                                             ("tile", 33, 3, 48, 5), ("tile", 33, 3, 2048, 32)])
def test_scan_with_given_probes(pattern, B, P, F, K):
    q32, gbits, offsets = case(F, B)
    probe = probes(pattern, B, P)
    for padded in (False, True):
        idx, sc = launch(q32, gbits, offsets, probe, K, padded)
        check(idx, sc, q32, gbits, offsets, probe, f"{pattern} B={B} P={P} F={F} K={K} padded={int(padded)}")


def test_fewer_candidates_than_k_and_ties():
    q32, gbits, offsets = case(72, 3)
    row = bf16_bits(torch.randn(72, generator=torch.Generator().manual_seed(9)))
    where = [int(offsets[2]), int(offsets[7]) + 3, int(offsets[7]) + R() + 1]    # two lists, two chunks of list 7
    gbits[where] = row
    q32[1] = 4.0 * bits64(row).astype(np.float32)                                # the copies are query 1's best match
    probe = np.array([[0, 1], [2, 7], [1, 0]], np.int32)
    idx, sc = launch(q32, gbits, offsets, probe, 5)
    check(idx, sc, q32, gbits, offsets, probe, "short and ties")
    assert idx[0].tolist() == [0, -1, -1, -1, -1] and idx[2].tolist() == idx[0].tolist()    # lists 0 and 1 hold one row
    assert idx[1, :3].tolist() == where and len(set(sc[1, :3].view(np.uint32).tolist())) == 1
    again = launch(q32, gbits, offsets, probe, 5)
    assert np.array_equal(idx, again[0]) and np.array_equal(sc.view(np.uint32), again[1].view(np.uint32))


@pytest.mark.parametrize("bad", [dict(P=33), dict(P=9), dict(g=("+", 8)), dict(F=12), dict(probe=None), dict(C=0)])
def test_refusals_launch_nothing(bad):
    q32, gbits, offsets = case(48, 4)
    launch(q32, gbits, offsets, np.zeros((4, bad.get("P", 3)), np.int32), 5, bad=bad)


SEED = 3           # of the engine test's centroids: the one kept (its coarse gap is asserted below)


def _indexed(tmp_path, n, lists, seed, F=2048):
    rng = np.random.default_rng(seed)
    gal, cen = rng.standard_normal((n, F)).astype(np.float32), rng.standard_normal((lists, F)).astype(np.float32)
    np.save(tmp_path / "gallery.npy", gal)
    np.save(tmp_path / "gallery_centroids.npy", cen)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    np.save(tmp_path / "gallery_lists.npy", np.argmax(unit(gal) @ unit(cen).T, axis=1).astype(np.int32))
    cbits, offsets, order = load_ivf(tmp_path / "gallery_centroids.npy", tmp_path / "gallery_lists.npy", n, F)
    return load_gallery(tmp_path / "gallery.npy", F)[order], cbits, offsets


def test_engine_probes_then_scans(xparams, tmp_path):
    from kdl.engine import registry
    from kdl.engine.base import Ivf, Similar, unpack_topk
    info, nprobe = registry.get("xception"), 2
    gbits, cbits, offsets = _indexed(tmp_path, 1000, 8, SEED)
    dev = lambda bits: torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    ivf = Ivf(dev(cbits), torch.from_numpy(chunk_table(offsets)).cuda(), torch.from_numpy(offsets), nprobe)
    eng = info.engine(xparams, 2, "cuda", similar=Similar(dev(gbits), 5, "cosine", None, ivf))
    x = torch.randint(0, 256, (2, 299, 299, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    eager = eng.forward(x, capture=False).cpu().numpy()
    for _ in range(3):                                             # replays of the captured program
        assert np.array_equal(eng.forward(x, capture=True).cpu().numpy().view(np.uint32), eager.view(np.uint32))
    q32 = eng.feature_slot(0)[:2].cpu().numpy()
    Sc, Ec = reference(q32, cbits)
    order = np.argsort(-Sc, axis=1, kind="stable")
    s, e = np.take_along_axis(Sc, order, axis=1), np.take_along_axis(Ec, order, axis=1)
    print(f"seed {SEED}: coarse gap at the probe boundary {s[:, nprobe - 1] - s[:, nprobe]}, bounds {e[:, nprobe - 1] + e[:, nprobe]}")
    assert (s[:, nprobe - 1] - s[:, nprobe] > e[:, nprobe - 1] + e[:, nprobe]).all()     # the probed set is certain
    check(*unpack_topk(eager), q32, gbits, offsets, order[:, :nprobe], "engine")
    assert torch.equal(eng.last_logits(0)[:2], info.engine(xparams, 2, "cuda").forward(x))
    with pytest.raises(ValueError):
        info.engine(xparams, 2, "cuda", similar=Similar(dev(gbits), 5, "cosine", None, Ivf(ivf.centroids, ivf.chunk_table[:-1].contiguous(), ivf.offsets, 2)))


def test_server_three_signatures_agree(tmp_path):
    import io

    import grpc
    from PIL import Image

    from kdl.gateway.client import PredictionStub, make_request
    from kdl.serving.backend import load_version_dir
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.embed import l2_rule
    from kdl.serving.server import ModelServer
    K, d = 5, tmp_path / "clothing-model" / "1"
    d.mkdir(parents=True)
    _indexed(d, 200, 4, 40)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, "similar": {"top_k": K, "index": "ivf", "nprobe": 2, "dtype": "fp8"}}))
    with pytest.raises(ValueError, match=r"gallery_centroids\.npy"):
        load_version_dir(d, synthetic=True)
    (d / "synthetic.json").write_text(json.dumps({"seed": 0, "similar": {"top_k": K, "index": "ivf", "nprobe": 2}}))
    u8, png = np.random.default_rng(2).integers(0, 256, (2, 299, 299, 3), dtype=np.uint8), [io.BytesIO(), io.BytesIO()]
    for im, b in zip(u8, png):
        Image.fromarray(im).save(b, "PNG")
    srv = ModelServer(ServerConfig(
        port=0, rest_api_port=0, model_base_path=str(d.parent), device="gpu", gpus=1, host="127.0.0.1",
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
        ivf = src.gallery_ivf
        rows = np.asarray(got["embed"]["embedding"].float_val, np.float32).reshape(2, 2048)
        S, E = reference(l2_rule(rows), src.gallery)
        order = ivf_rule(rows, ivf.centroids, src.gallery, ivf.offsets, K + 1, 2, "cosine")[0].astype(np.int64)
        assert (order >= 0).all()
        s, e = np.take_along_axis(S, order, axis=1), np.take_along_axis(E, order, axis=1)
        gap = s[:, :-1] - e[:, :-1] > s[:, 1:] + e[:, 1:]               # rank k lies clear of rank k + 1
        sure = gap & np.concatenate([gap[:, :1] | True, gap[:, :-1]], axis=1)
        ids = np.array(got["similar"]["ids"].string_val).reshape(2, K)
        want = np.array([i.encode() for i in src.gallery_ids])[order[:, :K]]
        assert sure.any() and np.array_equal(ids[sure], want[sure])
    finally:
        srv.stop(0)
