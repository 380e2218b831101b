"""The entropy decode of serving_bytes on the MI355X: jpeg_huff_decode + jpeg_dc_scan fill the
coefficient planes with exactly what the host decoder (jpeg_parse) writes, alone and batched,
write nothing outside them, report rejected scans through the error word and leave the stream
usable; the launchers refuse descriptors outside the buffers; BytesRunner(entropy="gpu") and a
GPU server with jpeg_entropy="gpu" give the rows and logits of the host path."""
import types

import grpc
import numpy as np
import pytest
import torch

from _jpeg_cases import encode, pants, smooth_noise
from _jpeg_huff_cases import (corrupted_files, emulate, noise_file, oracle, pants_file, small_files,
                              truncated_pants)
from kdl.gateway import preprocess as pp
from kdl.gateway.client import PredictionStub, make_request
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
SPARE = 64            # int16 behind each image's planes that nobody may touch


def gpu_entropy(files, slots=None, n_slots=None, spare=SPARE, edit=None, change=None):
    """One decode call: ``files[k]`` into coefficient slot ``slots[k]`` of ``n_slots`` (the others
    are nobody's) of a buffer that starts as SENTINEL. ``edit(words of descriptor k, lay)`` changes
    the staged descriptors, ``change`` the launch arguments.
    -> (coefficient buffer, status [n, 2], layout, headers, infos, args)"""
    from kdl.ops import _lib
    from kdl.serving.jpeg import CallLayout
    rt, C = _lib.rt(), _lib.lib()
    slots = list(range(len(files))) if slots is None else slots
    n_slots = len(files) if n_slots is None else n_slots
    sizes, bounds = [1024 + spare] * n_slots, [rt.jpeg_prepare_bound(0)] * n_slots
    for k, d in enumerate(files):
        st, hd = rt.jpeg_probe(d)
        assert st == rt.JPEG_OK, hd.why
        sizes[slots[k]], bounds[slots[k]] = hd.ncoef + spare, rt.jpeg_prepare_bound(len(d))
    lay = CallLayout(sizes, bounds)
    hin = np.zeros(lay.nbytes, np.uint8)
    heads, infos = [], []
    for k, d in enumerate(files):
        st, hd, info = rt.jpeg_scan_prepare(d, lay.prep(hin, slots[k]))
        assert st == rt.JPEG_OK and info.device_ok, hd.why
        lay.add_huff(hin, slots[k], hd, info)
        heads.append(hd)
        infos.append(info)
    if edit is not None:
        D = lay.huff_bytes
        for k in range(len(files)):
            edit(hin[lay.off_huff + k * D:lay.off_huff + (k + 1) * D].view(np.uint32), lay)
    d_in = torch.from_numpy(hin).cuda()
    coef = torch.full((lay.ncoef,), SENTINEL, dtype=torch.int16, device="cuda")
    n = len(files)
    status = torch.full((2 * n + 2,), -1, dtype=torch.int32, device="cuda")
    args = lay.huff_args(hin.ctypes.data, d_in.data_ptr(), coef.data_ptr(), status.data_ptr(), 2 * n)
    args.update(change or {})
    args["keep"] = (hin, d_in, coef, status)                # h_desc is the address of hin
    s = torch.cuda.current_stream().cuda_stream
    C.jpeg_huff_decode(args, s)
    C.jpeg_dc_scan(args, s)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert (st[2 * n:] == -1).all()
    return coef.cpu().numpy(), st[:2 * n].reshape(n, 2), lay, heads, infos, args


def expected(lay, files, slots, ok=None):
    """The whole coefficient buffer: jpeg_parse's planes in their slots, SENTINEL everywhere else."""
    from kdl.ops import _lib
    want = np.full(lay.ncoef, SENTINEL, np.int16)
    for k, d in enumerate(files):
        st, hd, coef = oracle(_lib.rt(), d)
        assert st == _lib.rt().JPEG_OK
        want[lay.coef_at[slots[k]]:lay.coef_at[slots[k]] + hd.ncoef] = coef
    return want


ALONE = list(small_files()) + ["pants 534x400"]


@pytest.mark.parametrize("case", ALONE)
def test_kernels_equal_the_host_decoder(case):
    data = pants_file() if case.startswith("pants") else small_files()[case]
    coef, status, lay, heads, _, _ = gpu_entropy([data])
    assert status[0, 0] == 0
    want = expected(lay, [data], [0])
    assert np.array_equal(coef, want)                       # the planes, and the sentinels behind them
    assert (want[heads[0].ncoef:heads[0].ncoef + SPARE] == SENTINEL).all()


def test_one_call_with_several_files():
    """Three files of different sampling and size -- one of them longer than two chunks -- into
    slots 2, 0, 3; slot 1 is nobody's and keeps its sentinels."""
    from kdl.ops import _lib
    rt = _lib.rt()
    files = [small_files()["17x9 4:2:0"], noise_file(), small_files()["64x64 grey optimised"]]
    slots = [2, 0, 3]
    coef, status, lay, heads, infos, _ = gpu_entropy(files, slots, 4)
    assert max(i.nbits for i in infos) > 2 * rt.JPEG_HUFF_SUB_BITS * rt.JPEG_HUFF_CHUNK
    assert (status[:, 0] == 0).all()
    assert np.array_equal(coef, expected(lay, files, slots))
    assert (coef[lay.coef_at[1]:lay.coef_at[2]] == SENTINEL).all()
    # the device took the rounds the emulation predicts
    assert [int(r) for r in status[:, 1]] == [emulate(rt, d)[1] for d in files]
    assert status[:, 1].max() >= 3


def test_bad_scans_set_the_error_word_and_the_stream_goes_on():
    from kdl.ops import _lib
    rt = _lib.rt()
    bad = [truncated_pants(), *corrupted_files()]
    for d in bad:                                           # the same bytes passed the host emulation first
        err, _, viol, _, _ = emulate(rt, d)
        assert err != 0 and viol == 0 and oracle(rt, d)[0] == rt.JPEG_MALFORMED
    coef, status, lay, heads, _, _ = gpu_entropy(bad)
    assert (status[:, 0] != 0).all()
    inside = np.zeros(lay.ncoef, bool)
    for k, hd in enumerate(heads):
        inside[lay.coef_at[k]:lay.coef_at[k] + hd.ncoef] = True
    assert (coef[~inside] == SENTINEL).all()
    good = small_files()["33x47 4:2:2"]
    coef, status, lay, _, _, _ = gpu_entropy([good])
    assert status[0, 0] == 0 and np.array_equal(coef, expected(lay, [good], [0]))


def test_launchers_reject_descriptors_outside_the_buffers():
    from kdl.ops import _lib
    C = _lib.lib()
    data = small_files()["33x47 4:2:2"]
    _, _, lay, heads, infos, args = gpu_entropy([data], spare=0)
    info, s = infos[0], torch.cuda.current_stream().cuda_stream
    assert args["coef_cap"] == heads[0].ncoef

    def field(value, new):
        def edit(words, lay):
            at = np.flatnonzero(words == value)
            assert at.size == 1, (value, at)
            words[at[0]] = new
        return edit
    short = lay.prep_at[0] + info.scan_off + info.scan_bytes - 4                                    # the scan's last word
    refused = [dict(change=dict(stage_cap=short)),
               dict(edit=field(info.nbits, 8 * info.scan_bytes + 1)),
               dict(change=dict(coef_cap=args["coef_cap"] - 64)),
               dict(edit=field(info.nblocks, info.nblocks + 1)),
               dict(edit=field(lay.prep_at[0], lay.nbytes)),                                        # a table offset
               dict(change=dict(status_cap=1))]
    for kw in refused:
        with pytest.raises(RuntimeError):
            gpu_entropy([data], spare=0, **kw)
    for fn in (C.jpeg_huff_decode, C.jpeg_dc_scan):          # each launcher checks for itself
        with pytest.raises(RuntimeError):
            fn({**args, "coef_cap": args["coef_cap"] - 64}, s)
        with pytest.raises(RuntimeError):
            fn({**args, "stage_cap": short}, s)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ the bytes runner
def _runner(spec=None, size=299):
    from kdl.serving.jpeg import BytesRunner
    inner = types.SimpleNamespace(source=types.SimpleNamespace(input_size=size, preprocess=pp.NEAREST_SPEC),
                                  takes_device_items=lambda: False)
    return BytesRunner(None, inner, [0], spec=spec, entropy="gpu")


def _entropy_counts():
    from kdl.serving.metrics import METRICS
    c = METRICS.snapshot()["counters"]
    return {w: c.get(f"kdl_jpeg_entropy_total{{where={w}}}", 0) for w in ("gpu", "host", "retry")}


def test_bytes_runner_decode_equals_pillow():
    data = pants_file()
    before = _entropy_counts()
    rows = _runner().decode([data])
    assert np.array_equal(rows[0], pp.to_uint8(pp.load_image(data), (299, 299)))
    # Resize(256) + CenterCrop needs a model input of at most 256: a 224 x 224 one
    spec = pp.ResizeSpec.parse("bilinear:256", 224)
    files = [data, small_files()["33x47 4:2:2"]]
    rows = _runner(spec, 224).decode(files)
    for row, d in zip(rows, files):
        assert np.array_equal(row, pp.apply_spec_pil(pp.load_image(d), spec, 224))
    after = _entropy_counts()
    assert after["gpu"] - before["gpu"] == 3 and after["host"] == before["host"] and after["retry"] == before["retry"]


# ------------------------------------------------------------------------------ the GPU server
@pytest.fixture(scope="module")
def gpu_server(tmp_path_factory):
    base = tmp_path_factory.mktemp("m") / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text('{"seed": 0}')
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1,
                       host="127.0.0.1", file_system_poll_wait_seconds=0, jpeg_entropy="gpu",
                       batching=BatchingParams(max_batch_size=8, batch_timeout_micros=1000,
                                               allowed_batch_sizes=[1, 2, 4, 8]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    yield srv
    srv.stop(0)


def test_gpu_server_with_device_entropy(gpu_server):
    """serving_bytes with the scans decoded on the GPU gives the logits of serving_image for the
    PIL-decoded pixels; a file with restart intervals goes to the host decoder, a truncated one is
    rejected with the host path's message after the retry."""
    stub = PredictionStub(grpc.insecure_channel(f"127.0.0.1:{gpu_server.grpc_port}"))
    a, b = pants(534, 400), smooth_noise(534, 400, 11)
    before = _entropy_counts()

    def same_logits(files):
        n = len(files)
        px = np.stack([np.asarray(pp.load_image(d), np.uint8) for d in files])
        r1 = stub.Predict(make_request(files, signature="serving_bytes", input_key="image_bytes"), timeout=60)
        r2 = stub.Predict(make_request(px, signature="serving_image", input_key="images"), timeout=60)
        got = np.asarray(r1.outputs["dense_7"].float_val, np.float32)
        assert got.size == 10 * n and np.array_equal(got, np.asarray(r2.outputs["dense_7"].float_val, np.float32))
    for files in ([encode(a, quality=90, subsampling=2), encode(b, quality=75, subsampling=0)],
                  [encode(b, quality=85, subsampling=1), encode(a, quality=90, progressive=True)],
                  [encode(smooth_noise(299, 299, 12), quality=90)]):
        same_logits(files)
    sent = 4                                                # baseline files without restart intervals so far
    r = gpu_server.manager.get("clothing-model", None, None).runner("serving_bytes")
    assert r.entropy == "gpu" and r.gpu and r.device_path
    assert _entropy_counts() == {"gpu": before["gpu"] + sent, "host": before["host"], "retry": before["retry"]}
    same_logits([encode(smooth_noise(150, 130, 9), subsampling=2, quality=80, restart_marker_blocks=3)])
    assert _entropy_counts() == {"gpu": before["gpu"] + sent, "host": before["host"] + 1, "retry": before["retry"]}
    cut = truncated_pants()
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(make_request([cut], signature="serving_bytes", input_key="image_bytes"), timeout=60)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert e.value.details() == "image 0: malformed JPEG (entropy-coded data is truncated)"
    sent += 1
    assert _entropy_counts() == {"gpu": before["gpu"] + sent, "host": before["host"] + 1, "retry": before["retry"] + 1}
    same_logits([encode(a, quality=90, subsampling=2)])     # the context serves on after the retry
    assert gpu_server.manager.get("clothing-model", None, None).device_alive()
