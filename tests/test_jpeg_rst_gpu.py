"""Restart intervals in the entropy decode of serving_bytes on the MI355X: jpeg_huff_rst_decode +
jpeg_dc_rst_scan, one workgroup per (image, group of intervals), fill the coefficient planes with
exactly what the host decoder (jpeg_parse) writes, alone and batched, write nothing outside them,
take the rounds the emulation predicts, report rejected scans through the error word and leave the
stream usable; the launchers refuse descriptors and tables outside the buffers;
BytesRunner(entropy="gpu_rst") and a GPU server with jpeg_entropy="gpu_rst" give the rows and logits
of the host path for plain and restart files in one request."""
import types

import grpc
import numpy as np
import pytest
import torch

from _jpeg_cases import encode, pants, smooth_noise
from _jpeg_huff_cases import oracle, pants_file, small_files
from _jpeg_rst_cases import (corrupted_rst_files, count_intervals, emulate, large_rst_files, prepare_files,
                             small_rst_files)
from kdl.gateway import preprocess as pp
from kdl.gateway.client import PredictionStub, make_request
from kdl.serving.config import BatchingParams, ServerConfig
from kdl.serving.server import ModelServer

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
SPARE = 64            # int16 behind each image's planes that nobody may touch


def gpu_rst_entropy(files, slots=None, n_slots=None, spare=SPARE, edit=None, change=None):
    """One decode call of restart files: ``files[k]`` into coefficient slot ``slots[k]`` of ``n_slots``
    (the others are nobody's) of a buffer that starts as SENTINEL. ``edit(words of descriptor k,
    staging, layout, info k)`` changes what is staged, ``change`` the launch arguments.
    -> (coefficient buffer, status [n, 2] in the order of ``files``, layout, headers, infos, args)"""
    from kdl.ops import _lib
    from kdl.serving.jpeg import CallLayout
    rt, C = _lib.rt(), _lib.lib()
    slots = list(range(len(files))) if slots is None else slots
    n_slots = len(files) if n_slots is None else n_slots
    sizes, bounds = [1024 + spare] * n_slots, [rt.jpeg_prepare_bound(0)] * n_slots
    for k, d in enumerate(files):
        st, hd = rt.jpeg_probe(d)
        assert st == rt.JPEG_OK, hd.why
        sizes[slots[k]] = hd.ncoef + spare
        bounds[slots[k]] = rt.jpeg_prepare_bound(len(d), count_intervals(rt, d))
    lay = CallLayout(sizes, bounds)
    hin = np.zeros(lay.nbytes, np.uint8)
    heads, infos = [], []
    for k, d in enumerate(files):
        st, hd, info = rt.jpeg_scan_prepare(d, lay.prep(hin, slots[k]))
        assert st == rt.JPEG_OK and info.restart_ok and not info.device_ok, hd.why
        lay.add_huff(hin, slots[k], hd, info)
        heads.append(hd)
        infos.append(info)
    n, D = len(files), lay.huff_bytes
    assert (lay.n_huff, lay.n_rst) == (0, n)
    where = [lay.off_huff + (lay.n_slots - 1 - k) * D for k in range(n)]     # restart descriptors fill from the back
    if edit is not None:
        for k in range(n):
            edit(hin[where[k]:where[k] + D].view(np.uint32), hin, lay, infos[k])
    d_in = torch.from_numpy(hin).cuda()
    coef = torch.full((lay.ncoef,), SENTINEL, dtype=torch.int16, device="cuda")
    status = torch.full((2 * n + 2,), -1, dtype=torch.int32, device="cuda")
    args = lay.huff_rst_args(hin.ctypes.data, d_in.data_ptr(), coef.data_ptr(), status.data_ptr(), 2 * n)
    args.update(change or {})
    args["keep"] = (hin, d_in, coef, status)                # h_desc and h_stage are addresses inside hin
    s = torch.cuda.current_stream().cuda_stream
    C.jpeg_huff_rst_decode(args, s)
    C.jpeg_dc_rst_scan(args, s)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert (st[2 * n:] == -1).all()                         # the words behind the call's range
    return coef.cpu().numpy(), st[:2 * n].reshape(n, 2)[::-1], lay, heads, infos, args


def expected(lay, files, slots):
    """The whole coefficient buffer: jpeg_parse's planes in their slots, SENTINEL everywhere else."""
    from kdl.ops import _lib
    want = np.full(lay.ncoef, SENTINEL, np.int16)
    for k, d in enumerate(files):
        st, hd, coef = oracle(_lib.rt(), d)
        assert st == _lib.rt().JPEG_OK
        want[lay.coef_at[slots[k]]:lay.coef_at[slots[k]] + hd.ncoef] = coef
    return want


ALL = {**prepare_files(), **small_rst_files(), **large_rst_files()}


@pytest.mark.parametrize("case", list(ALL))
def test_kernels_equal_the_host_decoder(case):
    from kdl.ops import _lib
    data = ALL[case]
    coef, status, lay, heads, _, _ = gpu_rst_entropy([data])
    assert status[0, 0] == 0
    want = expected(lay, [data], [0])
    assert np.array_equal(coef, want)                       # the planes, and the sentinels behind them
    assert (want[heads[0].ncoef:heads[0].ncoef + SPARE] == SENTINEL).all()
    assert int(status[0, 1]) == emulate(_lib.rt(), data)[1]         # the rounds the emulation predicts


def test_one_call_with_several_files():
    """Four files of different sampling and restart interval -- one of them the file of two 40 KB
    intervals, each longer than a chunk -- into slots 3, 0, 2, 5 of 6; slots 1 and 4 are nobody's."""
    from kdl.ops import _lib
    rt = _lib.rt()
    files = [small_rst_files()["17x9 4:2:0 blocks=2"], large_rst_files()["noise rows=25"],
             small_rst_files()["64x64 grey rows=1 optimised"], prepare_files()["blocks=3"]]
    slots = [3, 0, 2, 5]
    coef, status, lay, heads, infos, _ = gpu_rst_entropy(files, slots, 6)
    assert len({(i.ri, i.nb) for i in infos}) == 4
    assert max(i.nbits for i in infos) > 2 * rt.JPEG_HUFF_SUB_BITS * rt.JPEG_HUFF_CHUNK
    assert (status[:, 0] == 0).all()
    assert np.array_equal(coef, expected(lay, files, slots))
    for empty in (1, 4):
        assert (coef[lay.coef_at[empty]:lay.coef_at[empty + 1]] == SENTINEL).all()
    assert [int(r) for r in status[:, 1]] == [emulate(rt, d)[1] for d in files]


def test_bad_scans_set_the_error_word_and_the_stream_goes_on():
    from kdl.ops import _lib
    rt = _lib.rt()
    bad = list(corrupted_rst_files())
    for d in bad:                                           # the same bytes passed the host emulation first
        err, _, viol, _, _ = emulate(rt, d)
        assert err != 0 and viol == 0 and oracle(rt, d)[0] == rt.JPEG_MALFORMED
    coef, status, lay, heads, _, _ = gpu_rst_entropy(bad)
    assert (status[:, 0] != 0).all()
    inside = np.zeros(lay.ncoef, bool)
    for k, hd in enumerate(heads):
        inside[lay.coef_at[k]:lay.coef_at[k] + hd.ncoef] = True
    assert (coef[~inside] == SENTINEL).all()
    good = small_rst_files()["33x47 4:2:2 blocks=2"]
    coef, status, lay, _, _, _ = gpu_rst_entropy([good])
    assert status[0, 0] == 0 and np.array_equal(coef, expected(lay, [good], [0]))


def test_launchers_reject_descriptors_and_tables_outside_the_buffers():
    """The five restart fields are the descriptor's last words: ri, nint, ngroup, int_off, grp_off."""
    from kdl.ops import _lib
    C, rt = _lib.lib(), _lib.rt()
    data = large_rst_files()["pants blocks=4"]               # several groups
    _, _, lay, heads, infos, args = gpu_rst_entropy([data], spare=0)
    info, s = infos[0], torch.cuda.current_stream().cuda_stream
    base = lay.prep_at[0]
    assert info.ngroup > 1 and args["coef_cap"] == heads[0].ncoef

    def field(at, value):
        def edit(words, hin, lay, info):
            words[at] = value
        return edit

    def table(at, value):
        def edit(words, hin, lay, info):
            hin[base + at:base + at + 4].view(np.uint32)[0] = value
        return edit

    def one_group(words, hin, lay, info):
        words[-3] = 1
        hin[base + info.grp_off:base + info.grp_off + 8].view(np.uint32)[:] = (0, info.nint)
    hin = args["keep"][0]
    iv = hin[base + info.int_off:base + info.int_off + 16].view(np.uint32)
    refused = [dict(edit=field(-2, lay.nbytes)),                                          # table offset past the staging
               dict(edit=table(info.int_off + 8 * (info.nint - 1), info.scan_bytes // 4)),  # interval words past the scan
               dict(edit=table(info.int_off + 4, 32 * int(iv[2] - iv[0]) + 1)),           # interval bits > 32 x words
               dict(edit=field(-5, 0)),                                                    # Ri = 0
               dict(edit=field(-4, info.nint + 1)),                                        # wrong interval count
               dict(edit=one_group),                                                       # a group over the rule
               dict(change=dict(h_stage=None)),
               dict(change=dict(stage_cap=base + info.grp_off + 8 * info.ngroup - 4)),
               dict(change=dict(coef_cap=args["coef_cap"] - 64)),
               dict(change=dict(status_cap=1))]
    for kw in refused:
        with pytest.raises(RuntimeError):
            gpu_rst_entropy([data], spare=0, **kw)
    for fn in (C.jpeg_huff_rst_decode, C.jpeg_dc_rst_scan):  # each launcher checks for itself
        with pytest.raises(RuntimeError):
            fn({**args, "coef_cap": args["coef_cap"] - 64}, s)
        with pytest.raises(RuntimeError):
            fn({**args, "h_stage": None}, s)
    # each launcher takes its own kind of file
    for fn in (C.jpeg_huff_decode, C.jpeg_dc_scan):
        with pytest.raises(RuntimeError):
            fn(args, s)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ the bytes runner
def _runner(spec=None, size=299):
    from kdl.serving.jpeg import BytesRunner
    inner = types.SimpleNamespace(source=types.SimpleNamespace(input_size=size, preprocess=pp.NEAREST_SPEC),
                                  takes_device_items=lambda: False)
    return BytesRunner(None, inner, [0], spec=spec, entropy="gpu_rst")


def _entropy_counts():
    from kdl.serving.metrics import METRICS
    c = METRICS.snapshot()["counters"]
    return {w: c.get(f"kdl_jpeg_entropy_total{{where={w}}}", 0) for w in ("gpu", "host", "retry")}


def test_bytes_runner_decodes_plain_and_restart_files_in_one_request():
    files = [pants_file(), large_rst_files()["pants rows=1"],
             encode(smooth_noise(200, 120, 3), quality=85, progressive=True)]
    before = _entropy_counts()
    rows = _runner().decode(files)
    for row, d in zip(rows, files):
        assert np.array_equal(row, pp.to_uint8(pp.load_image(d), (299, 299)))
    # Resize(256) + CenterCrop needs a model input of at most 256: a 224 x 224 one
    spec = pp.ResizeSpec.parse("bilinear:256", 224)
    files = [small_files()["33x47 4:2:2"], files[2], prepare_files()["blocks=3"]]
    rows = _runner(spec, 224).decode(files)
    for row, d in zip(rows, files):
        assert np.array_equal(row, pp.apply_spec_pil(pp.load_image(d), spec, 224))
    after = _entropy_counts()
    assert after["gpu"] - before["gpu"] == 4 and after["host"] == before["host"] and after["retry"] == before["retry"]


def test_requests_that_are_the_host_decoders_stay_so():
    """Under ``gpu`` a restart file still sends its request to the host -- also one with so many
    intervals that the plain bound of the prepared buffer is too small for it -- and under ``gpu_rst``
    a file whose markers are out of order does, with the host decoder's answer."""
    from kdl.serving.jpeg import BytesRunner
    from _jpeg_rst_cases import marker_damage
    inner = types.SimpleNamespace(source=types.SimpleNamespace(input_size=299, preprocess=pp.NEAREST_SPEC),
                                  takes_device_items=lambda: False)
    many = prepare_files()["blocks=1"]
    before = _entropy_counts()
    rows = BytesRunner(None, inner, [0], entropy="gpu").decode([pants_file(), many])
    for row, d in zip(rows, [pants_file(), many]):
        assert np.array_equal(row, pp.to_uint8(pp.load_image(d), (299, 299)))
    after = _entropy_counts()
    assert (after["gpu"], after["host"], after["retry"]) == (before["gpu"], before["host"] + 2, before["retry"])
    swapped = marker_damage(prepare_files()["blocks=3"])["swapped"]
    with pytest.raises(Exception) as e:
        _runner().decode([many, swapped])
    assert "image 1: malformed JPEG (restart marker missing)" in str(e.value)
    assert _entropy_counts() == {"gpu": after["gpu"], "host": after["host"] + 2, "retry": after["retry"]}


# ------------------------------------------------------------------------------ the GPU server
@pytest.fixture(scope="module")
def gpu_server(tmp_path_factory):
    base = tmp_path_factory.mktemp("m") / "clothing-model"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text('{"seed": 0}')
    cfg = ServerConfig(port=0, rest_api_port=0, model_base_path=str(base), device="gpu", gpus=1,
                       host="127.0.0.1", file_system_poll_wait_seconds=0, jpeg_entropy="gpu_rst",
                       batching=BatchingParams(max_batch_size=8, batch_timeout_micros=1000,
                                               allowed_batch_sizes=[1, 2, 4, 8]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    yield srv
    srv.stop(0)


def test_gpu_server_with_restart_files_on_the_device(gpu_server):
    """serving_bytes with restart files decoded on the GPU gives the logits of serving_image for the
    PIL-decoded pixels; a corrupted restart file is rejected with the host path's message after the
    retry, and the server serves on."""
    from kdl.ops import _lib
    rt = _lib.rt()
    stub = PredictionStub(grpc.insecure_channel(f"127.0.0.1:{gpu_server.grpc_port}"))
    a = pants(534, 400)
    before = _entropy_counts()

    def same_logits(files):
        n = len(files)
        px = np.stack([np.asarray(pp.load_image(d), np.uint8) for d in files])
        r1 = stub.Predict(make_request(files, signature="serving_bytes", input_key="image_bytes"), timeout=60)
        r2 = stub.Predict(make_request(px, signature="serving_image", input_key="images"), timeout=60)
        got = np.asarray(r1.outputs["dense_7"].float_val, np.float32)
        assert got.size == 10 * n and np.array_equal(got, np.asarray(r2.outputs["dense_7"].float_val, np.float32))
    same_logits([large_rst_files()["pants blocks=4"]])
    same_logits([encode(a, quality=90, subsampling=2), large_rst_files()["pants rows=1"]])
    r = gpu_server.manager.get("clothing-model", None, None).runner("serving_bytes")
    assert r.entropy == "gpu_rst" and r.gpu and r.device_path
    assert _entropy_counts() == {"gpu": before["gpu"] + 3, "host": before["host"], "retry": before["retry"]}
    cut = corrupted_rst_files()[0]
    st, hd, _ = oracle(rt, cut)
    assert st == rt.JPEG_MALFORMED
    with pytest.raises(grpc.RpcError) as e:
        stub.Predict(make_request([cut], signature="serving_bytes", input_key="image_bytes"), timeout=60)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert e.value.details() == f"image 0: malformed JPEG ({hd.why})"
    assert _entropy_counts() == {"gpu": before["gpu"] + 4, "host": before["host"], "retry": before["retry"] + 1}
    same_logits([large_rst_files()["pants blocks=4"]])      # the context serves on after the retry
    assert gpu_server.manager.get("clothing-model", None, None).device_alive()
