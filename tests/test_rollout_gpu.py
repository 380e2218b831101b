"""attn_rollout / rollout_map (kernels/rollout.hip) alone, inside the ViT engines, against the fp32
rollout oracle, and behind the server.

Reference for the kernels: the definition in float64 torch on the CPU from the same bf16 QKV values,
P = softmax(Q K^T / 8) per head, A^ = (mean_h P + I) / 2, R_l = A^_l R_(l-1). Every layer has its own
random QKV with standard deviation 1.7, so the scores have standard deviation 2.9 and attention is
peaked. The figure compared is the full un-normalised R: max |got - ref| over the row's largest
reference value. fp32 torch on the CPU reads 0.4e-6 to 1.4e-6 on these shapes, a product whose
operands were rounded to bf16 6e-3 to 1.2e-2; the ceiling of 1e-4 is there for the second.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DH = 64
TS = [1, 15, 16, 17, 64, 65, 197, 256]
HS = [1, 3, 12]
BS = [1, 3]
LAYERS = 3
CEILING = 1e-4
# twice the largest figure measured on the device over TS x HS x BS x layers 1..3 x both row strides
# and the 12-layer case: 3.2331e-06 at T 256, H 1, B 3, layer 3 (profiles/rollout.txt; the largest row-sum
# offset there is 1.17e-06). v_exp_f32 and the fp32 chains account for it; bf16 operands would read 6e-3.
R_GATE = 2 * 3.2331e-6
ROWSUM_TOL = 1e-5


# ------------------------------------------------------------------------------------ reference
def make_qkv(L, B, T, H, seed, std=1.7):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((L, B, T, 3 * H * DH), generator=g) * std).to(torch.bfloat16)


def layer_ahat(qkv, H):
    """bf16 [B, T, 3*H*64] -> A^ float64 [B, T, T]."""
    B, T, _ = qkv.shape
    q, k, _ = qkv.double().view(B, T, 3, H, DH).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    return (p.mean(dim=1) + torch.eye(T, dtype=torch.float64)) / 2


def reference(qkvs, H):
    """[L, B, T, 3*H*64] -> list of R_l float64 [B, T, T], l = 1..L."""
    out, r = [], None
    for l in range(qkvs.shape[0]):
        a = layer_ahat(qkvs[l], H)
        r = a if r is None else a @ r
        out.append(r)
    return out


# ------------------------------------------------------------------------------------ launching
def r_buffer(B, T, ldr):
    """One image more than B, NaN everywhere: what the kernel leaves alone stays NaN."""
    return torch.full((B + 1, T, ldr), float("nan"), dtype=torch.float32, device="cuda")


def rollout(qkv_dev, r_in, r_out, B, T, H, Tq=None, ldr=None, over=None):
    from kdl.ops import _lib
    d = dict(qkv=qkv_dev.data_ptr(), r_in=None if r_in is None else r_in.data_ptr(), r_out=r_out.data_ptr(),
             B=B, T=T, Tq=T if Tq is None else Tq, H=H, dh=DH, scale=0.125,
             ldr=r_out.shape[2] if ldr is None else ldr)
    d.update(over or {})
    _lib.lib().attn_rollout(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return r_out


def chain(qkvs, H, ldr):
    """Device R after every layer of a chain, alternating two buffers: list of [B + 1, T, ldr]."""
    L, B, T, _ = qkvs.shape
    dev = qkvs.cuda()
    bufs, out, prev = [r_buffer(B, T, ldr), r_buffer(B, T, ldr)], [], None
    for l in range(L):
        cur = bufs[l & 1]
        rollout(dev[l], prev, cur, B, T, H)
        out.append(cur.clone())
        prev = cur
    return out


def figure(got, ref):
    """max |got - ref| over the row maximum of ref, and the largest |row sum - 1|."""
    g = got.double().cpu()
    err = ((g - ref).abs() / ref.amax(dim=-1, keepdim=True)).max().item()
    return err, (g.sum(dim=-1) - 1).abs().max().item()


def check_chain(T, H, B, ldr, L=LAYERS, seed=0):
    qkvs = make_qkv(L, B, T, H, seed + 1000 * T + 10 * H + B)
    refs = reference(qkvs, H)
    worst = 0.0
    for l, got in enumerate(chain(qkvs, H, ldr)):
        body = got[:B, :, :T]
        assert torch.isfinite(body).all(), (T, H, B, ldr, l)
        assert torch.isnan(got[:B, :, T:]).all() and torch.isnan(got[B]).all(), "padding or the next image written"
        assert (body > 0).all()
        err, rs = figure(body, refs[l])
        print(f"T {T:3d} H {H:2d} B {B} ldr {ldr:3d} layer {l + 1:2d}: error / row max {err:.3e}, row sum off {rs:.3e}")
        assert rs <= ROWSUM_TOL, (T, H, B, ldr, l, rs)
        assert err <= CEILING and err <= R_GATE, (T, H, B, ldr, l, err)
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize("T", TS)
def test_rollout_against_float64(T):
    ld0 = (T + 3) // 4 * 4
    worst = max(check_chain(T, H, B, ldr) for H in HS for B in BS for ldr in (ld0, ld0 + 8))
    print(f"T {T}: largest error / row max {worst:.3e} (gate {R_GATE:.3e}, ceiling {CEILING:.0e})")


def test_twelve_layers():
    worst = check_chain(197, 12, 2, 200, L=12, seed=7)
    print(f"12 layers: largest error / row max {worst:.3e}")


# ------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("T,H", [(17, 3), (197, 12), (256, 1)])
def test_null_r_in_is_the_identity(T, H):
    B, ldr = 2, (T + 3) // 4 * 4 + 4
    qkv = make_qkv(1, B, T, H, 3)[0].cuda()
    eye = r_buffer(B, T, ldr)
    eye[:B, :, :T] = torch.eye(T, device="cuda")
    a = rollout(qkv, None, r_buffer(B, T, ldr), B, T, H)
    b = rollout(qkv, eye, r_buffer(B, T, ldr), B, T, H)
    assert torch.equal(a[:B, :, :T].view(torch.int32), b[:B, :, :T].view(torch.int32))
    assert torch.isnan(b[:B, :, T:]).all() and torch.isnan(b[B]).all()


@pytest.mark.parametrize("T,H", [(1, 1), (17, 3), (197, 12), (256, 12)])
def test_one_query_row_is_row_zero_and_launches_repeat(T, H):
    B, ldr = 3, (T + 3) // 4 * 4
    qkvs = make_qkv(2, B, T, H, 4).cuda()
    r1 = rollout(qkvs[0], None, r_buffer(B, T, ldr), B, T, H)
    full = rollout(qkvs[1], r1, r_buffer(B, T, ldr), B, T, H)
    again = rollout(qkvs[1], r1, r_buffer(B, T, ldr), B, T, H)
    assert torch.equal(full[:B, :, :T].view(torch.int32), again[:B, :, :T].view(torch.int32))
    one = rollout(qkvs[1], r1, r_buffer(B, T, ldr), B, T, H, Tq=1)
    assert torch.equal(one[:B, 0, :T].view(torch.int32), full[:B, 0, :T].view(torch.int32))
    assert torch.isnan(one[:B, 1:]).all() and torch.isnan(one[:B, 0, T:]).all() and torch.isnan(one[B]).all()
    first = rollout(qkvs[0], None, r_buffer(B, T, ldr), B, T, H, Tq=1)       # the null path too
    assert torch.equal(first[:B, 0, :T].view(torch.int32), r1[:B, 0, :T].view(torch.int32))
    assert torch.isnan(first[:B, 1:]).all()
    if T > 20:                                                               # a Tq inside the second tile
        part = rollout(qkvs[1], r1, r_buffer(B, T, ldr), B, T, H, Tq=18)
        assert torch.equal(part[:B, :18, :T].view(torch.int32), full[:B, :18, :T].view(torch.int32))
        assert torch.isnan(part[:B, 18:]).all()


def test_nan_in_the_next_image_does_not_leak():
    B, T, H = 2, 65, 3
    qkv = make_qkv(1, B + 1, T, H, 5)[0]
    qkv[B] = float("nan")
    clean = rollout(qkv[:B].clone().cuda(), None, r_buffer(B, T, 68), B, T, H)
    got = rollout(qkv.cuda(), None, r_buffer(B, T, 68), B, T, H)
    assert torch.isfinite(got[:B, :, :T]).all()
    assert torch.equal(got[:B, :, :T].view(torch.int32), clean[:B, :, :T].view(torch.int32))
    nxt = rollout(qkv.cuda(), clean, r_buffer(B, T, 68), B, T, H)               # r_in's padding and next image are NaN
    assert torch.isfinite(nxt[:B, :, :T]).all()


def make_top(B):
    t = torch.empty((B, 2), dtype=torch.int32)
    t[:, 0] = torch.arange(B, dtype=torch.int32) * 7 + 3
    t[:, 1] = (torch.arange(B, dtype=torch.float32) * 0.125 + 0.25).view(torch.int32)
    return t.view(torch.float32).cuda()


def heat_rows(r, top, B, T, ldo):
    from kdl.ops import _lib
    out = torch.full((B + 1, ldo), float("nan"), dtype=torch.float32, device="cuda")
    d = dict(r=r.data_ptr(), top=top.data_ptr(), out=out.data_ptr(), B=B, T=T, ldr=r.shape[2], ldo=ldo)
    _lib.lib().rollout_map(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", [2, 17, 197, 256])
def test_rollout_map_divides_row_zero_by_its_maximum(T):
    B, ldr, ldo = 3, (T + 3) // 4 * 4 + 4, T + 1 + 3
    r = r_buffer(B, T, ldr)
    r[:B, :, :T] = torch.rand((B, T, T), generator=torch.Generator().manual_seed(T)).cuda() + 0.01
    top = make_top(B)
    out = heat_rows(r, top, B, T, ldo)
    v = r[:B, 0, 1:T].cpu().numpy()
    want = v / v.max(axis=1, keepdims=True)                 # fp32 division: exact agreement
    assert np.array_equal(out[:B, 2:T + 1].cpu().numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(out[:B, :2].view(torch.int32), top.view(torch.int32))
    assert torch.isnan(out[:B, T + 1:]).all() and torch.isnan(out[B]).all()


def test_planted_key_is_the_hottest_patch():
    """K of token j* is aligned with every query in every head and layer: every row attends to j*, so
    row 0 of the rollout peaks there and the map's argmax is patch j* - 1."""
    B, T, H, L, ldr = 2, 197, 12, 3, 200
    g = torch.Generator().manual_seed(9)
    jstar = [57, 140]
    qkvs = (torch.randn((L, B, T, 3, H, DH), generator=g) * 0.5)
    u = torch.randn((H, DH), generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    qkvs[:, :, :, 0] += 4.0 * u
    for b in range(B):
        qkvs[:, b, jstar[b], 1] = 12.0 * u
    dev = qkvs.reshape(L, B, T, 3 * H * DH).to(torch.bfloat16).cuda()
    bufs, prev = [r_buffer(B, T, ldr), r_buffer(B, T, ldr)], None
    for l in range(L):
        rollout(dev[l], prev, bufs[l & 1], B, T, H, Tq=1 if l == L - 1 else T)
        prev = bufs[l & 1]
    out = heat_rows(prev, make_top(B), B, T, T + 1)
    heat = out[:B, 2:].cpu().numpy()
    assert heat.argmax(axis=1).tolist() == [j - 1 for j in jstar]
    assert heat.max(axis=1).tolist() == [1.0, 1.0] and (heat > 0).all()


def test_launcher_refusals_launch_nothing():
    from kdl.ops import _lib
    C = _lib.lib()
    assert C.ROLLOUT_MAX_T == 256
    B, T, H, ldr = 2, 17, 3, 20
    qkv = make_qkv(1, B, T, H, 6)[0].cuda()
    r_in = r_buffer(B, T, ldr)
    r_in[:B, :, :T] = torch.eye(T, device="cuda")
    SENT = 777.0
    out = torch.full((B + 1, T, ldr), SENT, dtype=torch.float32, device="cuda")
    bad = [dict(dh=32), dict(T=257), dict(T=0), dict(H=0), dict(B=0), dict(Tq=0), dict(Tq=T + 1), dict(ldr=T - 1),
           dict(ldr=18), dict(qkv=None), dict(r_out=None), dict(r_in=out.data_ptr())]
    for over in bad:
        with pytest.raises(RuntimeError):
            rollout(qkv, r_in, out, B, T, H, over=over)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), over
    rollout(qkv, r_in, out, B, T, H)                       # the same arguments, unbroken, do write
    assert bool((out[:B, :, :T] != SENT).all()) and bool((out[:B, :, T:] == SENT).all())
    top = make_top(B)
    mbad = [dict(T=1), dict(T=257), dict(B=0), dict(ldr=T - 1), dict(ldr=18), dict(ldo=T), dict(r=None),
            dict(top=None), dict(out=None)]
    for over in mbad:
        rows = torch.full((B + 1, T + 1), SENT, dtype=torch.float32, device="cuda")
        d = dict(r=out.data_ptr(), top=top.data_ptr(), out=rows.data_ptr(), B=B, T=T, ldr=ldr, ldo=T + 1)
        d.update(over)
        with pytest.raises(RuntimeError):
            C.rollout_map(d, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((rows == SENT).all()), over


# ------------------------------------------------------------------------------------ engines
CUT = "encoder.layers.encoder_layer_5.mlp.3"


def _images(seed: int = 5, n: int = 2) -> torch.Tensor:
    return torch.randint(0, 256, (n, 224, 224, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def vparams():
    from kdl.models import vit as V
    return V.init_params(seed=0)


@pytest.fixture(scope="module")
def runs(vparams):
    """Per build (bf16 / fp8), computed once at max_batch 2: a plain engine's logits and step names, a
    topk=1 engine's rows, and a rollout engine's graph and eager rows, logits, rows from a second input
    slot and rows of one image at bucket 1 of 2; then four batches through a stage pipeline."""
    from kdl.engine.stages import StagePipe
    from kdl.engine.vit import ViTEngine
    done = {}

    def get(fp8: bool) -> dict:
        if fp8 in done:
            return done[fp8]
        mk = lambda **kw: ViTEngine(vparams, max_batch=2, device="cuda", fp8=fp8, **kw)   # noqa: E731
        x = _images().cuda()
        e = mk()
        r = dict(plain_logits=e.forward(x), plain_names=[s.name for s in e.steps], plain_bufs=sorted(e.bufs),
                 plain_shape=tuple(e.logits.shape), plain_slots=len(e.logit_slots), plain_rollout=e.rollout)
        del e
        e = mk(topk=1)
        r["top1"] = e.forward(x).cpu().numpy()
        del e
        eng = mk(rollout=True, buckets=[1, 2])
        r["steps"] = [(s.kind, s.name, s.src, s.res, s.dst, s.extra.get("Tq")) for s in eng.steps]
        r["shape"], r["bufs"] = tuple(eng.logits.shape), sorted(eng.bufs)
        r["graph"] = eng.forward(x, capture=True).cpu().numpy()
        r["logits"] = eng.last_logits(0)[:2].clone()
        r["state"] = eng.bufs[eng.steps[-1].src][:2, 0, :197].cpu().numpy()
        r["eager"] = eng.forward(x, capture=False).cpu().numpy()
        r["one"] = eng.forward(x[:1], capture=True).cpu().numpy()          # bucket 1 of 2
        slots = eng.add_input_slots(2)
        slots[1].copy_(x)
        torch.cuda.synchronize()
        eng.launch(2, eng.stream, slot=1)
        eng.stream.synchronize()
        r["slot1"] = eng.slot_logits(1).cpu().numpy()
        r["slot1_logits"] = eng.last_logits(1)[:2].clone()
        r["tunable"] = [s.name for s in eng.conv_steps()]
        del eng
        # four batches on two slots, as test_vit_gpu.py runs the plain pipeline: both parities of the
        # double-buffered R are used twice
        single = mk(rollout=True)
        pipe = StagePipe(mk(rollout=True), CUT)
        r["boundary"], r["ranges"] = list(pipe.boundary), list(pipe.ranges)
        pslots = pipe.add_input_slots(2)
        imgs = [_images(20 + i).cuda() for i in range(4)]
        r["pipe_refs"] = [single.forward(im).cpu().numpy() for im in imgs]
        outs, ev = [], [torch.cuda.Event() for _ in range(2)]
        for i, im in enumerate(imgs):
            j = i % 2
            if i >= 2:
                ev[j].synchronize()
                outs.append(pipe.slot_logits(j).cpu().numpy())
            pslots[j].copy_(im)
            ready = torch.cuda.Event()
            ready.record()
            pipe.launch_async(2, [ready], [ev[j]], slot=j)
        for i in (2, 3):
            ev[i % 2].synchronize()
            outs.append(pipe.slot_logits(i % 2).cpu().numpy())
        r["pipe"] = outs
        del pipe, single
        done[fp8] = r
        return r
    return get


BUILDS = [False, True]


@pytest.mark.parametrize("fp8", BUILDS)
def test_engine_rows_are_the_map_of_its_own_state(fp8, runs):
    from kdl.engine.base import unpack_explain
    r = runs(fp8)
    assert r["shape"] == (2, 198) and r["graph"].shape == (2, 198)
    assert np.array_equal(_bits(r["graph"]), _bits(r["eager"]))
    c, s, heat = unpack_explain(r["graph"], 14, 14)
    v = r["state"][:, 1:]
    assert np.array_equal(_bits(heat.reshape(2, 196)), _bits(v / v.max(axis=1, keepdims=True)))
    assert heat.max(axis=(1, 2)).tolist() == [1.0, 1.0] and heat.min() > 0
    assert abs(r["state"].sum(axis=1) - 1).max() <= ROWSUM_TOL       # row 0 of R_12 still sums to 1


@pytest.mark.parametrize("fp8", BUILDS)
def test_stage_pipeline_rows_are_bit_equal(fp8, runs):
    r = runs(fp8)
    assert "R1" in r["boundary"] and len(r["ranges"]) == 2           # layer 5's R crosses the cut
    for i, (got, want) in enumerate(zip(r["pipe"], r["pipe_refs"])):
        assert np.array_equal(_bits(got), _bits(want)), f"batch {i}"


@pytest.mark.parametrize("fp8", BUILDS)
def test_input_slot_and_bucket_rows_are_bit_equal(fp8, runs):
    r = runs(fp8)
    assert np.array_equal(_bits(r["slot1"]), _bits(r["graph"]))
    assert torch.equal(r["slot1_logits"], r["logits"])
    assert np.array_equal(_bits(r["one"]), _bits(r["graph"][:1]))


@pytest.mark.parametrize("fp8", BUILDS)
def test_class_score_and_logits_are_the_other_engines(fp8, runs):
    r = runs(fp8)
    assert r["top1"].shape == (2, 2) and np.array_equal(_bits(r["graph"][:, :2]), _bits(r["top1"]))
    assert torch.equal(r["logits"], r["plain_logits"])                # the head is untouched, bit for bit


@pytest.mark.parametrize("fp8", BUILDS)
def test_rollout_off_changes_nothing(fp8, runs):
    r = runs(fp8)
    assert r["plain_rollout"] is False and r["plain_slots"] == 0 and r["plain_shape"] == (2, 1000)
    assert "R0" not in r["plain_bufs"] and "R1" not in r["plain_bufs"]
    assert not any("rollout" in n for n in r["plain_names"]) and "top1" not in r["plain_names"]
    names = [s[1] for s in r["steps"]]
    added = [s for s in r["steps"] if s[0] in ("rollout", "top1", "rollout_map")]
    assert [n for n in names if n not in [a[1] for a in added]] == r["plain_names"]
    assert sorted(set(r["bufs"]) - set(r["plain_bufs"])) == ["R0", "R1"]
    roll = [s for s in added if s[0] == "rollout"]
    assert len(roll) == 12 and [a[0] for a in added[12:]] == ["top1", "rollout_map"]
    for i, (kind, name, src, res, dst, tq) in enumerate(roll):
        assert name == f"encoder.layers.encoder_layer_{i}.rollout" and src == "QKV" and dst == f"R{i & 1}"
        assert res == (None if i == 0 else f"R{(i - 1) & 1}") and tq == (1 if i == 11 else 197)
        assert names[names.index(name) - 1].endswith(".qkv") and names[names.index(name) + 1].endswith(".attn")
    assert added[-1][2] == "R1"                                       # the map names the last R: StagePipe renames it
    assert not any("rollout" in n or n == "top1" for n in r["tunable"])   # graph_tune walks these only


def test_rollout_excludes_the_other_outputs(vparams):
    from kdl.engine.base import Similar
    from kdl.engine.vit import ViTEngine
    g = torch.zeros((4, 768), dtype=torch.bfloat16, device="cuda")
    for kw in (dict(topk=3), dict(embed="raw"), dict(similar=Similar(g, 2))):
        with pytest.raises(ValueError, match="set one of them"):
            ViTEngine(vparams, max_batch=2, device="cuda", rollout=True, **kw)
    with pytest.raises(ValueError, match="spatial"):
        ViTEngine(vparams, max_batch=2, device="cuda", explain=True)
    with pytest.raises(ValueError, match="spatial"):
        ViTEngine(vparams, max_batch=2, device="cuda", explain=True, rollout=True)


# ------------------------------------------------------------------------------------ fp32 oracle
# max over two images of max_p |heat - heat_oracle|: bf16 (and e4m3) activations against an fp32 model,
# a figure that cannot be derived, so each build is gated at twice the largest value measured on the
# device over seeds 0..3 (profiles/rollout.txt). The run is deterministic; the margin is for other inputs.
ORACLE_GATE = {False: 0.00981, True: 0.08499}      # False: the bf16 build, True: fp8
FLAT = 0.5      # the oracle map's min / max has to be at most this, or a normalised map hides errors


def peaked_params(p: dict) -> dict:
    """Random-init attention is almost flat (the oracle map's min / max is 0.77), and dividing by the
    maximum then hides most of an error. With the Q and K rows of every in_proj_weight times sqrt(3)
    the scores are three times as large and the map's min / max is 0.39 to 0.46 for seeds 0..3."""
    from kdl.models import vit as V
    q = dict(p)
    for i in range(V.DEPTH):
        k = f"encoder.layers.encoder_layer_{i}.self_attention.in_proj_weight"
        w = p[k].clone()
        w[:2 * V.DIM] *= 3 ** 0.5
        q[k] = w
    return q


def oracle_error(fp8: bool, p: dict, seed: int) -> float:
    from kdl.engine import registry
    from kdl.engine.base import unpack_explain
    from kdl.engine.vit import ViTEngine
    imgs = _images(seed)
    k_o, score_o, heat_o = registry.get("vit_b16").rollout_oracle(p, imgs)
    flat = float((heat_o.amin(dim=(1, 2)) / heat_o.amax(dim=(1, 2))).max())
    assert flat <= FLAT, (seed, flat)
    eng = ViTEngine(p, max_batch=2, device="cuda", fp8=fp8, rollout=True)
    c, s, m = unpack_explain(eng.forward(imgs.cuda()).cpu().numpy(), 14, 14)
    del eng
    err = float(np.abs(m - heat_o.numpy()).max())
    print(f"{'fp8' if fp8 else 'bf16'} seed {seed}: oracle min/max {flat:.3f}, max |heat - oracle| {err:.6f}")
    return err


@pytest.mark.parametrize("fp8", BUILDS)
def test_rows_against_the_fp32_oracle(fp8, vparams):
    """Gate = 2 x the largest of 4 measured values (seeds 0..3, two images each):

      build   seed 0     seed 1     seed 2     seed 3     measured max   gate
      bf16    0.004487   0.004340   0.003761   0.004905   0.004905       0.00981
      fp8     0.042497   0.026379   0.037058   0.036344   0.042497       0.08499

    The oracle map's min / max is 0.438, 0.428, 0.452 and 0.453 for these seeds (the larger of the two
    images), under the 0.5 the comparison asks for. The rollout arithmetic itself is exact to 3e-6 (above);
    these figures are the bf16 / e4m3 residual stream and QKV against an fp32 model."""
    err = oracle_error(fp8, peaked_params(vparams), 0)
    assert err <= ORACLE_GATE[fp8], (fp8, err, ORACLE_GATE[fp8])


# ------------------------------------------------------------------------------------ server
def test_server_three_signatures_agree(tmp_path):
    """Two JPEGs through attention_bytes, their PIL-decoded pixels through attention_image, and the
    224 x 224 nearest-resized uint8 pixels through attention: the first two decode and resize on the
    device what the third receives, so the three answers are bit-equal."""
    import io
    from pathlib import Path

    import grpc
    from PIL import Image

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
    u8 = np.stack([pp.to_uint8(d, (224, 224)) for d in decoded])
    base = tmp_path / "vit"
    (base / "1").mkdir(parents=True)
    (base / "1" / "synthetic.json").write_text('{"seed": 0, "model": "vit_b16"}')
    cfg = ServerConfig(port=0, rest_api_port=0, model_name="vit", model_base_path=str(base), device="gpu", gpus=1,
                       host="127.0.0.1", file_system_poll_wait_seconds=0,
                       batching=BatchingParams(max_batch_size=2, batch_timeout_micros=1000, allowed_batch_sizes=[2]))
    srv = ModelServer(cfg).start(block_until_loaded=True)
    try:
        with grpc.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
            stub = PredictionStub(ch)
            got = {}
            for sig, key, X in (("attention_bytes", "image_bytes", files), ("attention_image", "images", px),
                                ("attention", "images", u8)):
                out = stub.Predict(make_request(X, model_name="vit", signature=sig, input_key=key), timeout=120).outputs
                assert sorted(out) == ["classes", "heatmap", "scores"]
                assert [d.size for d in out["classes"].tensor_shape.dim] == [2, 1]
                assert [d.size for d in out["heatmap"].tensor_shape.dim] == [2, 14, 14]
                got[sig] = (list(out["classes"].string_val), np.asarray(out["scores"].float_val, np.float32),
                            np.asarray(out["heatmap"].float_val, np.float32).reshape(2, 14, 14))
        s = srv.manager.get("vit", None, None)
        r = s.runner("attention")
        assert r.out_cols == 198 and r.executors and all(ex.engine.rollout for ex in r.executors)
        for sig in ("attention_bytes", "attention_image"):
            assert got[sig][0] == got["attention"][0]
            assert np.array_equal(_bits(got[sig][1]), _bits(got["attention"][1]))
            assert np.array_equal(_bits(got[sig][2]), _bits(got["attention"][2]))
        labels, scores, heat = got["attention"]
        assert all(v.decode() in s.source.labels for v in labels) and ((scores > 0) & (scores <= 1)).all()
        assert heat.max(axis=(1, 2)).tolist() == [1.0, 1.0] and heat.min() > 0
        assert s.device_alive()
    finally:
        srv.stop(0)
