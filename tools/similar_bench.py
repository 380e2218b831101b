"""Gallery search timings on one GPU (profiles/similar.txt).

  python -m tools.similar_bench [--rows 10000,100000,1000000] [--dtype bf16|fp8] [--out FILE]

1. The gallery_topk op alone (kernels/similar.hip) at F = 2048, B = 32, K = 5: microseconds per call
   and gallery bytes / time. "same" re-reads one gallery (a 41 MB or 410 MB one then sits partly or
   wholly in the 256 MiB Infinity Cache); "rotating" walks over copies of at least 1 GiB in total,
   so every call reads from HBM.
2. The same answer from torch: (q @ g.T).topk(K) with both operands bf16, and with both fp32.
3. An Xception ``similar`` engine's batch-32 forward (captured graph) against an ``embed="l2"``
   engine's, as interleaved pairs.

``--dtype fp8`` (profiles/similar_fp8.txt) stores the same rows as e4m3 codes with a scale per row
(kernels/similar_f8.hip): 1 times that gallery and counts how many of the float64 top-K of the
unquantised rows its ranking keeps, 2 is left out, and 3 pairs a bf16-gallery ``similar`` engine
with an fp8-gallery one. ``--embed-recall N`` adds the same count on a gallery of N Xception embed
rows with planted near-duplicates, for an fp8 and a bf16 gallery.

``--ivf L,nprobe`` (profiles/similar_ivf.txt) times the indexed search instead (kernels/similar_ivf.hip:
the coarse gallery_topk over L centroids, then gallery_ivf_topk over the rows of nprobe lists) against
the dense bf16 op on the same stored rows as interleaved pairs, on clustered rows (unit centres plus
noise) and on unit-norm random rows, the worst case for any index; it prints the share of chunks and
rows a call reads and the recall of the float64 dense top-K at nprobe 1, 4, 8, 16, 32, and 3 pairs a
dense ``similar`` engine with an indexed one. The index is two rounds of spherical k-means on the
device, in this tool only: the product builds its index on the CPU (``build-gallery --ivf_lists``).

Each time is the median of ``--repeats`` windows of ``--iters`` calls between two device events,
after warm-up calls of the same shapes."""
from __future__ import annotations

import argparse
import statistics
import sys

import torch

F, B, K = 2048, 32, 5


def window(fn, iters: int, repeats: int, warm: int = 5) -> tuple[float, float]:
    """(median, min) microseconds per call of fn(i)."""
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for r in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(r * iters + i)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out), min(out)


def unit_slices(n: int, seed: int):
    """(first row, fp32 unit rows) slices of the random gallery of a seed: no fp32 copy of the whole."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    for lo in range(0, n, 65536):
        yield lo, torch.nn.functional.normalize(torch.randn((min(65536, n - lo), F), generator=g, device="cuda"), dim=1)


def random_gallery(n: int, seed: int) -> torch.Tensor:
    out = torch.empty((n, F), dtype=torch.bfloat16, device="cuda")
    for lo, x in unit_slices(n, seed):
        out[lo:lo + x.shape[0]] = x.to(torch.bfloat16)
    return out


def random_gallery_fp8(n: int, seed: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(e4m3 codes uint8 [n, F], fp32 scales [n]) of the same rows: kdl.serving.similar.quantize_fp8's rule."""
    codes = torch.empty((n, F), dtype=torch.uint8, device="cuda")
    scale = torch.empty(n, dtype=torch.float32, device="cuda")
    for lo, x in unit_slices(n, seed):
        s = (x.double().abs().amax(dim=1) / 448.0).float()
        s[s == 0] = 1.0
        y = (x.double() / s.double()[:, None]).float().clamp(-448.0, 448.0)
        codes[lo:lo + x.shape[0]] = y.to(torch.float8_e4m3fn).view(torch.uint8)
        scale[lo:lo + x.shape[0]] = s
    return codes, scale


def fp8_rows(n: int, iters: int, repeats: int, say) -> None:
    from kdl.ops import _lib
    lib = _lib.lib()
    nbytes = n * F
    copies = max(1, -(-(1 << 30) // nbytes))
    gals = [random_gallery_fp8(n, 17 + c) for c in range(copies)]
    q = torch.nn.functional.normalize(torch.randn((B, F), generator=torch.Generator().manual_seed(3)), dim=1).cuda()
    out = torch.zeros((B, 2 * K), dtype=torch.int32, device="cuda")
    work = torch.zeros(lib.gallery_topk_workspace(B, n, K), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(g):
        lib.gallery_topk(dict(q=q.data_ptr(), g8=g[0].data_ptr(), scale=g[1].data_ptr(), out=out.data_ptr(),
                              work=work.data_ptr(), B=B, N=n, F=F, K=K, ldq=F, ldg=F), s)
    it = max(5, min(iters, (64 << 30) // nbytes))
    for name, pick in (("same", lambda i: gals[0]), ("rotating", lambda i: gals[i % copies])):
        if name == "rotating" and copies == 1:
            continue
        med, best = window(lambda i: call(pick(i)), it, repeats)
        say(f"N={n:8d} gallery_topk fp8 {name:8s} ({copies if name == 'rotating' else 1} x {nbytes / 1e6:7.1f} MB): "
            f"median {med:8.1f} us  min {best:8.1f} us  {nbytes / med / 1e6:6.2f} TB/s of gallery bytes")
    call(gals[0])
    torch.cuda.synchronize()
    mine = out[:, :K].cpu()
    ref = torch.cat([q.double() @ x.double().T for _, x in unit_slices(n, 17)], dim=1).topk(K).indices.cpu()
    kept = sum(len(set(mine[b].tolist()) & set(ref[b].tolist())) for b in range(B))
    say(f"N={n:8d} rows of the float64 top-{K} of the unquantised gallery that the fp8 ranking keeps: {kept}/{B * K}, "
        f"same row at the same rank {int((mine == ref).sum())}/{B * K}")
    del gals


def op_rows(n: int, iters: int, repeats: int, say) -> None:
    from kdl.ops import _lib
    lib = _lib.lib()
    nbytes = n * F * 2
    copies = max(1, -(-(1 << 30) // nbytes))
    gals = [random_gallery(n, 17 + c) for c in range(copies)]
    q = torch.nn.functional.normalize(torch.randn((B, F), generator=torch.Generator().manual_seed(3)), dim=1).cuda()
    out = torch.zeros((B, 2 * K), dtype=torch.int32, device="cuda")
    work = torch.zeros(lib.gallery_topk_workspace(B, n, K), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(g):
        lib.gallery_topk(dict(q=q.data_ptr(), g=g.data_ptr(), out=out.data_ptr(), work=work.data_ptr(), B=B, N=n, F=F,
                              K=K, ldq=F, ldg=F), s)
    it = max(5, min(iters, (64 << 30) // nbytes))
    for name, pick in (("same", lambda i: gals[0]), ("rotating", lambda i: gals[i % copies])):
        if name == "rotating" and copies == 1:
            continue
        med, best = window(lambda i: call(pick(i)), it, repeats)
        say(f"N={n:8d} gallery_topk {name:8s} ({copies if name == 'rotating' else 1} x {nbytes / 1e6:7.1f} MB): "
            f"median {med:8.1f} us  min {best:8.1f} us  {nbytes / med / 1e6:6.2f} TB/s of gallery bytes")
    call(gals[0])
    torch.cuda.synchronize()
    mine = out[:, :K].clone()
    g = gals[0]
    qb = q.to(torch.bfloat16)
    med, best = window(lambda i: (qb @ g.T).topk(K), it, repeats)
    say(f"N={n:8d} torch bf16 (q @ g.T).topk({K}):            median {med:8.1f} us  min {best:8.1f} us  "
        f"{nbytes / med / 1e6:6.2f} TB/s of gallery bytes")
    gf = g.float()
    med, best = window(lambda i: (q @ gf.T).topk(K), it, repeats)
    say(f"N={n:8d} torch fp32 (q @ g.T).topk({K}):            median {med:8.1f} us  min {best:8.1f} us  "
        f"(reads {2 * nbytes / 1e6:.1f} MB of fp32: {2 * nbytes / med / 1e6:5.2f} TB/s)")
    ref = (q.double() @ gf.double().T).topk(K).indices
    say(f"N={n:8d} indices equal to a float64 torch top-{K}: gallery_topk {int((mine == ref).sum())}/{B * K}, "
        f"torch fp32 {int(((q @ gf.T).topk(K).indices == ref).sum())}/{B * K}, "
        f"torch bf16 {int(((qb @ g.T).topk(K).indices == ref).sum())}/{B * K}")
    del gals, gf


def ivf_gallery(n: int, lists: int, kind: str, seed: int):
    """(stored bf16 rows [n, F] list by list, bf16 centroids [lists, F], offsets int32 numpy [lists + 1], B queries):
    "random" unit rows and queries, or "clustered": a unit centre per list plus noise of the same length
    in all, queries made the same way. Lists come from two rounds of spherical k-means from the first rows."""
    import numpy as np
    g = torch.Generator(device="cuda").manual_seed(seed)
    unit = torch.nn.functional.normalize
    centres = unit(torch.randn((lists, F), generator=g, device="cuda"), dim=1)

    def rows(m: int) -> torch.Tensor:
        x = torch.randn((m, F), generator=g, device="cuda")
        if kind == "clustered":
            x = centres[torch.randint(0, lists, (m,), generator=g, device="cuda")] + x / F ** 0.5
        return unit(x, dim=1)
    gal = torch.cat([rows(min(65536, n - lo)).to(torch.bfloat16) for lo in range(0, n, 65536)])
    c = gal[:lists].clone()
    assign = lambda: torch.cat([(gal[lo:lo + 65536] @ c.T).argmax(dim=1) for lo in range(0, n, 65536)])
    for _ in range(2):
        a = assign()
        sums = torch.zeros((lists, F), device="cuda")
        for lo in range(0, n, 65536):
            sums.index_add_(0, a[lo:lo + 65536], gal[lo:lo + 65536].float())
        c = torch.where(sums.norm(dim=1, keepdim=True) > 0, unit(sums, dim=1), c.float()).to(torch.bfloat16)
    a = assign()
    order = torch.argsort(a, stable=True)
    offsets = np.concatenate([[0], np.cumsum(torch.bincount(a, minlength=lists).cpu().numpy())]).astype(np.int32)
    return gal[order].contiguous(), c.contiguous(), offsets, rows(B).float().contiguous()


def ivf_rows(n: int, lists: int, nprobe: int, kind: str, iters: int, repeats: int, pairs: int, say) -> None:
    import numpy as np

    from kdl.ops import _lib
    from kdl.serving.similar import chunk_table
    lib = _lib.lib()
    gal, cen, offsets, q = ivf_gallery(n, lists, kind, 17)
    table = torch.from_numpy(chunk_table(offsets)).cuda()
    C = table.shape[0]
    lens = np.diff(offsets)
    say(f"N={n:8d} L={lists} {kind}: {C} chunks (dense: {-(-n // 256)}), list length min {lens.min()} median "
        f"{int(np.median(lens))} max {lens.max()}, empty lists {int((lens == 0).sum())}")
    out = torch.zeros((B, 2 * K), dtype=torch.int32, device="cuda")
    dwork = torch.zeros(lib.gallery_topk_workspace(B, n, K), dtype=torch.uint8, device="cuda")
    cwork = torch.zeros(lib.gallery_topk_workspace(B, lists, 32), dtype=torch.uint8, device="cuda")
    iwork = torch.zeros(lib.gallery_ivf_workspace(B, K, lists, C), dtype=torch.uint8, device="cuda")
    probe = torch.zeros((B, 64), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    base = dict(q=q.data_ptr(), B=B, F=F, ldq=F, ldg=F)

    def dense(i=0):
        lib.gallery_topk(dict(base, g=gal.data_ptr(), out=out.data_ptr(), work=dwork.data_ptr(), N=n, K=K), s)

    def coarse(p):
        lib.gallery_topk(dict(base, g=cen.data_ptr(), out=probe.data_ptr(), work=cwork.data_ptr(), N=lists, K=p), s)

    def scan(p):
        lib.gallery_ivf_topk(dict(base, g=gal.data_ptr(), out=out.data_ptr(), work=iwork.data_ptr(), N=n, K=K,
                                  probe=probe.data_ptr(), table=table.data_ptr(), L=lists, P=p, C=C, ldp=2 * p), s)

    def indexed(i=0, p=nprobe):
        coarse(p)
        scan(p)
    it = max(5, min(iters, (64 << 30) // (n * F * 2)))
    ratios = []
    for i in range(pairs):
        order = (dense, indexed) if i % 2 == 0 else (indexed, dense)
        t = {fn: window(fn, it, repeats)[0] for fn in order}
        ratios.append(t[dense] / t[indexed])
        say(f"N={n:8d} L={lists} nprobe={nprobe} {kind} pair {i}: dense gallery_topk {t[dense]:8.1f} us  "
            f"coarse + gallery_ivf_topk {t[indexed]:8.1f} us  dense / indexed {ratios[-1]:.2f}")
    tc, ts = window(lambda i: coarse(nprobe), it, repeats)[0], window(lambda i: scan(nprobe), it, repeats)[0]
    say(f"N={n:8d} L={lists} nprobe={nprobe} {kind}: median dense / indexed {statistics.median(ratios):.2f}; alone: "
        f"coarse gallery_topk {tc:.1f} us, gallery_ivf_topk {ts:.1f} us")
    ref = torch.cat([q.double() @ gal[lo:lo + 65536].double().T for lo in range(0, n, 65536)], dim=1).topk(K).indices.cpu()
    tab = table.cpu().numpy()
    for p in (1, 4, 8, 16, 32):
        if p > lists:
            continue
        indexed(0, p)
        torch.cuda.synchronize()
        mine = out[:, :K].cpu()
        hit = np.zeros(lists, bool)
        hit[probe.flatten()[:B * 2 * p].view(B, 2 * p)[:, :p].cpu().numpy().ravel()] = True      # rows of 2p words
        kept = sum(len(set(mine[b].tolist()) & set(ref[b].tolist())) for b in range(B))
        say(f"N={n:8d} L={lists} {kind} nprobe={p:2d}: recall of the float64 dense top-{K} {kept}/{B * K}; chunks read "
            f"{int(hit[tab[:, 0]].sum())}/{C} ({100 * hit[tab[:, 0]].mean():.2f} %), rows read {int(lens[hit].sum())}/{n} "
            f"({100 * lens[hit].sum() / n:.2f} %)")


def ivf_engine_pairs(n: int, lists: int, nprobe: int, pairs: int, say) -> None:
    from kdl.engine.base import Ivf, Similar
    from kdl.serving.similar import chunk_table
    gal, cen, offsets, _ = ivf_gallery(n, lists, "clustered", 5)
    ivf = Ivf(cen, torch.from_numpy(chunk_table(offsets)).cuda(), torch.from_numpy(offsets), nprobe)
    engine_pairs(n, pairs, say, sims={"dense": Similar(gal, K, "cosine"), "ivf": Similar(gal, K, "cosine", None, ivf)})


def embed_recall(n: int, say) -> None:
    """Recall on a gallery of embed rows: n images of random 8 x 8 colour blocks through an Xception
    embed="l2" engine, and for each of the B query images four near-duplicates (the image plus uniform
    noise of +-2, 4, 8, 16 levels) planted among them; the queries themselves are not in the gallery."""
    from kdl.engine import registry
    from kdl.ops import _lib
    lib, info = _lib.lib(), registry.get("xception")
    eng = info.engine(info.init_params(0), 32, "cuda", embed="l2")
    g = torch.Generator().manual_seed(11)
    S = info.input_size

    def blocks(m: int) -> torch.Tensor:
        small = torch.randint(0, 256, (m, 8, 8, 3), generator=g, dtype=torch.uint8)
        return small.repeat_interleave(38, 1).repeat_interleave(38, 2)[:, :S, :S].contiguous()
    qi = blocks(B)
    dup = [(qi.int() + torch.randint(-a, a + 1, qi.shape, generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
           for a in (2, 4, 8, 16)]
    imgs = torch.cat(dup + [blocks(n - 4 * B)])
    rows = torch.cat([eng.forward(imgs[lo:lo + 32].cuda()).clone() for lo in range(0, n, 32)])
    q = eng.forward(qi.cuda()).clone()
    ref = (q.double() @ rows.double().T).topk(K).indices.cpu()
    s = (rows.double().abs().amax(dim=1) / 448.0).float()
    codes = (rows.double() / s.double()[:, None]).float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    bf = rows.to(torch.bfloat16)
    out = torch.zeros((B, 2 * K), dtype=torch.int32, device="cuda")
    work = torch.zeros(lib.gallery_topk_workspace(B, n, K), dtype=torch.uint8, device="cuda")
    for name, gal in (("fp8", dict(g8=codes.data_ptr(), scale=s.data_ptr())), ("bf16", dict(g=bf.data_ptr()))):
        lib.gallery_topk(dict(q=q.data_ptr(), out=out.data_ptr(), work=work.data_ptr(), B=B, N=n, F=F, K=K, ldq=F, ldg=F,
                              **gal), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        mine = out[:, :K].cpu()
        kept = sum(len(set(mine[b].tolist()) & set(ref[b].tolist())) for b in range(B))
        dups = sum(len(set(mine[b].tolist()) & {b, B + b, 2 * B + b, 3 * B + b}) for b in range(B))
        say(f"N={n:8d} embed rows, {name:4s} gallery: rows of the float64 top-{K} kept {kept}/{B * K}, same row at the same "
            f"rank {int((mine == ref).sum())}/{B * K}, planted near-duplicates among the {K} returned {dups}/{4 * B}")
    say(f"N={n:8d} embed rows: planted near-duplicates in the float64 top-{K} "
        f"{sum(len(set(ref[b].tolist()) & {b, B + b, 2 * B + b, 3 * B + b}) for b in range(B))}/{4 * B}")


def engine_pairs(n: int, pairs: int, say, dtype: str = "bf16", sims: dict | None = None) -> None:
    """Pairs of an embed="l2" engine and a similar engine; dtype "fp8": of a bf16-gallery similar
    engine (in the "l2" column) and an fp8-gallery one; ``sims`` {"dense": Similar, "ivf": Similar}: of
    those two similar engines."""
    from kdl.engine import registry
    from kdl.engine.base import Similar
    from kdl.engine.tuning import tuning_path
    info = registry.get("xception")
    p = info.init_params(0)
    gal = None if sims else random_gallery(n, 5)
    if sims:
        engines = {"l2": info.engine(p, 32, "cuda", similar=sims["dense"]),
                   "similar": info.engine(p, 32, "cuda", similar=sims["ivf"])}
    elif dtype == "fp8":
        codes, scale = random_gallery_fp8(n, 5)
        engines = {"l2": info.engine(p, 32, "cuda", similar=Similar(gal, K, "cosine")),
                   "similar": info.engine(p, 32, "cuda", similar=Similar(codes, K, "cosine", scale))}
    else:
        engines = {"l2": info.engine(p, 32, "cuda", embed="l2"),
                   "similar": info.engine(p, 32, "cuda", similar=Similar(gal, K, "cosine"))}
    first = "similar dense" if sims else "similar bf16" if dtype == "fp8" else "embed=l2"
    x = torch.randint(0, 256, (32, info.input_size, info.input_size, 3), dtype=torch.uint8,
                      generator=torch.Generator().manual_seed(1)).cuda()
    tp = tuning_path(info.tuning or "xception", 32)
    for e in engines.values():
        if tp.exists():
            e.load_tuning(tp)
        e.forward(x)

    def timed(e) -> float:
        with torch.cuda.stream(e.stream):
            for _ in range(20):
                e.launch(32, e.stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(e.stream)
            for _ in range(100):
                e.launch(32, e.stream)
            e1.record(e.stream)
            e1.synchronize()
        return e0.elapsed_time(e1) / 100
    for i in range(pairs):
        order = ("l2", "similar") if i % 2 == 0 else ("similar", "l2")
        t = {k: timed(engines[k]) for k in order}
        d = (t["similar"] - t["l2"]) * 1e3
        say(f"pair {i}: {first} {t['l2']:.4f} ms  similar{' ivf' if sims else ' fp8' if dtype == 'fp8' else ''}(N={n}) {t['similar']:.4f} ms  diff {d:+.1f} us "
            f"({100 * d / 1e3 / t['l2']:+.2f} %)")
    prof = dict(engines["similar"].profile(32))
    say(f"similar engine.profile(32), eager launches, median of 20: embed_rows {prof['embed_rows'] * 1e3:.1f} us, "
        f"similar {prof['similar'] * 1e3:.1f} us, sum of all steps {sum(prof.values()):.3f} ms")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000,100000,1000000")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--engine-rows", type=int, default=100000)
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--embed-recall", type=int, default=0, metavar="N",
                    help="also count what an fp8 gallery of N Xception embed rows with planted near-duplicates keeps")
    ap.add_argument("--ivf", default="", metavar="L,NPROBE", help="time the indexed search of L lists, NPROBE probed")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("similar_bench needs a GPU", file=sys.stderr)
        return 1
    f = open(a.out, "w") if a.out else None

    def say(line: str) -> None:
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
    if a.ivf:
        lists, nprobe = (int(v) for v in a.ivf.split(","))
        say(f"== dense gallery_topk vs coarse gallery_topk + gallery_ivf_topk, L={lists} nprobe={nprobe}, F={F} B={B} K={K}")
        for n in (int(v) for v in a.rows.split(",") if v):
            for kind in ("clustered", "random"):
                ivf_rows(n, lists, nprobe, kind, a.iters, a.repeats, max(a.pairs, 1), say)
        if a.pairs and a.engine_rows:
            say("== xception b32 forward (captured graph, device events), dense similar vs indexed similar, interleaved pairs")
            ivf_engine_pairs(a.engine_rows, lists, nprobe, a.pairs, say)
        return 0
    say(f"== gallery_topk alone{' and torch' if a.dtype == 'bf16' else ', fp8 gallery'}, F={F} B={B} K={K}")
    for n in (int(v) for v in a.rows.split(",") if v):
        (fp8_rows if a.dtype == "fp8" else op_rows)(n, a.iters, a.repeats, say)
    if a.embed_recall:
        say(f"== recall on a gallery of Xception embed rows with planted near-duplicates, B={B} K={K}")
        embed_recall(a.embed_recall, say)
    if a.pairs:
        say("== xception b32 forward (captured graph, device events), "
            f"{'similar bf16 vs similar fp8' if a.dtype == 'fp8' else 'embed=l2 vs similar'}, interleaved pairs")
        engine_pairs(a.engine_rows, a.pairs, say, a.dtype)
    return 0


if __name__ == "__main__":
    sys.exit(main())
