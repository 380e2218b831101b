"""MI355X executor for ConvNeXt-Tiny (torchvision ``convnext_tiny``, kdl/models/convnext.py).

Lowering (captured into one hipGraph per batch bucket; stage i runs on B x H_i x H_i pixel rows of
C_i channels, H = 56 / 28 / 14 / 7, C = 96 / 192 / 384 / 768; every buffer is a [rows][C] bf16 matrix):

    patchify        uint8 image -> [B*56*56][64] bf16 patches (P = 4, K = 48; columns 48..63 stay
                    zero), mean/std on load
    conv_gemm PW    stem conv 48 -> 96 (+bias)
    layernorm       features.0.1, D = 96
    per block (3 / 3 / 9 / 3):
      dwconv7_ln    depthwise 7x7 + bias + LayerNorm over C, one launch (kernels/dwconv_ln.hip)
      conv_gemm PW  block.3 C -> 4C (+bias, exact GELU epilogue)
      conv_gemm PW  block.5 4C -> C (+bias) + residual, in place on the stage's X; layer_scale is
                    folded into its weights and bias on the host (ops/pack.py fold_layer_scale)
    per downsample (3):
      ln_s2d        LayerNorm2d, written space-to-depth: [B*H/2*H/2][4C]
      conv_gemm PW  the 2x2 / stride-2 conv as one GEMM with K = 4C (ops/pack.py s2d_weights)
    gap             mean of the 7 x 7 x 768 map (bf16 features; ``embed=`` pools the same map)
    layernorm       classifier.0 on the B feature rows, D = 768
    fc_mfma         classifier.2 768 -> 1000

= 3 + 18*3 + 3*2 + 3 = 66 launches. The pointwise convs are the ViT MLP's GEMMs (GELU and the residual
in the epilogue) on default tiles: no tuning table yet. With LayerNorm between the pool and the
classifier neither of ``class_map``'s closed-form heads applies, so ``explain=True`` is refused.
"""
from __future__ import annotations

from pathlib import Path

import torch

from ..models import convnext as CX
from ..ops import _lib
from ..ops.conv import MODE_PW, ConvGemmLayer, Geometry
from ..ops.pack import fold_layer_scale, pack_fragments, s2d_weights
from .base import EngineBase, Step


class ConvNeXtEngine(EngineBase):
    model_name = "convnext_tiny"

    def __init__(self, params: dict, max_batch: int = 32, device: str | torch.device = "cuda",
                 buckets=None, tune_file: str | Path | None = None, topk: int = 0, embed: str = "",
                 similar=None, explain: bool = False, rollout: bool = False, overlay=None, overlay_jpeg=None,
                 palette=None, locate=None, cutout=None, cutout_png=None):
        if explain or rollout:      # before anything touches the device
            raise ValueError("ConvNeXt normalises the pooled features in front of its classifier: neither "
                             "Grad-CAM head of class_map applies and it has no attention to roll out "
                             "(no explain / rollout outputs)")
        super().__init__(device, max_batch, buckets, topk, embed, similar, overlay=overlay,
                         overlay_jpeg=overlay_jpeg, palette=palette, locate=locate, cutout=cutout,
                         cutout_png=cutout_png)
        self.size = CX.INPUT_SIZE
        self.classes = params["classifier.2.bias"].numel()
        self.shapes: dict[str, tuple[int, int]] = {}     # buffer -> (pixels per image, channels)
        self.ln: dict[str, tuple] = {}                   # layernorm / ln_s2d step -> (gamma, beta)
        self._build(params)
        self._alloc()
        self._enable_outputs()
        if tune_file and Path(tune_file).exists():
            self.load_tuning(tune_file)

    # ------------------------------------------------------------------ lowering
    def _lin(self, name: str, w: torch.Tensor, b: torch.Tensor, relu_out: int = 0) -> ConvGemmLayer:
        lay = ConvGemmLayer(name, MODE_PW, w.double(), b.float(), cin_pad=w.shape[1], n=w.shape[0],
                            relu_out=relu_out, device=self.device)
        lay.krot = 1      # as the ViT linears run (profiles/krot_ab.txt)
        return lay

    def _vecs(self, p: dict, name: str) -> None:
        self.ln[name] = (p[f"{name}.weight"].float().contiguous().to(self.device),
                         p[f"{name}.bias"].float().contiguous().to(self.device))

    def _build(self, p: dict) -> None:
        dev = self.device
        H = self.size // CX.PATCH
        K0 = 3 * CX.PATCH * CX.PATCH
        self.shapes["patches"] = (H * H, 64)
        self.steps.append(Step("patchify", "patchify", src="input", dst="patches"))
        w0 = torch.zeros(CX.DIMS[0], 64, dtype=torch.float64)
        w0[:, :K0] = p["features.0.0.weight"].double().reshape(CX.DIMS[0], K0)      # k = c*16 + ky*4 + kx
        self.shapes["stem"] = self.shapes["X0"] = (H * H, CX.DIMS[0])
        self.steps.append(Step("conv", "features.0.0", self._lin("features.0.0", w0, p["features.0.0.bias"]),
                               "patches", "stem", geom=(H,)))
        self._vecs(p, "features.0.1")
        self.steps.append(Step("ln", "features.0.1", src="stem", dst="X0", geom=(H,)))
        self.dw: dict[str, tuple] = {}
        for i, (n, c) in enumerate(zip(CX.DEPTHS, CX.DIMS)):
            X, N, Hd = f"X{i}", f"N{i}", f"H{i}"
            if i:
                d, cp = f"features.{2 * i}", CX.DIMS[i - 1]
                D = f"D{i}"
                self.shapes[D] = (H * H // 4, 4 * cp)
                self._vecs(p, f"{d}.0")
                self.steps.append(Step("ln_s2d", f"{d}.0", src=f"X{i - 1}", dst=D, geom=(H,), extra=dict(C=cp)))
                H //= 2
                self.steps.append(Step("conv", f"{d}.1", self._lin(f"{d}.1", s2d_weights(p[f"{d}.1.weight"]),
                                                                    p[f"{d}.1.bias"]), D, X, geom=(H,)))
            self.shapes[X] = self.shapes[N] = (H * H, c)
            self.shapes[Hd] = (H * H, 4 * c)
            for j in range(n):
                b = f"{CX.stage_prefix(i)}.{j}"
                # depthwise weights [C][1][7][7] -> [49][C] fp32, as the kernel reads them
                self.dw[f"{b}.block.0"] = (
                    p[f"{b}.block.0.weight"].float().reshape(c, 49).t().contiguous().to(dev),
                    p[f"{b}.block.0.bias"].float().contiguous().to(dev))
                self._vecs(p, f"{b}.block.2")
                self.steps.append(Step("dwln", f"{b}.block.0", src=X, dst=N, geom=(H,), extra=dict(C=c, ln=f"{b}.block.2")))
                self.steps.append(Step("conv", f"{b}.block.3", self._lin(
                    f"{b}.block.3", p[f"{b}.block.3.weight"], p[f"{b}.block.3.bias"], relu_out=3), N, Hd, geom=(H,)))
                w5, b5 = fold_layer_scale(p[f"{b}.block.5.weight"], p[f"{b}.block.5.bias"], p[f"{b}.layer_scale"])
                self.steps.append(Step("conv", f"{b}.block.5", self._lin(f"{b}.block.5", w5, b5), Hd, X, res=X,
                                       geom=(H,)))
        F = CX.DIMS[-1]
        self._vecs(p, "classifier.0")
        self.steps.append(Step("gap", "avgpool", src="X3", dst="feat", geom=(H,), extra=dict(F=F)))
        self.steps.append(Step("ln", "classifier.0", src="feat", dst="featn", extra=dict(head=True)))
        nf = (self.classes + 15) // 16
        self.fc_wp = pack_fragments(p["classifier.2.weight"].float(), nf, F // 32).to(dev).contiguous()
        self.fc_nf = nf
        self.fc_b = p["classifier.2.bias"].float().to(dev)
        self.steps.append(Step("fc", "classifier.2", src="featn", dst="logits", extra=dict(F=F)))

    def _alloc(self) -> None:
        B, S, dev = self.max_batch, self.size, self.device
        self.inp = torch.zeros((B, S, S, 3), dtype=torch.uint8, device=dev)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.bfloat16, device=dev)  # noqa: E731
        self.bufs = {name: z(B * hw, c) for name, (hw, c) in self.shapes.items()}   # patches' pad columns stay 0
        F = CX.DIMS[-1]
        self.bufs["feat"] = z((B + 15) // 16 * 16, F)
        self.bufs["featn"] = z((B + 15) // 16 * 16, F)                              # rows >= B stay 0
        self.logits = torch.zeros((B, self.classes), dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ emission
    def _ptr(self, name: str) -> int:
        if name == "input":
            return self.input_ptr()
        if name == "logits":
            return self.output_ptr()
        return _lib.ptr(self.bufs[self._remap.get(name, name)])

    def _ld(self, name: str) -> int:
        return self.bufs[name].shape[1]

    def embed_source(self) -> tuple:
        """The input of the avgpool step: the last stage's output, 7 x 7 pixels of 768 bf16."""
        gap = next(s for s in self.steps if s.kind == "gap")
        hw, c = self.shapes[gap.src]
        return gap.src, hw, c, gap.extra["F"], 0

    def scratch_buffers(self) -> list[str]:
        return []

    def _emit_conv(self, prog, step: Step, b: int, split=None, cfg=None) -> None:
        rows = b * step.geom[0] * step.geom[0]
        step.layer.emit(prog, self._ptr(step.src), self._wptr(step.dst), Geometry(1, 1, rows, 1, rows),
                        res=self._ptr(step.res) if step.res else None, ldx=self._ld(step.src),
                        ldr=self._ld(step.res) if step.res else None, split=False, cfg=cfg)

    def _variants(self, step: Step):
        return step.layer.variants(None)

    def _emit(self, prog, step: Step, b: int) -> None:
        H = step.geom[0] if step.geom else 0
        if step.kind == "patchify":
            sc = [1.0 / (255.0 * s) for s in CX.STD]
            sh = [-m / s for m, s in zip(CX.MEAN, CX.STD)]
            prog.add_patchify(step.name, dict(x=self.input_ptr(), y=self._ptr("patches"), B=b, H=self.size,
                                              W=self.size, P=CX.PATCH, ldy=self._ld("patches"), scale0=sc[0],
                                              scale1=sc[1], scale2=sc[2], shift0=sh[0], shift1=sh[1], shift2=sh[2]))
        elif step.kind == "conv":
            self._emit_conv(prog, step, b)
        elif step.kind == "ln":
            g, bb = self.ln[step.name]
            rows = b if step.extra.get("head") else b * H * H
            D = g.numel()
            prog.add_layernorm(step.name, dict(x=self._ptr(step.src), y=self._ptr(step.dst), gamma=_lib.ptr(g),
                                               beta=_lib.ptr(bb), rows=rows, D=D, ldx=self._ld(step.src),
                                               ldy=self._ld(step.dst), eps=CX.LN_EPS))
        elif step.kind == "dwln":
            w, bias = self.dw[step.name]
            g, bb = self.ln[step.extra["ln"]]
            prog.add_dwconv7_ln(step.name, dict(x=self._ptr(step.src), w=_lib.ptr(w), bias=_lib.ptr(bias),
                                                gamma=_lib.ptr(g), beta=_lib.ptr(bb), y=self._ptr(step.dst), B=b,
                                                H=H, W=H, C=step.extra["C"], ldx=self._ld(step.src),
                                                ldy=self._ld(step.dst), eps=CX.LN_EPS))
        elif step.kind == "ln_s2d":
            g, bb = self.ln[step.name]
            prog.add_ln_s2d(step.name, dict(x=self._ptr(step.src), gamma=_lib.ptr(g), beta=_lib.ptr(bb),
                                            y=self._ptr(step.dst), B=b, H=H, W=H, C=step.extra["C"],
                                            ldx=self._ld(step.src), ldy=self._ld(step.dst), eps=CX.LN_EPS))
        elif step.kind == "gap":
            prog.add_gap(step.name, dict(x=self._ptr(step.src), y=None, yb=self._ptr("feat"), B=b, HW=H * H,
                                         ldx=self._ld(step.src), F=step.extra["F"], dt=0))
        elif step.kind == "fc":
            prog.add_fc_mfma(step.name, dict(xb=self._ptr("featn"), wp=_lib.ptr(self.fc_wp),
                                             bias=_lib.ptr(self.fc_b), out=self._ptr("logits"), B=b,
                                             F=step.extra["F"], N=self.classes, NF=self.fc_nf, relu=0, dt=0))
        else:  # pragma: no cover
            raise ValueError(step.kind)

    def flops_per_image(self) -> float:
        return 2.0 * CX.macs_per_image(self.size)
