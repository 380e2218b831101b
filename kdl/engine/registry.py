"""Model-family registry: oracle params + MI355X engine + benchmark metadata.

One entry per BASELINE.json config family the stack serves.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable


@dataclass(frozen=True)
class ModelInfo:
    name: str
    input_size: int
    classes: int
    params_total: int
    description: str
    init_params: Callable
    engine: Callable          # (params, max_batch, device, **kw) -> EngineBase
    oracle: Callable          # (params, uint8 NHWC) -> fp32 logits
    dtype: str = "bf16"       # compute dtype of the engine (bench.py's "dtype" field)
    tuning: str = ""          # tuning-table family name when it differs from ``name``
    stage_cut: str = ""       # default stage-pipeline cut (stages.py) for bench / serving; "" = lanes
    features: int = 0         # F: floats of the pooled feature vector in front of the head
    feature_oracle: Callable = None   # (params, uint8 NHWC) -> fp32 [n, F], what engines pool with embed=
    # (params, uint8 NHWC) -> (class int32 [n], score fp32 [n], heat fp32 [n, h, w]): the Grad-CAM map of
    # the predicted class over the feature map in front of the head, what engines answer with
    # explain=True; None for a family without a spatial map there (ViT)
    cam_oracle: Callable = None
    map_size: tuple = ()      # (h, w) of that map (or of the rollout map) at the family's input size
    # (params, uint8 NHWC) -> (class int32 [n], score fp32 [n], heat fp32 [n, h, w]): the attention-rollout
    # map of a transformer (Abnar & Zuidema 2020) in fp32 torch, what engines answer with rollout=True;
    # None for the CNN families. cam_oracle stays None for ViT: rollout is another method.
    rollout_oracle: Callable = None


def _no_grad_mean(base, p, x_nchw):
    """Spatial mean of a family's fp32 feature map [n, F, H, W]: Keras ``pooling="avg"``."""
    import torch
    with torch.no_grad():
        return base(p, x_nchw).mean(dim=(2, 3))


def _cam(base, head, p, x_nchw):
    """Grad-CAM as the Keras example defines it, by ``torch.autograd`` through a family's own head
    on its own fp32 feature map [n, F, H, W]: k the top-1 class, alpha_c the mean over the pixels of
    dlogit_k/dA (= (1/HW) dlogit_k/dg_c), raw_p = sum_c alpha_c A[p][c], heat = max(raw, 0) / its
    largest value, all zeros when that is 0. The score is the class's softmax probability."""
    import torch
    with torch.no_grad():
        a = base(p, x_nchw).float()
    a.requires_grad_(True)
    with torch.enable_grad():
        logits = head(p, a)
        k = logits.argmax(dim=1)
        (g,) = torch.autograd.grad(logits.gather(1, k[:, None]).sum(), a)
    with torch.no_grad():
        alpha = g.mean(dim=(2, 3), keepdim=True)
        raw = torch.relu((alpha * a.detach()).sum(dim=1))
        m = raw.amax(dim=(1, 2), keepdim=True)
        heat = torch.where(m > 0, raw / m.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(raw))
        score = torch.softmax(logits.detach(), dim=1).gather(1, k[:, None])[:, 0]
    return k.to(torch.int32), score.float(), heat.float()


def _linear_head(weight: str, bias: str):
    return lambda p, a: a.mean(dim=(2, 3)) @ p[weight].t() + p[bias]


def _xception():
    from ..models import xception as X
    from .xception import XceptionEngine
    return ModelInfo("xception", X.INPUT_SIZE, 10, 21_067_390,
                     "Keras Xception 299x299 + clothing head (21,067,390 params)",
                     lambda seed=0: X.init_params(seed=seed),
                     lambda p, max_batch, device, **kw: XceptionEngine(p, max_batch=max_batch, device=device,
                                                                       in_kind="u8", **kw),
                     lambda p, x: X.xception_forward(p, x.float() / 127.5 - 1.0),
                     stage_cut="block8_sepconv3", features=X.DEFAULT_HEAD.features,
                     feature_oracle=lambda p, x: _no_grad_mean(X.base_forward, p, (x.float() / 127.5 - 1.0)
                                                               .permute(0, 3, 1, 2).contiguous()),
                     cam_oracle=lambda p, x, head=X.DEFAULT_HEAD: _cam(
                         X.base_forward, lambda q, a: X.head_forward(q, a, head), p,
                         (x.float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()),
                     map_size=(10, 10))


def _resnet50(dtype: str = "fp16"):
    """BASELINE.json config 3 is "ResNet-50 224x224 fp16": fp16 by default,
    ``resnet50_bf16`` for the bf16 variant (same kernels, v_mfma_*_bf16)."""
    from ..models import resnet as R
    from .resnet import ResNetEngine
    return ModelInfo("resnet50" if dtype == "fp16" else "resnet50_bf16", R.INPUT_SIZE, 1000, R.TOTAL_PARAMS,
                     f"ResNet-50 v1.5 224x224 (torchvision layout, 25,557,032 params), {dtype}",
                     lambda seed=0: R.init_params(seed=seed),
                     lambda p, max_batch, device, **kw: ResNetEngine(p, max_batch=max_batch, device=device,
                                                                     dtype=dtype, **kw),
                     # three stages (3 compute streams): +1.3-1.9 % over the round-2 cut after layer3.1
                     # (profiles/stages3_ab_r3.txt)
                     R.resnet_forward, dtype=dtype, tuning="resnet50", stage_cut="layer2.1.conv3,layer3.3.conv3",
                     features=2048, feature_oracle=lambda p, x: _no_grad_mean(R.features, p, R.preprocess(x)),
                     cam_oracle=lambda p, x: _cam(R.features, _linear_head("fc.weight", "fc.bias"), p,
                                                  R.preprocess(x)),
                     map_size=(7, 7))


def _vit_b16():
    from ..models import vit as V
    from .vit import ViTEngine
    return ModelInfo("vit_b16", V.INPUT_SIZE, 1000, V.TOTAL_PARAMS,
                     "ViT-B/16 224x224 (torchvision layout, 86,567,656 params)",
                     lambda seed=0: V.init_params(seed=seed),
                     lambda p, max_batch, device, **kw: ViTEngine(p, max_batch=max_batch, device=device, **kw),
                     V.vit_forward, stage_cut="encoder.layers.encoder_layer_5.mlp.3",
                     features=V.DIM, feature_oracle=V.vit_features,
                     rollout_oracle=V.vit_rollout, map_size=(V.INPUT_SIZE // V.PATCH, V.INPUT_SIZE // V.PATCH))


def _efficientnet_b7():
    from ..models import efficientnet as E
    from .efficientnet import EfficientNetEngine
    return ModelInfo("efficientnet_b7", E.INPUT_SIZE, 1000, E.TOTAL_PARAMS,
                     "EfficientNet-B7 600x600 (torchvision layout, 66,347,960 params)",
                     lambda seed=0: E.init_params(seed=seed),
                     lambda p, max_batch, device, **kw: EfficientNetEngine(p, max_batch=max_batch, device=device,
                                                                           **kw),
                     E.efficientnet_forward, stage_cut="features.4.9.block.3",
                     features=E.HEAD, feature_oracle=lambda p, x: _no_grad_mean(E.features, p, E.preprocess(x)),
                     cam_oracle=lambda p, x: _cam(E.features, _linear_head("classifier.1.weight",
                                                                           "classifier.1.bias"), p,
                                                  E.preprocess(x)),
                     map_size=(19, 19))


def _vit_b16_fp8():
    from ..models import vit as V
    from .vit import ViTEngine
    return ModelInfo("vit_b16_fp8", V.INPUT_SIZE, 1000, V.TOTAL_PARAMS,
                     "ViT-B/16 224x224, e4m3 linears (static per-tensor activation / per-channel weight scales)",
                     lambda seed=0: V.init_params(seed=seed),
                     lambda p, max_batch, device, **kw: ViTEngine(p, max_batch=max_batch, device=device, fp8=True,
                                                                  **kw),
                     V.vit_forward, dtype="fp8-e4m3 linears / bf16 rest",
                     stage_cut="encoder.layers.encoder_layer_5.mlp.3",
                     features=V.DIM, feature_oracle=V.vit_features,
                     rollout_oracle=V.vit_rollout, map_size=(V.INPUT_SIZE // V.PATCH, V.INPUT_SIZE // V.PATCH))


_FACTORIES = {"xception": _xception, "resnet50": _resnet50, "resnet50_bf16": lambda: _resnet50("bf16"),
              "vit_b16": _vit_b16, "vit_b16_fp8": _vit_b16_fp8, "efficientnet_b7": _efficientnet_b7}


# (family, --dtype) -> engine variant; "auto" keeps the family's own default
_VARIANTS = {("resnet50", "bf16"): "resnet50_bf16", ("resnet50_bf16", "fp16"): "resnet50",
             ("vit_b16", "fp8"): "vit_b16_fp8", ("vit_b16_fp8", "bf16"): "vit_b16"}
_DTYPES = {"xception": {"bf16"}, "resnet50": {"fp16"}, "resnet50_bf16": {"bf16"}, "vit_b16": {"bf16"},
           "vit_b16_fp8": {"fp8"}, "efficientnet_b7": {"bf16"}}


def variant(family: str, dtype: str = "auto") -> str:
    """The engine variant of `family` computing in `dtype` (server ``--dtype``)."""
    if dtype in ("auto", "") or dtype in _DTYPES.get(family, set()):
        return family
    v = _VARIANTS.get((family, dtype))
    if v is None:
        raise ValueError(f"{family} has no {dtype} engine (available: "
                         f"{sorted(_DTYPES.get(family, set()) | {d for (f, d) in _VARIANTS if f == family})})")
    return v


def models() -> list[str]:
    return sorted(_FACTORIES)


def get(name: str) -> ModelInfo:
    if name not in _FACTORIES:
        raise KeyError(f"unknown model {name!r}; known: {', '.join(models())}")
    return _FACTORIES[name]()
