"""ConvNeXt-Tiny (Liu et al. 2022; torchvision ``convnext_tiny`` layout) as an fp32 torch oracle.

Parameters use torchvision's state_dict names (``features.0.0.weight`` .. ``classifier.2.bias``), so a
real checkpoint (``torch.load(..., weights_only=True)``) drops in:

    features.0            stem: Conv2d(3, 96, 4, stride 4) (.0), LayerNorm2d(96) (.1)
    features.1 / 3 / 5 / 7  stages of 3 / 3 / 9 / 3 blocks on 96 / 192 / 384 / 768 channels; a block is
                          depthwise 7x7 pad 3 (block.0), LayerNorm over C (block.2), Linear C -> 4C
                          (block.3), exact GELU, Linear 4C -> C (block.5), times ``layer_scale``
                          [C, 1, 1], plus the block's input (stochastic depth is off at inference)
    features.2 / 4 / 6    downsample: LayerNorm2d (.0), Conv2d(C, 2C, 2, stride 2) (.1)
    classifier            global average pool, LayerNorm2d(768) (.0), Linear(768, 1000) (.2)

LayerNorm eps 1e-6. Preprocessing is torchvision's: uint8 RGB -> x / 255 -> (x - mean) / std.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

INPUT_SIZE = 224
NUM_CLASSES = 1000
LN_EPS = 1e-6
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
DEPTHS = (3, 3, 9, 3)
DIMS = (96, 192, 384, 768)
PATCH = 4
TOTAL_PARAMS = 28_589_128          # torchvision convnext_tiny


def stage_prefix(i: int) -> str:
    """Stage i (0..3) is ``features.{2 i + 1}``; the downsample in front of it ``features.{2 i}``."""
    return f"features.{2 * i + 1}"


def block_names() -> list[tuple[str, int]]:
    """(prefix, channels) of the 18 blocks in forward order."""
    return [(f"{stage_prefix(i)}.{j}", c) for i, (n, c) in enumerate(zip(DEPTHS, DIMS)) for j in range(n)]


def param_shapes(num_classes: int = NUM_CLASSES) -> dict[str, tuple]:
    s = {"features.0.0.weight": (DIMS[0], 3, PATCH, PATCH), "features.0.0.bias": (DIMS[0],),
         "features.0.1.weight": (DIMS[0],), "features.0.1.bias": (DIMS[0],)}
    for i, (n, c) in enumerate(zip(DEPTHS, DIMS)):
        if i:
            d = f"features.{2 * i}"
            s.update({f"{d}.0.weight": (DIMS[i - 1],), f"{d}.0.bias": (DIMS[i - 1],),
                      f"{d}.1.weight": (c, DIMS[i - 1], 2, 2), f"{d}.1.bias": (c,)})
        for j in range(n):
            b = f"{stage_prefix(i)}.{j}"
            s.update({f"{b}.layer_scale": (c, 1, 1),
                      f"{b}.block.0.weight": (c, 1, 7, 7), f"{b}.block.0.bias": (c,),
                      f"{b}.block.2.weight": (c,), f"{b}.block.2.bias": (c,),
                      f"{b}.block.3.weight": (4 * c, c), f"{b}.block.3.bias": (4 * c,),
                      f"{b}.block.5.weight": (c, 4 * c), f"{b}.block.5.bias": (c,)})
    s.update({"classifier.0.weight": (DIMS[-1],), "classifier.0.bias": (DIMS[-1],),
              "classifier.2.weight": (num_classes, DIMS[-1]), "classifier.2.bias": (num_classes,)})
    return s


def count_params(num_classes: int = NUM_CLASSES) -> int:
    return sum(math.prod(v) for v in param_shapes(num_classes).values())


def init_params(seed: int = 0, num_classes: int = NUM_CLASSES) -> dict[str, torch.Tensor]:
    """Random init of the exact architecture. ``layer_scale`` is uniform in [0.05, 0.2], not
    torchvision's initial 1e-6: at 1e-6 every block is the identity to bf16 precision and no
    comparison against this oracle could see the block's kernels. (Trained checkpoints have
    layer scales of this order.) LayerNorm gains are near 1, their biases small."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k, shp in param_shapes(num_classes).items():
        if k.endswith("layer_scale"):
            t = 0.05 + 0.15 * torch.rand(shp, generator=g)
        elif len(shp) == 4:                       # convs: fan-in of one output
            t = torch.randn(shp, generator=g) * (1.0 / (shp[1] * shp[2] * shp[3])) ** 0.5
        elif len(shp) == 2:                       # linears [out, in]
            t = torch.randn(shp, generator=g) * (1.0 / shp[1]) ** 0.5
        elif k.endswith(".weight"):               # LayerNorm gains
            t = 0.8 + 0.4 * torch.rand(shp, generator=g)
        else:                                     # biases
            t = torch.randn(shp, generator=g) * 0.02
        p[k] = t.float()
    assert sum(v.numel() for v in p.values()) == (TOTAL_PARAMS if num_classes == NUM_CLASSES
                                                  else count_params(num_classes))
    return p


def preprocess(x_u8_nhwc: torch.Tensor) -> torch.Tensor:
    """uint8 NHWC -> normalised fp32 NCHW (torchvision transforms.Normalize)."""
    x = x_u8_nhwc.float().permute(0, 3, 1, 2) / 255.0
    return (x - torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)) / torch.tensor(STD, device=x.device).view(1, 3, 1, 1)


def layer_norm2d(p, name: str, x_nchw: torch.Tensor) -> torch.Tensor:
    """torchvision's LayerNorm2d: LayerNorm over the channels of every pixel."""
    c = x_nchw.shape[1]
    y = F.layer_norm(x_nchw.permute(0, 2, 3, 1), (c,), p[f"{name}.weight"], p[f"{name}.bias"], LN_EPS)
    return y.permute(0, 3, 1, 2)


def block(p, b: str, x_nchw: torch.Tensor) -> torch.Tensor:
    """One CNBlock: x + layer_scale * mlp(LN(dwconv7(x)))."""
    c = x_nchw.shape[1]
    h = F.conv2d(x_nchw, p[f"{b}.block.0.weight"], p[f"{b}.block.0.bias"], padding=3, groups=c)
    h = F.layer_norm(h.permute(0, 2, 3, 1), (c,), p[f"{b}.block.2.weight"], p[f"{b}.block.2.bias"], LN_EPS)
    h = F.gelu(h @ p[f"{b}.block.3.weight"].t() + p[f"{b}.block.3.bias"])
    h = h @ p[f"{b}.block.5.weight"].t() + p[f"{b}.block.5.bias"]
    return x_nchw + p[f"{b}.layer_scale"] * h.permute(0, 3, 1, 2)


@torch.no_grad()
def features(p, x_nchw: torch.Tensor, trace: dict | None = None) -> torch.Tensor:
    """Normalised fp32 NCHW -> the last stage's map [B, 768, H / 32, W / 32]. ``trace``: a dict that
    receives every block's and downsample's output by name (per-block comparisons)."""
    x = F.conv2d(x_nchw, p["features.0.0.weight"], p["features.0.0.bias"], stride=PATCH)
    x = layer_norm2d(p, "features.0.1", x)
    if trace is not None:
        trace["features.0"] = x
    for i, n in enumerate(DEPTHS):
        if i:
            d = f"features.{2 * i}"
            x = F.conv2d(layer_norm2d(p, f"{d}.0", x), p[f"{d}.1.weight"], p[f"{d}.1.bias"], stride=2)
            if trace is not None:
                trace[d] = x
        for j in range(n):
            x = block(p, f"{stage_prefix(i)}.{j}", x)
            if trace is not None:
                trace[f"{stage_prefix(i)}.{j}"] = x
    return x


@torch.no_grad()
def convnext_forward(p, x_u8_nhwc: torch.Tensor) -> torch.Tensor:
    """fp32 oracle: uint8 NHWC [B,224,224,3] -> logits [B,1000]."""
    f = features(p, preprocess(x_u8_nhwc)).mean(dim=(2, 3))
    f = F.layer_norm(f, (f.shape[1],), p["classifier.0.weight"], p["classifier.0.bias"], LN_EPS)
    return f @ p["classifier.2.weight"].t() + p["classifier.2.bias"]


def macs_per_image(size: int = INPUT_SIZE) -> int:
    """Multiply-accumulates of one forward (convs + linears)."""
    h = size // PATCH
    total = h * h * DIMS[0] * 3 * PATCH * PATCH
    for i, (n, c) in enumerate(zip(DEPTHS, DIMS)):
        if i:
            h //= 2
            total += h * h * c * DIMS[i - 1] * 4
        total += n * h * h * (c * 49 + 8 * c * c)
    return total + DIMS[-1] * NUM_CLASSES
