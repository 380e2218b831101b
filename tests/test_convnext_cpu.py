"""ConvNeXt-Tiny without a GPU: the oracle's layout and block, the host-side weight folds and the
registry entry."""
import torch
import torch.nn.functional as F

from kdl.engine import registry
from kdl.models import convnext as CX
from kdl.ops.pack import fold_layer_scale, s2d_weights

KEYS = {"features.0.0.weight": (96, 3, 4, 4), "features.1.0.block.0.weight": (96, 1, 7, 7),
        "features.1.0.layer_scale": (96, 1, 1), "features.2.1.weight": (192, 96, 2, 2),
        "classifier.0.weight": (768,), "classifier.2.weight": (1000, 768)}


def test_params_match_torchvision_layout():
    p = CX.init_params(seed=1)
    assert sum(v.numel() for v in p.values()) == CX.count_params() == CX.TOTAL_PARAMS == 28_589_128
    assert {k: tuple(p[k].shape) for k in KEYS} == KEYS
    assert list(p)[0] == "features.0.0.weight" and list(p)[-1] == "classifier.2.bias"
    ls = torch.cat([v.flatten() for k, v in p.items() if k.endswith("layer_scale")])
    assert 0.05 <= ls.min() and ls.max() <= 0.2


def test_block_is_the_functional_composition():
    p, b, c = CX.init_params(seed=2), "features.3.1", 192
    x = torch.randn(2, c, 6, 5, generator=torch.Generator().manual_seed(3))
    h = F.conv2d(x, p[f"{b}.block.0.weight"], p[f"{b}.block.0.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
    mu, var = h.mean(-1, keepdim=True), h.var(-1, unbiased=False, keepdim=True)
    h = (h - mu) / torch.sqrt(var + 1e-6) * p[f"{b}.block.2.weight"] + p[f"{b}.block.2.bias"]
    h = F.linear(F.gelu(F.linear(h, p[f"{b}.block.3.weight"], p[f"{b}.block.3.bias"])), p[f"{b}.block.5.weight"],
                 p[f"{b}.block.5.bias"])
    want = x + p[f"{b}.layer_scale"] * h.permute(0, 3, 1, 2)
    torch.testing.assert_close(CX.block(p, b, x), want, rtol=1e-5, atol=1e-5)


def test_layer_scale_fold_and_s2d_repack_reproduce_the_unfolded_result():
    g = torch.Generator().manual_seed(4)
    w, b, ls = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((24, 96), (24,), (24, 1, 1)))
    h = torch.randn(5, 96, generator=g, dtype=torch.float64)
    wf, bf = fold_layer_scale(w, b, ls)
    torch.testing.assert_close(h @ wf.t() + bf, ls.reshape(-1) * (h @ w.t() + b), rtol=1e-13, atol=1e-13)
    wc, x = torch.randn(16, 8, 2, 2, generator=g, dtype=torch.float64), torch.randn(2, 8, 4, 6, generator=g, dtype=torch.float64)
    rows = x.permute(0, 2, 3, 1).reshape(2, 2, 2, 3, 2, 8).permute(0, 1, 3, 2, 4, 5).reshape(12, 32)   # ln_s2d's order
    want = F.conv2d(x, wc, stride=2).permute(0, 2, 3, 1).reshape(12, 16)
    torch.testing.assert_close(rows @ s2d_weights(wc).t(), want, rtol=1e-13, atol=1e-13)


def test_registry_entry():
    info = registry.get("convnext_tiny")
    assert (info.input_size, info.classes, info.features, info.dtype) == (224, 1000, 768, "bf16")
    assert info.cam_oracle is None and info.rollout_oracle is None and info.feature_oracle is not None
    assert registry.variant("convnext_tiny", "auto") == registry.variant("convnext_tiny", "bf16") == "convnext_tiny"
