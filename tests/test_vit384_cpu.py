"""ViT-B/16 at 384 x 384 without a GPU: the parameter count of torchvision's IMAGENET1K_SWAG_E2E_V1, the
registry entry, and the oracle's shapes at 384 and at the default size."""
import torch

from kdl.engine import registry
from kdl.models import vit as V


def test_parameter_count_and_registry():
    assert V.count_params(size=384) == 86_859_496 and V.count_params() == V.TOTAL_PARAMS
    assert V.param_shapes(size=384)["encoder.pos_embedding"] == (1, 577, 768)
    info = registry.get("vit_b16_384")
    assert info.input_size == 384 and info.map_size == (24, 24) and info.params_total == 86_859_496
    assert registry.variant("vit_b16_384", "fp8") == "vit_b16_384_fp8"
    assert registry.get("vit_b16_384_fp8").input_size == 384


def test_oracle_shapes_follow_size():
    for size, hw in ((384, 24), (224, 14)):
        kw = dict(size=size) if size != 224 else {}           # the defaults still answer as before
        p = V.init_params(seed=0, **kw)
        x = torch.randint(0, 256, (1, size, size, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
        assert V.vit_forward(p, x, **kw).shape == (1, 1000)
        c, s, heat = V.vit_rollout(p, x, **kw)
        assert c.shape == (1,) and s.shape == (1,) and heat.shape == (1, hw, hw)
