"""ResNeXt-50 32x4d: the parametrised ResNet oracle, its registry entries (no GPU)."""
import json

import torch
import torch.nn.functional as F

from kdl.engine import registry
from kdl.models import resnet as R

ARCH = R.RESNEXT50_32X4D


def test_registry_entries_and_parameter_count():
    info = registry.get("resnext50_32x4d")
    assert info.params_total == 25_028_904 == R.count_params(**ARCH)
    assert (info.dtype, info.features, info.map_size, info.tuning) == ("fp16", 2048, (7, 7), "")
    assert registry.get("resnext50_32x4d_bf16").dtype == "bf16"
    assert registry.variant("resnext50_32x4d", "bf16") == "resnext50_32x4d_bf16"
    assert registry.variant("resnext50_32x4d_bf16", "fp16") == "resnext50_32x4d"
    assert registry.variant("resnext50_32x4d", "fp16") == registry.variant("resnext50_32x4d") == "resnext50_32x4d"
    shapes = R.param_shapes(**ARCH)
    assert set(shapes) == set(R.param_shapes())
    assert shapes["layer1.0.conv2.weight"] == (128, 4, 3, 3) and shapes["layer4.2.conv2.weight"] == (1024, 32, 3, 3)


def test_macs_equal_a_sum_over_the_layers():
    total, h = 112 * 112 * 64 * 147 + 2048 * 1000, 56
    for planes, n, stride in R.STAGES:
        width, cin = planes * 2, 64 if planes == 64 else planes * 2
        for i in range(n):
            oh = h // stride if i == 0 else h
            total += h * h * cin * width + oh * oh * width * (width // 32) * 9 + oh * oh * width * planes * 4
            if i == 0:
                total += oh * oh * cin * planes * 4
            h, cin = oh, planes * 4
    assert R.macs_per_image(**ARCH) == total


def test_oracle_equals_float64_blocks_with_grouped_conv2d():
    p = R.init_params(seed=1, calibrate=False, **ARCH)
    x = torch.randint(0, 256, (2, 64, 64, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    got = R.resnet_forward(p, x, **ARCH)
    q = {k: v.double() for k, v in p.items()}

    def bn(t, n):
        s = q[f"{n}.weight"] / torch.sqrt(q[f"{n}.running_var"] + R.BN_EPS)
        return t * s[None, :, None, None] + (q[f"{n}.bias"] - q[f"{n}.running_mean"] * s)[None, :, None, None]

    t = F.max_pool2d(torch.relu(bn(F.conv2d(R.preprocess(x).double(), q["conv1.weight"], stride=2, padding=3), "bn1")), 3, 2, 1)
    for si, (planes, n, stride) in enumerate(R.STAGES, start=1):
        for i in range(n):
            pre, s = f"layer{si}.{i}", stride if i == 0 else 1
            y = torch.relu(bn(F.conv2d(t, q[f"{pre}.conv1.weight"]), f"{pre}.bn1"))
            assert y.shape[1] == planes * 2
            y = torch.relu(bn(F.conv2d(y, q[f"{pre}.conv2.weight"], stride=s, padding=1, groups=32), f"{pre}.bn2"))
            y = bn(F.conv2d(y, q[f"{pre}.conv3.weight"]), f"{pre}.bn3")
            if i == 0:
                t = bn(F.conv2d(t, q[f"{pre}.downsample.0.weight"], stride=s), f"{pre}.downsample.1")
            t = torch.relu(y + t)
    want = t.mean(dim=(2, 3)) @ q["fc.weight"].t() + q["fc.bias"]
    assert got.shape == (2, 1000)
    assert (got.double() - want).abs().max() <= 1e-4 * want.abs().max()


def test_cpu_load_lists_the_signatures_of_resnet50(tmp_path):
    from kdl.serving.backend import load_version_dir
    sigs = {}
    for fam in ("resnet50", "resnext50_32x4d"):
        d = tmp_path / fam / "1"
        d.mkdir(parents=True)
        (d / "synthetic.json").write_text(json.dumps({"seed": 0, "model": fam}))
        src = load_version_dir(d, synthetic=True)
        assert src.family == fam and src.classes == 1000
        sigs[fam] = {n: (s.input_key, s.input_shape, s.output_key, s.output_shape) for n, s in src.signatures.items()}
    assert sigs["resnext50_32x4d"] == sigs["resnet50"] and len(sigs["resnet50"]) > 4
    assert src.params["layer3.0.conv2.weight"].shape == (512, 16, 3, 3)
