"""The engines' output tails emit the programs they always did, and a data-parallel follower sets up.

Program identity: for every output mode the list of steps, the launches of the emitted program and the
shape of the output rows equal what was recorded (tests/golden/outputs/programs.json) before the
tail steps were described in one table: no launch added, removed or reordered. The numbers those
programs compute are pinned by the oracle tests of each mode."""
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "outputs" / "programs.json"
XCEPTION_CASES = ["plain", "topk", "embed_l2", "similar", "explain", "explain_overlay"]
VIT_CASES = ["rollout", "rollout_overlay"]


def engine_kwargs(case: str, features: int) -> dict:
    from kdl.engine.base import Overlay, Similar
    if case == "similar":
        g = torch.Generator().manual_seed(3)
        gallery = torch.randn((2, features), generator=g).to(torch.bfloat16).cuda()
        return dict(similar=Similar(gallery, 2, "cosine"))
    return {"plain": {}, "topk": dict(topk=2), "embed_l2": dict(embed="l2"), "explain": dict(explain=True),
            "explain_overlay": dict(explain=True, overlay=Overlay()), "rollout": dict(rollout=True),
            "rollout_overlay": dict(rollout=True, overlay=Overlay())}[case]


def describe(engine) -> dict:
    return {"steps": [[s.kind, s.name, s.src, s.dst] for s in engine.steps],
            "ops": list(engine.program(1, capture=False).op_names()),
            "logits": list(engine.logits.shape)}


def build(case: str):
    if case in XCEPTION_CASES:
        from kdl.engine.xception import XceptionEngine
        from kdl.models import xception as X
        return XceptionEngine(X.init_params(seed=0), max_batch=1, device="cuda", buckets=[1],
                              **engine_kwargs(case, X.DEFAULT_HEAD.features))
    from kdl.engine.vit import ViTEngine
    from kdl.models import vit as V
    return ViTEngine(V.init_params(seed=0), max_batch=1, device="cuda", buckets=[1], **engine_kwargs(case, V.DIM))


@pytest.mark.parametrize("case", XCEPTION_CASES + VIT_CASES)
def test_program_identity(case):
    want = json.loads(GOLDEN.read_text())[case]
    got = json.loads(json.dumps(describe(build(case))))
    assert got["logits"] == want["logits"]
    assert got["steps"] == want["steps"]
    assert got["ops"] == want["ops"]


def test_follower_setup(tmp_path):
    """A data-parallel follower's executor builds its engine, graphs and backend from the runner
    stand-in alone: no batcher, no RCCL, one device."""
    from kdl.serving.backend import NATIVE_SIGNATURE, GPUExecutor, load_version_dir
    from kdl.serving.config import BatchingParams, ServerConfig
    from kdl.serving.dp import _FollowerRunner
    source = load_version_dir(tmp_path, synthetic=True)
    cfg = ServerConfig(device="gpu", gpus=1, exec_depth=1,
                       batching=BatchingParams(max_batch_size=1, allowed_batch_sizes=[1]))
    ex = GPUExecutor(_FollowerRunner(source, source.signatures[NATIVE_SIGNATURE], cfg), 0, cfg.engine_kwargs())
    ex.setup()
    assert ex.backend is not None and len(ex._native_keep) == 1 and ex.native is None
    torch.cuda.synchronize()
