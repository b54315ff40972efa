"""The top-k limit, stated once (ops.MAX_TOPK, the C checks' topk <= 1024): every scoring entry point refuses k outside [1, MAX_TOPK] with a
ValueError naming the limit before it touches a tensor -- so these run on CPU tensors, without a GPU or a key cache."""
import importlib

import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def idm():
    pkg = importlib.import_module("6dgs_amd")
    return pkg.IdentificationModule("dino")


def test_max_topk_matches_the_library_checks():
    ops = importlib.import_module("6dgs_amd.ops")
    assert ops.MAX_TOPK == 1024
    assert ops.check_topk(1) == 1 and ops.check_topk(1024) == 1024 and ops.check_topk(100.0) == 100
    for bad in (0, -1, 1025, 2000, 4096, 100.5, True):
        with pytest.raises(ValueError, match="1024"):
            ops.check_topk(bad)


@pytest.mark.parametrize("k", [0, 1025, 2000, 4096])
def test_scorers_refuse_k_outside_the_limit(idm, k):
    toks = [torch.zeros(5, 398)]
    rays = (torch.zeros(10, 3),) * 3
    for want in (False, True):
        with pytest.raises(ValueError, match="MAX_TOPK = 1024"):
            idm.score_tokens(toks, *rays, k, want_scores=want)
    with pytest.raises(ValueError, match="MAX_TOPK = 1024"):
        idm.score_tokens_streamed(toks, *rays, k)
    with pytest.raises(ValueError, match="MAX_TOPK = 1024"):
        idm.score_tokens_ray_sharded(toks, *rays, 0, 10, k)
    with pytest.raises(ValueError, match="MAX_TOPK = 1024"):
        idm.test_images([torch.zeros(3, 28, 28)], [None], *rays, k)
