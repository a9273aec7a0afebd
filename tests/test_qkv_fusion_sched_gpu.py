"""GPU: the fused QKV + attention kernel's wave schedule (csrc/qkv_attention.h).

The kernel refills a ring slot among the MFMAs of the step after the slot's last reads, reads its
fragments behind counted LDS waits and loads its epilogue operands before the barrier that frees
the ring.  A race between a refilled slot and a late reader would show as a mismatch against the
separate kernels or as run-to-run differences, and only once two workgroups share a CU: so the
comparisons run with more workgroups than the device has resident slots, and all are bitwise.
"""
import numpy as np
import pytest

from conftest import import_pkg
from oracle.weights import seeded_vit_msn_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vitmod(cuda):
    return import_pkg("vit")


@pytest.fixture(scope="module")
def embedder(vitmod):
    """Two seeded layers, both fused (whole last layer), one stream."""
    m = vitmod.VitMsnEmbedder(seeded_vit_msn_weights(1907, num_layers=2), device=0, max_batch=45)
    m.set_last_layer(False)
    m.set_parts(1)
    yield m
    m.close()


def _embed(m, imgs, mode):
    """(raw, nrm) as their bit patterns: equal means the same bits, NaNs and signed zeros included."""
    import torch

    m.set_qkv_fusion(mode)
    raw, nrm = m.embed(imgs)
    torch.cuda.synchronize()
    return raw.clone().view(torch.int32), nrm.clone().view(torch.int32)


def test_co_resident_blocks_bitwise_and_repeatable(embedder, cuda):
    """n = 45 images: 540 workgroups, more than the 512 resident slots (256 CUs x 2), so CUs hold
    two workgroups and a second round starts; odd n also takes the parity path.  Fused equals
    unfused bitwise, and three fused runs in a row equal each other bitwise."""
    import torch

    rng = np.random.default_rng(59)
    imgs = torch.from_numpy(rng.integers(0, 256, (45, 224, 224, 3), dtype=np.uint8))
    ref = _embed(embedder, imgs, 0)
    runs = [_embed(embedder, imgs, 2) for _ in range(3)]
    for i, (raw, nrm) in enumerate(runs):
        assert torch.equal(raw, ref[0]) and torch.equal(nrm, ref[1]), i
    for raw, nrm in runs[1:]:
        assert torch.equal(raw, runs[0][0]) and torch.equal(nrm, runs[0][1])


def test_extreme_row_scales_bitwise(embedder, cuda):
    """One all-zero and one all-255 image: constant rows, tiny variance, large rstd."""
    import torch

    imgs = torch.zeros((2, 224, 224, 3), dtype=torch.uint8)
    imgs[1] = 255
    ref = _embed(embedder, imgs, 0)
    got = _embed(embedder, imgs, 2)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
