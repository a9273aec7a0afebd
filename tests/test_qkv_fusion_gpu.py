"""GPU: the QKV projection fused into attention (rc_model_set_qkv_fusion, csrc/qkv_attention.h).

The fused kernel runs the same MFMA chain, LayerNorm-fold epilogue and attention arithmetic as
gemm_pp_kernel<EPI_BF16_LN> + attention_v2_kernel<197>, so every comparison between mode 2
(fused whenever the shape qualifies) and mode 0 (off) is bitwise; the oracle tolerances are
those of test_embed_gpu.py.
"""
import numpy as np
import pytest

from conftest import import_pkg
from oracle.preprocess import preprocess
from oracle.vit import cosine, embed_cls
from oracle.weights import seeded_vit_msn_weights

pytestmark = pytest.mark.gpu

BF16_COS_TOL = 1e-2       # test_embed_gpu.py: the bf16 path against the fp32 oracle
FP32_TIER_COS_TOL = 1e-3  # test_embed_gpu.py: this build's regression guard


@pytest.fixture(scope="module")
def vitmod(cuda):
    return import_pkg("vit")


@pytest.fixture(scope="module")
def weights2():
    return seeded_vit_msn_weights(1907, num_layers=2)


@pytest.fixture(scope="module")
def weights12():
    return seeded_vit_msn_weights(1907)


def _embed_modes(m, imgs, modes=(0, 2)):
    import torch

    out = {}
    for mode in modes:
        m.set_qkv_fusion(mode)
        raw, nrm = m.embed(imgs)
        torch.cuda.synchronize()
        out[mode] = (raw.clone(), nrm.clone())
    return out


def test_two_layer_fused_equals_unfused_bitwise(vitmod, weights2, cuda):
    """Both layers fused (whole last layer): n = 1 (12 blocks, far fewer than the CUs), n = 3 (odd:
    the odd-parity XCDs have one image fewer) and n = 64 as two parts of 32 (the last image's pad
    rows end the part); heads 0 and 11 are the column extremes of every image."""
    import torch

    m = vitmod.VitMsnEmbedder(weights2, device=0, max_batch=64)
    m.set_last_layer(False)
    m.set_parts(2)
    rng = np.random.default_rng(41)
    imgs = torch.from_numpy(rng.integers(0, 256, (64, 224, 224, 3), dtype=np.uint8))
    for n in (1, 3, 64):
        out = _embed_modes(m, imgs[:n])
        assert torch.equal(out[2][0], out[0][0]) and torch.equal(out[2][1], out[0][1]), n
    m.close()


def test_twelve_layer_fused_matches_unfused_and_oracle(vitmod, weights12, cuda):
    """12 layers, default CLS-only last layer (11 fused layers, then K/V GEMM + attention_cls)."""
    import torch

    m = vitmod.VitMsnEmbedder(weights12, device=0, max_batch=8)
    rng = np.random.default_rng(43)
    imgs = rng.integers(0, 256, (5, 224, 224, 3), dtype=np.uint8)
    out = _embed_modes(m, torch.from_numpy(imgs))
    assert torch.equal(out[2][0], out[0][0]) and torch.equal(out[2][1], out[0][1])
    ref = embed_cls(np.stack([preprocess(x) for x in imgs]), weights12)
    got = out[2][0].cpu().numpy()
    for i in range(5):
        d = 1.0 - cosine(got[i], ref[i])
        assert d <= BF16_COS_TOL, (i, d)
        assert d <= FP32_TIER_COS_TOL, (i, d)
    m.close()


def test_fold_off_ignores_fusion(vitmod, weights2, cuda):
    """Without the LayerNorm fold the shape does not qualify: mode 2 runs the separate kernels."""
    import torch

    m = vitmod.VitMsnEmbedder(weights2, device=0, max_batch=4)
    m.set_ln_fold(False)
    rng = np.random.default_rng(47)
    imgs = rng.integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    out = _embed_modes(m, torch.from_numpy(imgs))
    assert torch.equal(out[2][0], out[0][0]) and torch.equal(out[2][1], out[0][1])
    ref = embed_cls(np.stack([preprocess(x) for x in imgs]), weights2)
    got = out[2][0].cpu().numpy()
    for i in range(3):
        assert 1.0 - cosine(got[i], ref[i]) <= BF16_COS_TOL
    with pytest.raises(Exception):
        m.set_qkv_fusion(3)
    m.close()


def test_mode_toggle_drops_captured_graph(vitmod, weights2, cuda):
    """The batch-1 graph bakes the launch chain in: toggling the mode re-captures, same vector."""
    import torch

    m = vitmod.VitMsnEmbedder(weights2, device=0, max_batch=2)
    rng = np.random.default_rng(53)
    x = torch.from_numpy(rng.integers(0, 256, (1, 224, 224, 3), dtype=np.uint8)).to(cuda)
    raw, nrm = torch.empty((1, 768), device=cuda), torch.empty((1, 768), device=cuda)
    got, prev = [], None
    for mode in (0, 0, 2, 2, 1, 0):  # capture and replay; every toggle captures again
        if mode != prev:
            m.set_qkv_fusion(mode)
            prev = mode
        m.embed(x, out=(raw, nrm))
        torch.cuda.synchronize()
        got.append((mode, raw.clone(), nrm.clone()))
    for mode, r, v in got[1:]:
        assert torch.equal(r, got[0][1]) and torch.equal(v, got[0][2]), mode
    m.close()
