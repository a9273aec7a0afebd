"""GPU: the embedder at input sizes below 224 (rc_model_create takes every multiple of 16 up to 224).

Every size but 224 runs attention_v2_kernel<0> (the runtime token count: key tiles wholly or partly
masked, fewer than 13 query tiles, waves without a tile under qsplit = 4), GEMMs of M = n·tokens
rows at rows-per-image values of 2 .. 170, a patch GEMM of one patch per image at size 16, and
attention_cls_kernel below 64 tokens.  A two-layer seeded model per size against the numpy fp32
oracle at the project's bars; the cosine of the CLS row is a weak measure at these sizes too, so
the bitwise invariants (batch against single images, parts, fusion setting) carry most of the weight.
"""
import ctypes

import numpy as np
import pytest

from conftest import import_pkg
from oracle.pil_resample import BICUBIC, BILINEAR
from oracle.preprocess import VIT_MSN_PREPROCESS, preprocess
from oracle.vit import cosine, embed_cls
from oracle.weights import seeded_vit_msn_weights

pytestmark = pytest.mark.gpu

BF16_COS_TOL = 1e-2        # tests/test_embed_gpu.py: the bf16 path's bound
FP32_TIER_COS_TOL = 1e-3   # tests/test_embed_gpu.py: the fp32 tier's bound, this build's regression guard
SIZES = [16, 32, 64, 112, 192, 208]  # 2, 5, 17, 50, 145, 170 tokens
N_PARTS = 67  # two parts of 33 and 34 images (a part takes at least 32)


def tokens_of(S):
    return (S // 16) ** 2 + 1


def n_big(S):
    """A batch whose n·tokens rows cross 256: the tiled GEMMs instead of the skinny ones."""
    return max(5, 256 // tokens_of(S) + 1)


class SizedModel:
    def __init__(self, vitmod, S):
        self.S, self.n = S, n_big(S)
        self.sd = seeded_vit_msn_weights(1907, num_layers=2, image_size=S)
        self.params = dict(VIT_MSN_PREPROCESS, size=(S, S))
        self.m = vitmod.VitMsnEmbedder(self.sd, device=0, max_batch=max(self.n, N_PARTS),
                                       model_config={"image_size": S, "num_hidden_layers": 2}, preprocess=self.params)
        rng = np.random.default_rng(S)
        self.imgs = rng.integers(0, 256, (self.n, S, S, 3), dtype=np.uint8)
        self.ref = embed_cls(np.stack([preprocess(x, self.params) for x in self.imgs]), self.sd)  # computed once

    def embed(self, imgs):
        import torch

        raw, _ = self.m.embed(torch.from_numpy(np.ascontiguousarray(imgs)))
        torch.cuda.synchronize()
        return raw


@pytest.fixture(scope="module", params=SIZES, ids=lambda S: f"s{S}")
def sized(request, cuda):
    sm = SizedModel(import_pkg("vit"), request.param)
    yield sm
    sm.m.close()


def assert_within_bars(tag, got, ref):
    assert np.isfinite(got).all()
    d = 1.0 - cosine(got, ref)
    print(f"EMBED_SIZE_COS {tag} max_cosine_distance={float(np.max(d)):.3e}")
    assert np.all(d <= BF16_COS_TOL)
    assert np.all(d <= FP32_TIER_COS_TOL)


def test_matches_oracle_with_both_last_layer_forms(sized):
    """raw is finite and within BF16_COS_TOL and FP32_TIER_COS_TOL of the oracle at n = 1, n = 3 and
    the batch that crosses 256 rows, with the CLS-only last layer and with the whole last layer, and
    the two forms agree within the 1e-4 of test_cls_only_last_layer_matches_full_layer.

    Largest cosine distance to the oracle measured on the MI355X per size, over every run of this
    file (both last-layer forms, fold on and off, resized input): 16: 7.5e-5, 32: 1.0e-4,
    64: 9.4e-5, 112: 9.5e-5, 192: 7.3e-5, 208: 8.8e-5 — FP32_TIER_COS_TOL holds at every size."""
    s = sized
    outs = {}
    try:
        for cls_only in (True, False):
            s.m.set_last_layer(cls_only)
            for n in (1, 3, s.n):
                got = s.embed(s.imgs[:n]).cpu().numpy()
                assert_within_bars(f"S={s.S} n={n} cls_only={int(cls_only)}", got, s.ref[:n])
            outs[cls_only] = got
    finally:
        s.m.set_last_layer(True)
    assert np.all(1.0 - cosine(outs[True], outs[False]) <= 1e-4)


def test_resized_input_matches_oracle(sized):
    """Images of another size: the device resize to S x S runs first (Pillow-exact)."""
    s = sized
    rng = np.random.default_rng(1000 + s.S)
    imgs = rng.integers(0, 256, (3, 150, 97, 3), dtype=np.uint8)
    ref = embed_cls(np.stack([preprocess(x, s.params) for x in imgs]), s.sd)
    assert_within_bars(f"S={s.S} n=3 resized-from=150x97", s.embed(imgs).cpu().numpy(), ref)


def test_ln_fold_off_matches_fold(sized):
    """The standalone LayerNorm kernel against the fold: the 1e-3 of test_ln_fold_matches_unfused_and_oracle,
    and the unfolded form within the bars of the oracle as well."""
    s = sized
    fold = s.embed(s.imgs).cpu().numpy()
    try:
        s.m.set_ln_fold(False)
        plain = s.embed(s.imgs).cpu().numpy()
    finally:
        s.m.set_ln_fold(True)
    assert np.all(1.0 - cosine(fold, plain) <= 1e-3)
    assert_within_bars(f"S={s.S} n={s.n} ln_fold=0", plain, s.ref)


def test_batch_equals_single_images_bitwise(sized):
    """An image's embedding does not depend on its batch: skinny GEMMs (n = 1, 3), tiled ones (the
    batch that crosses 256 rows) and the batch-1 graph replay give the same bits."""
    import torch

    s = sized
    big = s.embed(s.imgs)
    three = s.embed(s.imgs[:3])
    assert torch.equal(three, big[:3])
    for i in sorted({0, 1, 2, s.n // 2, s.n - 1}):
        one = s.embed(s.imgs[i:i + 1])
        assert torch.equal(one[0], big[i]), i
        again = s.embed(s.imgs[i:i + 1])  # the captured graph's replay
        assert torch.equal(again[0], big[i]), i


def test_parts_and_fusion_setting_change_no_bits(sized):
    """set_parts(2) (67 images: parts of 33 and 34 on two streams) equals set_parts(1) bit for bit;
    set_qkv_fusion(2) equals 0 bit for bit (the shape does not qualify for the fused kernel, so
    nothing may change)."""
    import torch

    s = sized
    rng = np.random.default_rng(2000 + s.S)
    imgs = rng.integers(0, 256, (N_PARTS, s.S, s.S, 3), dtype=np.uint8)
    try:
        s.m.set_parts(1)
        s.m.set_qkv_fusion(0)
        one = s.embed(imgs)
        assert bool(torch.isfinite(one).all())
        s.m.set_qkv_fusion(2)
        assert torch.equal(s.embed(imgs), one)
        s.m.set_qkv_fusion(0)
        s.m.set_parts(2)
        assert torch.equal(s.embed(imgs), one)
    finally:
        s.m.set_parts(2)
        s.m.set_qkv_fusion(1)


@pytest.mark.parametrize("resample", [BICUBIC, BILINEAR])
def test_preprocess_at_112_bit_exact(cuda, resample):
    """rc_preprocess at image_size 112 equals oracle.preprocess bit for bit, for both filters."""
    import torch

    S = 112
    params = dict(VIT_MSN_PREPROCESS, size=(S, S), resample=resample)
    sd = seeded_vit_msn_weights(1907, num_layers=1, image_size=S)
    m = import_pkg("vit").VitMsnEmbedder(sd, device=0, max_batch=3, model_config={"image_size": S, "num_hidden_layers": 1},
                                         preprocess=params)
    try:
        for h, w in [(112, 112), (300, 168), (97, 480), (50, 112), (16, 16)]:
            rng = np.random.default_rng(h * 1000 + w)
            imgs = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
            got = m.preprocess(torch.from_numpy(imgs)).cpu().numpy()
            ref = np.stack([preprocess(x, params) for x in imgs])
            assert np.array_equal(got, ref), (h, w)
    finally:
        m.close()


@pytest.mark.parametrize("image_size", [240, 100])
def test_model_create_refuses_other_sizes(cuda, image_size):
    """Above 224 (more tokens than attention_v2_kernel's LDS holds) and not a multiple of 16."""
    L = import_pkg("_lib")
    lib = L.load()
    cfg = L.VitConfig(image_size, 16, 768, 2, 12, 3072, 1e-6, 2)
    m = ctypes.c_void_p()
    assert lib.rc_model_create(0, ctypes.byref(cfg), ctypes.byref(m)) == L.RC_ERR_UNSUPPORTED
    assert b"image_size" in lib.rc_last_error()
