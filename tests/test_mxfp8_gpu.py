"""The MXFP8 MLP (rc_model_set_mlp_dtype(1)): quantiser, fc2 kernel, fc1 epilogue and the model mode,
each against a plain high-precision restatement.

The format (include/retrieval_core.h, rc_mxfp8_quantize): blocks of 32 along K, a = max|x|,
e = floor(log2 a) - 8, one more if a > 448 * 2^e, clamped to [-127, 127], e = -127 for a == 0; scale
byte e + 127; element = e4m3fn nearest x * 2^-e, ties to even.
"""
import numpy as np
import pytest

from conftest import import_pkg
from oracle.preprocess import preprocess
from oracle.vit import cosine, embed_cls
from oracle.weights import seeded_vit_msn_weights

pytestmark = pytest.mark.gpu


def mx_exponent(a):
    """The rule's e for block maxima a (float64 array)."""
    _, ex = np.frexp(a)  # a = m * 2^ex, m in [0.5, 1): floor(log2 a) = ex - 1
    e = ex - 1.0 - 8.0
    e = e + (a > 448.0 * 2.0 ** e)
    return np.where(a == 0, -127.0, np.clip(e, -127.0, 127.0))


def mx_quantize_ref(x):
    """x [R][K] float32 numpy -> (bytes [R][K] u8, scale bytes [R][K/32] u8) by the rule."""
    import torch

    R, K = x.shape
    b = x.astype(np.float64).reshape(R, K // 32, 32)
    e = mx_exponent(np.abs(b).max(-1))
    scaled = torch.from_numpy((b * 2.0 ** -e[..., None]).astype(np.float32))
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8).numpy().reshape(R, K)
    return q, (e + 127).astype(np.uint8)


def mx_dequantize(q, s):
    """bytes [R][K] u8 and scale bytes [R][K/32] u8 (torch, any device) -> float64 numpy [R][K]."""
    import torch

    v = q.cpu().contiguous().view(torch.float8_e4m3fn).float().double().numpy()
    return v * np.repeat(2.0 ** (s.cpu().numpy().astype(np.float64) - 127.0), 32, axis=1)


def quantize(x):
    import torch

    L = import_pkg("_lib")
    R, K = x.shape
    q = torch.empty((R, K), dtype=torch.uint8, device=x.device)
    s = torch.empty((R, K // 32), dtype=torch.uint8, device=x.device)
    L.check(L.load().rc_mxfp8_quantize(x.data_ptr(), int(x.dtype == torch.bfloat16), R, K, q.data_ptr(), s.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return q, s


@pytest.mark.parametrize("src", ["f32", "bf16"])
@pytest.mark.parametrize("K", [32, 3072])
@pytest.mark.parametrize("R", [1, 33])
def test_quantize_bit_exact(cuda, R, K, src):
    """Equality.  Special blocks: zero; a power-of-two maximum; a maximum in (448, 512) * 2^e (the bump);
    1.0 beside 1e-30, e4m3 subnormals and a tie between two of them."""
    import torch

    rng = np.random.default_rng(R * 7 + K)
    nb = R * K // 32
    blocks = rng.standard_normal((nb, 32)) * 2.0 ** rng.integers(-20, 20, (nb, 1))
    pow2 = rng.uniform(-3, 3, 32)
    pow2[5] = -4.0
    bump = rng.uniform(-100, 100, 32)
    bump[3] = 480.0
    mix = np.zeros(32)
    mix[:4] = [1.0, 1e-30, 2.0 ** -16, 3 * 2.0 ** -18]
    for i, sp in enumerate([np.zeros(32), pow2, bump, mix]):
        blocks[(i * 5) % nb] = sp
    x = torch.from_numpy(blocks.reshape(R, K).astype(np.float32)).to(cuda)
    if src == "bf16":
        x = x.to(torch.bfloat16)
    q, s = quantize(x)
    rq, rs = mx_quantize_ref(x.float().cpu().numpy())
    assert np.array_equal(s.cpu().numpy(), rs)
    assert np.array_equal(q.cpu().numpy(), rq)


@pytest.mark.parametrize("K", [128, 3072])
@pytest.mark.parametrize("M", [257, 394, 512])
def test_fc2_kernel_matches_float64_of_dequantised_operands(cuda, M, K):
    """rc_gemm_mxfp8 against float64 of the dequantised operands (quantisation is outside this test).
    Bound: f32 accumulation over K terms, K * 2^-24 * sum|a||w|, times 2 for an accumulation tree that
    may truncate, plus the stream's rounding of the stored sum, 2^-9 |ref| ("MXFP8 MLP", has
    the figures against the first term alone).  A holds exactly M rows (rows past M are clamped), out
    three rows more, which stay untouched."""
    import torch

    L = import_pkg("_lib")
    g = torch.Generator(device=cuda).manual_seed(M + K)
    A8, As = quantize(torch.randn(M, K, device=cuda, generator=g) * torch.rand(M, 1, device=cuda, generator=g) * 4)
    W8, Ws = quantize(torch.randn(768, K, device=cuda, generator=g) * 0.05)
    bias = torch.randn(768, device=cuda, generator=g) * 0.1
    resid = torch.randn(M + 3, 768, device=cuda, generator=g)
    out = resid.clone()
    L.check(L.load().rc_gemm_mxfp8(A8.data_ptr(), As.data_ptr(), W8.data_ptr(), Ws.data_ptr(), bias.data_ptr(), M, 768, K,
                                   out.data_ptr(), 197, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    a, w = mx_dequantize(A8, As), mx_dequantize(W8, Ws)
    b, r = bias.double().cpu().numpy(), resid.double().cpu().numpy()
    ref = a @ w.T + b + r[:M]
    tol = 2 * K * 2.0 ** -24 * (np.abs(a) @ np.abs(w).T) + 2.0 ** -9 * np.abs(ref)
    assert (np.abs(out[:M].double().cpu().numpy() - ref) <= tol).all()
    assert torch.equal(out[M:], resid[M:])


@pytest.mark.parametrize("M", [257, 512])
def test_fc1_epilogue_matches_float64(cuda, M):
    """rc_gemm_bf16(epi = 4) against float64 GELU(A W^T + b): half an e4m3 ulp or half a subnormal step,
    max(2^-4 |ref|, 2^(e - 10)), e the block's stored exponent, plus the bf16 GELU test's atol 2e-3,
    rtol 1e-2 (tests/test_gemm_gpu.py).  Stored exponents follow the rule on the dequantised block
    maximum within one (the f32 maximum may sit on either side of a power of two)."""
    import torch

    L = import_pkg("_lib")
    N, K, Mp = 3072, 768, (M + 255) // 256 * 256
    g = torch.Generator(device=cuda).manual_seed(M)
    A = (torch.randn(Mp, K, device=cuda, generator=g) * 0.5).to(torch.bfloat16)
    W = (torch.randn(N, K, device=cuda, generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, device=cuda, generator=g) * 0.1
    out = torch.full((Mp * (N + N // 32),), 0x7B, dtype=torch.uint8, device=cuda)
    L.check(L.load().rc_gemm_bf16(4, 0, A.data_ptr(), W.data_ptr(), bias.data_ptr(), M, N, K, out.data_ptr(), None, 0,
                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    q, s = out[:Mp * N].view(Mp, N), out[Mp * N:].view(Mp, N // 32)
    assert bool((q[M:] == 0x7B).all()) and bool((s[M:] == 0x7B).all())  # rows >= M untouched
    ref = torch.nn.functional.gelu(A[:M].double() @ W.double().T + bias.double()).cpu().numpy()
    got = mx_dequantize(q[:M], s[:M])
    e = s[:M].cpu().numpy().astype(np.float64) - 127.0
    tol = np.maximum(2.0 ** -4 * np.abs(ref), np.repeat(2.0 ** (e - 10), 32, axis=1)) + 2e-3 + 1e-2 * np.abs(ref)
    assert (np.abs(got - ref) <= tol).all()
    assert (np.abs(e - mx_exponent(np.abs(got).reshape(M, N // 32, 32).max(-1))) <= 1).all()


@pytest.fixture(scope="module")
def model_case(cuda):
    """12-layer seeded model, three images (591 token rows: the tiled kernels), the fp32 oracle once."""
    sd = seeded_vit_msn_weights(1907)
    imgs = np.random.default_rng(5).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    m = import_pkg("vit").VitMsnEmbedder(sd, device=0, max_batch=4)
    yield m, imgs, embed_cls(np.stack([preprocess(x) for x in imgs]), sd)
    m.close()


@pytest.mark.parametrize("ln_fold", [True, False])
def test_model_mode(model_case, ln_fold):
    """"mxfp8" stays inside the bf16 tier (1e-2 to the fp32 oracle), differs in bits from "bf16", reads
    back what was set, and leaves a batch of one (skinny kernels) with the "bf16" bits."""
    import torch

    m, imgs, ref = model_case
    x = torch.from_numpy(imgs)
    m.set_ln_fold(ln_fold)
    m.set_mlp_dtype("bf16")
    assert m.mlp_dtype == "bf16"
    base, _ = m.embed(x)
    one, _ = m.embed(x[:1])
    m.set_mlp_dtype("mxfp8")
    assert m.mlp_dtype == "mxfp8"
    got, _ = m.embed(x)
    one_mx, _ = m.embed(x[:1])
    torch.cuda.synchronize()
    m.set_mlp_dtype("bf16")
    assert torch.equal(one_mx, one)
    assert not torch.equal(got, base)
    for i in range(3):
        assert 1.0 - cosine(got[i].cpu().numpy(), ref[i]) <= 1e-2
