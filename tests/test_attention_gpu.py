"""The attention kernels (rc_attention_bf16) against a float64 reference of the same operation.

rc_attention_bf16 launches attention_v2_kernel<197> / <0> and attention_cls_kernel through the
launcher the model uses, on caller buffers.  The reference takes the same bf16 inputs widened to
float64: P = softmax(Q·Kᵀ / 8) per (image, head), ref = P·V.

Per-element bound (derived, not measured):

    |out − ref| <= 1.25 · 2⁻⁸ · (|ref| + Σ_j P_ij·|V_jd|) + 2⁻²⁴

The kernels round P to bf16 (unit roundoff 2⁻⁸) for P·V, sum the unrounded p in f32 and round
the output to bf16 once (another 2⁻⁸); the factor 1.25 covers the second-order terms and the f32
and exp2 error (about 1e-6 relative), 2⁻²⁴ the outputs near zero.

Every case has 3 images and 12 heads with different data in each; `out` starts as NaN-pattern
sentinels between sentinel guard rows, so an element the kernel does not write misses the bound
and a write outside the output rows changes a guard.
"""
import functools

import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

IMAGES, HEADS, HD = 3, 12, 64
H = HEADS * HD
GUARD = 4  # sentinel rows before and after the output rows
SENTINEL = 0x7FC1  # a bf16 NaN: never a result of finite inputs

FULL_TOKENS = [1, 2, 5, 15, 16, 17, 50, 64, 65, 145, 170, 192, 193, 196, 197, 208]
CLS_TOKENS = sorted(FULL_TOKENS + [63, 256])
FULL, FORCE_RT, CLS = 0, 1, 2  # rc_attention_bf16 kinds

# (kind, tokens), the kinds of one token count side by side (they share inputs and reference)
CASES = [(k, t) for t in CLS_TOKENS for k in (FULL, FORCE_RT, CLS) if k == CLS or t in FULL_TOKENS]
# family 4 needs pad keys in the last 16-key tile of the full kernels: token counts that are a
# multiple of 16 have none and are left out there (the CLS kernel has no key tiles: every count)
PAD_CASES = [(k, t) for k, t in CASES if k == CLS or t % 16 != 0]
CASE_IDS = [f"kind{k}-t{t}" for k, t in CASES]
PAD_CASE_IDS = [f"kind{k}-t{t}" for k, t in PAD_CASES]
FAMILIES = ("random", "random_s3", "random_x3", "one_hot", "last_key", "uniform_heavy_last")
# one-hot families: Q_i = 3·K_j puts 3·|K_j|²/8 = 3·64·σ²/8 on the target's logit, against 3·σ²·N(0, 1)
# on the others; σ = 2 leaves the target a weight >= 0.999 in every row (asserted on the reference)
ONE_HOT_K_STD = 2.0
RANDOM_QK_STD = {"random": 1.3, "random_s3": 3.0, "random_x3": 3.9}  # logit standard deviation 1.7, 9, 15


def _bf16_round(x):
    import torch

    return x.to(torch.bfloat16).to(torch.float64)


@functools.lru_cache(maxsize=3)
def case(family, tokens):
    """Inputs (CPU) and float64 reference of one (family, tokens), shared by the three kinds:
    qkv [images·tokens][3·H] bf16, ref and absref = Σ_j P_ij·|V_jd| as [images][tokens][H] f64,
    V as [images][heads][tokens][64] f64, P's largest weight per row, and the family's target key
    per query (or None)."""
    import torch

    T = tokens
    g = torch.Generator().manual_seed(1000 * T + FAMILIES.index(family))
    rnd = lambda: torch.randn(IMAGES, HEADS, T, HD, generator=g, dtype=torch.float64)
    target = None
    if family in RANDOM_QK_STD:
        s = RANDOM_QK_STD[family]
        q, k, v = rnd() * s, rnd() * s, rnd()
    elif family == "one_hot":
        k, v = rnd() * ONE_HOT_K_STD, rnd()
        target = torch.stack([torch.stack([torch.randperm(T, generator=g) for _ in range(HEADS)]) for _ in range(IMAGES)])
        q = 3.0 * torch.gather(_bf16_round(k), 2, target[..., None].expand(-1, -1, -1, HD))
    elif family == "last_key":
        k, v = rnd() * ONE_HOT_K_STD, rnd()
        target = torch.full((IMAGES, HEADS, T), T - 1, dtype=torch.int64)
        q = 3.0 * _bf16_round(k)[:, :, T - 1:T].expand(-1, -1, T, -1)
    elif family == "uniform_heavy_last":
        q, k, v = torch.zeros(IMAGES, HEADS, T, HD, dtype=torch.float64), rnd() * 1.3, rnd()
        v[:, :, T - 1] = 32.0
    else:
        raise ValueError(family)
    q, k, v = _bf16_round(q), _bf16_round(k), _bf16_round(v)
    p = torch.softmax(q @ k.transpose(2, 3) / 8.0, dim=-1)
    rows = lambda x: x.permute(0, 2, 1, 3).reshape(IMAGES, T, H)  # [img][head][t][d] -> [img][t][head·64 + d]
    qkv = torch.cat([rows(q), rows(k), rows(v)], dim=2).reshape(IMAGES * T, 3 * H).to(torch.bfloat16)
    return {"qkv": qkv, "ref": rows(p @ v), "absref": rows(p @ v.abs()), "v": v, "pmax": p.max(dim=-1).values,
            "target": target}


def attention(cuda, kind, qkv, tokens, qsplit=0, q_cls=None):
    """Run rc_attention_bf16 and return the output rows ([images·tokens][H], or [images][H] for the
    CLS kind) as bf16 on the device; the guard rows around them must come back untouched."""
    import torch

    L = import_pkg("_lib")
    lib = L.load()
    rows = IMAGES if kind == CLS else IMAGES * tokens
    buf = torch.full((rows + 2 * GUARD, H), SENTINEL, dtype=torch.int16, device=cuda)
    out = buf[GUARD:GUARD + rows]
    L.check(lib.rc_attention_bf16(kind, qkv.data_ptr(), None if q_cls is None else q_cls.data_ptr(), out.data_ptr(),
                                  IMAGES, tokens, HEADS, qsplit, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + rows:] == SENTINEL).all()), "guard rows written"
    return out.view(torch.bfloat16)


def check_bound(name, kind, tokens, got, c):
    """got within the derived bound of the reference; prints the largest error / bound."""
    import torch

    ref, absref = c["ref"], c["absref"]
    if kind == CLS:
        ref, absref = ref[:, 0], absref[:, 0]
    got = got.cpu().to(torch.float64).reshape(ref.shape)
    bound = 1.25 * 2.0 ** -8 * (ref.abs() + absref) + 2.0 ** -24
    err = (got - ref).abs()
    ok = err <= bound  # False for NaN: an element left as the sentinel
    ratio = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
    print(f"ATTN_RATIO {name} kind={kind} tokens={tokens} max_err_over_bound={ratio:.4f}")
    assert bool(ok.all()), f"{int((~ok).sum())} elements outside the bound, largest error / bound = {ratio:.3f}"
    return got


def check_rows_select_target(kind, tokens, got, c):
    """argmin_j ‖out_i − V_j‖ == target(i), for every query row (row 0 for the CLS kind)."""
    import torch

    o = got.reshape(IMAGES, -1, HEADS, HD).permute(0, 2, 1, 3)  # [img][head][q][d]
    nearest = torch.cdist(o, c["v"]).argmin(dim=-1)
    want = c["target"][:, :, :o.shape[2]]
    assert torch.equal(nearest, want), f"{int((nearest != want).sum())} query rows returned another key's V row"


@pytest.mark.parametrize("scale", list(RANDOM_QK_STD))
@pytest.mark.parametrize("kind,tokens", CASES, ids=CASE_IDS)
def test_random_matches_float64(cuda, kind, tokens, scale):
    """Q, K ~ N(0, σ²) with σ = 1.3 (logit standard deviation about 1.7), σ = 3 (about 9) and
    σ = 3.9 (the first ×3: about 15, near-peaked rows); V ~ N(0, 1).

    Largest error / bound measured on the MI355X over the token counts, full kinds (0 and 1, the
    same bits) / CLS kind: σ = 1.3: 0.650 / 0.541; σ = 3: 0.714 / 0.635; σ = 3.9: 0.708 / 0.584."""
    c = case(scale, tokens)
    check_bound(scale, kind, tokens, attention(cuda, kind, c["qkv"].to(cuda), tokens), c)


@pytest.mark.parametrize("kind,tokens", CASES, ids=CASE_IDS)
def test_one_hot_permutation_returns_the_permuted_v_rows(cuda, kind, tokens):
    """Q_i = 3·K_π(i) for a random permutation π per (image, head): the reference's top weight is at
    least 0.999, so out_i is V_π(i) to one bf16 rounding; a wrong key row, swizzle chunk, transposed
    V read, head or image offset returns another row outright.

    Largest error / bound measured on the MI355X: 0.105 (full kinds), 0.000 (CLS kind)."""
    c = case("one_hot", tokens)
    assert float(c["pmax"].min()) >= 0.999
    got = check_bound("one_hot", kind, tokens, attention(cuda, kind, c["qkv"].to(cuda), tokens), c)
    check_rows_select_target(kind, tokens, got, c)


@pytest.mark.parametrize("kind,tokens", CASES, ids=CASE_IDS)
def test_last_key_dominant(cuda, kind, tokens):
    """Every query points at key tokens − 1 (Q_i = 3·K_last): a mask that drops the last valid key
    returns a different row.

    Largest error / bound measured on the MI355X: 0.000 on every kind (the target's weight rounds
    to 1 and V is bf16 already, so the outputs are V_last exactly)."""
    c = case("last_key", tokens)
    assert float(c["pmax"].min()) >= 0.999
    got = check_bound("last_key", kind, tokens, attention(cuda, kind, c["qkv"].to(cuda), tokens), c)
    check_rows_select_target(kind, tokens, got, c)


@pytest.mark.parametrize("kind,tokens", PAD_CASES, ids=PAD_CASE_IDS)
def test_uniform_attention_with_a_heavy_last_row(cuda, kind, tokens):
    """Q = 0, so p = 1 / tokens exactly; V ~ N(0, 1) except V[tokens − 1] = 32 in every dimension.
    The full kernels re-read the last token for the pad keys of the last 16-key tile: one pad key
    let through the mask moves every output by about 32 / (tokens + 1) (0.15 at 197 tokens, against
    a bound of about 5e-3).  Token counts that are a multiple of 16 have no pad keys there and are
    not in the full kernels' cases.

    Largest error / bound measured on the MI355X: 0.398 on every kind (at 2 tokens; 0.167 at 197)."""
    c = case("uniform_heavy_last", tokens)
    check_bound("uniform_heavy_last", kind, tokens, attention(cuda, kind, c["qkv"].to(cuda), tokens), c)


def test_compile_time_and_runtime_token_count_same_bits(cuda):
    """attention_v2_kernel<197> (kind 0 at 197 tokens) and attention_v2_kernel<0> (kind 1)."""
    import torch

    for family in ("random", "random_x3", "one_hot", "uniform_heavy_last"):
        qkv = case(family, 197)["qkv"].to(cuda)
        for qsplit in (1, 4):
            a = attention(cuda, FULL, qkv, 197, qsplit)
            b = attention(cuda, FORCE_RT, qkv, 197, qsplit)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (family, qsplit)


@pytest.mark.parametrize("kind,tokens", [(FORCE_RT, t) for t in FULL_TOKENS] + [(FULL, 197)])
def test_qsplit_1_and_4_same_bits(cuda, kind, tokens):
    """One block per (image, head) against four (query tiles qs·4 + wave, stepping 16): below 16
    query tiles (every count here) some waves of the split form have no tile.  Kind 0 differs from
    kind 1 at 197 tokens only (the compile-time instantiation)."""
    import torch

    for family in ("random_x3", "one_hot"):
        qkv = case(family, tokens)["qkv"].to(cuda)
        a = attention(cuda, kind, qkv, tokens, 1)
        b = attention(cuda, kind, qkv, tokens, 4)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), family


@pytest.mark.parametrize("tokens", CLS_TOKENS)
def test_cls_compact_queries_same_bits(cuda, tokens):
    """attention_cls_kernel with the queries compact in q_cls (the last layer's CLS-only Q) against
    the same queries read from row 0 of each image in qkv.  The q_cls run gets a qkv whose row-0
    queries are overwritten, so a kernel that ignored q_cls would differ."""
    import torch

    for family in ("random_x3", "one_hot"):
        qkv = case(family, tokens)["qkv"].to(cuda)
        from_qkv = attention(cuda, CLS, qkv, tokens)
        q_cls = qkv.reshape(IMAGES, tokens, 3 * H)[:, 0, :H].contiguous()
        other = qkv.clone()
        other.reshape(IMAGES, tokens, 3 * H)[:, 0, :H] = 7.0
        compact = attention(cuda, CLS, other, tokens, q_cls=q_cls)
        assert torch.equal(from_qkv.view(torch.int16), compact.view(torch.int16)), family


def test_refusals_on_the_device(cuda):
    """The limits the kernels' comments state, refused with a GPU present too."""
    import torch

    L = import_pkg("_lib")
    lib = L.load()
    x = torch.zeros(8, 3 * H, dtype=torch.bfloat16, device=cuda)
    s = torch.cuda.current_stream().cuda_stream
    for kind, tokens, qsplit in [(FULL, 209, 0), (FORCE_RT, 209, 0), (CLS, 257, 0), (FULL, 0, 0), (FULL, 2, 3), (3, 2, 0)]:
        assert lib.rc_attention_bf16(kind, x.data_ptr(), None, x.data_ptr(), 1, tokens, HEADS, qsplit, s) == L.RC_ERR_INVALID
