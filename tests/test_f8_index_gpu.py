"""GPU tests of the float8 (OCP e4m3fn) index dtype, ``dtype="float8_e4m3fn"`` / ``"f8"``.

Storage rule under test: a stored element is the e4m3fn byte (round to nearest even) of x̂_c · 2⁸,
x̂ the f32 normalised row every dtype forms at upsert; the stored value — what every score,
``stored_rows`` and ``fetch`` use — is decode(byte) · 2⁻⁸; norms stay f32; a row is ld bytes with
ld a multiple of 256.

Data: ``PCG64(1907)``; rows are ``standard_normal((n, dim))`` scaled per row by ``exp(normal(0, 1))``
(the metrics need spread norms; the cosine does not see them), four queries scaled by 0.5, 1, 3, 20.

References and tolerances
  encoding   exact: torch's CPU f32 -> float8_e4m3fn conversion (round to nearest even, OCP) of the
             f32 index's stored rows x 256, and the exported bytes decoded by torch.
  cosine     ``oracle.cosine_topk`` in float64 on ``stored_rows``, the project's cosine tolerance
             1e-5: the device runs the same f32 FMA chain over exactly representable values.
  metrics    float64 on ``stored_rows`` and the exported f32 norms n_r: with qn = ‖q‖ and
             c = (q / qn) · x̂_r, dot = qn·n_r·c and euclidean = qn² − 2·qn·n_r·c + n_r²; the
             cosine tolerance propagated through the rule plus the f32 rounding of its two FMAs:
             dot 2e-5·qn·n_r + 1e-6·|ref|, euclidean 2e-5·qn·n_r + 1e-6·(qn + n_r)².
  paths      bit equality: every search path returns the single-query scan's rows and score bits.
"""
import json
import os

import numpy as np
import pytest

from conftest import import_pkg
from oracle.cosine_topk import cosine_topk, topk_equal_modulo_ties

pytestmark = pytest.mark.gpu

F8 = "float8_e4m3fn"
SHAPES = [(100, 1000), (512, 1000), (768, 3000)]  # ld 256 (padded; 4 queries a pass), 512 (2 a pass), 768 (several scan blocks)
LD = {100: 256, 512: 512, 768: 768}
KS = [10, 100, 200]  # list sizes 128, 256, 512
METRICS = ["dotproduct", "euclidean"]
QSCALE = np.array([0.5, 1.0, 3.0, 20.0])


@pytest.fixture(scope="module")
def idxmod(cuda):
    return import_pkg("index")


_DATA = {}


def data(dim, n):
    """Rows and queries, computed once per shape and left unchanged."""
    if (dim, n) not in _DATA:
        rng = np.random.Generator(np.random.PCG64(1907))
        X = rng.standard_normal((n, dim)) * np.exp(rng.normal(0.0, 1.0, n))[:, None]
        Q = rng.standard_normal((4, dim)) * QSCALE[:, None]
        _DATA[dim, n] = (X.astype(np.float32), Q.astype(np.float32))
    return _DATA[dim, n]


_DEVS = {}


@pytest.fixture(scope="module")
def devs(idxmod, cuda):
    """float8 DeviceIndex per shape with its stored rows, raw bytes and norms: built once."""
    import torch

    def get(dim, n):
        if (dim, n) not in _DEVS:
            X, _ = data(dim, n)
            dev = idxmod.DeviceIndex(dim, dtype=F8, capacity=n, device=cuda)
            dev.upsert_rows(torch.from_numpy(X), torch.arange(n))
            stored = dev.stored_rows(n).cpu().numpy()
            raw, norms = dev.export_rows(0, n)
            torch.cuda.synchronize()
            _DEVS[dim, n] = (dev, stored, raw.cpu(), norms.cpu().numpy())
        return _DEVS[dim, n]

    yield get
    for dev, *_ in _DEVS.values():
        dev.close()
    _DEVS.clear()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


# ------------------------------------------------------------------ 1. encoding
@pytest.mark.parametrize("dim,n", SHAPES)
def test_encoding(idxmod, cuda, devs, dim, n):
    import torch

    dev, stored, raw, norms = devs(dim, n)
    X, _ = data(dim, n)
    assert dev.ld == LD[dim] and dev.ld % 256 == 0
    assert tuple(raw.shape) == (n, dev.ld) and raw.dtype == torch.uint8  # one byte per element
    dec = raw.view(torch.float8_e4m3fn).float() * 2.0 ** -8
    assert torch.equal(dec[:, :dim], torch.from_numpy(stored))  # decoded values: +0 and -0 agree
    assert torch.count_nonzero(dec[:, dim:]) == 0  # pad columns
    f32 = idxmod.DeviceIndex(dim, dtype="float32", capacity=n, device=cuda)
    f32.upsert_rows(torch.from_numpy(X), torch.arange(n))
    xhat = f32.stored_rows(n).cpu()
    _, norms32 = f32.export_rows(0, n)
    torch.cuda.synchronize()
    f32.close()
    want = (xhat * 256.0).to(torch.float8_e4m3fn).float() / 256.0  # OCP e4m3fn, round to nearest even
    assert torch.equal(torch.from_numpy(stored), want)
    assert norms.view(np.uint32).tolist() == norms32.cpu().numpy().view(np.uint32).tolist()
    # the rounding is really 3 mantissa bits: something moved, nothing by more than 2^-4 relative
    # (normal range) or half a subnormal step of 2^-17
    err = (want - xhat).abs()
    assert float(err.max()) > 0 and bool((err <= torch.maximum(xhat.abs() * 2.0 ** -4, torch.tensor(2.0 ** -18))).all())


def test_row_width_is_a_multiple_of_256(idxmod, cuda):
    for dim, ld in ((1, 256), (256, 256), (257, 512), (300, 512), (513, 768), (769, 1024), (1100, 1536), (2048, 2048)):
        dev = idxmod.DeviceIndex(dim, dtype="f8", capacity=1, device=cuda)
        assert dev.ld == ld, dim
        dev.close()


# ------------------------------------------------------------------ 2. oracle parity of the scan
def oracle_check(stored, Q, k, s, r, tol=1e-5):
    ref_r, ref_s = cosine_topk(stored, Q, k, rows_normalized=True)
    kk = min(k, stored.shape[0])
    for q in range(Q.shape[0]):
        assert topk_equal_modulo_ties(r[q, :kk], s[q, :kk], ref_r[q], ref_s[q], tol), q
        qn = Q[q].astype(np.float64) / np.linalg.norm(Q[q].astype(np.float64))
        assert np.allclose(s[q, :kk], stored[r[q, :kk]].astype(np.float64) @ qn, atol=tol, rtol=0)
        assert np.all(np.diff(s[q, :kk]) <= 0), "scores not descending"
        assert np.all(r[q, kk:] == -1) and np.all(np.isneginf(s[q, kk:]))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim,n", SHAPES)
def test_scan_matches_oracle(devs, dim, n, k):
    import torch

    dev, stored, _, _ = devs(dim, n)
    Q = data(dim, n)[1]
    s, r = dev.search(torch.from_numpy(Q), k, n, mode="scan")
    oracle_check(stored, Q, k, s.cpu().numpy(), r.cpu().numpy())


@pytest.mark.parametrize("n", [1, 15, 17, 33, 65])  # around the 16-row wave step and the 64-row block step
def test_more_slots_than_rows(devs, n):
    import torch

    dim, k = 100, 100
    dev, stored, _, _ = devs(dim, 1000)
    Q = data(dim, 1000)[1]
    s, r = dev.search(torch.from_numpy(Q), k, n, mode="scan")  # rows [0, n) only
    oracle_check(stored[:n], Q, k, s.cpu().numpy(), r.cpu().numpy())


# ------------------------------------------------------------------ 3. metrics
def metric_reference(stored, norms, Q):
    q = Q.astype(np.float64)
    qn = np.linalg.norm(q, axis=1)
    c = (q / qn[:, None]) @ stored.astype(np.float64).T
    nr = norms.astype(np.float64)[None, :]
    return {"dotproduct": qn[:, None] * nr * c, "euclidean": -(qn[:, None] ** 2 - 2.0 * qn[:, None] * nr * c + nr ** 2)}, qn


def metric_tolerance(metric, qn, nr, ref):
    if metric == "dotproduct":
        return 2e-5 * qn * nr + 1e-6 * np.abs(ref)
    return 2e-5 * qn * nr + 1e-6 * (qn + nr) ** 2


def top(scores, k):
    rows = np.arange(scores.shape[0])
    return rows[np.lexsort((rows, -scores))[:k]]


_MREF = {}


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim,n", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_metric_scan_matches_reference(devs, metric, dim, n, k):
    import torch

    dev, stored, _, norms = devs(dim, n)
    Q = data(dim, n)[1]
    if (dim, n) not in _MREF:
        _MREF[dim, n] = metric_reference(stored, norms, Q)
    ref, qn = _MREF[dim, n]
    dev.set_metric(metric)
    try:
        s, r = dev.search(torch.from_numpy(Q), k, n, mode="scan")
    finally:
        dev.set_metric("cosine")
    s, r = s.cpu().numpy(), r.cpu().numpy()
    nmax = float(norms.max())
    for q in range(Q.shape[0]):
        want = top(ref[metric][q], k)
        bound = qn[q] * nmax if metric == "dotproduct" else 0.0
        tol_kth = float(metric_tolerance(metric, qn[q], nmax, bound))
        rows = r[q]
        assert np.all(rows >= 0) and len(set(rows.tolist())) == k, (q, rows)
        assert topk_equal_modulo_ties(rows, s[q], want, ref[metric][q][want], tol_kth), (q, rows, want)
        rr = ref[metric][q][rows]
        err = np.abs(s[q].astype(np.float64) - rr)
        tol = metric_tolerance(metric, qn[q], norms[rows].astype(np.float64), rr)
        assert np.all(err <= tol), (q, float((err / tol).max()))
        assert np.all(np.diff(s[q]) <= 0), "scores not descending"


# ------------------------------------------------------------------ 4. one answer on every path
def as_lists(matches):
    return [m["id"] for m in matches], bits([m["score"] for m in matches])


@pytest.mark.parametrize("k", [10, 100])  # both list sizes of the one-launch query and of the multi-query passes
@pytest.mark.parametrize("dim,n", SHAPES)  # 4, 2 and 1 queries per scan pass
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_every_path_gives_the_same_bits(idxmod, cuda, devs, metric, dim, n, k):
    import torch

    X, Q = data(dim, n)
    Q5 = np.concatenate([Q, Q[:1] * np.float32(7.0)])
    ids = [f"v{i}" for i in range(n)]
    dev = devs(dim, n)[0]
    dev.set_metric(metric)
    try:  # the yardstick: one query per call, the single-query scan kernels
        base = [dev.search(torch.from_numpy(Q5[q:q + 1]), k, n, mode="scan") for q in range(5)]
    finally:
        dev.set_metric("cosine")
    want = []
    for s, r in base:
        s = s.cpu().numpy()[0]
        if metric == "euclidean":  # what Index reports
            s = np.maximum(np.float32(0.0), -s)
        want.append(([ids[i] for i in r.cpu().numpy()[0].tolist()], bits(s)))
    mk = lambda name, **kw: idxmod.Index(name, dimension=dim, metric=metric, dtype=F8, capacity=n, device=cuda, **kw)  # noqa: E731
    one, many, remote = mk("one"), mk("many", shards=3), mk("remote", shards=3)
    remote.shard_set.force_remote()
    xt = torch.from_numpy(X).to(cuda)
    try:
        for ix in (one, many, remote):
            ix.upsert_tensor(ids, xt)
            for q in range(5):  # Index.query: the one-launch path on `one`, per shard on the others
                assert as_lists(ix.query(vector=Q5[q].tolist(), top_k=k)["matches"]) == want[q], (ix.name, q)
            for nq in (1, 4, 5):  # single-query kernel; a full multi-query pass; a pass and a ragged tail
                got = ix.query_batch(torch.from_numpy(Q5[:nq]), top_k=k, mode="scan")
                for q in range(nq):
                    assert as_lists(got[q]["matches"]) == want[q], (ix.name, nq, q)
    finally:
        for ix in (one, many, remote):
            ix.close()


@pytest.mark.parametrize("dim,n", SHAPES)
def test_masked_scan(idxmod, cuda, dim, n):
    import torch

    X, Q = data(dim, n)
    k = 10
    ids = [f"v{i}" for i in range(n)]
    # "third": every third row; "run": alternate runs of 24 rows (whole 16-row wave steps stay
    # clear and are skipped); "few": 7 rows, fewer than k, on both sides of a 32-row boundary
    few = {29, 30, 31, 32, 33, 500, n - 1}
    md = [{"third": i % 3, "run": (i // 24) % 2, "few": int(i in few)} for i in range(n)]
    idx = idxmod.Index("m", dimension=dim, dtype="f8", capacity=n, device=cuda)
    idx.upsert_tensor(ids, torch.from_numpy(X).to(cuda), md)
    try:
        full = [{m["id"]: m["score"] for m in idx.query(vector=Q[q].tolist(), top_k=256)["matches"]} for q in range(4)]
        for flt, eligible in (({"third": 0}, [i % 3 == 0 for i in range(n)]), ({"run": 1}, [(i // 24) % 2 == 1 for i in range(n)])):
            batch = idx.query_batch(torch.from_numpy(Q), top_k=k, mode="scan", filter=flt)  # masked multi-query passes
            for q in range(4):
                m = idx.query(vector=Q[q].tolist(), top_k=k, filter=flt)["matches"]
                # the k best eligible rows of the unmasked order (its top-256 holds more than k
                # of them: a third, or half, of 256), each with the unmasked search's score bits
                best = [vid for vid in full[q] if eligible[int(vid[1:])]][:k]
                assert len(best) == k and [x["id"] for x in m] == best, (flt, q)
                assert bits([x["score"] for x in m]) == bits([full[q][vid] for vid in best]), (flt, q)
                assert as_lists(batch[q]["matches"]) == as_lists(m), (flt, q)
        # fewer eligible rows than k: only those; a row's score does not depend on where it is
        # stored, so an index of those 7 rows alone gives the unmasked bits
        rows = sorted(few)
        small = idxmod.DeviceIndex(dim, dtype="f8", capacity=len(rows), device=cuda)
        small.upsert_rows(torch.from_numpy(X[rows]), torch.arange(len(rows)))
        s7, r7 = small.search(torch.from_numpy(Q), len(rows), len(rows), mode="scan")
        small.close()
        for q in range(4):
            m = idx.query(vector=Q[q].tolist(), top_k=k, filter={"few": 1})["matches"]
            assert [int(x["id"][1:]) for x in m] == [rows[j] for j in r7[q].tolist()], q
            assert bits([x["score"] for x in m]) == bits(s7[q].cpu().numpy()), q
    finally:
        idx.close()


# ------------------------------------------------------------------ 5. row life cycle
def test_fetch_delete_save_load(idxmod, cuda, tmp_path):
    import torch

    dim, n = 100, 1000
    X, Q = data(dim, n)
    ids = [f"v{i}" for i in range(n)]
    idx = idxmod.Index("life", dimension=dim, dtype=F8, capacity=256, device=cuda, shards=2)  # grows twice
    idx.upsert_tensor(ids, torch.from_numpy(X).to(cuda), [{"i": i} for i in range(n)])
    try:
        sset = idx.shard_set
        assert sset.ld == 256
        # fetch = stored value x norm (f32 product), through fetch and through include_values
        stored = sset.fetch_rows(list(range(n)), stored=True).numpy()
        raw, norms = sset.export_rows(n)
        assert raw.shape == (n, 256) and raw.dtype == np.uint8
        got = idx.fetch(ids[:40])["vectors"]
        for i in range(40):
            assert bits(got[ids[i]]["values"]) == bits(stored[i] * norms[i]), i
        m = idx.query(vector=Q[1].tolist(), top_k=5, include_values=True)["matches"]
        for x in m:
            i = int(x["id"][1:])
            assert bits(x["values"]) == bits(stored[i] * norms[i])
        # delete on both sides of a 32-row boundary: every survivor keeps its bytes and its norm
        gone = ["v30", "v31", "v32", "v33", "v500"]
        idx.delete(ids=gone)
        assert len(idx) == n - 5
        raw2, norms2 = sset.export_rows(n - 5)
        for vid, row in idx._rows.items():
            old = int(vid[1:])
            assert vid not in gone and raw2[row].tobytes() == raw[old].tobytes() and norms2[row] == norms[old], vid
        # save / load: the manifest carries the dtype; the same answers, in another shard count too
        idx.save(str(tmp_path))
        man = json.load(open(os.path.join(str(tmp_path), "manifest.json")))
        assert man["dtype"] == F8 and man["ld"] == 256
        assert np.load(os.path.join(str(tmp_path), "rows.npy")).shape == (n - 5, 256)
        for shards in (2, 3):
            back = idxmod.Index.load(str(tmp_path), device=cuda, shards=shards)
            assert back.dtype == F8
            for q in range(4):
                assert back.query(vector=Q[q].tolist(), top_k=20, include_metadata=True) == \
                    idx.query(vector=Q[q].tolist(), top_k=20, include_metadata=True), (shards, q)
            back.close()
    finally:
        idx.close()


def test_one_process_per_gpu_index(cuda, devs):
    import torch

    dim, n, k = 512, 1000, 10
    X, Q = data(dim, n)
    dev = devs(dim, n)[0]
    sh = import_pkg("sharded").ShardedIndex(dim, dtype="f8", capacity_per_rank=n, device=cuda)
    sh.upsert_rows(torch.from_numpy(X), torch.arange(n))
    s, r = sh.search(torch.from_numpy(Q), k, mode="scan")
    s0, r0 = dev.search(torch.from_numpy(Q), k, n, mode="scan")
    assert torch.equal(r.cpu(), r0.cpu()) and torch.equal(s.cpu().view(torch.int32), s0.cpu().view(torch.int32))
    sh.close()


# ------------------------------------------------------------------ 6. limits
def test_refusals(idxmod, cuda, devs):
    import torch

    dim, n = 512, 1000
    dev = devs(dim, n)[0]
    Q = torch.from_numpy(data(dim, n)[1])
    with pytest.raises(ValueError):
        dev.search(Q, 5, n, mode="mfma")
    with pytest.raises(ValueError):
        dev.set_filter("i8")
    assert dev.filter == "native"
    sset = idxmod.ShardSet(dim, dtype=F8, capacity_per_shard=64, devices=[cuda, cuda])
    with pytest.raises(ValueError):
        sset.set_filter("i8")
    assert sset.filter == "native"
    sset.close()
    with pytest.raises(ValueError):
        idxmod.Index("x", dimension=dim, dtype="f8", filter="i8", device=cuda)
    with pytest.raises(ValueError):
        idxmod.DeviceIndex(dim, dtype="float8_e5m2", capacity=64, device=cuda)
    idx = idxmod.Index("x", dimension=dim, dtype="f8", capacity=64, device=cuda)
    assert idx._masked_mode("auto", 64, 1 << 20, 1 << 20) == "scan"  # where an f16 index would pick MFMA
    idx.close()


def test_auto_scans_above_the_mfma_thresholds(idxmod, cuda):
    import torch

    dim, n, nq, k = 256, 70_000, 16, 10  # >= 8 queries and >= 65536 rows: an f16 index takes the MFMA path here
    dev = idxmod.DeviceIndex(dim, dtype=F8, capacity=n, device=cuda)
    dev.fill_random(11, 0, n)
    Q = torch.from_numpy(np.random.Generator(np.random.PCG64(1907)).standard_normal((nq, dim)).astype(np.float32))
    dev.timing(True)
    dev.gemm_timing_read()
    sa, ra = dev.search(Q, k, n, mode="auto")
    torch.cuda.synchronize()
    _, launches, _, fallbacks = dev.gemm_timing_read()
    assert launches == 0 and fallbacks == 0  # no filter launch
    ss, rs = dev.search(Q, k, n, mode="scan")
    assert torch.equal(ra, rs) and torch.equal(sa.view(torch.int32), ss.view(torch.int32))
    assert bool((ra >= 0).all())
    dev.timing(False)
    dev.close()
