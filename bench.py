"""Benchmark of the MI355X retrieval core (driver contract: one JSON line on rank 0).

Headline (``value``): BASELINE.json config 2 — batch-256 224x224 synthetic u8
images through the full embedding path (preprocess → ViT-MSN-base 12 layers →
CLS + L2) per GPU, images/s summed over ranks (data parallel, no collectives,
weak scaling).  ``roofline`` prices the dominant kernel (the fc1 GEMM) from HIP
events recorded around its launches inside the timed steps.

Secondary (``search``): config 4's single-query variant, weak-scaled — each
rank holds ``--rows-per-gpu`` x 512 fp16 rows (125M/GPU → 1B at 8 GPUs), a
query is broadcast, every rank runs the HIP scan + top-k over its shard, the
per-rank top-k lists are all-gathered over RCCL and merged on the device.  Also
config 3 (1M x 512 f32, top-10, one GPU).  Its roofline is HBM: bytes = rows x
512 x dtype bytes per query pass.

``cpu_baseline`` (rank 0, N=1 only): the reference's own arithmetic library —
a torch-CPU fp32 forward of the same seeded ViT-MSN (torch.nn.functional
linear / layer_norm / erf-GELU / SDPA, as transformers' ViTMSNModel runs it) —
and numpy cosine top-k, timed on bounded samples on this host's cores.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run does only what the headline needs: set up, warm up, time ``--steps``
embed steps, print the line (``value``, ``ms_per_step`` and the configuration).
``--full`` adds everything else described above — the per-GEMM roofline and the
vendor yardstick, config 5 ingest, the JPEG lines, batch-1 latency, the search
configs and the CPU baselines — each still governed by its own switch
(``--no-cpu``, ``--no-search``, ``--no-latency``, ``--ingest-images 0``,
``--jpeg-images 0``).  ``--dump-outputs DIR`` writes what the last timed step
returned (``raw`` and ``nrm``, the two [batch, 768] float32 arrays ``embed``
hands its caller) as ``DIR/raw.npy`` and ``DIR/nrm.npy`` (rank r > 0:
``raw.rank<r>.npy``); the inputs are seeded, so two builds run with the same
arguments can be compared output for output.

``--gpus N`` without a torch.distributed launcher re-launches this script under
``python -m torch.distributed.run --nproc-per-node N`` (one process per GPU)
before anything touches the GPU; ``--dry-run`` checks that rank plumbing on CPU
(gloo, no GPU) and prints the world size it saw.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PKG = "end-to-end-image-retrieval-service-with-k8s-jenkins_amd"
METRIC = "top-k queries/s over 1B×512 index + embed images/s; % HBM/MFMA roofline"
PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBPS = 8000.0      # MI355X HBM3E spec
PEAK_I8_TOPS = 5000.0       # MI355X dense int8 MFMA: 2x bf16 (16x16x64 in the cycles of bf16 16x16x32)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def load_profile_traffic(kernel_key: str):
    """HBM traffic per launch from the committed PMC summary (profiles/pmc_*.json), if present."""
    path = os.path.join(REPO, "profiles", "pmc_latest.json")
    try:
        with open(path) as f:
            d = json.load(f)
        return d.get(kernel_key, {}).get("hbm_bytes_per_launch")
    except Exception:
        return None


def cpu_model_name() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def torch_vit_forward(sd):
    """u8 [B,224,224,3] → raw CLS [B,768]: ViTImageProcessor rescale/normalize + ViTMSNModel fp32
    forward restated with torch.nn.functional (modeling_vit_msn.py:57-66 patch conv, :143-154 CLS +
    pos, :254-283 pre-LN layers with SDPA scale 1/8 and exact-erf GELU, :381 final LN)."""
    import torch
    import torch.nn.functional as F

    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)

    def encoder(e):  # patch-conv output [B,768,14,14] -> raw CLS
        e = e.flatten(2).transpose(1, 2)
        B = e.shape[0]
        h = torch.cat([sd["embeddings.cls_token"].expand(B, -1, -1), e], 1) + sd["embeddings.position_embeddings"]
        for i in range(12):
            p = f"encoder.layer.{i}."
            y = F.layer_norm(h, (768,), sd[p + "layernorm_before.weight"], sd[p + "layernorm_before.bias"], 1e-6)
            qkv = [F.linear(y, sd[p + f"attention.attention.{n}.weight"], sd[p + f"attention.attention.{n}.bias"])
                   .view(B, -1, 12, 64).transpose(1, 2) for n in ("query", "key", "value")]
            a = F.scaled_dot_product_attention(*qkv, scale=0.125).transpose(1, 2).reshape(B, -1, 768)
            h = h + F.linear(a, sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"])
            y = F.layer_norm(h, (768,), sd[p + "layernorm_after.weight"], sd[p + "layernorm_after.bias"], 1e-6)
            y = F.gelu(F.linear(y, sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"]))
            h = h + F.linear(y, sd[p + "output.dense.weight"], sd[p + "output.dense.bias"])
        return F.layer_norm(h, (768,), sd["layernorm.weight"], sd["layernorm.bias"], 1e-6)[:, 0]

    def forward(u8):  # u8 [B,224,224,3]
        x = u8.permute(0, 3, 1, 2).to(torch.float64) * (1 / 255.0)
        x = ((x.to(torch.float32) - mean) / std).contiguous()
        return encoder(F.conv2d(x, sd["embeddings.patch_embeddings.projection.weight"],
                                sd["embeddings.patch_embeddings.projection.bias"], stride=16))

    forward.encoder = encoder
    return forward


def _cgroup_cpu_quota():
    """CPUs the job's cgroup may use (cgroup v2 cpu.max / v1 cfs quota), or None if unlimited."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else max(1, int(int(q) / int(p)))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else max(1, q // p)
    except (OSError, ValueError):
        return None


def host_cores() -> dict:
    """The cores this job may use: the smallest of its CPU affinity, its cgroup CPU quota and
    OMP_NUM_THREADS (the GPU box sets 16 per GPU; affinity and os.cpu_count() show the whole
    machine there).  The CPU baselines run torch's intra-op pool at exactly that count."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = _cgroup_cpu_quota()
    omp = int(os.environ["OMP_NUM_THREADS"]) if os.environ.get("OMP_NUM_THREADS", "").isdigit() else None
    use = min(x for x in (aff, quota, omp) if x)
    return {"use": use, "affinity": aff, "cgroup_quota": quota, "omp_num_threads": omp, "os_cpu_count": os.cpu_count()}


def _torch_threads():
    import torch

    torch.set_num_threads(host_cores()["use"])
    return torch.get_num_threads()


def cpu_embed_baseline(budget_s: float = 15.0, batch: int = 16):
    """The reference's CPU path for config 2: ViTImageProcessor's rescale/normalize (224x224
    input: the resize is an identity) and ViTMSNModel's fp32 forward, restated with the same
    torch.nn.functional ops transformers calls (modeling_vit_msn.py: conv patch embed, pre-LN
    layers, SDPA attention with scale 1/8, exact-erf GELU, final LN), seeded weights, on every
    core this process may use (torch threads set to the affinity count), bounded by time."""
    import torch

    from oracle.weights import seeded_vit_msn_weights

    threads = _torch_threads()
    sd = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in seeded_vit_msn_weights(0).items()}
    forward = torch_vit_forward(sd)

    g = torch.Generator().manual_seed(3)
    imgs = torch.randint(0, 256, (batch, 224, 224, 3), dtype=torch.uint8, generator=g)
    with torch.inference_mode():
        forward(imgs[:2])  # warm
        done, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget_s or done == 0:
            forward(imgs)
            done += batch
    el = time.perf_counter() - t0
    return {"value": done / el, "unit": "images/s", "cores": threads, "kind": "reference-lib",
            "cpu": cpu_model_name(), "host_cores": host_cores(),
            "cores_note": "torch intra-op threads = min(CPU affinity, cgroup CPU quota, OMP_NUM_THREADS): the cores "
                          "this job may use on the box (16 per GPU there), not the machine's total",
            "sample": f"{done} synthetic 224x224 images (batches of {batch}) through rescale/normalize + a torch fp32 "
                      f"ViT-MSN-base forward (torch.nn.functional, the library the reference's transformers path "
                      f"runs on), {el:.1f}s"}


def synthetic_jpegs(n: int, seed: int, size=224) -> list[bytes]:
    """Baseline 4:2:0 q90 JPEGs of smooth random content plus noise (PIL encoder); size = side
    or (width, height)."""
    from PIL import Image

    w, h = (size, size) if isinstance(size, int) else size
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        arr = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR)).astype(np.int16)
        arr = np.clip(arr + rng.integers(-12, 13, arr.shape), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(arr).save(b, format="JPEG", quality=90, subsampling=2)
        out.append(b.getvalue())
    return out


def cpu_jpeg_baseline(datas: list[bytes], budget_s: float = 4.0):
    """The reference decode (embedding/main.py:97: PIL open + convert RGB), one host thread."""
    from PIL import Image

    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < budget_s or done == 0:
        Image.open(io.BytesIO(datas[done % len(datas)])).convert("RGB").load()
        done += 1
    el = time.perf_counter() - t0
    return {"value": done / el, "unit": "images/s", "cores": 1, "kind": "reference",
            "sample": f"{done} decodes of the same 224x224 JPEGs with Pillow (the reference's own decode), {el:.1f}s"}


def cpu_ingest_baseline(total_images: int, budget_s: float = 15.0, index_rows: int = 10_000):
    """Config 5's CPU baseline: the reference's per-image ingest path (ingesting/main.py:101-168 —
    one upload at a time: PIL decode, the embedding pod's ViTImageProcessor + fp32 ViTMSNModel at
    batch 1 (embedding/main.py:97-114), then index.upsert of one vector) on the host cores, with a
    numpy array standing in for Pinecone's upsert (L2-normalised row written at its slot; GCS upload
    and HTTP hops omitted, which only flatters the CPU).  Timed on a bounded sample of synthetic
    224x224 JPEGs and extrapolated linearly to `total_images`."""
    import torch
    from PIL import Image

    from oracle.preprocess import preprocess
    from oracle.weights import seeded_vit_msn_weights

    threads = _torch_threads()
    sd = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in seeded_vit_msn_weights(0).items()}
    fwd = torch_vit_forward_pixels(sd)
    datas = synthetic_jpegs(16, seed=55)
    X = np.zeros((index_rows, 768), np.float32)

    def one(i):
        im = np.asarray(Image.open(io.BytesIO(datas[i % len(datas)])).convert("RGB"))
        with torch.inference_mode():
            v = fwd(torch.from_numpy(preprocess(im)[None]))[0].numpy()
        X[i % index_rows] = v / max(float(np.linalg.norm(v)), 1e-12)

    one(0)  # warm
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < budget_s or done == 0:
        one(done)
        done += 1
    el = time.perf_counter() - t0
    rate = done / el
    return {"value": rate, "unit": "images/s", "cores": threads, "kind": "reference-lib", "cpu": cpu_model_name(),
            "extrapolated_hours": total_images / rate / 3600.0, "extrapolated_images": total_images,
            "sample": f"{done} synthetic 224x224 q90 JPEGs one at a time: PIL decode + ViTImageProcessor arithmetic "
                      f"(numpy restatement, bit-exact) + torch fp32 ViT-MSN-base forward at batch 1 + upsert of the "
                      f"L2-normalised vector into a numpy index, {el:.1f}s; extrapolated linearly to "
                      f"{total_images:,} images (BASELINE config 5)"}


def cpu_search_baseline(n_rows=1_000_000, dim=512, budget_s=6.0):
    from threadpoolctl import threadpool_info

    from oracle.cosine_topk import cosine_topk_f32

    rng = np.random.default_rng(2)
    X = rng.standard_normal((n_rows, dim), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    q = rng.standard_normal(dim).astype(np.float32)
    cosine_topk_f32(X, q, 10)
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < budget_s or done == 0:
        cosine_topk_f32(X, q, 10)
        done += 1
    el = time.perf_counter() - t0
    threads = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
    return {"value": done / el, "unit": "queries/s", "cores": threads, "kind": "port",
            "sample": f"{done} single queries, exact top-10 over {n_rows}x{dim} f32 (numpy X@q + argpartition), {el:.1f}s"}


def cpu_batch_search_baseline(n_rows=1_000_000, dim=512, nq=256, k=100, index_rows=1_000_000_000, budget_s=8.0):
    """numpy fp32 batched exact top-k (X @ Q^T, argpartition per query) on a row sample, extrapolated to the index size."""
    from threadpoolctl import threadpool_info

    rng = np.random.default_rng(2)
    X = rng.standard_normal((n_rows, dim), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)

    def once():
        S = Q @ X.T
        part = np.argpartition(-S, k - 1, axis=1)[:, :k]
        sc = np.take_along_axis(S, part, axis=1)
        order = np.lexsort((part, -sc), axis=1)
        return np.take_along_axis(part, order, axis=1)

    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < budget_s or done == 0:
        once()
        done += 1
    el = (time.perf_counter() - t0) / done
    threads = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
    scale = index_rows / n_rows
    return {"value": nq / (el * scale), "unit": "queries/s", "cores": threads, "kind": "port",
            "sample": f"{done} x ({nq} queries x {n_rows}x{dim} f32 rows, top-{k}: numpy X@Q^T + argpartition) "
                      f"= {el:.2f}s each, extrapolated linearly to {index_rows:,} rows"}


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q / 100.0 * (len(xs) - 1))))]


def _lat(fn, reps: int, warm: int = 3):
    """fn() timed reps times after warm calls (host wall clock, each call synchronous): p50/p99 ms."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"p50_ms": _pct(ts, 50), "p99_ms": _pct(ts, 99), "mean_ms": sum(ts) / len(ts), "reps": reps}


def planted_index_rows(n=10_000, dim=768, seed=0, query=None, planted=5):
    """Config 1's synthetic index: n x dim N(0,1) rows (seed 0) with `planted` near-duplicates of
    the query (query + small noise) at known rows, so the exact top-5 is known."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    rows = []
    if query is not None:
        q = np.asarray(query, np.float32)
        rows = list(range(17, 17 + 97 * planted, 97))
        for j, r in enumerate(rows):
            X[r] = q + (0.02 * (j + 1)) * np.linalg.norm(q) / np.sqrt(dim) * rng.standard_normal(dim).astype(np.float32)
    return X, rows


def latency_lines(pkg: str, reps: int = 40, cpu: bool = True):
    """Batch-1 request latency, the reference's own request shape: /embed of the reference's
    test image (embedding/main.py:88-124), search top-5 over config 1's 10k x 768 index
    (retriever/main.py:127-130 times exactly this call) and /search_image end to end through
    the FastAPI app (TestClient, in process).  CPU reference beside each: PIL decode +
    ViTImageProcessor arithmetic + a torch fp32 forward at batch 1, numpy exact top-5."""
    import importlib

    import torch

    emb = importlib.import_module(f"{pkg}.embedding.main")
    ing = importlib.import_module(f"{pkg}.ingesting.utils")
    ret = importlib.import_module(f"{pkg}.retriever.utils")
    retmain = importlib.import_module(f"{pkg}.retriever.main")
    img_path = os.path.join(REPO, "tests", "golden", "test_image.jpeg")  # the reference's fixture
    data = open(img_path, "rb").read()
    out = {}
    log("bench: latency /embed")
    out["embed"] = dict(_lat(lambda: emb.embed_bytes(data), reps), what="embed_bytes (the /embed core): 300x168 "
                        "baseline JPEG -> GPU decode -> device resize -> ViT-MSN-base -> 768 floats on the host")
    vec = emb.embed_bytes(data)
    X, planted = planted_index_rows(query=vec)
    ix = ing.get_index("bench-latency-10k", dimension=768, dtype="float32", capacity=len(X))
    ix.upsert_tensor([f"r{i}" for i in range(len(X))], torch.from_numpy(X).to(torch.cuda.current_device()),
                     [{"gcs_path": f"images/r{i}.jpg"} for i in range(len(X))])
    got = ret.search(ix, vec, top_k=5)
    log("bench: latency search top-5")
    out["search_top5"] = dict(_lat(lambda: ret.search(ix, vec, top_k=5), reps * 5),
                              what="retriever.utils.search(index, emb, top_k=5) over 10,000 x 768 f32 rows "
                                   "(index.query with include_values=True, as the reference calls it), emb as "
                                   "embed_bytes returns it in process (retriever/main.py:122-128)",
                              planted_found=sorted(got) == sorted(f"r{r}" for r in planted))
    plain = [float(x) for x in vec]  # the same vector as a plain JSON list (an HTTP client's body)
    out["search_top5"]["plain_list"] = dict(
        _lat(lambda: ret.search(ix, plain, top_k=5), reps * 5),
        what="the same search with emb a plain list of 768 Python floats (parsed to f32 per call)")
    # where a request's time goes: the library call alone (one launch pair + sync, results as host
    # arrays) and the Python list building the Pinecone-shaped response needs on top
    qv = np.ascontiguousarray(np.asarray(vec, np.float32)[None])
    out["search_top5"]["library_call"] = dict(
        _lat(lambda: ix._set.query_host(qv, 5, len(X), True), reps * 5),
        what="rc_sharded_query_host alone (query in, scores + rows + 5 x 768 values out as host arrays)")
    vals = np.zeros((5, 768), np.float32)
    idxmod = importlib.import_module(f"{pkg}.index")
    out["search_top5"]["python_lists"] = dict(
        _lat(lambda: (idxmod._as_vector_np(plain, 768), vals.astype(np.float64).tolist()), reps * 5),
        what="what the request path no longer does: a 768-float query list parsed to an array, and 5 x 768 "
             "values built as lists (Index.query's matches build them only when read)")
    from fastapi.testclient import TestClient

    log("bench: latency /search_image")
    old_index = retmain.index
    retmain.index = lambda: ix
    try:
        # one TestClient session (its event-loop thread kept across requests, as a served app keeps
        # its loop): without the context manager TestClient starts a thread and an event loop per
        # request, ~0.8 ms that no deployment pays (tools/search_image_breakdown.py)
        with TestClient(retmain.app) as client:
            def post():
                r = client.post("/search_image", files={"file": ("test_image.jpeg", data, "image/jpeg")})
                assert r.status_code == 200 and len(r.json()) == 5
            out["search_image"] = dict(_lat(post, reps), what="POST /search_image through the FastAPI app (one "
                                       "TestClient session): multipart parse, GPU decode + embed (validating the "
                                       "upload), exact top-5, fetch, 5 URLs")
    finally:
        retmain.index = old_index
    if cpu:
        log("bench: latency CPU baselines")
        from PIL import Image

        from oracle.cosine_topk import cosine_topk_f32
        from oracle.preprocess import preprocess
        from oracle.weights import seeded_vit_msn_weights

        threads = _torch_threads()
        sd = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in seeded_vit_msn_weights(0).items()}
        fwd = torch_vit_forward_pixels(sd)

        def cpu_embed():
            im = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            with torch.inference_mode():
                return fwd(torch.from_numpy(preprocess(im)[None]))

        out["embed"]["cpu_baseline"] = dict(_lat(cpu_embed, 10, warm=2), cores=threads, kind="reference-lib",
                                            what="PIL decode + ViTImageProcessor arithmetic (resize, rescale, "
                                                 "normalize) + torch fp32 ViT-MSN-base forward, batch 1")
        Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
        q = np.asarray(vec, np.float32)
        out["search_top5"]["cpu_baseline"] = dict(_lat(lambda: cosine_topk_f32(Xn, q, 5), reps * 5), kind="port",
                                                  what="numpy exact cosine top-5 over the same 10k x 768 rows")
    ix.close()
    return out


def torch_vit_forward_pixels(sd):
    """pixel_values [B,3,224,224] f32 -> raw CLS: torch_vit_forward without the u8 rescale."""
    import torch.nn.functional as F

    fwd_u8 = torch_vit_forward(sd)

    def forward(x):
        e = F.conv2d(x, sd["embeddings.patch_embeddings.projection.weight"], sd["embeddings.patch_embeddings.projection.bias"], stride=16)
        return fwd_u8.encoder(e)

    return forward


def jpeg_300x168_line(model, B: int, world: int, rank: int, barrier, max_over_ranks, reps: int = 8, cpu: bool = True):
    """Batches of the reference fixture's shape (300 x 168 baseline JPEGs, tests/test_embedding.py:17;
    resize at embedding/main.py:107) through the bulk path: host Huffman of batch i+1 under GPU
    IDCT / colour / resize / embed of batch i.  CPU beside: Pillow decode + the processor's
    resize/rescale/normalize + torch fp32 forward, bounded."""
    import torch

    datas = synthetic_jpegs(B, 7100 + rank, size=(168, 300))  # W x H of tests/data/test_image.jpeg
    for _ in model.embed_jpeg_stream([datas] * 2):
        pass
    torch.cuda.synchronize()
    barrier()
    t0 = time.perf_counter()
    for _ in model.embed_jpeg_stream([datas] * reps):
        pass
    torch.cuda.synchronize()
    barrier()
    el = max_over_ranks(time.perf_counter() - t0)
    long_reps = 3 * reps  # steady state: the pipeline fill (first batch's host Huffman) cancels out
    barrier()
    t0 = time.perf_counter()
    for _ in model.embed_jpeg_stream([datas] * long_reps):
        pass
    torch.cuda.synchronize()
    barrier()
    el_long = max_over_ranks(time.perf_counter() - t0)
    out = {"workload": f"{B} synthetic 168x300 (WxH, the reference fixture's shape) q90 4:2:0 baseline JPEGs per "
                       f"batch per GPU, {reps} batches: GPU JPEG "
                       f"decode (bit-exact with PIL) -> Pillow-exact bicubic resize to 224 -> ViT-MSN-base",
           "value": world * B * reps / el, "unit": "images/s (JPEG bytes -> embedding)",
           "marginal_value": world * B * (long_reps - reps) / max(el_long - el, 1e-9),
           "marginal_note": f"({long_reps} - {reps}) batches / (t({long_reps}) - t({reps})): steady state without "
                            f"the pipeline fill"}
    if cpu:
        from PIL import Image

        from oracle.preprocess import preprocess
        from oracle.weights import seeded_vit_msn_weights

        threads = _torch_threads()
        sd = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in seeded_vit_msn_weights(0).items()}
        fwd = torch_vit_forward_pixels(sd)
        done, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 10.0 or done == 0:
            batch = [np.asarray(Image.open(io.BytesIO(datas[(done + j) % len(datas)])).convert("RGB")) for j in range(16)]
            with torch.inference_mode():
                fwd(torch.from_numpy(np.stack([preprocess(im) for im in batch])))
            done += 16
        cel = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": done / cel, "unit": "images/s", "cores": threads, "kind": "reference-lib",
                               "sample": f"{done} of the same JPEGs: PIL decode + ViTImageProcessor arithmetic (numpy "
                                         f"restatement, bit-exact) + torch fp32 forward in batches of 16, {cel:.1f}s"}
    return out


def gemm_roofline(args, model, images, raw, nrm, B: int, dev):
    """Roofline of the projection GEMMs (--full): the timed steps run the batch as --parts
    concurrent slices, so a GEMM launch there shares the GPU; each GEMM's own efficiency is
    timed on the unsplit batch (the GEMM alone on the chip), with HIP events on the launch
    stream around every full-batch launch of that projection.  `roofline` prices the one that
    takes the most time per step; `gemms` lists all four.  Returns (gemms, the dominant one,
    GEMM ms per step, attention ms, attention launches)."""
    import torch

    M = B * 197
    shapes = {"qkv": (M, 2304, 768, "gemm_pp_kernel<4,0,12> (QKV, LayerNorm 1 folded in)"),
              "oproj": (M, 768, 768, "gemm_w2_kernel<6,0> (O-proj + residual + LN-2 statistics; two workgroups per CU)"),
              "fc1": (M, 3072, 768, "gemm_pp_kernel<5,0,12> (fc1 + GELU, LayerNorm 2 folded in)"),
              "fc2": (M, 768, 3072, "gemm_pp_kernel<6,0,48> (fc2 + residual + LN-1 statistics)")}
    model.set_parts(1)
    model.embed(images, out=(raw, nrm))
    torch.cuda.synchronize()
    model.timing(list(shapes) + ["attention"])
    model.timing_reset()
    for _ in range(args.roofline_steps):
        model.embed(images, out=(raw, nrm))
    torch.cuda.synchronize()
    gemms = {}
    for role, (gm, gn, gk, kname) in shapes.items():
        ms, n, fl = model.timing_read(role)
        avg = ms / max(n, 1)
        tf = (fl / max(n, 1)) / (avg / 1e3) / 1e12 if avg > 0 else 0.0
        gemms[role] = {"kernel": f"{kname}: M={gm} N={gn} K={gk}", "avg_launch_ms": avg, "launches": n,
                       "flops_per_launch": fl / max(n, 1), "achieved_tflops": tf, "frac": tf / PEAK_BF16_TFLOPS,
                       "ms_per_step": ms / args.roofline_steps, "traffic": load_profile_traffic(role)}
    att_ms, att_n, _ = model.timing_read("attention")
    model.timing(False)
    model.set_parts(args.parts)
    # yardstick: the vendor library's plain GEMM on each shape (torch.mm -> hipBLASLt, random bf16
    # operands, no epilogue; min over 3 rounds of 10); never on the product path
    for role, (gm, gn, gk, _) in shapes.items():
        gv = torch.Generator(device=dev).manual_seed(7)
        Av = (torch.rand(gm, gk, device=dev, generator=gv) * 2 - 1).to(torch.bfloat16)
        Wv = ((torch.rand(gn, gk, device=dev, generator=gv) * 2 - 1) * 0.05).to(torch.bfloat16)
        best = float("inf")
        for _ in range(3):
            torch.mm(Av, Wv.t())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                torch.mm(Av, Wv.t())
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / 10)
        gemms[role]["vendor_ms"] = best
        gemms[role]["vs_vendor"] = gemms[role]["avg_launch_ms"] / best
        del Av, Wv
    dominant = max(gemms, key=lambda r: gemms[r]["ms_per_step"])
    gemm_step_ms = sum(g["ms_per_step"] for g in gemms.values())
    return gemms, gemms[dominant], gemm_step_ms, att_ms, att_n


def main():
    import faulthandler

    faulthandler.dump_traceback_later(120, repeat=True, file=sys.stderr)  # a stuck stage names itself
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows-per-gpu", type=int, default=125_000_000)
    ap.add_argument("--search-queries", type=int, default=20)
    ap.add_argument("--batch-queries", type=int, default=1024)
    ap.add_argument("--batch-reps", type=int, default=3)
    ap.add_argument("--roofline-steps", type=int, default=5)
    ap.add_argument("--parts", type=int, default=2, help="concurrent batch slices per GPU (rc_model_set_parts)")
    ap.add_argument("--full-last-layer", action="store_true",
                    help="run the last encoder layer on every row (default: CLS rows only, rc_model_set_last_layer)")
    ap.add_argument("--no-ln-fold", action="store_true",
                    help="run the standalone LayerNorm kernel instead of folding LN into QKV / fc1 (A/B)")
    ap.add_argument("--ingest-images", type=int, default=1_250_000,
                    help="config 5: images embedded + upserted per GPU (10M / 8 GPUs; 0 = skip)")
    ap.add_argument("--no-latency", action="store_true", help="skip the batch-1 latency lines")
    ap.add_argument("--jpeg-images", type=int, default=256, help="JPEG decode sample per GPU (0 = skip)")
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--dry-run", action="store_true", help="rank plumbing only (gloo, no GPU)")
    ap.add_argument("--full", action="store_true",
                    help="also measure the GEMM roofline, ingest, JPEG, latency, search and the CPU baselines "
                         "(default: the timed embed steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (raw, nrm) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not args.full:  # a plain run: the headline only
        args.ingest_images = args.jpeg_images = 0
        args.no_latency = args.no_search = args.no_cpu = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one process per GPU: hand off to torch.distributed.run BEFORE anything touches the GPU
        import socket
        import subprocess

        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        log("bench: launching", " ".join(cmd))
        sys.exit(subprocess.call(cmd))

    import importlib

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench: --gpus {args.gpus} but the launcher started {world} ranks")
    if args.dry_run:
        if world > 1:
            dist.init_process_group("gloo")
            t = torch.tensor([1.0])
            dist.all_reduce(t)
            seen = int(t.item())
            dist.destroy_process_group()
        else:
            seen = 1
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "ranks_seen": seen}), flush=True)
        return
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
        assert dist.get_world_size() == args.gpus

    def barrier():
        if world > 1:
            dist.barrier()

    def max_over_ranks(x: float) -> float:
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    vit = importlib.import_module(f"{PKG}.vit")
    index = importlib.import_module(f"{PKG}.index")

    # ------------------------------------------------------ embed (value) --
    if rank == 0:
        log("bench: stage: embed (timed steps)")
    B = args.batch
    model = vit.VitMsnEmbedder(vit.random_state_dict(seed=0), device=local, max_batch=B)
    model.set_parts(args.parts)
    model.set_last_layer(not args.full_last_layer)
    model.set_ln_fold(not args.no_ln_fold)
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    images = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev, generator=g)
    raw = torch.empty((B, 768), dtype=torch.float32, device=dev)
    nrm = torch.empty((B, 768), dtype=torch.float32, device=dev)
    for _ in range(args.warmup):
        model.embed(images, out=(raw, nrm))
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model.embed(images, out=(raw, nrm))
    torch.cuda.synchronize()
    barrier()
    el = max_over_ranks(time.perf_counter() - t0)
    assert torch.isfinite(raw).all()
    imgs_per_s = world * B * args.steps / el
    if args.dump_outputs:
        # what the last timed step handed its caller, before anything below writes raw / nrm again
        os.makedirs(args.dump_outputs, exist_ok=True)
        suffix = "" if rank == 0 else f".rank{rank}"
        for name, t in (("raw", raw), ("nrm", nrm)):
            np.save(os.path.join(args.dump_outputs, f"{name}{suffix}.npy"), t.cpu().numpy().astype(np.float32))
    gemms, dom, gemm_step_ms, att_ms, att_n = {}, None, 0.0, 0.0, 0
    if args.full:
        gemms, dom, gemm_step_ms, att_ms, att_n = gemm_roofline(args, model, images, raw, nrm, B, dev)
    # FLOPs rc_embed executes per image (the CLS-only last layer skips the rows
    # /embed never returns); the full-model figure is reported beside it
    gflop = vit.gflop_per_image(cls_only_last=not args.full_last_layer)
    model_tflops = imgs_per_s / world * gflop / 1e3

    # ------------------------------------ config 5: end-to-end ingest + retrieve --
    if rank == 0:
        log("bench: stage: config 5 ingest")
    ingest = None
    if args.ingest_images > 0:
        sharded_mod = importlib.import_module(f"{PKG}.sharded")
        n_img = (args.ingest_images + B - 1) // B * B
        sidx5 = sharded_mod.ShardedIndex(768, dtype="float16", capacity_per_rank=n_img, device=local)
        local_rows = torch.arange(B, dtype=torch.int64, device=dev)
        g5 = torch.Generator(device=dev).manual_seed(6000 + rank)
        model.embed(images, out=(raw, nrm))  # warm
        sidx5.upsert_local(nrm, local_rows)
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tlog = t0
        for b0 in range(0, n_img, B):
            batch = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev, generator=g5)
            model.embed(batch, out=(raw, nrm))
            sidx5.upsert_local(nrm, local_rows + b0)  # each rank fills its own shard: no collective
            if rank == 0 and time.perf_counter() - tlog > 15:
                tlog = time.perf_counter()
                log(f"bench: config 5 ingest {b0 + B:,}/{n_img:,} images ({(b0 + B) / (tlog - t0):,.0f}/s)")
        torch.cuda.synchronize()
        barrier()
        el5 = max_over_ranks(time.perf_counter() - t0)
        n_rows5 = sidx5.publish_rows()  # local row j of rank r is global row j * world + r
        # retrieve: queries = rank 0's first ingested images, regenerated and embedded on every rank
        nq5 = args.batch_queries
        gq5 = torch.Generator(device=dev).manual_seed(6000)
        q5 = torch.empty((nq5, 768), dtype=torch.float32, device=dev)
        for q0 in range(0, nq5, B):
            qimgs = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device=dev, generator=gq5)
            model.embed(qimgs, out=(raw, nrm))
            q5[q0:q0 + B] = nrm[:min(B, nq5 - q0)]
        sidx5.search(q5, 100, mode="mfma")
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        s5, r5 = sidx5.search(q5, 100, mode="mfma")
        torch.cuda.synchronize()
        barrier()
        el5q = max_over_ranks(time.perf_counter() - t0)
        recall1 = float((r5[:, 0].cpu() == torch.arange(nq5) * world).float().mean())  # rank 0's rows j*world
        ingest = {
            "workload": f"BASELINE config 5 at its per-GPU size: {n_img:,} synthetic 224x224 images per GPU "
                        f"({world * n_img:,} in all) generated on device, embedded (ViT-MSN-base, batches of {B}) "
                        f"and upserted rank-locally into a row-sharded 768-d fp16 index, then {nq5} queries top-100 "
                        f"(batched MFMA search + RCCL all-gather merge)",
            "value": world * n_img / el5, "unit": "images/s (embed + upsert)", "seconds": el5,
            "index_rows": n_rows5,
            "retrieve": {"value": nq5 / el5q, "unit": "queries/s", "ms_per_batch": el5q * 1e3,
                         "queries": nq5, "k": 100, "index_rows": n_rows5, "top1_self_recall": recall1},
        }
        sidx5.close()
        del sidx5

    # --------------------------- JPEG decode + decode→embed --
    if rank == 0:
        log("bench: stage: JPEG decode + ingest core")
    jpeg = None
    if args.jpeg_images > 0:
        J = importlib.import_module(f"{PKG}.jpeg")
        datas = synthetic_jpegs(args.jpeg_images, 7000 + rank)
        dec = J.JpegDecoder(local, max_images=len(datas), max_pixels=len(datas) * 224 * 224)
        dec.decode(datas)
        torch.cuda.synchronize()
        reps = 5
        barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            dec.decode(datas)
        torch.cuda.synchronize()
        barrier()
        eld = max_over_ranks(time.perf_counter() - t0)
        dec.close()
        # a bulk-ingest stream long enough that the pipeline's fill (the first
        # batch's host decode, not overlapped) does not dominate the rate
        stream_reps = 12
        stream_batches = [datas[:B]] * stream_reps
        for _ in model.embed_jpeg_stream(stream_batches[:1]):
            pass
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for _ in model.embed_jpeg_stream(stream_batches):  # host decode of i+1 overlaps embed of i
            pass
        torch.cuda.synchronize()
        barrier()
        ele = max_over_ranks(time.perf_counter() - t0)
        # marginal (steady-state) rate: a 3x longer stream minus the 12-batch one
        # cancels the fill; Huffman thread count is not the limiter (RC_JPEG_THREADS A/B)
        long_reps = 3 * stream_reps
        barrier()
        t0 = time.perf_counter()
        for _ in model.embed_jpeg_stream([datas[:B]] * long_reps):
            pass
        torch.cuda.synchronize()
        barrier()
        ele_long = max_over_ranks(time.perf_counter() - t0)
        marginal = world * min(B, len(datas)) * (long_reps - stream_reps) / max(ele_long - ele, 1e-9)
        jpeg = {"workload": f"{len(datas)} synthetic 224x224 q90 4:2:0 baseline JPEGs per GPU (~{sum(map(len, datas)) // len(datas) // 1024} KB "
                            f"each): host Huffman decode (threaded) + HIP islow IDCT / fancy upsampling / YCbCr->RGB, "
                            f"bit-exact with PIL; host buffers in, device HWC RGB out",
                "value": world * len(datas) * reps / eld, "unit": "images/s (decode)",
                "decode_embed": {"value": world * min(B, len(datas)) * stream_reps / ele, "unit": "images/s (JPEG bytes -> embedding)",
                                 "batches": stream_reps,
                                 "marginal_value": marginal,
                                 "marginal_note": f"({long_reps} - {stream_reps}) batches / (t({long_reps}) - t({stream_reps})): steady state without the pipeline fill",
                                 "pipeline": "embed_jpeg_stream: host Huffman of batch i+1 (worker thread, side stream) under the GPU embed of batch i"}}
        if rank == 0 and world == 1 and not args.no_cpu:
            jpeg["cpu_baseline"] = cpu_jpeg_baseline(datas)
        # the batched ingest core behind POST /push_images (ingesting/core.py: the reference's
        # push_image steps per image, one decode / embed / upsert pass per batch)
        core = importlib.import_module(f"{PKG}.ingesting.core")
        importlib.import_module(f"{PKG}.config").Config.EMBED_MAX_BATCH = B  # the service embedder's batch
        files = [(f"img{i}.jpg", d, "image/jpeg") for i, d in enumerate(datas[:B])]
        ireps = 4
        ix = importlib.import_module(f"{PKG}.index").Index("bench-ingest", dimension=768, dtype="float16",
                                                           capacity=len(files) * (ireps + 1), device=local)
        core.ingest_many(files, ix)  # warm: creates the service embedder
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for _ in range(ireps):
            resp = core.ingest_many(files, ix)
        torch.cuda.synchronize()
        barrier()
        eli = max_over_ranks(time.perf_counter() - t0)
        jpeg["ingest_core"] = {
            "value": world * len(files) * ireps / eli,
            "unit": "images/s (JPEG bytes -> validated, GPU-decoded, embedded, upserted, per-image responses)",
            "what": f"ingesting.core.ingest_many over {len(files)} JPEG uploads per call, {ireps} calls, uuid ids, "
                    f"string-id fp16 Index (host id map + metadata); GCS is a no-op hook",
            "responses_ok": len(resp) == len(files) and all(r["message"] == "Successfully!" for r in resp),
        }
        ix.close()
        # bulk ingest: the same batches through ingest_stream (decode of batch i+1 under the
        # embed + upsert of batch i)
        sreps = 16
        ix = importlib.import_module(f"{PKG}.index").Index("bench-ingest-stream", dimension=768, dtype="float16",
                                                           capacity=len(files) * (sreps + 2), device=local)
        for _ in core.ingest_stream([files] * 2, ix):  # warm
            pass
        torch.cuda.synchronize()
        import gc

        gc.collect()  # a full collection of this large process inside the timed loop costs ~60 ms
        barrier()
        t0 = time.perf_counter()
        nresp = 0
        tb = time.perf_counter()
        for resp in core.ingest_stream([files] * sreps, ix):
            nresp += len(resp)
            if os.environ.get("BENCH_DEBUG"):
                log(f"ingest_stream batch {nresp // len(files)}: {(time.perf_counter() - tb) * 1e3:.1f} ms")
                tb = time.perf_counter()
        torch.cuda.synchronize()
        barrier()
        els = max_over_ranks(time.perf_counter() - t0)
        jpeg["ingest_core"]["stream"] = {
            "value": world * len(files) * sreps / els,
            "unit": "images/s (JPEG bytes -> responses, pipelined)",
            "what": f"ingesting.core.ingest_stream over {sreps} batches of {len(files)} JPEG uploads: validation + "
                    f"decode of batch i+1 (worker thread, side stream) under the embed + upsert of batch i",
            "responses_ok": nresp == len(files) * sreps,
        }
        ix.close()

    if jpeg is not None:
        if rank == 0:
            log("bench: stage: 168x300 JPEG line")
        jpeg["fixture_shape"] = jpeg_300x168_line(model, B, world, rank, barrier, max_over_ranks,
                                                  cpu=rank == 0 and world == 1 and not args.no_cpu)
    latency = None
    if not args.no_latency:
        latency = latency_lines(PKG, cpu=rank == 0 and world == 1 and not args.no_cpu)

    model.close()
    del images, raw, nrm
    torch.cuda.empty_cache()

    result = {
        "metric": METRIC,
        "value": imgs_per_s,
        "unit": "images/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": el / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic (uniform u8 224x224x3 images, random-init ViT-MSN-base weights; no checkpoint offline)",
        "config": {
            "workload": "BASELINE config 2: batch-256 224x224 images per GPU through preprocess + ViT-MSN-base (12 layers) + CLS/L2-norm",
            "global_batch": B * world,
            "seq_len": 197,
            "parallelism": f"dp{world}",
        },
        "embed_parts": args.parts,
        "layernorm": "standalone kernel" if args.no_ln_fold else
        "folded into QKV / fc1 epilogues (producers emit bf16(x) + per-tile mean/M2)",
        "last_layer": "full" if args.full_last_layer else
        "CLS rows only after QKV (the rows /embed returns, embedding/main.py:113)",
        "gflop_per_image_executed": gflop,
        "gflop_per_image_full_model": vit.gflop_per_image(),
        "model_tflops_per_gpu": model_tflops,
        "model_mfma_frac": model_tflops / PEAK_BF16_TFLOPS,
    }
    if args.full:
        result.update({
            "roofline": {
                "kernel": dom["kernel"] + " — the projection GEMM with the most time per step",
                "bound": "mfma",
                "achieved": dom["achieved_tflops"],
                "peak": PEAK_BF16_TFLOPS,
                "unit": "TFLOP/s",
                "frac": dom["achieved_tflops"] / PEAK_BF16_TFLOPS,
                "traffic": dom["traffic"],
                "avg_launch_ms": dom["avg_launch_ms"],
                "launches": dom["launches"],
                "flops_per_launch": dom["flops_per_launch"],
                "measured_on": "unsplit batch (parts=1), HIP events on the launch stream around each full-batch launch",
            },
            "gemms": gemms,
            "gemm_ms_per_step": gemm_step_ms,
            "attention_ms_per_step": att_ms / args.roofline_steps,
            "attention_avg_launch_ms": att_ms / max(att_n, 1),
        })
    if ingest is not None:
        result["ingest"] = ingest
    if jpeg is not None:
        result["jpeg"] = jpeg
    if latency is not None:
        result["latency"] = latency

    # ------------------------------------------------- search (secondary) --
    if rank == 0:
        log("bench: stage: search")
    if not args.no_search:
        dim = 512
        rows = args.rows_per_gpu
        sharded = importlib.import_module(f"{PKG}.sharded")
        sidx = sharded.ShardedIndex(dim, dtype="float16", capacity_per_rank=rows, device=local)
        sidx.fill_random(4 + rank, rows)
        shard = sidx.local
        shard.reserve(1, 10)
        gq = torch.Generator(device=dev).manual_seed(5)
        queries = torch.randn((args.search_queries, dim), device=dev, generator=gq)  # same on every rank
        k = 10

        def one_query(qi):
            return sidx.search(queries[qi:qi + 1], k)

        for qi in range(2):
            one_query(qi)
        torch.cuda.synchronize()
        shard.timing(True)
        barrier()
        t0 = time.perf_counter()
        for qi in range(args.search_queries):
            one_query(qi)
        torch.cuda.synchronize()
        barrier()
        sel = max_over_ranks(time.perf_counter() - t0)
        scan_ms, scan_n, scan_bytes = shard.timing_read()
        shard.timing(False)
        scan_gbps = scan_bytes / (scan_ms / 1e3) / 1e9
        result["search"] = {
            "workload": f"BASELINE config 4 single-query variant: {rows * world:,} x 512 fp16 rows ({rows:,}/GPU), exact cosine top-{k}",
            "value": args.search_queries / sel,
            "unit": "queries/s",
            "ms_per_query": sel / args.search_queries * 1e3,
            "roofline": {"kernel": "scan_topk_kernel<f16,4,1,128>", "bound": "hbm", "achieved": scan_gbps,
                         "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": scan_gbps / PEAK_HBM_GBPS,
                         "traffic": load_profile_traffic("scan_f16"), "avg_launch_ms": scan_ms / max(scan_n, 1),
                         "bytes_per_launch": scan_bytes / max(scan_n, 1)},
        }
        # config 4 as named: a batch of 1024 queries, top-100, batched MFMA path
        # (staged filter GEMM + exact rescoring per shard, RCCL all-gather + merge), first
        # with the f16 filter on the stored rows, then with the int8 filter copy
        nqb, kb = args.batch_queries, 100
        gqb = torch.Generator(device=dev).manual_seed(6)
        qbatch = torch.randn((nqb, dim), device=dev, generator=gqb)

        def batched_run(tag):
            sidx.search(qbatch, kb, mode="mfma")
            torch.cuda.synchronize()
            shard.timing(True)
            shard.gemm_timing_read()
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.batch_reps):
                out = sidx.search(qbatch, kb, mode="mfma")
            torch.cuda.synchronize()
            barrier()
            bel = max_over_ranks(time.perf_counter() - t0)
            g_ms, g_n, g_flops, g_fb = shard.gemm_timing_read()
            shard.timing(False)
            g_tf = g_flops / (g_ms / 1e3) / 1e12 if g_ms > 0 else 0.0
            i8 = tag == "i8"
            peak = PEAK_I8_TOPS if i8 else PEAK_BF16_TFLOPS
            kern = ("filter_i8_kernel<4> (int8 copy of the rows: 256 queries per block, 32 per wave in registers x "
                    "128-row tiles, 8-step LDS ring, per-row scale + residual-norm bound epilogue)" if i8 else
                    "filter_qs_kernel<f16,8,0> (256 queries per block, 32 per wave in registers x 128-row tiles, "
                    "8-step LDS ring, candidate epilogue)")
            return out, {
                "value": nqb * args.batch_reps / bel,
                "unit": "queries/s",
                "ms_per_batch": bel / args.batch_reps * 1e3,
                "filter": ("int8 copy (rc_index_set_filter(RC_FILTER_I8)); candidates rescored exactly on the fp16 rows"
                           if i8 else "fp16 stored rows"),
                "roofline": {"kernel": kern, "bound": "mfma", "achieved": g_tf, "peak": peak,
                             "unit": "TOP/s" if i8 else "TFLOP/s", "frac": g_tf / peak,
                             "traffic": load_profile_traffic("filter_i8" if i8 else "filter_f16"),
                             "avg_launch_ms": g_ms / max(g_n, 1), "launches": g_n,
                             "ops_per_batch": g_flops / max(args.batch_reps, 1)},
                "gemm_share_of_batch": (g_ms / args.batch_reps) / (bel / args.batch_reps * 1e3),
                "exact_fallbacks": g_fb,
            }

        (s_f16, r_f16), native = batched_run("f16")
        t0 = time.perf_counter()
        shard.set_filter("i8")  # quantises the shard's rows once (int8 copy + per-row scale / bound)
        torch.cuda.synchronize()
        quant_s = time.perf_counter() - t0
        (s_i8, r_i8), best = batched_run("i8")
        same = bool(torch.equal(r_f16, r_i8) and torch.equal(s_f16, s_i8))
        if rank == 0:
            log(f"bench: batched f16 {native['value']:.0f} q/s, int8 filter {best['value']:.0f} q/s, identical={same}")
        result["search"]["batched"] = {
            "workload": f"BASELINE config 4: {rows * world:,} x 512 fp16 rows ({rows:,}/GPU), batch of {nqb} queries, exact top-{kb}",
            **best,
            "identical_to_f16_filter": same,
            "quantise_seconds": quant_s,
            "f16_filter": native,
        }
        shard.set_filter("native")
        sidx.close()
        del shard, sidx
        torch.cuda.empty_cache()
        # config 3: 1M x 512 f32, single query top-10 on one GPU (rank-local)
        c3 = index.DeviceIndex(dim, dtype="float32", capacity=1_000_000, device=local)
        c3.fill_random(2, 0, 1_000_000)
        for qi in range(3):
            c3.search(queries[qi:qi + 1], 10, 1_000_000)
        torch.cuda.synchronize()
        c3.timing(True)
        t0 = time.perf_counter()
        nq3 = 200
        for qi in range(nq3):
            c3.search(queries[qi % args.search_queries:qi % args.search_queries + 1], 10, 1_000_000)
        torch.cuda.synchronize()
        el3 = time.perf_counter() - t0
        ms3, n3, b3 = c3.timing_read()
        c3.timing(False)
        # recall@10 of an f16 index against the unquantised f32 rows (north_star: "recall@k
        # against the fp32 oracle"; the f32 scan is exact against the float64 oracle, tests/)
        c3h = index.DeviceIndex(dim, dtype="float16", capacity=1_000_000, device=local)
        c3h.fill_random(2, 0, 1_000_000)
        gr = torch.Generator(device=dev).manual_seed(11)
        qr = torch.randn((256, dim), device=dev, generator=gr)
        _, r32 = c3.search(qr, 10, 1_000_000, mode="scan")
        _, r16 = c3h.search(qr, 10, 1_000_000, mode="mfma")
        r32c, r16c = r32.cpu().tolist(), r16.cpu().tolist()
        recall = sum(len(set(a) & set(b)) for a, b in zip(r32c, r16c)) / (10 * len(r32c))
        c3h.close()
        c3.close()
        result["search"]["config3"] = {"workload": "BASELINE config 3: 1M x 512 f32, single query exact top-10, 1 GPU",
                                       "value": nq3 / el3, "unit": "queries/s (per GPU)",
                                       "scan_GBps": b3 / (ms3 / 1e3) / 1e9, "scan_frac": b3 / (ms3 / 1e3) / 1e9 / PEAK_HBM_GBPS}
        result["search"]["recall_vs_fp32"] = {
            "value": recall, "k": 10, "queries": len(r32c),
            "what": "recall@10 of a 1M x 512 fp16 index (batched MFMA path) against the exact top-10 of the same "
                    "rows unquantised in fp32; misses are rows whose fp32 score lies within the fp16 storage "
                    "rounding (2 x 2^-11) of the 10th (tests/test_batched_search_gpu.py)"}

    if rank == 0 and world == 1 and not args.no_cpu:
        log("bench: stage: CPU baselines")
        try:
            result["cpu_baseline"] = cpu_embed_baseline()
            if result.get("ingest") is not None:
                result["ingest"]["cpu_baseline"] = cpu_ingest_baseline(10_000_000)
            if "search" in result:
                result["search"]["cpu_baseline"] = cpu_search_baseline()
                if "batched" in result["search"]:
                    result["search"]["batched"]["cpu_baseline"] = cpu_batch_search_baseline(
                        index_rows=args.rows_per_gpu * world)
        except Exception as e:  # the baseline must not kill the GPU bench line
            result["cpu_baseline"] = {"error": repr(e)}

    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
