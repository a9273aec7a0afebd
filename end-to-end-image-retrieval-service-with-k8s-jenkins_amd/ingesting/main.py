"""Ingest service on the MI355X core (mirror of reference ``ingesting/main.py``).

Contract kept (``ingesting/main.py:91-168``):
  GET  /             → {"message": "Welcome to the Image Ingestion API. Visit /docs to test."}
  GET  /healthz      → {"status": "healthy"}
  POST /push_image   multipart ``file`` → {"message", "file_id", "gcs_path", "signed_url"}
                     400 "Only .jpg/.jpeg/.png allowed" / "Invalid image file"; 422 without ``file``
  POST /push_images  (batched form) repeated ``files`` → one such dict per image (ingesting.core.ingest_many)
  POST /delete_images JSON ``{"ids": [...]}`` → {"deleted_count": ids that existed}; 422 without a list ``ids``
                     (no reference counterpart: ``Index.delete``)
  /push_image and /push_images take an optional form field ``namespace``, /delete_images an optional
  JSON key ``"namespace"`` (a string; 422 otherwise): the index namespace written to or deleted from
  (absent = the default one)

``get_feature_vector`` is a module-level name, as in the reference (whose tests
monkeypatch ``ingesting.main.get_feature_vector``); by default it embeds in
process on the GPU (``RC_EMBED_IN_PROCESS=0`` POSTs to the /embed service like the
reference).  The index is opened on first use (the reference opens Pinecone at
import, ``:37``).  GCS is a no-op ``StorageHook`` (blob storage is out of scope);
OTel/Prometheus instrumentation is out of scope.
"""
from __future__ import annotations

import json

from fastapi import FastAPI, Request
from fastapi.exceptions import RequestValidationError

from ..config import Config
from ..multipart import parse_form, parse_form_all
from . import core
from .utils import embed_locally, get_index
from .utils import get_feature_vector as _remote_feature_vector

app = FastAPI(title="Image Ingestion Service")
get_feature_vector = embed_locally if Config.EMBED_IN_PROCESS else _remote_feature_vector
storage = core.StorageHook()


def index():
    return get_index(Config.INDEX_NAME)


def _feature_fn(request: Request):
    """The app serving this request may embed its own way (service.py's one-process app sets
    ``app.state.feature_vector``); otherwise this module's ``get_feature_vector`` (the name the
    reference's tests monkeypatch)."""
    fn = getattr(request.app.state, "feature_vector", None)
    return fn if fn is not None else get_feature_vector


def _missing_file(field: str):
    return RequestValidationError([{"type": "missing", "loc": ("body", field), "msg": "Field required", "input": None}])


@app.get("/")
def read_root():
    return {"message": "Welcome to the Image Ingestion API. Visit /docs to test."}


@app.get("/healthz")
def health_check():
    return {"status": "healthy"}


@app.post("/push_image")
async def push_image(request: Request):
    form = parse_form(await request.body(), request.headers.get("content-type", ""))
    f = form.get("file")
    if f is None:
        raise _missing_file("file")
    return core.push_one(f.filename, f.data, index, content_type=f.content_type, storage=storage,
                         feature_fn=_feature_fn(request), namespace=core.form_namespace(form.get("namespace")))


@app.post("/push_images")
async def push_images(request: Request):
    form = parse_form_all(await request.body(), request.headers.get("content-type", ""))
    parts = form.get("files")
    if not parts:
        raise _missing_file("files")
    ns = form.get("namespace")
    return core.ingest_many([(f.filename, f.data, f.content_type) for f in parts], index, storage=storage,
                            namespace=core.form_namespace(ns[-1] if ns else None))


@app.post("/delete_images")
async def delete_images(request: Request):
    """Remove ingested images from the index by the ``file_id`` /push_image returned
    (``Index.delete``; the reference has no such route: its Pinecone index is only ever
    written).  Unknown ids are ignored; the stored blob is the storage hook's business."""
    try:
        body = json.loads(await request.body() or b"null")
    except ValueError:
        body = None
    ids = body.get("ids") if isinstance(body, dict) else None
    if not isinstance(ids, list) or not all(isinstance(i, str) for i in ids):
        raise RequestValidationError([{"type": "list_type", "loc": ("body", "ids"), "msg": "Input should be a list of ids",
                                       "input": None}])
    namespace = body.get("namespace", "")
    if not isinstance(namespace, str):
        raise RequestValidationError([{"type": "string_type", "loc": ("body", "namespace"), "msg": "Input should be a string",
                                       "input": None}])
    # Index.delete is Pinecone's call and returns {}; its body reports how many ids existed
    if not ids:
        return {"deleted_count": 0}
    return {"deleted_count": index()._delete(ids, False, None, namespace) if namespace else index()._delete(ids, False, None)}
