"""Retrieve helpers on the MI355X core (mirror of reference ``retriever/utils.py``).

``get_index`` and ``get_feature_vector`` are the ingest helpers (the reference
duplicates them verbatim, ``retriever/utils.py:23-56``); ``search`` keeps the
reference's contract (``:59-66``): ``ValueError("Input embedding is empty")`` on a
falsy input, otherwise ``index.query(vector, top_k, include_values=True)``
→ ids, best first.  The query itself is the HIP exact cosine scan + top-k.
``filter`` (not in the reference) is a Pinecone-style metadata filter; it is passed to
``index.query`` only when given, so an index object that knows nothing of filters keeps working.
``namespace`` (Pinecone's; ``""`` = the default one) likewise travels only when it names one,
and ``sparse_vector`` (the sparse part of a sparse-dense query) only when given.
"""
from __future__ import annotations

from ..ingesting.utils import embed_locally, get_feature_vector, get_index  # noqa: F401


def search(index, input_emb, top_k, filter=None, namespace="", sparse_vector=None):
    if input_emb is None or len(input_emb) == 0:
        raise ValueError("Input embedding is empty")
    extra = {}
    if filter is not None:
        extra["filter"] = filter
    if namespace:
        extra["namespace"] = namespace
    if sparse_vector is not None:
        extra["sparse_vector"] = sparse_vector
    matching = index.query(vector=input_emb, top_k=top_k, include_values=True, **extra)["matches"]
    match_ids = [match_id["id"] for match_id in matching]
    return match_ids
