"""``POST /search_image`` with the optional ``filter`` form field (a Pinecone-style metadata
filter as a JSON object), through the one-process app: push, then search filtered."""
import io
import json

import numpy as np
import pytest
from fastapi.testclient import TestClient

from conftest import import_pkg

pytestmark = pytest.mark.gpu


def _jpeg(seed, w=224, h=224):
    from PIL import Image

    arr = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", quality=85)
    return b.getvalue()


def test_search_image_with_a_metadata_filter(cuda, monkeypatch):
    cfg = import_pkg("config").Config
    name = "filtered-search-service"
    monkeypatch.setattr(cfg, "INDEX_NAME", name)
    svc = TestClient(import_pkg("service").app)
    try:
        a, b = _jpeg(501), _jpeg(502, 256, 200)
        pushed = {}
        for fn, blob in (("first.jpg", a), ("second.jpg", b)):
            r = svc.post("/push_image", files={"file": (fn, blob, "image/jpeg")})
            assert r.status_code == 200
            pushed[fn] = r.json()["signed_url"]
        # no filter field: today's behaviour (both images, the query's own first)
        plain = svc.post("/search_image", files={"file": ("q.jpg", a, "image/jpeg")})
        assert plain.status_code == 200 and plain.json() == [pushed["first.jpg"], pushed["second.jpg"]]
        # the filter restricts the search to the OTHER image, although the query is image a
        for fn in ("first.jpg", "second.jpg"):
            r = svc.post("/search_image", files={"file": ("q.jpg", a, "image/jpeg")},
                         data={"filter": json.dumps({"filename": fn})})
            assert r.status_code == 200 and r.json() == [pushed[fn]], fn
        r = svc.post("/search_image", files={"file": ("q.jpg", a, "image/jpeg")},
                     data={"filter": json.dumps({"filename": {"$in": ["nope.jpg"]}})})
        assert r.status_code == 200 and r.json() == []
        # an empty filter object is no filter
        r = svc.post("/search_image", files={"file": ("q.jpg", a, "image/jpeg")}, data={"filter": "{}"})
        assert r.status_code == 200 and r.json() == plain.json()
        # not JSON, not an object, not a valid filter: 400
        for bad in ("{not json", "[1, 2]", '"filename"', json.dumps({"filename": {"$regex": "x"}})):
            r = svc.post("/search_image", files={"file": ("q.jpg", a, "image/jpeg")}, data={"filter": bad})
            assert r.status_code == 400 and r.json()["detail"] == "Invalid filter.", bad
    finally:
        utils = import_pkg("ingesting.utils")
        ix = utils._indexes.pop(name, None)
        if ix is not None:
            ix.close()
