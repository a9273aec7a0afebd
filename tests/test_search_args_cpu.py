"""The argument contract of every search entry point of the C ABI, on a host without a GPU: a
null handle, a bad ``k``, a negative query count and a null buffer are refused with
RC_ERR_INVALID before anything reads the handle (``check_search_args``, index_common.h), so a
handle that points at garbage survives each of these calls."""
import ctypes

import pytest

from conftest import import_pkg

TOPK, DEEP = 256, 10000

# name -> (k bound, argument list from (h, queries, nq, k, scores, rows)); P stands for any valid
# pointer the checks never reach (sparse queries, values), N for null (mask, stream), 1 for n_rows /
# n_pos, 0 for slot / with_values / mode.  The scores calls take one query and no k: bound None,
# (h, query, out) only.
P, N = "P", None
ENTRIES = {
    "rc_index_search": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, s, r, N)),
    "rc_index_search_ex": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, s, r, 0, N)),
    "rc_index_search_masked": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, N, s, r, 0, N)),
    "rc_index_search_pages": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, N, s, r, N)),
    "rc_index_search_pages_ex": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, N, s, r, 0, N)),
    "rc_index_search_deep": (DEEP, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, N, s, r, N)),
    "rc_index_search_pages_deep": (DEEP, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, N, s, r, N)),
    "rc_index_search_hybrid": (DEEP, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, N, P, P, P, s, r, N)),
    "rc_index_search_pages_hybrid": (DEEP, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, N, P, P, P, s, r, N)),
    "rc_index_scores": (None, lambda h, q, s: (h, q, 1, s, N)),
    "rc_index_scores_pages": (None, lambda h, q, s: (h, q, 0, 1, s, N)),
    "rc_index_scores_hybrid": (None, lambda h, q, s: (h, q, -1, 1, P, P, P, s, N)),
    "rc_sharded_search": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, s, r, 0, N)),
    "rc_sharded_search_masked": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, N, s, r, 0, N)),
    "rc_sharded_search_pages": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, N, s, r, N)),
    "rc_sharded_search_pages_ex": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, N, s, r, 0, N)),
    "rc_sharded_search_deep": (DEEP, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, N, s, r, N)),
    "rc_sharded_search_pages_deep": (DEEP, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, N, s, r, N)),
    "rc_sharded_search_hybrid": (DEEP, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, N, P, P, P, s, r, N)),
    "rc_sharded_search_pages_hybrid": (DEEP, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, N, P, P, P, s, r, N)),
    "rc_sharded_query_host": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, 0, s, r, N)),
    "rc_sharded_query_host_masked": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 1, k, 0, N, s, r, N)),
    "rc_sharded_query_host_pages": (TOPK, lambda h, q, nq, k, s, r: (h, q, nq, 0, 1, k, 0, N, s, r, N)),
}


@pytest.fixture(scope="module")
def env():
    L = import_pkg("_lib")
    lib = L.load()
    buf = (ctypes.c_char * 256)()
    fake = (ctypes.c_char * 64)()  # a non-null handle that is no index: 64 zero bytes
    return L, lib, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(fake, ctypes.c_void_p), (buf, fake)


def call(env, name, build, *a):
    """The status and the message of one call; "P" in the argument list becomes the valid pointer."""
    _, lib, p, _, _ = env
    st = getattr(lib, name)(*[p if x is P else x for x in build(*a)])
    return st, lib.rc_last_error()


def test_the_table_is_the_search_family_of_the_abi():
    sig = import_pkg("_lib").SIGNATURES
    family = {n for n in sig if n.startswith(("rc_index_search", "rc_index_scores", "rc_sharded_search", "rc_sharded_query_host"))}
    assert family == set(ENTRIES)
    for name, (_, build) in ENTRIES.items():
        n_args = len(build(*([0] * (3 if ENTRIES[name][0] is None else 6))))
        assert n_args == len(sig[name][1]), name


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_handle(env, name):
    L, _, p, _, _ = env
    bound, build = ENTRIES[name]
    st, msg = call(env, name, build, None, p, p) if bound is None else call(env, name, build, None, p, 1, 5, p, p)
    assert st == L.RC_ERR_INVALID and b"null index" in msg


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_bad_arguments_are_refused_before_the_handle_is_read(env, name):
    L, _, p, fake, _ = env
    bound, build = ENTRIES[name]
    INV = L.RC_ERR_INVALID
    if bound is None:  # one query, no k: the two buffers
        for q, s in ((None, p), (p, None)):
            st, msg = call(env, name, build, fake, q, s)
            assert st == INV and b"null" in msg, (q, s)
        return
    for k in (0, bound + 1):
        st, msg = call(env, name, build, fake, p, 1, k, p, p)
        assert st == INV and b"top_k" in msg, k
    st, msg = call(env, name, build, fake, p, -1, 5, p, p)
    assert st == INV and b"query count" in msg
    for q, s, r in ((None, p, p), (p, None, p), (p, p, None)):
        st, msg = call(env, name, build, fake, q, 1, 5, s, r)
        assert st == INV and b"null" in msg, (q, s, r)
