"""CPU checks of the scoped search entry points (orr_search_batch_scoped, orr_search_shard_scoped, orr_index_scope_count and
the service mirror's orrh_service_search_documents_json): declared, exported, bound, and the argument checks that come before
any HIP call answer on a machine without a GPU."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np

from helpers import ROOT, pkg

HIP = ("orr_search_batch_scoped", "orr_search_shard_scoped", "orr_index_scope_count")
HOST = "orrh_service_search_documents_json"


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(orrh?_[a-z0-9_]+)\s*\(", txt))


def test_scoped_entry_points_are_declared_exported_and_bound():
    P = pkg()
    for name in HIP:
        assert name in _declared("omnirecall_hip.h")
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        assert getattr(P.native.hip, name).restype is C.c_int
    assert HOST in _declared("omnirecall_host.h")
    assert HOST in P.native.EXPORTED_HOST_SYMBOLS
    assert getattr(P.native.host, HOST).restype is C.c_int
    assert len(P.native.hip.orr_search_batch_scoped.argtypes) == 16
    assert len(P.native.hip.orr_search_shard_scoped.argtypes) == 16
    assert len(P.native.hip.orr_index_scope_count.argtypes) == 6
    assert len(getattr(P.native.host, HOST).argtypes) == 10
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    for method in ("search_scoped", "search_shard_scoped", "scope_count"):
        assert callable(getattr(P.RecallIndex, method))
    assert callable(getattr(import_module(P.__name__ + ".service").RecallSearchService, "SearchInDocuments"))


class _Args:
    def __init__(self, B=2, dim=8, k=4):
        self.q = np.zeros((B, dim), np.float32)
        self.pool = np.frombuffer(b"ab\0", np.uint8).copy()
        self.toff = np.array([0, 2], np.uint32)
        self.qoff = np.array([0, 1, 1], np.uint32)
        self.ids = np.arange(5, dtype=np.int64)
        self.off = np.array([0, 2, 5], np.uint64)
        self.rows = np.full((B, k), 7, np.int64)
        self.scores = np.zeros((B, k))
        self.counts = np.zeros(B, np.int32)
        self.recs = np.zeros((B, k + 1, 56), np.uint8)
        self.live = np.zeros(B, np.int64)
        self.B, self.dim, self.k = B, dim, k


def _calls(P, a):
    """name -> callable(index, n_ids, ids, off) with every other argument valid"""
    h = P.native.hip
    return {
        "orr_search_batch_scoped": lambda idx, n, ids, off: h.orr_search_batch_scoped(
            idx, a.B, a.dim, a.q.ctypes.data, a.pool.ctypes.data, a.toff.ctypes.data, a.qoff.ctypes.data, 0, a.k, 300, n, ids, off,
            a.rows.ctypes.data, a.scores.ctypes.data, a.counts.ctypes.data),
        "orr_search_shard_scoped": lambda idx, n, ids, off: h.orr_search_shard_scoped(
            idx, a.B, a.dim, a.q.ctypes.data, a.pool.ctypes.data, a.toff.ctypes.data, a.qoff.ctypes.data, 0, a.k, 300, 0, n, ids, off,
            None, a.recs.ctypes.data),
        "orr_index_scope_count": lambda idx, n, ids, off: h.orr_index_scope_count(idx, a.B, n, ids, off, a.live.ctypes.data),
    }


def test_scoped_argument_errors_before_any_device_call():
    """Without a GPU no index can be made, so every case passes a null index: a scope error is reported all the same because
    the library checks the scope (count, ids, offsets) BEFORE the index -- this test pins that order on purpose.  The same
    errors on a real sealed handle are in tests/test_gpu_scoped_search.py."""
    P = pkg()
    E = P.native.ORR_EINVAL
    a = _Args()
    ids, off = a.ids.ctypes.data, a.off.ctypes.data
    decreasing = np.array([0, 4, 3], np.uint64)
    short_end = np.array([0, 2, 4], np.uint64)
    past_end = np.array([0, 2, 6], np.uint64)
    for name, call in _calls(P, a).items():
        cases = {
            "null index": (None, 5, ids, off),
            "null index, shared scope": (None, 5, ids, None),
            "n_scope_ids < 0": (None, -1, ids, None),
            "ids NULL with a count": (None, 5, None, off),
            "offsets decrease": (None, 5, ids, decreasing.ctypes.data),
            "offsets end before n_scope_ids": (None, 5, ids, short_end.ctypes.data),
            "offsets end behind n_scope_ids": (None, 5, ids, past_end.ctypes.data),
        }
        seen = set()
        for what, (idx, n, p_ids, p_off) in cases.items():
            assert call(idx, n, p_ids, p_off) == E, (name, what)
            msg = P.native.hip.orr_last_error()
            assert name.encode() in msg, (name, what, msg)
            seen.add(msg)
        assert len(seen) >= 4, seen                                        # the messages tell the errors apart
        assert call(None, 5, ids, off) == E and b"null index" in P.native.hip.orr_last_error()
        assert call(None, -1, ids, None) == E and b"negative" in P.native.hip.orr_last_error()
        assert call(None, 5, None, off) == E and b"scope_ids is NULL" in P.native.hip.orr_last_error()
        assert call(None, 5, ids, decreasing.ctypes.data) == E and b"scope_off" in P.native.hip.orr_last_error()
    assert (a.rows == 7).all()                                             # nothing was written


def test_search_documents_argument_errors_before_any_device_call():
    P = pkg()
    f, E = getattr(P.native.host, HOST), P.native.ORR_EINVAL
    out, ln = C.c_void_p(), C.c_int64()
    docs = (C.c_char_p * 1)(b"doc")
    assert f(None, b"alpha", None, 0, 5, 0, docs, 1, C.byref(out), C.byref(ln)) == E
    assert HOST.encode() in P.native.host.orrh_last_error()
    store = P.native.host.orrh_store_create()
    svc = P.native.host.orrh_service_create(store, 0, 300)
    try:
        assert f(svc, b"alpha", None, 0, 5, 0, None, 2, C.byref(out), C.byref(ln)) == E          # documents NULL with a count
        assert HOST.encode() in P.native.host.orrh_last_error()
        assert f(svc, b"alpha", None, 0, 5, 0, docs, -1, C.byref(out), C.byref(ln)) == E
        assert f(svc, b"  \t ", None, 0, 5, 0, docs, 1, C.byref(out), C.byref(ln)) == E           # a blank query
        assert b"Query is required." in P.native.host.orrh_last_error()
        assert f(svc, b"alpha", None, 0, 5, 0, docs, 1, None, C.byref(ln)) == E
    finally:
        P.native.host.orrh_service_destroy(svc)
        P.native.host.orrh_store_destroy(store)
