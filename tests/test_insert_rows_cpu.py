"""CPU checks of the in-place insert entry points (orr_index_insert_rows, orr_cluster_insert_rows, the service mirror's
"insert_older" option): declared, exported, bound, and the argument checks that come before any HIP call answer on a
machine without a GPU."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np

from helpers import ROOT, pkg


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(orrh?_[a-z0-9_]+)\s*\(", txt))


def test_insert_rows_is_declared_exported_and_bound():
    P = pkg()
    for name in ("orr_index_insert_rows", "orr_cluster_insert_rows"):
        assert name in _declared("omnirecall_hip.h")
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        assert hasattr(P.native.hip, name)
        assert getattr(P.native.hip, name).restype is C.c_int
    assert len(P.native.hip.orr_index_insert_rows.argtypes) == 9
    assert len(P.native.hip.orr_cluster_insert_rows.argtypes) == 10
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    assert callable(getattr(P.RecallIndex, "insert_rows"))
    assert callable(getattr(import_module(P.__name__ + ".index").RecallCluster, "insert_rows"))


def _rows(n=4, dim=8):
    return (np.zeros((n, dim), np.float32), np.arange(n, dtype=np.int64), np.frombuffer(b"abcd" * n, np.uint8).copy(),
            (4 * np.arange(n + 1)).astype(np.uint64), np.arange(n, dtype=np.int64))


def test_insert_rows_argument_errors_before_any_device_call():
    P = pkg()
    f, E = P.native.hip.orr_index_insert_rows, P.native.ORR_EINVAL
    emb, ticks, pool, off, ids = _rows()
    done = C.c_int64(7)
    out = C.cast(C.byref(done), C.c_void_p)
    assert f(None, 4, 8, emb.ctypes.data, ticks.ctypes.data, pool.ctypes.data, off.ctypes.data, ids.ctypes.data, out) == E
    assert done.value == 0                                                # zeroed on error
    msg = P.native.hip.orr_last_error()
    assert b"orr_index_insert_rows" in msg and b"null index" in msg
    done.value = 7
    assert f(None, -1, 8, emb.ctypes.data, ticks.ctypes.data, pool.ctypes.data, off.ctypes.data, ids.ctypes.data, out) == E
    assert done.value == 0
    assert f(None, 4, 8, emb.ctypes.data, ticks.ctypes.data, pool.ctypes.data, off.ctypes.data, None, None) == E        # row_ids are required
    assert f(None, 4, 8, emb.ctypes.data, None, pool.ctypes.data, off.ctypes.data, ids.ctypes.data, None) == E          # created_ticks
    assert f(None, 0, 0, None, None, None, None, None, None) == E         # a null index is an error even with nothing to do


def test_cluster_insert_rows_argument_errors_before_any_device_call():
    P = pkg()
    f, E = P.native.hip.orr_cluster_insert_rows, P.native.ORR_EINVAL
    emb, ticks, pool, off, ids = _rows()
    done = C.c_int64(7)
    assert f(None, 0, 4, 8, emb.ctypes.data, ticks.ctypes.data, pool.ctypes.data, off.ctypes.data, ids.ctypes.data,
             C.cast(C.byref(done), C.c_void_p)) == E
    assert done.value == 0
    assert b"orr_cluster_insert_rows" in P.native.hip.orr_last_error()


def test_python_insert_rows_wants_row_ids():
    P = pkg()
    idx = P.RecallIndex.__new__(P.RecallIndex)                            # no handle: the check comes before the call
    idx._h = None
    emb, ticks, pool, off, _ = _rows()
    try:
        idx.insert_rows(emb, ticks, pool, off)
    except ValueError as e:
        assert "row_ids" in str(e)
    else:
        raise AssertionError("insert_rows without row_ids must raise")


def test_service_insert_option_is_exported():
    P = pkg()
    for name in ("orrh_service_set_option", "orrh_service_inserted_rows"):
        assert name in _declared("omnirecall_host.h")
        assert name in P.native.EXPORTED_HOST_SYMBOLS
        assert hasattr(P.native.host, name)
    assert P.native.host.orrh_service_inserted_rows(None) == 0
    assert P.native.host.orrh_service_set_option(None, b"insert_older", 1) == P.native.ORR_EINVAL
    S = import_module(P.__name__ + ".service")
    assert callable(getattr(S.RecallSearchService, "SetOption"))
    assert callable(getattr(S.RecallSearchService, "InsertedRows"))
    # a service over an empty store builds no index until the first search: options are plain host state
    store = S.InMemoryIngestionStore()
    sut = S.RecallSearchService(store, S.StubQueryEmbeddingClient([1.0]), candidate_limit=300, now_ticks=1)
    try:
        assert sut.InsertedRows() == 0
        sut.SetOption("insert_older", 1)
        sut.SetOption("insert_older", 0)
        for name, value in (("insert_newer", 1), ("", 1), ("insert_older", 2), ("insert_older", -1)):
            try:
                sut.SetOption(name, value)
            except S.HostError as e:
                assert e.code == P.native.ORR_EINVAL, (name, value)
            else:
                raise AssertionError("SetOption(%r, %r) must be ORR_EINVAL" % (name, value))
        assert P.native.host.orrh_service_set_option(sut._h, None, 1) == P.native.ORR_EINVAL
    finally:
        sut.close()
        store.close()
