"""CPU checks of the in-place reindex entry points (orr_index_update_rows, orrh_service_updated_rows): declared, exported,
and the argument checks that come before any HIP call answer on a machine without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from helpers import ROOT, pkg


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(orrh?_[a-z0-9_]+)\s*\(", txt))


def test_update_rows_is_declared_and_exported():
    P = pkg()
    assert "orr_index_update_rows" in _declared("omnirecall_hip.h")
    assert "orr_index_update_rows" in P.native.EXPORTED_HIP_SYMBOLS
    assert hasattr(P.native.hip, "orr_index_update_rows")
    assert P.native.hip.orr_index_update_rows.restype is C.c_int
    assert P.native.hip.orr_abi_version() == 1                            # adding a function is compatible


def test_update_rows_argument_errors_before_any_device_call():
    P = pkg()
    f, E = P.native.hip.orr_index_update_rows, P.native.ORR_EINVAL
    ids = np.arange(4, dtype=np.int64)
    emb = np.zeros((4, 8), dtype=np.float32)
    done = C.c_int64(7)
    assert f(None, 4, ids.ctypes.data, 8, emb.ctypes.data, C.cast(C.byref(done), C.c_void_p)) == E
    assert done.value == 0
    msg = P.native.hip.orr_last_error()
    assert b"orr_index_update_rows" in msg and b"bad argument" in msg
    assert f(None, -1, ids.ctypes.data, 8, emb.ctypes.data, None) == E
    assert f(None, 4, None, 8, emb.ctypes.data, None) == E
    assert f(None, 0, None, 0, None, None) == E                           # a null index is an error even with nothing to do


def test_service_updated_rows_is_exported():
    P = pkg()
    assert "orrh_service_updated_rows" in _declared("omnirecall_host.h")
    assert "orrh_service_updated_rows" in P.native.EXPORTED_HOST_SYMBOLS
    assert hasattr(P.native.host, "orrh_service_updated_rows")
    assert P.native.host.orrh_service_updated_rows(None) == 0
    from importlib import import_module
    S = import_module(P.__name__ + ".service")
    assert callable(getattr(S.RecallSearchService, "UpdatedRows"))
