"""CPU checks of the cluster forms of the scoped and the masked search (orr_cluster_search_batch_scoped,
orr_cluster_search_batch_masked) and of the shard call the masked one drives (orr_search_shard_masked): declared, exported,
bound, documented, and the argument checks that come before any HIP call answer on a machine without a GPU (the method of
tests/test_scoped_search_cpu.py)."""
import ctypes as C
import os
import re

import numpy as np

from helpers import ROOT, pkg

SYMBOLS = {"orr_search_shard_masked": 16, "orr_cluster_search_batch_scoped": 16, "orr_cluster_search_batch_masked": 15}


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return txt


def test_entry_points_are_declared_exported_bound_and_documented():
    P = pkg()
    decl = _declared("omnirecall_hip.h")
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, decl)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        f = getattr(P.native.hip, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    assert callable(P.RecallIndex.search_shard_masked)
    assert callable(P.RecallCluster.search_scoped) and callable(P.RecallCluster.search_masked)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8j" in design and "is not built" not in design.split("8j")[0].split("8h")[-1]


class _Args:
    def __init__(self, B=2, dim=8, k=4):
        self.q = np.zeros((B, dim), np.float32)
        self.pool = np.frombuffer(b"ab\0", np.uint8).copy()
        self.toff = np.array([0, 2], np.uint32)
        self.qoff = np.array([0, 1, 1], np.uint32)
        self.ids = np.arange(5, dtype=np.int64)
        self.off = np.array([0, 2, 5], np.uint64)
        self.rows = np.full((B, k), 7, np.int64)
        self.scores = np.full((B, k), 7.0)
        self.counts = np.full(B, 7, np.int32)
        self.recs = np.full((B, k + 1, 56), 7, np.uint8)
        self.B, self.dim, self.k = B, dim, k

    def untouched(self):
        return (self.rows == 7).all() and (self.scores == 7.0).all() and (self.counts == 7).all() and (self.recs == 7).all()


def _cluster_calls(P, a):
    h = P.native.hip
    front = lambda: (a.B, a.dim, a.q.ctypes.data, a.pool.ctypes.data, a.toff.ctypes.data, a.qoff.ctypes.data, 0, a.k, 300)
    back = lambda: (a.rows.ctypes.data, a.scores.ctypes.data, a.counts.ctypes.data)
    return {
        "orr_cluster_search_batch_scoped": lambda c, n, ids, off: h.orr_cluster_search_batch_scoped(c, *front(), n, ids, off, *back()),
        "orr_cluster_search_batch_masked": lambda c, n, ids, off: h.orr_cluster_search_batch_masked(c, *front(), n, ids, *back()),
    }


def _shard_call(P, a, idx, n, ids, kprime=4, topk=0, shard_pass=0, before=0, out=True):
    return P.native.hip.orr_search_shard_masked(idx, a.B, a.dim, a.q.ctypes.data, a.pool.ctypes.data, a.toff.ctypes.data, a.qoff.ctypes.data,
                                                0, kprime, 300, topk, shard_pass, n, ids, before, a.recs.ctypes.data if out else None)


def test_argument_errors_before_any_device_call():
    """Without a GPU no cluster and no index can be made, so every case passes a null handle: the other errors are reported all
    the same because the library checks them BEFORE the handle -- this test pins that order on purpose.  The same errors on
    real sealed handles are in tests/test_gpu_cluster_scope.py."""
    P = pkg()
    E = P.native.ORR_EINVAL
    err = P.native.hip.orr_last_error
    a = _Args()
    ids, off = a.ids.ctypes.data, a.off.ctypes.data
    decreasing = np.array([0, 4, 3], np.uint64)
    short_end = np.array([0, 2, 4], np.uint64)
    for name, call in _cluster_calls(P, a).items():
        assert call(None, 5, ids, off) == E and b"null cluster" in err() and name.encode() in err(), name
        assert call(None, 5, ids, None) == E and b"null cluster" in err(), name
        assert call(None, 0, None, None) == E and b"null cluster" in err(), name
        assert call(None, -1, ids, None) == E and b"negative" in err() and name.encode() in err(), name
        assert call(None, 5, None, None) == E and b"scope_ids is NULL" in err(), name
        if name.endswith("scoped"):
            assert call(None, 5, ids, decreasing.ctypes.data) == E and b"scope_off" in err(), name
            assert call(None, 5, ids, short_end.ctypes.data) == E and b"scope_off" in err(), name
        assert a.untouched(), name
    fn = b"orr_search_shard_masked"
    assert _shard_call(P, a, None, 5, ids) == E and b"null index" in err() and fn in err()
    assert _shard_call(P, a, None, -1, ids) == E and b"negative" in err() and fn in err()
    assert _shard_call(P, a, None, 5, None) == E and b"scope_ids is NULL" in err()
    assert _shard_call(P, a, None, 5, ids, kprime=0) == E and b"kprime" in err() and fn in err()
    assert _shard_call(P, a, None, 5, ids, topk=-1) == E and b"topk" in err()
    assert _shard_call(P, a, None, 5, ids, shard_pass=2) == E and b"pass" in err() and fn in err()
    assert _shard_call(P, a, None, 5, ids, shard_pass=-1) == E and b"pass" in err()
    assert _shard_call(P, a, None, 5, ids, before=-1) == E and b"scope_before" in err() and fn in err()
    assert _shard_call(P, a, None, 5, ids, out=False) == E and b"out is NULL" in err()
    assert a.untouched()
