"""CPU checks of the cluster scope handles (orr_cluster_scope): the host rules of csrc/orr_cluster_handle_plan.h through their
selftest, the eleven entry points declared, exported, bound and documented, and the argument checks that come before any
device call and before a handle is looked at, which answer on a machine without a GPU (the method of
tests/test_scope_handle_cpu.py).  The handles at work are in tests/test_gpu_cluster_scope_handle.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_cluster_handle_plan_selftest")

# name -> (arguments, ctypes restype)
SYMBOLS = {
    "orr_cluster_scope_create": (4, C.c_int), "orr_cluster_scope_create_ticks": (4, C.c_int),
    "orr_cluster_scope_create_terms": (6, C.c_int), "orr_cluster_scope_add_ids": (4, C.c_int),
    "orr_cluster_scope_combine": (3, C.c_int), "orr_cluster_scope_rows": (1, C.c_int64),
    "orr_cluster_scope_row_ids": (4, C.c_int), "orr_cluster_scope_shard": (2, C.c_void_p),
    "orr_cluster_scope_destroy": (1, None), "orr_search_shard_in_scope": (15, C.c_int),
    "orr_cluster_search_batch_in_scope": (14, C.c_int),
}


def test_cluster_handle_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_cluster_handle_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_cluster_handle_plan_selftest: ok"


def test_the_library_uses_the_rules_the_selftest_checks():
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    header = open(os.path.join(CSRC, "orr_cluster_handle_plan.h")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_cluster_handle_plan_selftest.cpp")).read()
    for name in ("row_id_plan", "pair_valid", "holds", "handle_split"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert f"chandle::{name}(" in api, name
        assert f"chandle::{name}(" in selftest, name
    assert "cscope::split_limit(" in header                               # the split itself is not restated


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entry_points_are_declared_exported_bound_and_documented():
    P = pkg()
    decl = _declared("omnirecall_hip.h")
    for name, (n_args, restype) in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, decl)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        f = getattr(P.native.hip, name)
        assert f.restype is restype and len(f.argtypes) == n_args, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    assert "typedef struct orr_cluster_scope orr_cluster_scope;" in decl
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    for meth in ("scope", "scope_ticks", "scope_terms", "search_in_scope"):
        assert callable(getattr(P.RecallCluster, meth)), meth
    for meth in ("close", "row_ids", "add_ids", "and_", "or_", "andnot", "shard"):
        assert callable(getattr(P.RecallClusterScope, meth)), meth
    assert isinstance(P.RecallClusterScope.rows, property)
    assert callable(P.RecallIndex.search_shard_in_scope)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8m" in design
    # the "out of scope: the cluster forms" remarks of 8k and 8l point to 8m
    for line in design.splitlines():
        if line.startswith("**Out of scope**") and "the cluster forms" in line:
            assert "8m" in line, line


class _Args:
    def __init__(self, B=2, dim=8, k=4):
        self.q = np.zeros((B, dim), np.float32)
        self.pool = np.frombuffer(b"ab\0", np.uint8).copy()
        self.toff = np.array([0, 2], np.uint32)
        self.qoff = np.array([0, 1, 1], np.uint32)
        self.ids = np.arange(5, dtype=np.int64)
        self.rows = np.full((B, k), 7, np.int64)
        self.scores = np.full((B, k), 7.0)
        self.counts = np.full(B, 7, np.int32)
        self.out_ids = np.full(8, 7, np.int64)
        self.recs = np.full((B, k + 1, 56), 7, np.uint8)
        self.B, self.dim, self.k = B, dim, k

    def front(self, B=None, dim=None, q=True, qoff=True):
        return (self.B if B is None else B, self.dim if dim is None else dim, self.q.ctypes.data if q else None, self.pool.ctypes.data,
                self.toff.ctypes.data, self.qoff.ctypes.data if qoff else None, 0, self.k, 300)

    def back(self, rows=True, scores=True):
        return (self.rows.ctypes.data if rows else None, self.scores.ctypes.data if scores else None, self.counts.ctypes.data)

    def untouched(self):
        return ((self.rows == 7).all() and (self.scores == 7.0).all() and (self.counts == 7).all() and (self.out_ids == 7).all()
                and (self.recs == 7).all())


def test_argument_errors_before_any_device_call():
    """Without a GPU neither a cluster nor a scope can be made, so every case passes null handles: the value errors are
    reported all the same because the library checks them BEFORE the handles, and a NULL scope before a NULL cluster -- this
    test pins the order the header states.  The errors that need real handles (an unsealed cluster, a scope of another cluster
    or shard, an orphaned scope, a cap that is too small, ids in device memory) are in tests/test_gpu_cluster_scope_handle.py."""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    a = _Args()
    ids = a.ids.ctypes.data
    out = C.c_void_p(7)
    n = C.c_int64(7)
    n_p = C.cast(C.byref(n), C.c_void_p)

    fn = b"orr_cluster_scope_create"
    assert h.orr_cluster_scope_create(None, 5, ids, None) == E and b"out is NULL" in err() and fn in err()
    assert h.orr_cluster_scope_create(None, -1, ids, C.byref(out)) == E and b"negative" in err() and fn in err()
    assert h.orr_cluster_scope_create(None, 5, None, C.byref(out)) == E and b"ids is NULL" in err() and fn in err()
    assert h.orr_cluster_scope_create(None, 5, ids, C.byref(out)) == E and b"null cluster" in err() and fn in err()
    assert h.orr_cluster_scope_create(None, 0, None, C.byref(out)) == E and b"null cluster" in err()
    fn = b"orr_cluster_scope_create_ticks"
    assert h.orr_cluster_scope_create_ticks(None, 0, 10, None) == E and b"out is NULL" in err() and fn in err()
    assert h.orr_cluster_scope_create_ticks(None, 0, 10, C.byref(out)) == E and b"null cluster" in err() and fn in err()

    # create_terms: out NULL, n_terms, the arrays, mode, the terms themselves, then the cluster
    fn = b"orr_cluster_scope_create_terms"
    pool = np.frombuffer(b"abcd", np.uint8).copy()
    toff = np.array([0, 2, 4], np.uint32)
    empty = np.array([0, 2, 2], np.uint32)
    decreasing = np.array([0, 3, 2], np.uint32)
    terms = lambda n_terms, p, o, mode, outp: h.orr_cluster_scope_create_terms(None, n_terms, p, o, mode, outp)
    assert terms(-1, None, None, 9, None) == E and b"out is NULL" in err() and fn in err()
    for bad in (-1, 257):
        assert terms(bad, None, None, 9, C.byref(out)) == E and b"n_terms must be in 0 .. 256" in err() and fn in err()
    assert terms(2, None, toff.ctypes.data, 9, C.byref(out)) == E and b"is NULL with 2 terms" in err()
    assert terms(2, pool.ctypes.data, None, 9, C.byref(out)) == E and b"is NULL with 2 terms" in err()
    for bad in (-1, 2):
        assert terms(2, pool.ctypes.data, empty.ctypes.data, bad, C.byref(out)) == E and b"mode must be" in err() and fn in err()
    assert terms(2, pool.ctypes.data, empty.ctypes.data, 0, C.byref(out)) == E and b"term 1 is empty" in err()
    assert terms(2, pool.ctypes.data, decreasing.ctypes.data, 1, C.byref(out)) == E and b"not monotone" in err()
    assert terms(2, pool.ctypes.data, toff.ctypes.data, 0, C.byref(out)) == E and b"null cluster" in err() and fn in err()
    assert terms(0, None, None, 1, C.byref(out)) == E and b"null cluster" in err()
    assert out.value == 7                                                 # no handle was written

    fn = b"orr_cluster_scope_add_ids"
    assert h.orr_cluster_scope_add_ids(None, -1, ids, n_p) == E and b"negative" in err() and fn in err()
    assert h.orr_cluster_scope_add_ids(None, 5, None, n_p) == E and b"ids is NULL" in err() and fn in err()
    assert h.orr_cluster_scope_add_ids(None, 5, ids, n_p) == E and b"null scope" in err() and fn in err()
    fn = b"orr_cluster_scope_combine"
    for op in (-1, 3, 64):
        assert h.orr_cluster_scope_combine(None, op, None) == E and b"op must be" in err() and fn in err()
    for op in (0, 1, 2):
        assert h.orr_cluster_scope_combine(None, op, None) == E and b"null scope" in err() and fn in err()
    fn = b"orr_cluster_scope_row_ids"
    assert h.orr_cluster_scope_row_ids(None, -1, a.out_ids.ctypes.data, n_p) == E and b"cap is negative" in err() and fn in err()
    assert h.orr_cluster_scope_row_ids(None, 8, a.out_ids.ctypes.data, None) == E and b"out_n is NULL" in err() and fn in err()
    assert h.orr_cluster_scope_row_ids(None, 8, None, n_p) == E and b"out_ids is NULL" in err() and fn in err()
    assert h.orr_cluster_scope_row_ids(None, 8, a.out_ids.ctypes.data, n_p) == E and b"null scope" in err() and fn in err()
    assert n.value == 7
    assert h.orr_cluster_scope_rows(None) == -1
    assert h.orr_cluster_scope_shard(None, 0) is None and b"orr_cluster_scope_shard" in err()
    h.orr_cluster_scope_destroy(None)                                     # allowed

    # the cluster search: the batch's value errors, then the scope, then the cluster
    fn = b"orr_cluster_search_batch_in_scope"
    search = lambda front, back: h.orr_cluster_search_batch_in_scope(None, *front, None, *back)
    assert search(a.front(B=0), a.back()) == E and b"batch size" in err() and fn in err()
    assert search(a.front(dim=-1), a.back()) == E and b"negative query dimension" in err() and fn in err()
    assert search(a.front(q=False), a.back()) == E and b"q is NULL" in err() and fn in err()
    assert search(a.front(qoff=False), a.back()) == E and b"query_term_off" in err() and fn in err()
    assert search(a.front(), a.back(rows=False)) == E and b"output buffers" in err() and fn in err()
    assert search(a.front(), a.back(scores=False)) == E and b"output buffers" in err()
    assert search(a.front(), a.back()) == E and b"null scope" in err() and fn in err()
    fake = C.c_void_p(a.out_ids.ctypes.data)                              # any non-null scope: it is not looked at before the cluster
    assert h.orr_cluster_search_batch_in_scope(None, *a.front(), fake, *a.back()) == E and b"null cluster" in err() and fn in err()

    # the shard form: orr_search_shard_masked's value errors, then the scope, then the index
    fn = b"orr_search_shard_in_scope"

    def shard(idx=None, scope=None, kprime=4, topk=0, shard_pass=0, before=0, out=True):
        return h.orr_search_shard_in_scope(idx, a.B, a.dim, a.q.ctypes.data, a.pool.ctypes.data, a.toff.ctypes.data, a.qoff.ctypes.data,
                                           0, kprime, 300, topk, shard_pass, scope, before, a.recs.ctypes.data if out else None)
    assert shard(kprime=0) == E and b"kprime" in err() and fn in err()
    assert shard(topk=-1) == E and b"topk" in err() and fn in err()
    for bad in (-1, 2):
        assert shard(shard_pass=bad) == E and b"pass takes" in err() and fn in err()
    assert shard(before=-1) == E and b"scope_before" in err() and fn in err()
    assert shard(out=False) == E and b"out is NULL" in err() and fn in err()
    assert shard() == E and b"null scope" in err() and fn in err()
    assert shard(scope=fake) == E and b"null index" in err() and fn in err()
    assert a.untouched()
