"""CPU checks of the scope handles (orr_scope): the rules of csrc/orr_scope_set_plan.h through their selftest, the nine entry
points declared, exported, bound and documented, and the argument checks that come before any HIP call, which answer on a
machine without a GPU (the method of tests/test_cluster_scope_cpu.py).  The handles at work are in
tests/test_gpu_scope_handle.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_scope_set_plan_selftest")

# name -> (arguments, ctypes restype)
SYMBOLS = {
    "orr_scope_create": (4, C.c_int), "orr_scope_create_ticks": (4, C.c_int), "orr_scope_add_ids": (4, C.c_int),
    "orr_scope_combine": (3, C.c_int), "orr_scope_rows": (1, C.c_int64), "orr_scope_row_ids": (4, C.c_int),
    "orr_scope_destroy": (1, None), "orr_search_batch_in_scope": (14, C.c_int), "orr_search_batch_in_scopes": (16, C.c_int),
}


def test_scope_set_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_scope_set_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_scope_set_plan_selftest: ok"


def test_the_kernels_and_the_selftest_share_their_inlines():
    header = open(os.path.join(CSRC, "orr_scope_set_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_scope_set_plan_selftest.cpp")).read()
    for name in ("range_word", "combine_word", "remap_source", "bit_at"):
        assert len(re.findall(r"inline \w+ %s\(" % name, header)) == 1, name
        assert f"scope_set::{name}(" in kernels, name
        assert f" {name}(" not in kernels.replace(f"scope_set::{name}(", ""), name      # no second definition beside the kernels
    for name in ("ticks_range", "range_word", "combine_word", "remap_word", "n_clip_all"):
        assert f"scope_set::{name}(" in selftest, name
    assert "remap_source(" in header.split("inline uint32_t remap_word(")[1]   # the host's word is the kernel's rule
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    assert "scope_set::ticks_range(" in api


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
    assert "typedef struct orr_scope orr_scope;" in decl
    for macro, value in (("ORR_SCOPE_AND", 0), ("ORR_SCOPE_OR", 1), ("ORR_SCOPE_ANDNOT", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), decl), macro
        assert getattr(P.native, macro) == value
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    for meth in ("scope", "scope_ticks", "search_in_scope", "search_in_scopes"):
        assert callable(getattr(P.RecallIndex, meth)), meth
    for meth in ("close", "row_ids", "add_ids", "and_", "or_", "andnot"):
        assert callable(getattr(P.RecallScope, meth)), meth
    assert isinstance(P.RecallScope.rows, property)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8k" in design
    # the three "not built" remarks about a persistent resolved-scope handle became references to 8k
    for line in design.splitlines():
        if "resolved-scope handle" in line or "resolved scope handle" in line:
            assert "8k" in line, line


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
        self.B, self.dim, self.k = B, dim, k

    def front(self):
        return (self.B, self.dim, self.q.ctypes.data, self.pool.ctypes.data, self.toff.ctypes.data, self.qoff.ctypes.data, 0, self.k, 300)

    def back(self):
        return (self.rows.ctypes.data, self.scores.ctypes.data, self.counts.ctypes.data)

    def untouched(self):
        return (self.rows == 7).all() and (self.scores == 7.0).all() and (self.counts == 7).all() and (self.out_ids == 7).all()


def test_argument_errors_before_any_device_call():
    """Without a GPU neither an index nor a scope can be made, so every case passes null handles: the value errors are reported
    all the same because the library checks them BEFORE the handles -- this test pins that order on purpose.  The errors that
    need real handles (a scope of another shard, a combine across two shards, an orphaned scope, a cap that is too small) are
    in tests/test_gpu_scope_handle.py."""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    a = _Args()
    ids = a.ids.ctypes.data
    out = C.c_void_p(7)
    n = C.c_int64(7)
    n_p = C.cast(C.byref(n), C.c_void_p)

    fn = b"orr_scope_create"
    assert h.orr_scope_create(None, 5, ids, None) == E and b"out is NULL" in err() and fn in err()
    assert h.orr_scope_create(None, -1, ids, C.byref(out)) == E and b"negative" in err() and fn in err()
    assert h.orr_scope_create(None, 5, None, C.byref(out)) == E and b"ids is NULL" in err() and fn in err()
    assert h.orr_scope_create(None, 5, ids, C.byref(out)) == E and b"null index" in err() and fn in err()
    assert h.orr_scope_create(None, 0, None, C.byref(out)) == E and b"null index" in err()
    fn = b"orr_scope_create_ticks"
    assert h.orr_scope_create_ticks(None, 0, 10, None) == E and b"out is NULL" in err() and fn in err()
    assert h.orr_scope_create_ticks(None, 0, 10, C.byref(out)) == E and b"null index" in err() and fn in err()
    assert out.value == 7                                                 # no handle was written

    fn = b"orr_scope_add_ids"
    assert h.orr_scope_add_ids(None, -1, ids, n_p) == E and b"negative" in err() and fn in err()
    assert h.orr_scope_add_ids(None, 5, None, n_p) == E and b"ids is NULL" in err() and fn in err()
    assert h.orr_scope_add_ids(None, 5, ids, n_p) == E and b"null scope" in err() and fn in err()
    fn = b"orr_scope_combine"
    for op in (-1, 3, 64):
        assert h.orr_scope_combine(None, op, None) == E and b"op must be" in err() and fn in err()
    for op in (0, 1, 2):
        assert h.orr_scope_combine(None, op, None) == E and b"null scope" in err() and fn in err()
    fn = b"orr_scope_row_ids"
    assert h.orr_scope_row_ids(None, -1, a.out_ids.ctypes.data, n_p) == E and b"cap is negative" in err() and fn in err()
    assert h.orr_scope_row_ids(None, 8, a.out_ids.ctypes.data, None) == E and b"out_n is NULL" in err() and fn in err()
    assert h.orr_scope_row_ids(None, 8, None, n_p) == E and b"out_ids is NULL" in err() and fn in err()
    assert h.orr_scope_row_ids(None, 8, a.out_ids.ctypes.data, n_p) == E and b"null scope" in err() and fn in err()
    assert n.value == 7
    assert h.orr_scope_rows(None) == -1
    h.orr_scope_destroy(None)                                             # allowed

    fn = b"orr_search_batch_in_scope"
    assert h.orr_search_batch_in_scope(None, *a.front(), None, *a.back()) == E and b"null scope" in err() and fn in err()

    fn = b"orr_search_batch_in_scopes"
    nulls = (C.c_void_p * 64)()
    scopes = C.cast(nulls, C.c_void_p)
    qs = np.zeros(a.B, np.int32)
    call = lambda n_scopes, sc, q: h.orr_search_batch_in_scopes(None, *a.front(), n_scopes, sc, q, *a.back())
    for bad in (0, -1, 65):
        assert call(bad, scopes, qs.ctypes.data) == E and b"n_scopes must be in 1 .. 64" in err() and fn in err()
    assert call(2, None, qs.ctypes.data) == E and b"scopes is NULL" in err() and fn in err()
    assert call(2, scopes, None) == E and b"query_scope is NULL" in err() and fn in err()
    for bad in (np.array([0, 2], np.int32), np.array([-1, 0], np.int32)):
        assert call(2, scopes, bad.ctypes.data) == E and b"query_scope must name a scope" in err() and fn in err()
    assert call(2, scopes, qs.ctypes.data) == E and b"null scope" in err() and fn in err()
    assert call(64, scopes, qs.ctypes.data) == E and b"null scope" in err()
    assert a.untouched()
