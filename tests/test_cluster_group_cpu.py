"""CPU checks of the grouped search over a cluster's shards (orr_cluster_search_batch_in_scopes and the shard form
orr_search_shard_in_scopes): the host rules of csrc/orr_cluster_group_plan.h through their selftest, the two entry points
declared, exported, bound and documented, and the argument checks that come before any device call and before a handle is looked
at, which answer on a machine without a GPU (the method of tests/test_cluster_scope_handle_cpu.py).  The calls at work are in
tests/test_gpu_cluster_grouped.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_cluster_group_plan_selftest")

# name -> (arguments, ctypes restype)
SYMBOLS = {"orr_cluster_search_batch_in_scopes": (16, C.c_int), "orr_search_shard_in_scopes": (17, C.c_int)}


def test_cluster_group_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_cluster_group_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_cluster_group_plan_selftest: ok"


def test_the_library_uses_the_rules_the_selftest_checks():
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    header = open(os.path.join(CSRC, "orr_cluster_group_plan.h")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_cluster_group_plan_selftest.cpp")).read()
    for name in ("distinct", "holds", "splits", "first", "route"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert f"cgroup::{name}(" in api, name
        assert f"cgroup::{name}(" in selftest, name
    # nothing the other plan headers define is restated: the split, the rungs and the handle's own rules are called
    assert "chandle::handle_split(" in header
    for theirs in ("split_limit", "shard_took", "first_rung", "next_rung", "merge_slice", "took_of", "sample_rows", "screen_pays"):
        assert not re.search(r"inline [\w:<>]+ %s\(" % theirs, header), theirs
    # one front for the index call and the shard form, one clip rule for both kernels
    assert len(re.findall(r"^int grouped_front\(", api, flags=re.M)) == 1
    assert api.count("grouped_front(idx,") == 2
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    assert len(re.findall(r"void mask_clip_rule\(", kernels)) == 1 and kernels.count("mask_clip_rule(") == 3
    rule = kernels[kernels.index("void mask_clip_rule("):kernels.index("void mask_clip_kernel(")]
    assert rule.count("scope::clip_word(") == 1                            # the last word's only definition, used in the one rule
    gather = kernels[kernels.index("void group_gather_clip_kernel("):kernels.index("hipError_t launch_group_gather_clip(")]
    assert "clip_word" not in gather and "atomic" not in gather
    assert "launch_group_gather_clip(" in open(os.path.join(CSRC, "orr_kernels.h")).read()


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
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    assert callable(P.RecallCluster.search_in_scopes) and callable(P.RecallIndex.search_shard_in_scopes)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8n" in design
    # the "not built" remarks about a cluster form of the grouped call point to 8n
    for line in design.splitlines():
        if "cluster form of `orr_search_batch_in_scopes`" in line:
            assert "8n" in line, line


class _Args:
    def __init__(self, B=2, dim=8, k=4):
        self.q = np.zeros((B, dim), np.float32)
        self.pool = np.frombuffer(b"ab\0", np.uint8).copy()
        self.toff = np.array([0, 2], np.uint32)
        self.qoff = np.array([0, 1, 1], np.uint32)
        self.rows = np.full((B, k), 7, np.int64)
        self.scores = np.full((B, k), 7.0)
        self.counts = np.full(B, 7, np.int32)
        self.recs = np.full((B, k + 1, 56), 7, np.uint8)
        self.B, self.dim, self.k = B, dim, k

    def front(self, B=None, dim=None, q=True, qoff=True):
        return (self.B if B is None else B, self.dim if dim is None else dim, self.q.ctypes.data if q else None, self.pool.ctypes.data,
                self.toff.ctypes.data, self.qoff.ctypes.data if qoff else None, 0, self.k, 300)

    def back(self, rows=True, scores=True):
        return (self.rows.ctypes.data if rows else None, self.scores.ctypes.data if scores else None, self.counts.ctypes.data)

    def untouched(self):
        return (self.rows == 7).all() and (self.scores == 7.0).all() and (self.counts == 7).all() and (self.recs == 7).all()


def test_argument_errors_before_any_device_call_in_the_stated_order():
    """Without a GPU neither a cluster nor a scope can be made, so every case passes a null cluster or index and scopes that are
    never looked at: each case makes ONE argument wrong beside all the errors that come later in the stated order, and the
    message names the first.  The errors that need real handles (an unsealed cluster, a scope of another cluster or shard, an
    orphaned scope, device-resident vectors) are in tests/test_gpu_cluster_grouped.py."""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    a = _Args()
    fake = np.full(8, 7, np.int64)                                         # any non-null scope: it is not looked at before the handle
    two = (C.c_void_p * 2)(fake.ctypes.data, fake.ctypes.data)
    holed = (C.c_void_p * 2)(fake.ctypes.data, None)
    sc = lambda arr: C.cast(arr, C.c_void_p)
    qs = np.array([0, 1], np.int32)
    qs_bad = np.array([0, 2], np.int32)
    qs_neg = np.array([-1, 0], np.int32)

    # ---- the cluster call: n_scopes; scopes / an entry; query_scope / an entry; the batch's value errors; the cluster
    fn = b"orr_cluster_search_batch_in_scopes"
    call = lambda front, n, scopes, qscope, back: h.orr_cluster_search_batch_in_scopes(None, *front, n, scopes, qscope, *back)
    worst_front, worst_back = a.front(B=0, q=False, qoff=False), a.back(rows=False)
    for n in (0, -1, 65):
        assert call(worst_front, n, None, None, worst_back) == E and b"n_scopes must be in 1 .. 64" in err() and fn in err()
    assert call(worst_front, 2, None, None, worst_back) == E and b"scopes is NULL" in err() and fn in err()
    assert call(worst_front, 2, sc(holed), None, worst_back) == E and b"scopes[1] is a null scope" in err() and fn in err()
    assert call(a.front(dim=-1), 2, sc(two), None, worst_back) == E and b"query_scope is NULL" in err() and fn in err()
    for bad in (qs_bad, qs_neg):
        assert call(a.front(dim=-1), 2, sc(two), bad.ctypes.data, worst_back) == E and b"query_scope must name a scope in 0 .. 1" in err()
    assert call(a.front(B=0), 2, sc(two), qs.ctypes.data, a.back()) == E and b"batch size" in err() and fn in err()
    assert call(a.front(dim=-1), 2, sc(two), qs.ctypes.data, a.back()) == E and b"negative query dimension" in err() and fn in err()
    assert call(a.front(q=False), 2, sc(two), qs.ctypes.data, a.back()) == E and b"q is NULL" in err() and fn in err()
    assert call(a.front(qoff=False), 2, sc(two), qs.ctypes.data, a.back()) == E and b"query_term_off" in err() and fn in err()
    assert call(a.front(), 2, sc(two), qs.ctypes.data, a.back(rows=False)) == E and b"output buffers" in err() and fn in err()
    assert call(a.front(), 2, sc(two), qs.ctypes.data, a.back(scores=False)) == E and b"output buffers" in err()
    assert call(a.front(), 2, sc(two), qs.ctypes.data, a.back()) == E and b"null cluster" in err() and fn in err()
    assert call(a.front(), 64, sc((C.c_void_p * 64)(*([fake.ctypes.data] * 64))), qs.ctypes.data, a.back()) == E and b"null cluster" in err()
    assert a.untouched()

    # ---- the shard form: the same three, then scope_before, then the in-scope shard form's own, then the index
    fn = b"orr_search_shard_in_scopes"
    before = np.array([0, 5], np.int64)
    before_neg = np.array([0, -1], np.int64)

    def shard(n=2, scopes=sc(two), qscope=qs, scope_before=before, kprime=4, topk=0, shard_pass=0, out=True, B=None):
        return h.orr_search_shard_in_scopes(None, a.B if B is None else B, a.dim, a.q.ctypes.data, a.pool.ctypes.data, a.toff.ctypes.data,
                                            a.qoff.ctypes.data, 0, kprime, 300, topk, shard_pass, n, scopes,
                                            None if qscope is None else qscope.ctypes.data,
                                            None if scope_before is None else scope_before.ctypes.data, a.recs.ctypes.data if out else None)
    for n in (0, -1, 65):
        assert shard(n=n, scopes=None, qscope=None, scope_before=None, kprime=0, out=False) == E and b"n_scopes must be in 1 .. 64" in err() and fn in err()
    assert shard(scopes=None, qscope=None, scope_before=None, kprime=0) == E and b"scopes is NULL" in err() and fn in err()
    assert shard(scopes=sc(holed), qscope=None, scope_before=None, kprime=0) == E and b"scopes[1] is a null scope" in err() and fn in err()
    assert shard(qscope=None, scope_before=None, kprime=0) == E and b"query_scope is NULL" in err() and fn in err()
    for bad in (qs_bad, qs_neg):
        assert shard(qscope=bad, scope_before=None, kprime=0) == E and b"query_scope must name a scope in 0 .. 1" in err() and fn in err()
    assert shard(scope_before=None, kprime=0) == E and b"scope_before is NULL" in err() and fn in err()
    assert shard(scope_before=before_neg, kprime=0) == E and b"scope_before[1] is negative" in err() and fn in err()
    assert shard(kprime=0, topk=-1) == E and b"kprime" in err() and fn in err()
    assert shard(topk=-1, shard_pass=2) == E and b"topk" in err() and fn in err()
    for bad in (-1, 2):
        assert shard(shard_pass=bad, out=False) == E and b"pass takes" in err() and fn in err()
    assert shard(out=False, B=0) == E and b"out is NULL" in err() and fn in err()
    assert shard() == E and b"null index" in err() and fn in err()
    assert a.untouched()
