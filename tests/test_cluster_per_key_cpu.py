"""CPU checks of the per-key search over a cluster (orr_cluster_keys_*, orr_cluster_scope_create_keys,
orr_cluster_search_batch_per_key): the rules a cluster adds (csrc/orr_cluster_per_key_plan.h) through their selftest, built here
from the sources and as build() leaves it; the driver made of those rules and of the single index's pieces; the eight symbols
declared, exported, bound and documented; and every argument error on NULL handles in the stated order with the outputs
untouched -- so on a machine without a GPU (the method of tests/test_cluster_diverse_cpu.py).  The calls at work are in
tests/test_gpu_cluster_per_key.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_cluster_per_key_plan_selftest")
NAMES = ("orr_cluster_keys_create", "orr_cluster_keys_set", "orr_cluster_keys_get", "orr_cluster_keys_rows", "orr_cluster_keys_shard",
         "orr_cluster_keys_destroy", "orr_cluster_scope_create_keys", "orr_cluster_search_batch_per_key")
N_ARGS = (5, 5, 4, 1, 2, 1, 5, 19)
I64_MIN = -(1 << 63)


def _passes(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_cluster_per_key_plan_selftest: ok"
    m = re.search(r"random placements: 2000, (\d+) rounds, (\d+) with more than one round, (\d+) shares that end inside a shard", r.stdout)
    assert m and int(m.group(1)) > 2_000 and int(m.group(2)) > 300 and int(m.group(3)) > 500, r.stdout
    assert int(re.search(r"checks: (\d+)", r.stdout).group(1)) > 10_000


def test_cluster_per_key_plan_selftest_passes(tmp_path):
    exe = tmp_path / "selftest"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(CSRC, "host", "orr_cluster_per_key_plan_selftest.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    _passes(str(exe))
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_cluster_per_key_plan_selftest)"
    _passes(SELFTEST)


def test_the_selftest_covers_what_the_plan_promises():
    src = open(os.path.join(CSRC, "host", "orr_cluster_per_key_plan_selftest.cpp")).read()
    header = open(os.path.join(CSRC, "orr_cluster_per_key_plan.h")).read()
    for name in ("gather_plan", "seen_of_shard", "prefix_rows", "scope_share", "holds"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert re.search(r"\b%s\(" % name, src), name
    # the single index's rules and the other plans' are used, not restated
    for used in ("cdiverse::locate(", '#include "orr_per_key_plan.h"', '#include "orr_cluster_scope_plan.h"'):
        assert used in header, used
    for restated in ("inline bool locate(", "walk_round(State", "build_table(const", "inline Split split_limit("):
        assert restated not in header, restated
    for piece in ("{5, 0, 3, 0, 0, 7, 0}", "!bad.ok && bad.bad_query == 1 && bad.bad_key == 99",                # an empty shard in the middle, a key outside
                  "s1.push_back(base[g] - 1); s1.push_back(base[g]);", "never a position the shard does not hold",       # both sides of every border
                  "share(3, 0) == 4", "share(4, 0) == 6 && share(4, 2) == 0", "share(5, 2) == 2", "share(1000, 2) == 5",   # inside, at the border, beyond, deleted rows in front
                  "Part::Clipped", "Part::Whole", "Part::Empty", "brute_prefix(",
                  "per_key::walk_all(", "per_key::walk_round(", "per_key::build_table(", "CHECK(kept == want)", "trial < 2000"):
        assert piece in src, piece


def test_the_driver_is_made_of_the_plan_and_the_single_indexs_pieces():
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    run = api.split("int cluster_per_key_run(")[1].split("\nint orr_cluster_keys_create(")[0]
    for piece in ("cper_key::gather_plan(", "cper_key::seen_of_shard(", "cper_key::scope_share(", "cper_key::holds(", "cscope::split_limit(",
                  "per_key::walk_round(", "per_key::build_table(", "per_key::take_of(", "std::vector<per_key::State>",
                  "per_key_gather(", "per_key_freeze(", "per_key_slice_scopes(", "cluster_plain_search(c, pa", "cluster_scope_on_lanes(c, fn, pa, cs, lanes",
                  "cluster_grouped_on_lanes(", "cluster_extents(lanes"):
        assert piece in run, piece
    assert run.count("cluster_scope_lanes(c, lanes)") == 2 and "acquire_lane(" not in run            # ONE set of lanes, on either path
    assert "orr::launch_" not in run                                                                 # every launch is the single index's stage
    assert run.index("cluster_scope_lanes(c, lanes);\n            ORR_TRY(hold_parts())") < run.index("cluster_scope_on_lanes(c, fn, pa")     # the holds behind the lanes
    # the rows below a limit: one rule, the plan's, for the plain search and for the frozen set
    assert "cper_key::prefix_rows(candidate_limit, idx->row_base, idx->dead_before" in api.split("int64_t participating_rows(")[1].split("\n}\n")[0]
    # the grouped cluster search on lanes the caller holds; the entry point is its caller
    entry = api.split("\nint cluster_grouped_search(")[1].split("\n}\n")[0]
    assert "cluster_scope_begin(" in entry and "cluster_scope_lanes(c, lanes)" in entry and "return cluster_grouped_on_lanes(" in entry and "for_each_shard" not in entry
    # the one per-shard device half serves both drivers, with the launches it had
    half = api.split("\nint per_key_slice_scopes(")[2].split("\n// orr_search_batch_per_key on the lane")[0]       # ([1]: its declaration)
    for launch in ("launch_keys_exclude(", "launch_keys_clear_seen(", "launch_scope_counts(", "launch_mask_clip_slots("):
        assert half.count("orr::" + launch) == 1, launch
    for launch in ("launch_keys_exclude(", "launch_keys_clear_seen(", "launch_mask_clip_slots("):       # ... and nowhere else
        assert api.count("orr::" + launch) == 1, launch
    assert half.count("hipStreamSynchronize(") == 1
    assert "per_key_slice_scopes(lane, keys, S, tk, tm, seen_pos, seen_slot, w, tmp)" in api.split("\nint per_key_round(")[1].split("\nint per_key_slice_scopes(")[0]
    # no kernel was added for the feature: the keys_* kernels are the six the single index has
    assert sorted(set(re.findall(r"void (keys_\w+)_kernel\(", kernels))) == ["keys_clear_seen", "keys_count", "keys_exclude", "keys_fill_none", "keys_gather",
                                                                             "keys_member", "keys_remap", "keys_scatter"]
    search = api.split("\nint orr_cluster_search_batch_per_key(")[1].split("\n}\n")[0]
    order = [search.index(p) for p in ("per_key::first_invalid(", "if (!c)", "if (B == 0)", "shared_lock<std::shared_mutex> lock(c->mu)", "!c->sealed",
                                       "the keys belong to another cluster", "the scope belongs to another cluster", "cluster_keys_owner(keys, fn",
                                       "cluster_scope_owner(within, fn", "is_device_pointer(q_host)", "check_batch(", "cluster_per_key_run(")]
    assert order == sorted(order), order
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_cluster_per_key_plan_selftest" in makefile.split("all:")[0]                      # in SELFTEST: build() makes it
    assert "orr_cluster_per_key_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]
    assert "-Wall" in makefile.split("host/orr_cluster_per_key_plan_selftest:")[1].split("\n")[1]


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entry_points_are_declared_exported_bound_and_documented():
    P = pkg()
    decl = _declared("omnirecall_hip.h")
    for name, n_args in zip(NAMES, N_ARGS):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, decl)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, m.group(1)
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        f = getattr(P.native.hip, name)
        assert len(f.argtypes) == n_args, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    h = P.native.hip
    assert h.orr_cluster_keys_rows.restype is C.c_int64 and h.orr_cluster_keys_destroy.restype is None and h.orr_cluster_keys_shard.restype is C.c_void_p
    assert h.orr_cluster_search_batch_per_key.restype is C.c_int
    assert h.orr_cluster_search_batch_per_key.argtypes == h.orr_search_batch_per_key.argtypes
    assert h.orr_cluster_keys_set.argtypes == h.orr_keys_set.argtypes and h.orr_cluster_keys_get.argtypes == h.orr_keys_get.argtypes
    assert h.orr_cluster_scope_create_keys.argtypes == h.orr_scope_create_keys.argtypes
    assert re.search(r"typedef struct orr_cluster_keys orr_cluster_keys;", decl)
    assert h.orr_abi_version() == 1                                       # adding functions is compatible
    for name in ("keys", "scope_keys", "search_per_key"):
        assert callable(getattr(P.RecallCluster, name)), name
    for name in ("set", "get", "shard", "close"):
        assert callable(getattr(P.RecallClusterKeys, name)), name
    assert isinstance(P.RecallClusterKeys.rows, property) and P.RecallClusterKeys.KEY_NONE == I64_MIN
    import inspect
    assert list(inspect.signature(P.RecallCluster.search_per_key).parameters) == list(inspect.signature(P.RecallIndex.search_per_key).parameters)
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    block = full.split("row keys and the per-key search over the shards")[1]
    for said in ("COUNTS TWICE", "LOWEST shard", "borrowed", "both destroy orders are legal", "a key closes\n *   cluster-wide",
                 "sharded.py", "record (shard) form", "service mirror", "micro-batcher", "keys in the shard file", "pools above\n * 56", "diverse search",
                 "de-duplicating the union table per shard"):
        assert said in block, said
    assert "built since: orr_cluster_keys and orr_cluster_search_batch_per_key" in full and "Not offered: the cluster per-key search" not in full
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design.split("### 8u.")[1].split("\n## ")[0]
    for part in ("**Why.**", "**Contract.**", "**The plan.**", "**Holds and lanes.**", "**Tests.**", "**Out of scope.**", "**Measurements.**"):
        assert part in section, part
    for said in ("orr_cluster_per_key_plan.h", "gather_plan", "seen_of_shard", "prefix_rows", "scope_share", "cluster_grouped_on_lanes",
                 "sharded.py", "record (shard) form", "micro-batcher", "keys in the shard file", "pools above 56", "de-duplicating"):
        assert said in section, said
    assert "built since: §8u" in design.split("### 8s.")[1].split("### 8t.")[0] and "built since: §8u" in design.split("### 8t.")[1].split("### 8u.")[0]


def test_argument_errors_in_their_order_before_the_handle_with_the_outputs_untouched():
    """every case passes NULL handles, each holding exactly one error more than the one behind it"""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    B, k = 3, 10
    q = np.ones((B, 4), np.float32)
    qoff = np.zeros(B + 1, np.uint32)
    rows = np.full((B, k), 7, np.int64)
    scores = np.full((B, k), 7.0)
    keys = np.full((B, k), 7, np.int64)
    counts = np.full(B, 7, np.int32)
    rounds = np.full(B, 7, np.int32)
    qp, op, rp, sp, kp, cp, np_ = (a.ctypes.data for a in (q, qoff, rows, scores, keys, counts, rounds))
    fake = C.c_void_p(8)                                                  # a keys handle that is not NULL and is never looked at

    def call(topk, pool, cap, handle, r=rp, s=sp, kk=kp, c=cp, batch=B):
        ret = h.orr_cluster_search_batch_per_key(None, batch, 4, qp, None, None, op, 0, topk, 300, None, handle, cap, pool, r, s, kk, c, np_)
        assert b"orr_cluster_search_batch_per_key:" in err()
        return ret

    for r, s, kk, c in ((None, sp, kp, cp), (rp, None, kp, cp), (rp, sp, None, cp), (rp, sp, kp, None)):
        assert call(99, 0, 0, None, r, s, kk, c) == E and b"are required" in err()
    for pool in (0, -1, 57, 1 << 30):
        assert call(99, pool, 0, None) == E and b"pool must be in 1 .. 56" in err()
    for topk, pool in ((57, 56), (11, 10), (2, 1)):
        assert call(topk, pool, 0, None) == E and b"exceeds the pool" in err()
    for cap in (0, -1, -(1 << 31)):
        assert call(10, 10, cap, None) == E and b"max_per_key must be at least 1" in err()
    for topk, pool, cap in ((10, 10, 1), (0, 1, 1), (-3, 1, 5), (56, 56, (1 << 31) - 1)):
        assert call(topk, pool, cap, None) == E and b"null keys" in err()
        assert call(topk, pool, cap, fake) == E and b"null cluster" in err()
        assert call(topk, pool, cap, fake, batch=0) == E and b"null cluster" in err()
    assert (rows == 7).all() and (scores == 7.0).all() and (keys == 7).all() and (counts == 7).all() and (rounds == 7).all()

    # orr_cluster_scope_create_keys: first_invalid_scope_keys' order, then the cluster
    out = C.c_void_p(77)
    some = np.arange(4, dtype=np.int64)

    def scope(o, n_keys, ks, handle):
        ret = h.orr_cluster_scope_create_keys(None, handle, n_keys, ks, o)
        assert b"orr_cluster_scope_create_keys:" in err()
        return ret

    assert scope(None, -1, None, None) == E and b"out is NULL" in err()
    for n_keys in (-1, 65_537):
        assert scope(C.byref(out), n_keys, None, None) == E and b"n_keys must be in 0 .. 65536" in err()
    assert scope(C.byref(out), 4, None, None) == E and b"keys is NULL with 4 keys" in err()
    assert scope(C.byref(out), 4, some.ctypes.data, None) == E and b"null keys handle" in err()
    assert scope(C.byref(out), 0, None, None) == E and b"null keys handle" in err()
    assert scope(C.byref(out), 4, some.ctypes.data, fake) == E and b"null cluster" in err()
    assert out.value == 77

    # the keys calls: n, the arrays, then the handle
    got = np.full(4, 7, np.int64)
    done = C.c_int64(7)
    dp = C.cast(C.byref(done), C.c_void_p)
    assert h.orr_cluster_keys_create(None, 4, some.ctypes.data, some.ctypes.data, None) == E and b"orr_cluster_keys_create: out is NULL" in err()
    assert h.orr_cluster_keys_create(None, -1, None, None, C.byref(out)) == E and b"n is negative" in err()
    assert h.orr_cluster_keys_create(None, 4, None, some.ctypes.data, C.byref(out)) == E and b"row_ids or keys is NULL" in err()
    assert h.orr_cluster_keys_create(None, 4, some.ctypes.data, None, C.byref(out)) == E and b"row_ids or keys is NULL" in err()
    assert h.orr_cluster_keys_create(None, 4, some.ctypes.data, some.ctypes.data, C.byref(out)) == E and b"null cluster" in err()
    assert h.orr_cluster_keys_set(None, -1, None, None, dp) == E and b"orr_cluster_keys_set: n is negative" in err()
    assert h.orr_cluster_keys_set(None, 4, some.ctypes.data, None, dp) == E and b"row_ids or keys is NULL" in err()
    assert h.orr_cluster_keys_set(None, 4, some.ctypes.data, some.ctypes.data, dp) == E and b"null keys" in err()
    assert h.orr_cluster_keys_get(None, -1, None, None) == E and b"orr_cluster_keys_get: n is negative" in err()
    assert h.orr_cluster_keys_get(None, 4, some.ctypes.data, None) == E and b"row_ids or out_keys is NULL" in err()
    assert h.orr_cluster_keys_get(None, 4, some.ctypes.data, got.ctypes.data) == E and b"null keys" in err()
    assert h.orr_cluster_keys_rows(None) == -1 and h.orr_cluster_keys_shard(None, 0) is None
    h.orr_cluster_keys_destroy(None)                                      # NULL is allowed
    assert out.value == 77 and done.value == 7 and (got == 7).all()
