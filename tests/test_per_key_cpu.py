"""CPU checks of row keys and the per-key search (orr_keys_*, orr_scope_create_keys, orr_search_batch_per_key): the rules of
csrc/orr_per_key_plan.h through their selftest (the argument order, the union table and its lookup, the word / ballot rule of
keys_exclude, the rounds against the one-walk definition), the lookup and the ballot rule compiled for the host against the
header once more, the kernels, the driver and the selftest made of the shared inlines, the seven symbols declared, exported,
bound and documented, and every argument error on NULL handles with the outputs untouched -- so on a machine without a GPU (the
method of tests/test_diverse_cpu.py).  The calls at work are in tests/test_gpu_per_key.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_per_key_plan_selftest")
NAMES = ("orr_keys_create", "orr_keys_set", "orr_keys_get", "orr_keys_rows", "orr_keys_destroy", "orr_scope_create_keys",
         "orr_search_batch_per_key")
N_ARGS = (5, 5, 4, 1, 1, 5, 19)
KERNELS = ("keys_exclude", "keys_clear_seen", "keys_member", "keys_gather", "keys_scatter", "keys_remap")
I64_MIN = -(1 << 63)


def test_per_key_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_per_key_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_per_key_plan_selftest: ok"
    m = re.search(r"round cases checked: (\d+) \(more than one round: (\d+), most rounds: (\d+), candidates ran out: (\d+)\)", r.stdout)
    assert m and int(m.group(1)) > 5000 and int(m.group(2)) > 500 and int(m.group(3)) >= 6 and int(m.group(4)) > 0, r.stdout
    m = re.search(r"table lookups checked: (\d+)", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout
    m = re.search(r"exclusion words checked: (\d+)", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout


def test_the_lookup_and_the_ballot_rule_compiled_for_the_host(tmp_path):
    """the header's table_find / table_mask / exclude_bits as the kernels call them: a table of 5,000 keys (beyond the LDS
    cut-over) holding the extreme key values, every key found at its place, every absent key missed, ORR_KEY_NONE passed over
    even when listed; and a wave's 64 bits formed slot by slot equal base AND NOT closed"""
    src = tmp_path / "lookup.cpp"
    src.write_text('#include "orr_per_key_plan.h"\n#include <cstdio>\n#include <vector>\n' + """
int main()
{
    using namespace per_key;
    long bad = 0, found = 0;
    std::vector<int64_t> keys;
    std::vector<uint64_t> masks;
    keys.push_back(kNone);                              // listed against the rule: still never closed
    keys.push_back(INT64_MIN + 1);
    for (int64_t k = -2499; k < 2498; ++k) keys.push_back(k * 3);
    keys.push_back(INT64_MAX);
    for (size_t i = 0; i < keys.size(); ++i) masks.push_back(0x8000000000000001ull ^ ((uint64_t)i << 7));
    const int32_t n = (int32_t)keys.size();
    bad += n != 5000 || table_in_lds(n) || !table_in_lds(kLdsTable);
    for (int32_t i = 0; i < n; ++i) {
        bad += table_find(keys.data(), n, keys[i]) != i;
        const uint64_t m = table_mask(keys.data(), masks.data(), n, keys[i]);
        bad += m != (keys[i] == kNone ? 0ull : masks[i]);
        found += m != 0ull;
    }
    for (int64_t k = -2499; k < 2497; ++k) {
        bad += table_find(keys.data(), n, k * 3 + 1) != -1;
        bad += table_mask(keys.data(), masks.data(), n, k * 3 + 2) != 0ull;
    }
    bad += table_find(keys.data(), 0, 7) != -1 || table_mask(nullptr, nullptr, 0, 7) != 0ull;
    bad += table_find(keys.data(), 1, kNone) != 0;     // (keys_member: a key like any other)
    // the ballot rule: lane l of a wave holds mask m[l]; slot s's word pair is base & ~ballot((m[l] >> s) & 1)
    uint64_t x = 88172645463325252ull;
    for (int rep = 0; rep < 2000; ++rep) {
        uint64_t m[64], base;
        for (int l = 0; l < 64; ++l) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; m[l] = (x % 5 == 0) ? x : 0ull; }
        x ^= x << 13; x ^= x >> 7; x ^= x << 17; base = x;
        for (int s = 0; s < kMaxSlots; ++s) {
            uint64_t ballot = 0, want = 0;
            for (int l = 0; l < 64; ++l) ballot |= (uint64_t)slot_closed(m[l], s) << l;
            for (int l = 0; l < 64; ++l) want |= (uint64_t)(((base >> l) & 1ull) && !((m[l] >> s) & 1ull)) << l;
            bad += exclude_bits(base, ballot) != want;
        }
    }
    printf("%ld %ld\\n", bad, found);
    return bad != 0;
}
""")
    exe = tmp_path / "lookup"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["0", "4999"], r.stdout + r.stderr


def test_the_kernels_the_driver_and_the_selftest_share_the_rules():
    header = open(os.path.join(CSRC, "orr_per_key_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_per_key_plan_selftest.cpp")).read()
    for name in ("first_invalid", "first_invalid_scope_keys", "table_find", "table_mask", "exclude_bits", "slot_closed", "build_table",
                 "member_table", "walk_round", "walk_all", "take_of", "table_in_lds"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert re.search(r"\b%s\(" % name, selftest), name
    assert "kMaxPool = kSelWidth - 8" in header and "kSelWidth = 64" in header and "kLdsTable = 2048" in header
    # keys_exclude: one lookup per key through the shared inline, a ballot per slot, whole vectors out, no atomics
    ex = kernels.split("void keys_exclude_kernel(")[1].split("hipError_t launch_keys_exclude(")[0]
    for piece in ("per_key::table_mask(tk, tm, n_tab, k)", "__ballot(per_key::slot_closed(m[it], s))", "per_key::exclude_bits(b, closed)",
                  "__syncthreads_or(any)", "reinterpret_cast<uint4 *>(out + (int64_t)s * words + w0)[j]", "r < n_rows ? key[r] : per_key::kNone"):
        assert piece in ex, piece
    assert "atomic" not in ex
    launcher = kernels.split("hipError_t launch_keys_exclude(")[1].split("\n}\n")[0]
    assert "per_key::table_in_lds(n_tab)" in launcher and "n_slots > per_key::kMaxSlots" in launcher and "n_rows > words * 32" in launcher
    member = kernels.split("void keys_member_kernel(")[1].split("hipError_t launch_keys_member(")[0]
    assert "per_key::table_find(tk, n_tab, key[r])" in member and "r < n_rows" in member and "atomic" not in member
    remap = kernels.split("void keys_remap_kernel(")[1].split("hipError_t launch_keys_remap(")[0]
    assert "scope_set::remap_source(d, first, n_new, src)" in remap and "per_key::kNone" in remap
    # the driver: every kernel timed under its name, exactly once; the existing searches reused, not copied
    for k in KERNELS:
        assert api.count('"%s"' % k) >= 1, k
    for k in ("keys_exclude", "keys_clear_seen", "keys_member", "keys_scatter", "keys_remap"):
        assert api.count('Timed t(lane, "%s"' % k) + api.count('Timed t(idx, "%s"' % k) == 1, k
        assert api.count("orr::launch_%s(" % k) == 1, k
    run = api.split("int per_key_run(")[1].split("\nint orr_search_batch_per_key(")[0]
    for piece in ("masked_batch(lane, pa, ScopeSource{nullptr, within}", "escalate(index_backend(lane, fn, n), pa, escalation::initial_kprime(pool, n, orr::kSelWidth)",
                  "per_key::walk_round(", "per_key_freeze(", "per_key_round(", "per_key::kMaxSlots", "- lane->row_base"):
        assert piece in run, piece
    rnd = api.split("int per_key_round(")[1].split("int per_key_run(")[0]
    for piece in ("per_key::build_table(", "grouped_batch(lane, cur, ga", "masked_batch(lane, cur, ScopeSource{nullptr, ptrs[0]}",
                  "orr::launch_scope_counts(", "orr::launch_mask_clip_slots("):
        assert piece in rnd, piece
    for name in ("plan_pass", "run_shard_once", "run_large_k", "run_masked_pass"):
        assert name not in run and name not in rnd, name
    entry = api.split("\nint orr_search_batch_per_key(")[1].split("\nint orr_search_shard_scoped(")[0]
    assert entry.index("per_key::first_invalid(") < entry.index("if (!idx)") < entry.index("check_batch(") < entry.index("acquire_lane(")
    # maintenance: the columns are allocated before the first row moves and remapped while the sources are there
    insert = api.split("\nint orr_index_insert_rows(")[1].split("\n}\n")[0]
    assert insert.index("key_cols.alloc(idx, total)") < insert.index("auto body = [&]() -> int {") < insert.index("key_cols.run(fr.src, first)")
    compact = api.split("\nint orr_index_compact(")[1].split("\n}\n")[0]
    assert compact.index("key_cols.alloc(idx, n_new)") < compact.index("key_cols.run(d_live.as<int64_t>(), 0)") < compact.index("key_cols.commit()")
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_per_key_plan_selftest" in makefile.split("all:")[0]                          # in SELFTEST: build() makes it
    assert "orr_per_key_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]
    assert "host/orr_per_key_plan_selftest: host/orr_per_key_plan_selftest.cpp orr_per_key_plan.h" in makefile


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
    assert h.orr_keys_rows.restype is C.c_int64 and h.orr_keys_destroy.restype is None and h.orr_search_batch_per_key.restype is C.c_int
    assert re.search(r"#define ORR_KEY_NONE INT64_MIN\b", decl) and P.native.ORR_KEY_NONE == I64_MIN
    assert h.orr_abi_version() == 1                                       # adding functions is compatible
    for name in ("keys", "scope_keys", "search_per_key"):
        assert callable(getattr(P.RecallIndex, name)), name
    for name in ("set", "get", "close"):
        assert callable(getattr(P.RecallKeys, name)), name
    assert isinstance(P.RecallKeys.rows, property) and P.RecallKeys.KEY_NONE == I64_MIN
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    assert "8s" in design and all(k in design for k in KERNELS)
    assert "THE CALL LOOKS OUTSIDE THE POOL" in full and "UNSPECIFIED" in full
    assert "a per-document cap are not offered" not in full and "a per-document cap is\n * orr_search_batch_per_key" in full
    for out_of_scope in ("cluster forms", "sharded.py", "record (shard) form", "service mirror", "micro-batcher", "keys in the shard file",
                         "pools above 56", "diverse search"):
        assert out_of_scope in full.split("orr_search_batch_per_key.  Let R be")[1].split("#define ORR_KEY_NONE")[0], out_of_scope


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
    qp, op, rp, sp, kp, cp, dp = (a.ctypes.data for a in (q, qoff, rows, scores, keys, counts, rounds))
    fake = C.c_void_p(kp)                               # a non-NULL keys handle that is never looked at: the index is NULL

    def call(topk, pool, cap, kh, r=rp, s=sp, ko=kp, c=cp, batch=B):
        ret = h.orr_search_batch_per_key(None, batch, 4, qp, None, None, op, 0, topk, 300, None, kh, cap, pool, r, s, ko, c, dp)
        assert b"orr_search_batch_per_key:" in err()
        return ret

    for r, s, ko, c in ((None, sp, kp, cp), (rp, None, kp, cp), (rp, sp, None, cp), (rp, sp, kp, None)):
        assert call(99, 0, 0, None, r, s, ko, c) == E and b"are required" in err()
    for pool in (0, -1, 57, 1 << 30):
        assert call(99, pool, 0, None) == E and b"pool must be in 1 .. 56" in err()
    for topk, pool in ((57, 56), (11, 10), (2, 1)):
        assert call(topk, pool, 0, None) == E and b"exceeds the pool" in err()
    for cap in (0, -1, -(1 << 31)):
        assert call(10, 10, cap, None) == E and b"max_per_key must be at least 1" in err()
    for cap in (1, 2, (1 << 31) - 1):
        assert call(10, 10, cap, None) == E and b"null keys" in err()
    # then the NULL index: every legal combination gets that far, B == 0 included
    for topk, pool, cap in ((10, 10, 1), (0, 1, 1), (-3, 1, 5), (10, 56, (1 << 31) - 1), (56, 56, 56), (1, 24, 2)):
        assert call(topk, pool, cap, fake) == E and b"null index" in err()
        assert call(topk, pool, cap, fake, batch=0) == E and b"null index" in err()
    assert (rows == 7).all() and (scores == 7.0).all() and (keys == 7).all() and (counts == 7).all() and (rounds == 7).all()

    # orr_keys_create / set / get / rows / destroy
    out = C.c_void_p(7)
    ids = np.arange(4, dtype=np.int64)
    ip = ids.ctypes.data
    assert h.orr_keys_create(None, -1, None, None, None) == E and b"orr_keys_create: out is NULL" in err()
    assert h.orr_keys_create(None, -1, None, None, C.byref(out)) == E and b"n is negative" in err()
    assert h.orr_keys_create(None, 4, None, ip, C.byref(out)) == E and b"row_ids or keys is NULL" in err()
    assert h.orr_keys_create(None, 4, ip, None, C.byref(out)) == E and b"row_ids or keys is NULL" in err()
    assert h.orr_keys_create(None, 4, ip, ip, C.byref(out)) == E and b"null index" in err()
    assert h.orr_keys_create(None, 0, None, None, C.byref(out)) == E and b"null index" in err()
    assert out.value == 7
    done = C.c_int64(7)
    dn = C.cast(C.byref(done), C.c_void_p)
    assert h.orr_keys_set(None, -1, None, None, dn) == E and b"orr_keys_set: n is negative" in err()
    assert h.orr_keys_set(None, 4, ip, None, dn) == E and b"row_ids or keys is NULL" in err()
    assert h.orr_keys_set(None, 4, ip, ip, dn) == E and b"null keys" in err()
    assert done.value == 7
    got = np.full(4, 7, np.int64)
    assert h.orr_keys_get(None, -1, None, None) == E and b"orr_keys_get: n is negative" in err()
    assert h.orr_keys_get(None, 4, ip, None) == E and b"row_ids or out_keys is NULL" in err()
    assert h.orr_keys_get(None, 4, ip, got.ctypes.data) == E and b"null keys" in err()
    assert (got == 7).all()
    assert h.orr_keys_rows(None) == -1
    h.orr_keys_destroy(None)

    # orr_scope_create_keys, in orr_scope_create_terms's pattern
    assert h.orr_scope_create_keys(None, None, -1, None, None) == E and b"orr_scope_create_keys: out is NULL" in err()
    for n in (-1, 65537):
        assert h.orr_scope_create_keys(None, None, n, None, C.byref(out)) == E and b"n_keys must be in 0 .. 65536" in err()
    assert h.orr_scope_create_keys(None, None, 4, None, C.byref(out)) == E and b"keys is NULL with 4 keys" in err()
    assert h.orr_scope_create_keys(None, None, 4, ip, C.byref(out)) == E and b"null keys handle" in err()
    assert h.orr_scope_create_keys(None, None, 0, None, C.byref(out)) == E and b"null keys handle" in err()
    assert h.orr_scope_create_keys(None, fake, 4, ip, C.byref(out)) == E and b"null index" in err()
    assert out.value == 7
