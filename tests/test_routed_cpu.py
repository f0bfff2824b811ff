"""CPU checks of the routed search (orr_search_batch_routed): the rules of csrc/orr_routed_plan.h through their selftest (the
argument order, the canonical set of a route, the slots by first appearance, the slices of at most 64 slots, the union table,
include_bits against a bit-by-bit emulation of one keys_include workgroup), the plan's slots, slices and tables against this
file's own restatement on random routes -- 130 distinct sets in slices of 64, 64 and 2, an all-empty batch, ORR_KEY_NONE
dropped among the cases --, include_bits against numpy on random words, the selftest in make, the symbol declared, exported,
bound and documented, and every argument error on NULL handles in the documented order with the outputs untouched -- so on a
machine without a GPU.  The call at work is in tests/test_gpu_routed.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_routed_plan_selftest")
NAME, N_ARGS = "orr_search_batch_routed", 19
NONE = -(1 << 63)
MAX_SLOTS = 64


def test_routed_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_routed_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_routed_plan_selftest: ok"


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def _canonical(row, n):
    return tuple(sorted({int(k) for k in row[:n] if int(k) != NONE}))


def _plan(route_keys, route_n):
    """(sets by first appearance, slot_of, [(slot0, n_slots, queries, query_slot, table keys, table masks)])"""
    sets, slot_of, seen = [], [], {}
    for row, n in zip(route_keys, route_n):
        c = _canonical(row, max(0, min(int(n), len(row))))
        if not c:
            slot_of.append(-1)
            continue
        if c not in seen:
            seen[c] = len(sets)
            sets.append(c)
        slot_of.append(seen[c])
    slices = []
    for s0 in range(0, len(sets), MAX_SLOTS):
        ns = min(MAX_SLOTS, len(sets) - s0)
        qs = [b for b, s in enumerate(slot_of) if s0 <= s < s0 + ns]
        table = {}
        for i in range(ns):
            for k in sets[s0 + i]:
                table[k] = table.get(k, 0) | (1 << i)
        tk = sorted(table)
        slices.append((s0, ns, qs, [slot_of[b] - s0 for b in qs], tk, [table[k] for k in tk]))
    return sets, slot_of, slices


def _plan_native(tmp_path, route_keys, route_n, tag):
    route_keys = np.ascontiguousarray(route_keys, np.int64)
    B, route = route_keys.shape
    src, dst = tmp_path / ("in_%s.bin" % tag), tmp_path / ("out_%s.bin" % tag)
    with open(src, "wb") as f:
        f.write(np.array([B, route], np.int64).tobytes())
        f.write(route_keys.tobytes())
        f.write(np.asarray(route_n, np.int64).tobytes())
    subprocess.run([SELFTEST, "slots", str(src), str(dst)], check=True, timeout=60)
    raw = np.fromfile(dst, np.int64)
    n_slots, at = int(raw[0]), 1
    slot_of = [int(v) for v in raw[at:at + B]]
    at += B
    sets = []
    for _ in range(n_slots):
        n = int(raw[at])
        sets.append(tuple(int(v) for v in raw[at + 1:at + 1 + n]))
        at += 1 + n
    n_slices = int(raw[at])
    at += 1
    slices = []
    for _ in range(n_slices):
        s0, ns, nq = (int(v) for v in raw[at:at + 3])
        at += 3
        qs = [int(v) for v in raw[at:at + nq]]
        qslot = [int(v) for v in raw[at + nq:at + 2 * nq]]
        at += 2 * nq
        nt = int(raw[at])
        tk = [int(v) for v in raw[at + 1:at + 1 + nt]]
        tm = [int(v) for v in raw[at + 1 + nt:at + 1 + 2 * nt].view(np.uint64)]
        at += 1 + 2 * nt
        slices.append((s0, ns, qs, qslot, tk, tm))
    assert at == len(raw)
    return sets, slot_of, slices


def _both(tmp_path, route_keys, route_n, tag):
    want = _plan(np.asarray(route_keys, np.int64), route_n)
    got = _plan_native(tmp_path, route_keys, route_n, tag)
    assert got == want, (tag, got[1][:8], want[1][:8])
    return got


def test_canonical_sets_and_dedupe_by_first_appearance(tmp_path):
    rk = np.array([[5, 9, NONE], [9, 5, 5], [4, 4, 4], [NONE, 8, 8], [1, NONE, NONE], [9, 5, NONE], [-1, (1 << 63) - 1, NONE + 1]], np.int64)
    rn = [2, 3, 0, 1, 1, 3, 3]
    sets, slot_of, slices = _both(tmp_path, rk, rn, "hand")
    assert sets == [(5, 9), (1,), (NONE + 1, -1, (1 << 63) - 1)]            # sorted as signed integers, ORR_KEY_NONE dropped
    assert slot_of == [0, 0, -1, -1, 1, 0, 2]                               # n = 0 and ORR_KEY_NONE alone: the slot "none"
    assert len(slices) == 1 and slices[0][2] == [0, 1, 4, 5, 6] and slices[0][3] == [0, 0, 1, 0, 2]
    assert slices[0][4] == [NONE + 1, -1, 1, 5, 9, (1 << 63) - 1] and slices[0][5] == [4, 4, 2, 1, 1, 4]
    rng = np.random.default_rng(8)
    for n, (B, route, pool) in enumerate([(1, 1, 3), (24, 3, 6), (256, 10, 14), (300, 40, 5_000), (64, 1024, 70_000)]):
        rk = rng.integers(0, pool, (B, route))
        rk = np.where(rng.random((B, route)) < 0.05, NONE, rk)
        rn = rng.integers(0, route + 1, B)
        _both(tmp_path, rk, rn, "rnd%d" % n)


def test_130_distinct_sets_give_slices_of_64_64_and_2_and_an_all_empty_batch_gives_none(tmp_path):
    B = 260
    rk = np.array([[10 * (b % 130), 5] if b < 130 else [5, 10 * (b % 130)] for b in range(B)], np.int64)
    sets, slot_of, slices = _both(tmp_path, rk, [2] * B, "130")
    assert len(sets) == 130 and slot_of == [b % 130 for b in range(B)]
    assert [(s[0], s[1]) for s in slices] == [(0, 64), (64, 64), (128, 2)]
    for s0, ns, qs, qslot, tk, tm in slices:
        assert qs == sorted(qs) and len(qs) == 2 * ns                       # a slice carries its slots' queries, ascending
        assert tm[tk.index(5)] == (1 << ns) - 1                             # key 5: every slot of the slice
    sets, slot_of, slices = _both(tmp_path, rk, [0] * B, "empty")
    assert sets == [] and slices == [] and slot_of == [-1] * B
    sets, slot_of, slices = _both(tmp_path, np.full((7, 4), NONE, np.int64), [4] * 7, "none")
    assert sets == [] and slices == []


def test_include_bits_against_numpy(tmp_path):
    rng = np.random.default_rng(5)
    n = 4_096
    base = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    inc = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    inc[:100] = 0
    base[100:200] = 0
    inc[200:300] = np.uint64((1 << 64) - 1)
    src, dst = tmp_path / "in_inc.bin", tmp_path / "out_inc.bin"
    with open(src, "wb") as f:
        f.write(np.array([n], np.int64).tobytes())
        f.write(base.tobytes())
        f.write(inc.tobytes())
    subprocess.run([SELFTEST, "include", str(src), str(dst)], check=True, timeout=60)
    got = np.fromfile(dst, np.uint64)
    assert np.array_equal(got, base & inc)
    assert not np.array_equal(got, inc)                                     # (the data tells a rule that ignores the base apart)


def test_one_definition_shared_with_the_kernel_and_the_selftest_in_make():
    header = open(os.path.join(CSRC, "orr_routed_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_routed_plan_selftest.cpp")).read()
    for name in ("first_invalid", "include_bits", "canonical", "slots", "slices", "slice_table"):
        assert len(re.findall(r"inline [\w:<>, ]+ %s\(" % name, header)) == 1, name
        assert re.search(r"\b%s\(" % name, selftest), name
    assert "ORR_PK_HD inline uint64_t include_bits(" in header and "kMaxRoute = 1024" in header
    assert "per_key::kMaxSlots * kMaxRoute == per_key::kMaxScopeKeys" in header
    assert "build_table(" in header.split("inline void slice_table(")[1]   # the union table is the per-key search's, reused
    body = kernels.split("void routed_include_kernel(")[1].split("hipError_t launch_keys_include(")[0]
    assert "routed::include_bits(" in body and "per_key::table_mask(" in body and "atomic" not in body
    exclude = kernels.split("void keys_exclude_kernel(")[1].split("hipError_t launch_keys_exclude(")[0]
    assert "include_bits" not in exclude                                    # the sibling is left as it was
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_routed_plan_selftest" in makefile.split("all:")[0]     # in SELFTEST: build() makes it
    assert "orr_routed_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]


def test_the_entry_point_is_declared_exported_bound_and_documented():
    P = pkg()
    txt = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % NAME, decl)
    assert m and len(m.group(1).split(",")) == N_ARGS, m and m.group(1)
    assert NAME in P.native.EXPORTED_HIP_SYMBOLS
    f = getattr(P.native.hip, NAME)
    assert len(f.argtypes) == N_ARGS and f.restype is C.c_int
    assert P.native.hip.orr_abi_version() == 1                              # adding functions is compatible
    assert callable(P.RecallIndex.search_routed)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
    part = txt.split("---- routed search:")[1].split("int %s(" % NAME)[0]
    for piece in ("THE CONTRACT IS A TWIN", "candidate_limit = every row of", "orr_scope_create_keys(idx, keys, D_b without ORR_KEY_NONE)",
                  "orr_search_batch_in_scope(idx, 1,", "route is 1 .. 1024", "never holds both", "keys_include", "no output is written"):
        assert piece in part, piece
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 8y." in design and "keys_include" in design.split("### 8y.")[1]


def test_argument_errors_in_their_order_before_the_handles_with_the_outputs_untouched():
    """every case passes NULL handles, each holding exactly one error more than the one behind it"""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    rows, scores = np.full(8, 7, np.int64), np.full(8, 7.0)
    counts, rk, rn = np.full(2, 7, np.int32), np.full(8, 7, np.int64), np.full(2, 7, np.int32)
    qoff = np.zeros(3, np.uint32)
    r, s, c, k, n = (a.ctypes.data for a in (rows, scores, counts, rk, rn))
    fake = C.c_void_p(0)                                # a NULL handle

    def call(docs, idx, keys, route, o_rows, o_scores, o_counts, B=2):
        return h.orr_search_batch_routed(docs, idx, keys, B, 0, None, None, None, qoff.ctypes.data, 0, route, 4, 300, None,
                                         o_rows, o_scores, o_counts, k, n)

    for outs in ((None, s, c), (r, None, c), (r, s, None)):             # 1: an output NULL (with every later error present too)
        assert call(fake, fake, fake, 0, *outs) == E and b"out_rows, out_scores and out_counts are required" in err()
    for route in (0, -3, 1025):                                          # 2: route outside 1 .. 1024
        assert call(fake, fake, fake, route, r, s, c) == E and b"route must be in 1 .. 1024" in err()
    assert call(fake, fake, fake, 1, r, s, c) == E and b"null keys" in err()                  # 3
    assert call(fake, fake, fake, 1024, r, s, c) == E and b"null keys" in err()
    # 4 (docs NULL) and the index behind it need a keys handle that is not NULL: tests/test_gpu_routed.py
    assert (rows == 7).all() and (scores == 7.0).all() and (counts == 7).all() and (rk == 7).all() and (rn == 7).all()
