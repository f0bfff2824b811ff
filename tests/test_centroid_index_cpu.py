"""CPU checks of the document index (orr_keys_centroid_index) and of the read-back of stored rows (orr_index_get_rows): the
rules of csrc/orr_centroid_index_plan.h through their selftest (the argument order, the merge of the participating runs into
the list of all keys, the kept keys of a slice, their destination rows, the slice walk, the one finish expression), the plan's
kept-key numbering and slice walk against this file's own restatement on random data -- a slice whose keys are all skipped and
a slice boundary between two kept keys among the cases --, the one finish expression, the build flags and the selftest in make, the two
symbols declared, exported, bound and documented, and every argument error on NULL handles in the documented order with the
outputs untouched -- so on a machine without a GPU (the method of tests/test_key_groups_cpu.py).  The calls at work are in
tests/test_gpu_centroid_index.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_centroid_index_plan_selftest")
NAMES = ("orr_keys_centroid_index", "orr_index_get_rows")
N_ARGS = (5, 6)


def test_centroid_index_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_centroid_index_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_centroid_index_plan_selftest: ok"


# ---- the restatement: which keys are kept, where their rows go, how the slices walk ------------------------------------------

def _walk(used, first, per_slice):
    """[(key0, n_keys, row0, [(slot, n, first), ...])]: the keys in slices of per_slice, the kept ones (used > 0) numbered in key
    order without a gap; a slice's kept keys carry their number IN the slice (their row of its sums)"""
    out, row = [], 0
    for key0 in range(0, len(used), per_slice):
        n_keys = min(per_slice, len(used) - key0)
        kept = [(j, int(used[key0 + j]), int(first[key0 + j])) for j in range(n_keys) if used[key0 + j] > 0]
        out.append((key0, n_keys, row, kept))
        row += len(kept)
    return out


def _plan_walk(tmp_path, used, first, per_slice, tag):
    src, dst = tmp_path / ("in_%s.bin" % tag), tmp_path / ("out_%s.bin" % tag)
    with open(src, "wb") as f:
        f.write(np.array([len(used), per_slice], np.int64).tobytes())
        f.write(np.asarray(used, np.int64).tobytes())
        f.write(np.asarray(first, np.int64).tobytes())
    subprocess.run([SELFTEST, "walk", str(src), str(dst)], check=True, timeout=60)
    raw = np.fromfile(dst, np.int64)
    at, out = 1, []
    for _ in range(int(raw[0])):
        key0, n_keys, row0, n_kept = (int(v) for v in raw[at:at + 4])
        at += 4
        kept = [tuple(int(v) for v in raw[at + 3 * i:at + 3 * i + 3]) for i in range(n_kept)]
        at += 3 * n_kept
        out.append((key0, n_keys, row0, kept))
    assert at == len(raw)
    return out


def test_the_kept_keys_their_rows_and_the_slice_walk_equal_the_restatement(tmp_path):
    rng = np.random.default_rng(31)
    cases = []
    # by hand: slice 2 of 4 is all skipped; the boundary between slices 0 and 1 lies between two kept keys
    cases.append((np.array([2, 0, 7, 1, 300, 0, 0, 0, 0, 0, 5]), 3))
    cases.append((np.zeros(9, np.int64), 4))                            # nothing is kept
    cases.append((np.ones(8, np.int64), 4))                             # everything is kept; the boundary falls after key 3
    cases.append((np.zeros(0, np.int64), 5))
    for T in (1, 2, 17, 300, 5_000):
        used = rng.integers(0, 600, T) * (rng.random(T) < 0.7)
        for per in (1, 7, 256, 65_536):
            cases.append((used, per))
    for n, (used, per) in enumerate(cases):
        used = np.asarray(used, np.int64)
        first = np.concatenate([[0], np.cumsum(used)[:-1]]).astype(np.int64) if len(used) else used
        want = _walk(used, first, per)
        got = _plan_walk(tmp_path, used, first, per, str(n))
        assert got == want, (n, per, got[:3], want[:3])
        rows = [s[2] + i for s in got for i in range(len(s[3]))]
        assert rows == list(range(int((used > 0).sum())))               # destination rows: dense, in key order
    hand = _plan_walk(tmp_path, np.asarray(cases[0][0], np.int64), np.arange(11, dtype=np.int64), 3, "hand")
    assert [len(s[3]) for s in hand] == [2, 2, 0, 1] and [s[2] for s in hand] == [0, 2, 4, 4]
    assert hand[0][3][-1][0] == 2 and hand[1][3][0][0] == 0             # key 2 -> row 1, key 3 -> row 2: across the boundary


def test_one_finish_expression_the_build_flags_and_the_selftest_in_make():
    header = open(os.path.join(CSRC, "orr_centroid_index_plan.h")).read()
    groups = open(os.path.join(CSRC, "orr_key_groups_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_centroid_index_plan_selftest.cpp")).read()
    for name in ("first_invalid", "first_invalid_get_rows", "kept", "merge_runs", "slice_kept", "walk", "get_rows_slice"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert re.search(r"\b%s\(" % name, selftest), name
    # ONE definition of the finish expression, shared by the host's finish and the kernel
    assert len(re.findall(r"\bfloat finish_one\(", groups)) == 1 and "ORR_KG_HD inline float finish_one(" in groups
    assert "finish_one(" in groups.split("inline void finish(")[1].split("\n}\n")[0]
    assert "key_groups::finish_one(" in kernels.split("void key_groups_centroid_finish_kernel(")[1].split("hipError_t launch_keys_centroid_finish(")[0]
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off -fno-fast-math" in makefile.split("CXXFLAGS ?=")[1].split("\n")[0]
    assert "host/orr_centroid_index_plan_selftest" in makefile.split("all:")[0]                 # in SELFTEST: build() makes it
    assert "orr_centroid_index_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]


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
        assert len(f.argtypes) == n_args and f.restype is C.c_int, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    assert P.native.hip.orr_abi_version() == 1              # adding functions is compatible
    assert callable(P.RecallKeys.centroid_index) and callable(P.RecallIndex.get_rows)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    assert "### 8x." in design and "keys_centroid_finish" in design and "keys_first_ticks" in design
    part = full.split("---- document index:")[1].split("int orr_keys_centroid_index(")[0]
    for piece in ("THE CONTRACT IS A TWIN", "(float)(S[d] / (double)n)", "round to nearest even", "first participating member", "row_id = the key itself",
                  "*out is not written", "8 bytes per key each", "key_groups_slice"):
        assert piece in part, piece
    section = design.split("### 8x.")[1].split("\n## 9.")[0]
    for out_of_scope in ("cluster form", "content per document", "two-level call", "in step with the source", "sharded.py", "service mirror",
                         "micro-batcher", "keys in the shard file", "pinned return path"):
        assert out_of_scope in part, out_of_scope
        assert out_of_scope in section, out_of_scope
    groups_part = full.split("---- key groups:")[1].split("#define ORR_KEY_GROUPS_BLOCK")[0]
    assert "ranks documents by centroid (built since:" in " ".join(groups_part.replace(" * ", " ").split())


def test_argument_errors_in_their_order_before_the_handle_with_the_outputs_untouched():
    """every case passes NULL handles, each holding exactly one error more than the one behind it"""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    out = C.c_void_p(0x7777)
    docs, skipped = C.c_int64(7), C.c_int64(7)
    pd, ps = C.cast(C.byref(docs), C.c_void_p), C.cast(C.byref(skipped), C.c_void_p)
    # orr_keys_centroid_index: out NULL; the keys handle NULL
    assert h.orr_keys_centroid_index(None, None, None, pd, ps) == E and b"orr_keys_centroid_index: out is NULL" in err()
    assert h.orr_keys_centroid_index(None, None, C.byref(out), pd, ps) == E and b"null keys" in err()
    assert h.orr_keys_centroid_index(None, None, C.byref(out), None, None) == E and b"null keys" in err()
    assert out.value == 0x7777 and docs.value == 7 and skipped.value == 7
    # orr_index_get_rows: n negative; row_ids or out_emb NULL; the index NULL
    ids = np.full(4, 7, np.int64)
    emb = np.full((4, 8), 7, np.float32)
    found = np.full(4, 7, np.uint8)
    ip, ep, fp = ids.ctypes.data, emb.ctypes.data, found.ctypes.data
    assert h.orr_index_get_rows(None, -1, None, 8, None, None) == E and b"orr_index_get_rows: n is negative" in err()
    assert h.orr_index_get_rows(None, 4, None, 8, ep, fp) == E and b"row_ids or out_emb is NULL with 4 entries" in err()
    assert h.orr_index_get_rows(None, 4, ip, 8, None, fp) == E and b"row_ids or out_emb is NULL with 4 entries" in err()
    assert h.orr_index_get_rows(None, 4, ip, 8, ep, fp) == E and b"null index" in err()
    assert h.orr_index_get_rows(None, 4, ip, 0, ep, None) == E and b"null index" in err()             # (dim is looked at with the handle)
    assert h.orr_index_get_rows(None, 0, None, 8, None, None) == E and b"null index" in err()
    assert (emb == 7).all() and (found == 7).all() and (ids == 7).all()
