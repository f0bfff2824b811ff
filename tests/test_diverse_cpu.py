"""CPU checks of the diverse search (orr_search_batch_diverse, orr_index_pair_dots): the rules of csrc/orr_diverse_plan.h through
their selftest (the argument order, both greedy rules against brute-force restatements, the kernel's work split), the work split
compiled for the host against the header once more, the kernel, the driver and the selftest made of the shared inlines, the two
symbols declared, exported, bound and documented, and every argument error on a NULL handle with the outputs untouched -- so on
a machine without a GPU (the method of tests/test_range_bulk_cpu.py).  The calls at work are in tests/test_gpu_diverse.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_diverse_plan_selftest")
NAMES = ("orr_search_batch_diverse", "orr_index_pair_dots")
INF, NAN = float("inf"), float("nan")


def test_diverse_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_diverse_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_diverse_plan_selftest: ok"
    m = re.search(r"greedy cases checked: (\d+) \(collapses shorter than take: (\d+), MMR picks out of rank order: (\d+)\)", r.stdout)
    assert m and int(m.group(1)) > 5000 and int(m.group(2)) > 0 and int(m.group(3)) > 0, r.stdout


def test_the_work_split_covers_every_pair_once(tmp_path):
    """the header's owned_pair / pair_of as the kernel calls them, compiled for the host: for every list length 0 .. 56 every
    (i <= j) pair has exactly one (thread, slot), and no slot names a pair outside the list"""
    src = tmp_path / "split.cpp"
    src.write_text('#include "orr_diverse_plan.h"\n#include <cstdio>\n#include <vector>\n' + """
int main()
{
    using namespace diverse;
    long bad = 0, pairs = 0;
    for (int cnt = 0; cnt <= kMaxPool; ++cnt) {
        std::vector<int> seen((size_t)(cnt * cnt), 0);
        for (int t = 0; t < kPairThreads; ++t)
            for (int s = 0; s < kPairsPerThread; ++s) {
                const int p = owned_pair(t, s);
                if (p >= pair_count(cnt)) continue;
                int i = -1, j = -1;
                pair_of(p, cnt, &i, &j);
                if (i < 0 || j < i || j >= cnt) { ++bad; continue; }
                seen[(size_t)(i * cnt + j)] += 1;
                ++pairs;
            }
        for (int i = 0; i < cnt; ++i)
            for (int j = 0; j < cnt; ++j) bad += seen[(size_t)(i * cnt + j)] != (i <= j ? 1 : 0);
    }
    printf("%ld %ld\\n", bad, pairs);
    return bad != 0;
}
""")
    exe = tmp_path / "split"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    want_pairs = sum(c * (c + 1) // 2 for c in range(57))
    assert r.returncode == 0 and r.stdout.split() == ["0", str(want_pairs)], r.stdout + r.stderr


def test_the_kernel_the_driver_and_the_selftest_share_the_rules():
    header = open(os.path.join(CSRC, "orr_diverse_plan.h")).read()
    gemm = open(os.path.join(CSRC, "orr_gemm.hip")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_diverse_plan_selftest.cpp")).read()
    for name in ("first_invalid", "first_invalid_pairs", "mode_valid", "needs_dots", "collapse_keeps", "mmr_fold", "mmr_penalty_cosine", "mmr_value",
                 "select_collapse", "select_mmr", "mat_index", "pair_count", "owned_pair", "pair_of", "compare_double", "take_of"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert re.search(r"\b%s\(" % name, selftest), name
    assert "kMaxPool = kSelWidth - 8" in header and "kSelWidth = 64" in header
    # the kernel: the header's split and indexing, the reference's loop, no atomics
    kernel = gemm.split("void pair_dots_kernel(")[1].split("hipError_t launch_pair_dots(")[0]
    for piece in ("diverse::owned_pair(t, s)", "diverse::pair_of(p, n, &i, &j)", "diverse::pair_count(n)", "diverse::mat_index(stride, i, j)",
                  "diverse::mat_index(stride, j, i)", "acc[s] += (double)p;", "p < n_rows", "__syncthreads()"):
        assert piece in kernel, piece
    for absent in ("atomic", "cosine_of", "sqrt", "fma"):
        assert absent not in kernel, absent
    launcher = gemm.split("hipError_t launch_pair_dots(")[1].split("\n}\n")[0]
    assert "dim3 grid((unsigned)n_lists)" in launcher and "stride > diverse::kMaxPool" in launcher
    # the driver: one diverse_run for both modes, the existing searches unchanged in front, the host's cosine, the header's rules
    assert api.count("static int diverse_run(") == 1
    run = api.split("static int diverse_run(")[1].split("\nint orr_search_batch_diverse(")[0]
    for piece in ("masked_batch(lane, pa, ScopeSource{nullptr, within}", "escalate(index_backend(lane, fn, n), pa, escalation::initial_kprime(pool, n, orr::kSelWidth)",
                  "pa.out_keys = p_keys.data()", "diverse::needs_dots(d.mode, d.param, p_cnt[(size_t)b], lane->dim)", "pair_dots_on_lane(",
                  "scope_near::cosine_of(", "diverse::select_collapse(", "diverse::select_mmr(", "- lane->row_base"):
        assert piece in run, piece
    for name in ("plan_pass", "run_shard_once", "run_large_k"):
        assert name not in run, name
    entry = api.split("\nint orr_search_batch_diverse(")[1].split("\nint orr_index_pair_dots(")[0]
    assert entry.index("diverse::first_invalid(") < entry.index("if (!idx)") < entry.index("check_batch(") < entry.index("acquire_lane(")
    pairs = api.split("\nint orr_index_pair_dots(")[1].split("\n}\n")[0]
    assert pairs.index("positions[e] >= lane->n_rows") < pairs.index("pair_dots_on_lane(")       # checked before any launch
    assert api.count('Timed t(lane, "pair_dots"') == 1 and api.count("orr::launch_pair_dots(") == 1
    # every existing entry point leaves the new pointer null
    assert api.count("out_keys = p_keys.data()") == 1 and "int64_t *out_keys = nullptr;" in api
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_diverse_plan_selftest" in makefile.split("all:")[0]                          # in SELFTEST: build() makes it
    assert "orr_diverse_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]
    rule = makefile.split("host/orr_diverse_plan_selftest: ")[1].split("\n")[1]
    assert "-ffp-contract=off" in rule


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entry_points_are_declared_exported_bound_and_documented():
    P = pkg()
    decl = _declared("omnirecall_hip.h")
    for name, n_args in zip(NAMES, (18, 6)):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, decl)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, m.group(1)
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        f = getattr(P.native.hip, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    assert P.native.hip.orr_search_batch_diverse.argtypes[13] is C.c_double
    assert re.search(r"#define ORR_DIVERSE_COLLAPSE 0\b", decl) and re.search(r"#define ORR_DIVERSE_MMR\s+1\b", decl)
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    assert callable(P.RecallIndex.search_diverse) and callable(P.RecallIndex.pair_dots)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    assert "8r" in design and "pair_dots" in design and "pair_dots" in full
    assert "NEVER LOOKS OUTSIDE THE POOL" in full                         # the header says so


def test_argument_errors_in_their_order_before_the_handle_with_the_outputs_untouched():
    """every case passes a NULL handle, each holding exactly one error more than the one behind it"""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    B, k = 3, 10
    q = np.ones((B, 4), np.float32)
    qoff = np.zeros(B + 1, np.uint32)
    rows = np.full((B, k), 7, np.int64)
    scores = np.full((B, k), 7.0)
    counts = np.full(B, 7, np.int32)
    ranks = np.full((B, k), 7, np.int32)
    qp, op, rp, sp, cp, kp = (a.ctypes.data for a in (q, qoff, rows, scores, counts, ranks))

    def call(topk, pool, mode, param, r=rp, s=sp, c=cp, handle=None, batch=B):
        ret = h.orr_search_batch_diverse(handle, batch, 4, qp, None, None, op, 0, topk, 300, None, pool, mode, param, r, s, c, kp)
        assert b"orr_search_batch_diverse:" in err()
        return ret

    for r, s, c in ((None, sp, cp), (rp, None, cp), (rp, sp, None)):
        assert call(99, 0, 7, NAN, r, s, c) == E and b"are required" in err()
    for pool in (0, -1, 57, 1 << 30):
        assert call(99, pool, 7, NAN) == E and b"pool must be in 1 .. 56" in err()
    assert call(57, 56, 7, NAN) == E and b"exceeds the pool" in err()
    assert call(11, 10, 7, NAN) == E and b"exceeds the pool" in err()
    assert call(2, 1, 7, NAN) == E and b"exceeds the pool" in err()
    for mode in (7, -1, 2):
        assert call(10, 10, mode, NAN) == E and b"mode must be" in err()
    for mode in (0, 1):
        assert call(10, 10, mode, NAN) == E and b"param is NaN" in err()
    for lam in (-0.001, 1.0000000000000002, INF, -INF):
        assert call(10, 10, 1, lam) == E and b"lambda must be in [0, 1]" in err()
    # then the NULL handle: every legal combination gets that far, B == 0 included
    for topk, pool, mode, param in ((10, 10, 0, 0.9), (0, 1, 0, -INF), (-3, 1, 1, 0.0), (10, 56, 0, INF), (56, 56, 1, 1.0), (1, 24, 0, 2.5)):
        assert call(topk, pool, mode, param) == E and b"null index" in err()
        assert call(topk, pool, mode, param, batch=0) == E and b"null index" in err()
    assert (rows == 7).all() and (scores == 7.0).all() and (counts == 7).all() and (ranks == 7).all()

    # orr_index_pair_dots
    off = np.array([0, 2, 3], np.uint32)
    pos = np.array([0, 1, 2], np.int64)
    out = np.full((2, 4, 4), 7.0)
    fp, pp, tp = off.ctypes.data, pos.ctypes.data, out.ctypes.data

    def pairs(n_lists, o, p, stride, dst):
        ret = h.orr_index_pair_dots(None, n_lists, o, p, stride, dst)
        assert b"orr_index_pair_dots:" in err()
        return ret

    assert pairs(-1, None, None, 57, None) == E and b"out is NULL" in err()
    assert pairs(-1, None, None, 57, tp) == E and b"n_lists is negative" in err()
    for stride in (57, 0, -1):
        assert pairs(2, None, None, stride, tp) == E and b"stride must be in 1 .. 56" in err()
    assert pairs(2, None, None, 4, tp) == E and b"list_off is NULL" in err()
    assert pairs(2, fp, None, 4, tp) == E and b"positions is NULL" in err()
    assert pairs(2, fp, pp, 4, tp) == E and b"null index" in err()
    assert (out == 7.0).all()
