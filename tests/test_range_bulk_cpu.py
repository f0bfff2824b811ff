"""CPU checks of the bulk cosine range search (orr_search_range_cosine_bulk): the rules of csrc/orr_range_bulk_plan.h through their
selftest (which screen a query gets, the launch groups, the argument rules with the limit of 1024, the bound for the one-level
query, the ending's lane map), the lane map against the kernel's own tile16_c_of / tile16_g_of, the kernel and the driver made
of the shared inlines, the new symbols declared, exported, bound and documented, and every argument error on a NULL handle with
the outputs untouched -- so on a machine without a GPU (the method of tests/test_range_cosine_cpu.py).  The call at work is in
tests/test_gpu_range_bulk.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_range_bulk_plan_selftest")
NAMES = ("orr_search_range_cosine_bulk", "orr_cluster_search_range_cosine_bulk")


def test_range_bulk_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_range_bulk_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_range_bulk_plan_selftest: ok"
    # the two-level error would NOT have bounded the one-level product: the selftest met such pairs
    m = re.search(r"pairs the two-level error would not have covered: (\d+)", r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout


def test_the_lane_map_is_the_kernels(tmp_path):
    """the header's restatement of the ending's lane map against the three one-line functions of orr_epilogue.h the kernel calls,
    compiled for the host: the same (c, g) for every lane of a wave"""
    epilogue = open(os.path.join(CSRC, "orr_epilogue.h")).read()
    lines = []
    for name in ("tile16_row", "tile16_c_of", "tile16_g_of"):
        m = re.search(r"^__device__ __forceinline__ (int %s\(int \w+\) \{[^\n]*\})$" % name, epilogue, flags=re.M)
        assert m, name
        lines.append("static " + m.group(1))
    src = tmp_path / "lane_map.cpp"
    src.write_text('#include "orr_range_bulk_plan.h"\n#include <cstdio>\n' + "\n".join(lines) + """
int main()
{
    int bad = 0;
    for (int lane = 0; lane < 64; ++lane)
        bad += tile16_c_of(lane) != range_bulk::lane_c(lane) || tile16_g_of(lane) != range_bulk::lane_g(lane);
    printf("%d\\n", bad);
    return bad != 0;
}
""")
    exe = tmp_path / "lane_map"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stdout + r.stderr


def test_the_kernel_the_driver_and_the_selftest_share_the_rules():
    header = open(os.path.join(CSRC, "orr_range_bulk_plan.h")).read()
    old_header = open(os.path.join(CSRC, "orr_range_plan.h")).read()
    screen = open(os.path.join(CSRC, "orr_screen.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_range_bulk_plan_selftest.cpp")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    for name in ("first_invalid", "gemm_valid", "stream_shape", "gemm_shape", "stream_applies", "gemm_takes", "path_of", "group_queries", "query_tiles"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert re.search(r"\b%s\(" % name, selftest), name
    assert "kMaxQueries = 64" in old_header                                # the old call's limit stands
    # the ending: between the DOTS branch and the scoring epilogue of screen_tile16_kernel
    kernel = screen.split("void screen_tile16_kernel(")[1].split("// K2g:")[0]
    ending = kernel.split("} else if constexpr (RANGE) {")[1].split("    } else {\n        uint32_t salt = 0;")[0]
    for piece in ("range::cos_bound(re, rh, k.qe1)", "range::screen_keeps(", "atomicAdd(&ra.cnt[qi], 1u)", "slot < ra.cap", "ra.count_planes[",
                  "qi < B", "row < n_rows", "acc16_as_int_here<4 * (8 * i + j) + e>(acc_token)", "16 * i + 4 * g + e", "16 * j + c",
                  "tile16_c_of(lane_t)", "tile16_g_of(lane_t)", "ra.err2_level1[q]", "s_waitcnt vmcnt(0)"):
        assert piece in ending, piece
    for absent in ("i8_rowf", "kw_matches", "rowc", "created", "epilogue_requests", "fused_epilogue16"):
        assert absent not in ending, absent
    # the driver: one range_run, the list of its stages; which form a query gets and which screen is the header's walk plan,
    # called once; nothing sized by 64 any more
    assert api.count("static int range_run(") == 1 and api.count("// ---- cosine range search") == 1
    section = api.split("// ---- cosine range search")[1].split("\nstatic int range_on_lane(")[0]
    run = section.split("static int range_run(")[1]
    assert section.count("range_bulk::walk_of(") == 1 and "range_bulk::walk_of(w.B, a.dim, w.D, " in run
    walk = header.split("inline Walk walk_of(")[1].split("\n}\n")[0]
    for piece in ("range::at_zero(dim, index_dim, ", "stream_applies(index_dim, shadow, ", "gemm_takes(index_dim, w.n_screen, range_gemm, bulk)"):
        assert piece in walk, piece
    assert re.search(r"\bwalk_of\(", selftest)
    for name in ("stream_applies(", "gemm_takes(", "range::at_zero(", "isfinite("):    # the classification exists once, in the header
        assert name not in section, name
    for piece in ("range_bulk::group_queries(cap, w.walk.gemm ? 1 : range::kScreenQ)",
                  "orr::launch_screen_tile16_range(", "orr::launch_screen_gemv_i8_range(", "\"screen_tile16_range\"", "range::grown_cap("):
        assert piece in section, piece
    assert section.count("range::grown_cap(") == 1                             # the growth rule exists once
    assert "[&]" not in section                                                # stages are functions, not closures over the call
    assert "range::kMaxQueries" not in section and "kMaxQueries]" not in section
    for name in ("plan_pass", "run_shard_once", "sstats"):
        assert name not in section, name
    launcher = screen.split("hipError_t launch_screen_tile16_range(")[1].split("\n}\n")[0]
    assert "screen_grid(blocks, D / 64)" in launcher and "ensure_max_dynamic_lds<screen_tile16_kernel<NT, false, false, true>>" in launcher
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_range_bulk_plan_selftest" in makefile.split("all:")[0]               # in SELFTEST: build() makes it
    assert "orr_range_bulk_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entry_points_are_declared_exported_bound_and_documented():
    P = pkg()
    decl = _declared("omnirecall_hip.h")
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, decl)
        assert m, name
        assert len(m.group(1).split(",")) == 10, m.group(1)
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        f = getattr(P.native.hip, name)
        assert f.restype is C.c_int and len(f.argtypes) == 10 and f.argtypes[6] is C.c_int32
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    assert callable(P.RecallIndex.range_cosine_bulk) and callable(P.RecallCluster.range_cosine_bulk)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    assert "range_gemm" in design and "range_gemm" in full and "8q" in design
    assert "screen_tile16_range" in design and "screen_tile16_range" in full


def test_argument_errors_in_their_order_before_any_device_call_with_the_outputs_untouched():
    """orr_search_range_cosine's cases with the first rule reading 0 .. 1024: every case passes a NULL handle, each holding exactly
    one error more than the one in front of it."""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    B_big = 1024
    q = np.ones((B_big, 4), np.float32)
    t = np.full(B_big, 0.5)
    t[1], t[2] = -np.inf, np.inf
    t_nan = t.copy()
    t_nan[700], t_nan[900] = np.nan, np.nan
    hits = np.full((B_big, 5), 7, dtype=P.index.RANGE_HIT_DTYPE)
    n = np.full(B_big, 7, np.int32)
    total = np.full(B_big, 7, np.int64)
    qp, tp, tn, hp, np_, op = (a.ctypes.data for a in (q, t, t_nan, hits, n, total))
    for name, handle in ((NAMES[0], b"null index"), (NAMES[1], b"null cluster")):
        fn = getattr(h, name)

        def call(B, dim, qq, tt, max_hits, hh, nn, oo):
            r = fn(None, B, dim, qq, tt, None, max_hits, hh, nn, oo)
            assert name.encode() + b":" in err()
            return r

        # 1. the batch size, with everything behind it wrong as well
        for B in (-1, 1025, 1 << 30):
            assert call(B, -1, None, None, -1, None, None, None) == E and b"batch size must be in 0 .. 1024" in err()
        # 2. dim negative, 3. max_hits negative: they hold for an empty batch too
        for B in (0, 3, 65, 1024):
            assert call(B, -1, None, None, -1, None, None, None) == E and b"dim is negative" in err()
            assert call(B, 4, None, None, -1, None, None, None) == E and b"max_hits is negative" in err()
        for B in (3, 65, 1024):
            assert call(B, 4, None, None, 5, None, None, None) == E and b"q is NULL with dim 4" in err()
            assert call(B, 4, qp, None, 5, None, None, None) == E and b"min_cosine is NULL" in err()
            assert call(B, 0, None, None, 5, None, None, None) == E and b"min_cosine is NULL" in err()
            assert call(B, 4, qp, tn, 5, None, None, None) == E and b"out_hits is NULL with max_hits 5" in err()
            assert call(B, 4, qp, tn, 5, hp, None, None) == E and b"out_n is NULL" in err()
            assert call(B, 4, qp, tn, 0, None, None, None) == E and b"out_n is NULL" in err()
            assert call(B, 4, qp, tn, 5, hp, np_, None) == E and b"out_total is NULL" in err()
        # 9. a NaN threshold beyond the old limit, named; a batch that ends in front of it has none
        assert call(1024, 4, qp, tn, 5, hp, np_, op) == E and b"min_cosine[700] is NaN" in err()
        assert call(700, 4, qp, tn, 5, hp, np_, op) == E and handle in err()
        # then the NULL handle
        for B in (3, 65, 1024):
            assert call(B, 4, qp, tp, 5, hp, np_, op) == E and handle in err()
            assert call(B, 4, qp, tp, 0, None, np_, op) == E and handle in err()
            assert call(B, 0, None, tp, 5, hp, np_, op) == E and handle in err()
        assert call(0, 4, None, None, 5, None, None, None) == E and handle in err()
    # nothing was written
    assert (hits["row_id"] == 7).all() and (hits["order_key"] == 7).all() and (hits["cosine"] == 7).all()
    assert (n == 7).all() and (total == 7).all()
    # the old entry point keeps its limit
    assert h.orr_search_range_cosine(None, 65, 4, qp, tp, None, 5, hp, np_, op) == E and b"batch size must be in 0 .. 64" in err()
