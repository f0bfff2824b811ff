"""CPU checks of the cosine range search (orr_search_range_cosine): the rules of csrc/orr_range_plan.h through their selftest, the
kernels, the driver and the selftest sharing the header's inlines, the two entry points declared, exported, bound and
documented, and every argument error in its stated order, answered before any HIP call and before the handle is looked at
with the outputs untouched -- so on a machine without a GPU (the method of tests/test_scope_near_cpu.py).  The call at work is
in tests/test_gpu_range_cosine.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_range_plan_selftest")
NAMES = ("orr_search_range_cosine", "orr_cluster_search_range_cosine")


def test_range_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_range_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_range_plan_selftest: ok"


def test_the_kernels_the_driver_and_the_selftest_share_the_inlines():
    header = open(os.path.join(CSRC, "orr_range_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    screen = open(os.path.join(CSRC, "orr_screen.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_range_plan_selftest.cpp")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    for name in ("first_invalid", "at_zero", "cos_bound", "screen_keeps", "device_keeps", "grown_cap", "buffer_cap", "compare_to",
                 "before", "hit_before", "merge_lists", "pair_cap_valid", "buffer_valid", "form_valid"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert f"range::{name}" in selftest, name
    # the screen's ending is made of the header's bound and keep rule; the two collecting kernels of its device rule and of the
    # cosine scope's (the host finish's) expression
    ending = screen.split("if (RANGE) {")[1].split("continue;\n            }\n            const double2 rc")[0]
    assert "range::cos_bound(" in ending and "range::screen_keeps(" in ending and "epi.cnt[b]" in ending and "epi.cap" in ending
    assert "kw_matches" not in ending and "rowc" not in ending and "created" not in ending     # no keywords, no row constants, no recency
    for kernel in ("range_collect", "range_collect_dense"):
        body = kernels.split(f"void {kernel}(")[1].split("\n}\n")[0]
        assert "range::device_keeps(scope_near::cosine_of(" in body, kernel
    # the host decides every pair it receives with cosine_of and >=, and orders by the header's rule
    finish = api.split("static void range_finish_query(")[1].split("\n}\n")[0]
    assert "scope_near::cosine_of(e.dot, norm_a, e.norm_b)" in finish and "scope_near::verdict(c, t)" in finish and "range::before(" in finish
    assert "sqrt" not in finish
    for name in ("first_invalid", "grown_cap", "buffer_cap", "merge_lists", "pair_cap_valid", "buffer_valid", "form_valid"):
        assert f"range::{name}(" in api, name
    # ... and which queries are AT ZERO through the walk plan it calls (orr_range_bulk_plan.h, both entry points')
    walk = open(os.path.join(CSRC, "orr_range_bulk_plan.h")).read().split("inline Walk walk_of(")[1].split("\n}\n")[0]
    assert "range::at_zero(" in walk and "range_bulk::walk_of(" in api
    # beside the search passes, not through them
    assert api.count("static int range_run(") == 1 and api.count("// ---- cosine range search") == 1
    section = api.split("// ---- cosine range search")[1].split("\nstatic int range_on_lane(")[0]
    for name in ("plan_pass", "run_shard_once", "sstats"):
        assert name not in section, name
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_range_plan_selftest" in makefile.split("all:")[0]                    # in SELFTEST: build() makes it
    assert "orr_range_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]


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
    assert re.search(r"ORR_ELIMIT\s*=\s*-7\b", decl) and P.native.ORR_ELIMIT == -7
    m = re.search(r"typedef struct orr_range_hit \{([^}]*)\} orr_range_hit;", decl)
    assert m and [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == ["row_id", "order_key", "cosine"]
    assert P.index.RANGE_HIT_DTYPE.itemsize == 24 and P.index.RANGE_HIT_DTYPE.names == ("row_id", "order_key", "cosine")
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    assert callable(P.RecallIndex.range_cosine) and callable(P.RecallCluster.range_cosine)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    for option in ("range_pair_cap", "range_buffer", "range_form"):
        assert option in design and option in full, option
    assert "8p" in design


def test_argument_errors_in_their_order_before_any_device_call_with_the_outputs_untouched():
    """Every case passes a NULL handle: the value errors are reported all the same, each case holding exactly one error more
    than the one in front of it, so the order is pinned.  ORR_ESTATE for an unsealed index and the scope errors need a real
    handle: the GPU file."""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    q = np.ones((3, 4), np.float32)
    t = np.array([0.5, -np.inf, np.inf])
    t_nan = np.array([0.5, np.nan, np.nan])
    hits = np.full((3, 5), 7, dtype=P.index.RANGE_HIT_DTYPE)
    n = np.full(3, 7, np.int32)
    total = np.full(3, 7, np.int64)
    qp, tp, tn, hp, np_, op = (a.ctypes.data for a in (q, t, t_nan, hits, n, total))
    for name, handle in ((NAMES[0], b"null index"), (NAMES[1], b"null cluster")):
        fn = getattr(h, name)

        def call(B, dim, qq, tt, max_hits, hh, nn, oo):
            r = fn(None, B, dim, qq, tt, None, max_hits, hh, nn, oo)
            assert name.encode() + b":" in err()
            return r

        # 1. the batch size, with everything behind it wrong as well
        for B in (-1, 65, 1 << 30):
            assert call(B, -1, None, None, -1, None, None, None) == E and b"batch size must be in 0 .. 64" in err()
        # 2. dim negative, 3. max_hits negative: they hold for an empty batch too
        for B in (0, 3, 64):
            assert call(B, -1, None, None, -1, None, None, None) == E and b"dim is negative" in err()
            assert call(B, 4, None, None, -1, None, None, None) == E and b"max_hits is negative" in err()
        # 4. q NULL with a dimension to read
        assert call(3, 4, None, None, 5, None, None, None) == E and b"q is NULL with dim 4" in err()
        # 5. min_cosine NULL (q may be NULL with dim 0)
        assert call(3, 4, qp, None, 5, None, None, None) == E and b"min_cosine is NULL" in err()
        assert call(3, 0, None, None, 5, None, None, None) == E and b"min_cosine is NULL" in err()
        # 6. out_hits NULL with hits asked for
        assert call(3, 4, qp, tn, 5, None, None, None) == E and b"out_hits is NULL with max_hits 5" in err()
        # 7. out_n NULL, 8. out_total NULL (out_hits may be NULL when only totals are asked for)
        assert call(3, 4, qp, tn, 5, hp, None, None) == E and b"out_n is NULL" in err()
        assert call(3, 4, qp, tn, 0, None, None, None) == E and b"out_n is NULL" in err()
        assert call(3, 4, qp, tn, 5, hp, np_, None) == E and b"out_total is NULL" in err()
        # 9. a NaN threshold, named
        assert call(3, 4, qp, tn, 5, hp, np_, op) == E and b"min_cosine[1] is NaN" in err()
        # then the NULL handle: the infinities are thresholds like any other, and an empty batch still needs a handle
        assert call(3, 4, qp, tp, 5, hp, np_, op) == E and handle in err()
        assert call(3, 4, qp, tp, 0, None, np_, op) == E and handle in err()
        assert call(3, 0, None, tp, 5, hp, np_, op) == E and handle in err()
        assert call(0, 4, None, None, 5, None, None, None) == E and handle in err()
    # nothing was written
    assert (hits["row_id"] == 7).all() and (hits["order_key"] == 7).all() and (hits["cosine"] == 7).all()
    assert (n == 7).all() and (total == 7).all()
