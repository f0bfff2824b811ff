"""CPU checks of cosine scopes (orr_scope_create_near): the rules of csrc/orr_scope_near_plan.h through their selftest, the kernel,
the driver and the selftest sharing the header's inlines, the two entry points declared, exported, bound and documented, and
every argument error in its stated order, answered before any HIP call and before the handle is looked at -- so on a machine
without a GPU (the method of tests/test_scope_terms_cpu.py).  Cosine scopes at work are in tests/test_gpu_scope_near.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_scope_near_plan_selftest")
NAMES = ("orr_scope_create_near", "orr_cluster_scope_create_near")


def test_scope_near_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_scope_near_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_scope_near_plan_selftest: ok"


def test_the_kernel_and_the_selftest_share_the_inlines():
    header = open(os.path.join(CSRC, "orr_scope_near_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_scope_near_plan_selftest.cpp")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    for name in ("cosine_of", "row_state", "in_band", "tail_mask"):
        assert len(re.findall(r"inline \w+ %s\(" % name, header)) == 1, name
        assert f"scope_near::{name}(" in kernels, name
        assert f" {name}(" not in kernels.replace(f"scope_near::{name}(", ""), name      # no second definition beside the kernel
        assert f"scope_near::{name}(" in selftest, name
    # the row rule is made of the fold, the band and the verdict
    body = header.split("inline int32_t row_state(")[1].split("\n}\n")[0]
    assert all(f"{name}(" in body for name in ("fold_identity", "fold_verdict", "fold_settled", "in_band", "verdict"))
    for name in ("fold_identity", "fold_verdict", "fold_settled", "verdict", "band_width", "pending_row_in", "first_invalid",
                 "foreign_dim", "all_rows_at_zero", "grown_cap", "band_cap_valid", "mode_valid", "probes_valid"):
        assert len(re.findall(r"inline \w+ %s\(" % name, header)) == 1, name
        assert f"scope_near::{name}(" in selftest, name
    # the driver decides with the header's rules, and the host finish's cosine IS the band's: one expression, three callers
    for name in ("cosine_of", "pending_row_in", "first_invalid", "foreign_dim", "all_rows_at_zero", "grown_cap", "band_cap_valid"):
        assert f"scope_near::{name}(" in api, name
    score = api.split("double exact_score(")[1].split("\n}\n")[0]
    assert "scope_near::cosine_of(c.dot, norm_a, c.norm_b)" in score and "sqrt" not in score
    assert "sqrt" not in api.split("static int scope_fill_near(")[1].split("\n}\n")[0]
    # ONE walk: the exact dot kernel and the cosine scope's kernel instantiate the same inline
    assert len(re.findall(r"void exact_walk_tiled\(", kernels)) == 1
    assert kernels.count("exact_walk_tiled<") == 2
    assert kernels.count("__builtin_nontemporal_load") == 1
    for kernel in ("dot_exact_tiled", "scope_near_tiled"):
        assert "exact_walk_tiled<" in kernels.split(f"void {kernel}(")[1].split("\n}\n")[0], kernel
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_scope_near_plan_selftest" in makefile.split("all:")[0]               # in SELFTEST: build() makes it


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entry_points_are_declared_exported_bound_and_documented():
    P = pkg()
    decl = _declared("omnirecall_hip.h")
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, decl)
        assert m, name
        assert len(m.group(1).split(",")) == 7, m.group(1)
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        f = getattr(P.native.hip, name)
        assert f.restype is C.c_int and len(f.argtypes) == 7 and f.argtypes[4] is C.c_double
        for doc in ("README.md", "DESIGN.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    for macro, value in (("ORR_NEAR_ALL", 0), ("ORR_NEAR_ANY", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), decl), macro
        assert getattr(P.native, macro) == value
    assert P.native.hip.orr_abi_version() == 1                            # adding functions is compatible
    assert callable(P.RecallIndex.scope_near) and callable(P.RecallCluster.scope_near)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8o" in design and "near_band_cap" in design
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    assert "near_band_cap" in full and "AT MOST 8 PROBES" in full         # the cap and the option are stated where the call is
    assert "orr_index_update_rows does not evaluate it again" in full     # the maintenance paragraph's sentence


def test_argument_errors_in_their_order_before_any_device_call():
    """Every case passes a NULL handle: the value errors are reported all the same, each case holding exactly one error more
    than the one in front of it, so the order is pinned.  ORR_ESTATE for an unsealed index needs a real handle: the GPU file."""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    probes = np.ones((8, 4), np.float32)
    p = probes.ctypes.data
    nan, inf = float("nan"), float("inf")
    out = C.c_void_p(7)
    o = C.byref(out)
    for name, handle in ((NAMES[0], b"null index"), (NAMES[1], b"null cluster")):
        fn = getattr(h, name)

        def call(n, dim, pr, t, mode, outp):
            r = fn(None, n, dim, pr, t, mode, outp)
            assert name.encode() + b":" in err()
            return r

        # 1. out NULL wins over everything behind it
        assert call(9, -1, None, nan, 2, None) == E and b"out is NULL" in err()
        assert call(2, 4, p, 0.5, 0, None) == E and b"out is NULL" in err()
        # 2. n_probes negative or above 8, with everything behind it wrong as well
        for n in (-1, 9, 1 << 30):
            assert call(n, -1, None, nan, 2, o) == E and b"n_probes must be in 0 .. 8" in err()
        # 3. dim negative
        for n in (0, 8):
            assert call(n, -1, None, nan, 2, o) == E and b"dim is negative" in err()
        # 4. probes NULL with probes and a dimension to read
        assert call(8, 4, None, nan, 2, o) == E and b"probes is NULL with 8 probes" in err()
        # 5. mode outside 0 .. 1 (NULL probes are fine with no probes, and with dim 0)
        for mode in (-1, 2, 64):
            assert call(8, 4, p, nan, mode, o) == E and b"mode must be" in err()
            assert call(0, 4, None, nan, mode, o) == E and b"mode must be" in err()
            assert call(3, 0, None, nan, mode, o) == E and b"mode must be" in err()
        for mode in (0, 1):
            # 6. min_cosine NaN
            assert call(8, 4, p, nan, mode, o) == E and b"min_cosine is NaN" in err()
            assert call(0, 0, None, nan, mode, o) == E and b"min_cosine is NaN" in err()
            # 7. then the NULL handle: the infinities are thresholds like any other
            for t in (0.5, -inf, inf, 0.0, -2.0):
                assert call(8, 4, p, t, mode, o) == E and handle in err()
            assert call(0, 0, None, 0.5, mode, o) == E and handle in err()
            assert call(0, 4, None, 0.5, mode, o) == E and handle in err()
            assert call(3, 0, None, 0.5, mode, o) == E and handle in err()
    assert out.value == 7                                                 # no handle was written
