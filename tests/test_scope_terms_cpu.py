"""CPU checks of term scopes (orr_scope_create_terms): the rules of csrc/orr_scope_terms_plan.h through their selftest, the kernel
and the selftest sharing the header's inlines, the entry point declared, exported, bound and documented, and every argument
error in its stated order, answered before any HIP call and before the index handle is looked at -- so on a machine without a
GPU (the method of tests/test_scope_handle_cpu.py).  Term scopes at work are in tests/test_gpu_scope_terms.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_scope_terms_plan_selftest")
NAME = "orr_scope_create_terms"


def test_scope_terms_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_scope_terms_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_scope_terms_plan_selftest: ok"


def test_the_kernel_and_the_selftest_share_the_inlines():
    header = open(os.path.join(CSRC, "orr_scope_terms_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_scope_terms_plan_selftest.cpp")).read()
    for name in ("fold_identity", "fold_word", "tail_mask"):
        assert len(re.findall(r"inline \w+ %s\(" % name, header)) == 1, name
        assert f"scope_terms::{name}(" in kernels, name
        assert f" {name}(" not in kernels.replace(f"scope_terms::{name}(", ""), name     # no second definition beside the kernel
        assert f"scope_terms::{name}(" in selftest, name
    # the host's word is the kernel's rule: scope_word is made of the three inlines
    body = header.split("inline uint32_t scope_word(")[1]
    assert all(f"{name}(" in body for name in ("fold_identity", "fold_word", "tail_mask"))
    for name in ("scope_word", "mode_valid", "terms_valid", "first_bad_term"):
        assert f"scope_terms::{name}(" in selftest, name
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_scope_terms_plan_selftest" in makefile.split("all:")[0]             # in SELFTEST: build() makes it
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    for name in ("mode_valid", "terms_valid", "first_bad_term"):
        assert f"scope_terms::{name}(" in api, name
    # the cleanup behind a keyword chain is ONE function, which the search's last stage and the term scope both call
    assert len(re.findall(r"^int clean_keyword_side\(", api, flags=re.M)) == 1
    assert api.count("clean_keyword_side(") >= 3
    assert api.count("idx->kw_clean.grant_bitmaps(") == 1 and api.count("idx->kw_clean.grant_counters(") == 1
    assert api.count("grant_bitmaps(") == 2 and api.count("grant_counters(") == 2      # each: KwVouchers' definition and that one call


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entry_point_is_declared_exported_bound_and_documented():
    P = pkg()
    decl = _declared("omnirecall_hip.h")
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % NAME, decl)
    assert m, NAME
    assert len(m.group(1).split(",")) == 6, m.group(1)
    assert NAME in P.native.EXPORTED_HIP_SYMBOLS
    f = getattr(P.native.hip, NAME)
    assert f.restype is C.c_int and len(f.argtypes) == 6
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
    for macro, value in (("ORR_TERMS_ALL", 0), ("ORR_TERMS_ANY", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), decl), macro
        assert getattr(P.native, macro) == value
    assert P.native.hip.orr_abi_version() == 1                            # adding a function is compatible
    assert callable(P.RecallIndex.scope_terms)
    assert "8l" in open(os.path.join(ROOT, "DESIGN.md")).read()
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    assert "orr_scope_create_ticks(INT64_MIN, INT64_MAX)" in full         # the scope of all rows, named where n_terms == 0 is


def test_argument_errors_in_their_order_before_any_device_call():
    """Every case passes a NULL index: the value errors are reported all the same, each case holding exactly one error more
    than the one in front of it, so the order is pinned.  ORR_ESTATE for an unsealed index needs a real handle: the GPU file."""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    pool = np.frombuffer(b"abcde\0", np.uint8).copy()
    good = np.array([0, 2, 5], np.uint32)
    out = C.c_void_p(7)
    o = C.byref(out)
    p, g = pool.ctypes.data, good.ctypes.data

    def call(n, terms, off, mode, outp):
        r = h.orr_scope_create_terms(None, n, terms, off, mode, outp)
        assert NAME.encode() in err()
        return r

    # 1. out NULL wins over everything behind it
    assert call(-1, None, None, 9, None) == E and b"out is NULL" in err()
    assert call(2, p, g, 0, None) == E and b"out is NULL" in err()
    # 2. n_terms negative or above 256, with everything behind it wrong as well
    for n in (-1, 257, 1 << 30):
        assert call(n, None, None, 9, o) == E and b"n_terms must be in 0 .. 256" in err()
    # 3. NULL arrays with n_terms > 0, with a bad mode behind it
    assert call(2, None, g, 9, o) == E and b"is NULL with 2 terms" in err()
    assert call(2, p, None, 9, o) == E and b"is NULL with 2 terms" in err()
    # 4. mode outside 0 .. 1, with bad offsets behind it
    empty = np.array([0, 2, 2], np.uint32)
    for mode in (-1, 2, 64):
        assert call(2, p, empty.ctypes.data, mode, o) == E and b"mode must be" in err()
        assert call(0, None, None, mode, o) == E and b"mode must be" in err()
    # 5. an empty term, offsets that decrease
    for mode in (0, 1):
        assert call(2, p, empty.ctypes.data, mode, o) == E and b"term 1 is empty" in err()
        first_empty = np.array([3, 3, 5], np.uint32)
        assert call(2, p, first_empty.ctypes.data, mode, o) == E and b"term 0 is empty" in err()
        back = np.array([0, 4, 2], np.uint32)
        assert call(2, p, back.ctypes.data, mode, o) == E and b"not monotone at term 1" in err()
        # 6. then the NULL index: 256 terms, two terms, and no terms at all
        assert call(2, p, g, mode, o) == E and b"null index" in err()
        assert call(0, None, None, mode, o) == E and b"null index" in err()
        many = np.arange(257, dtype=np.uint32)
        big = np.full(257, ord("a"), np.uint8)
        assert call(256, big.ctypes.data, many.ctypes.data, mode, o) == E and b"null index" in err()
    assert out.value == 7                                                 # no handle was written
