"""CPU checks of the keyword chain's diagnostic (orr_index_keyword_bitmaps): declared, exported, bound and documented, and every
argument error answered with ORR_EINVAL before any HIP call and before the index handle is looked at -- so on a machine without
a GPU (the method of tests/test_scope_terms_cpu.py).  The chain at work is in tests/test_gpu_keyword_chain.py."""
import ctypes as C
import os
import re

import numpy as np

from helpers import ROOT, pkg

NAME = "orr_index_keyword_bitmaps"


def test_entry_point_is_declared_exported_bound_and_documented():
    P = pkg()
    txt = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % NAME, decl)
    assert m, NAME
    assert len(m.group(1).split(",")) == 10, m.group(1)
    assert "deleted rows are NOT cleared" in " ".join(txt.split())        # the header says that the bits are raw
    assert NAME in P.native.EXPORTED_HIP_SYMBOLS
    f = getattr(P.native.hip, NAME)                                      # (the library exports it: ctypes resolved the symbol)
    assert f.restype is C.c_int and len(f.argtypes) == 10
    assert P.native.hip.orr_abi_version() == 1                            # adding a function is compatible
    assert callable(P.RecallIndex.keyword_bitmaps)
    for doc in ("DESIGN.md", "ADVICE.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
    # the two overrides are per-call state read ahead of the environment switches, which stay
    api = open(os.path.join(ROOT, "omni-recall-rag_amd", "csrc", "orr_api.hip")).read()
    assert 'getenv("ORR_VOCAB_LOOKUP")' in api and 'getenv("ORR_VOCAB_MID")' in api
    # (the precedence itself is keyword::short_form's and keyword::mid_tokens': the driver hands them the override, then the
    # environment's value, and the plan's selftest goes through all nine combinations of the two)
    assert re.search(r"keyword::short_form\([^;]*, idx->kw_force_form, kw_env\(\)\.lookup\);", api)
    assert re.search(r"keyword::mid_tokens\([^;]*, idx->kw_force_mid, kw_env\(\)\.mid_off\);", api)
    from test_keyword_plan_cpu import run_selftest
    assert "forced x env combinations checked: 9" in run_selftest()


def test_argument_errors_before_any_device_call():
    """Every case passes a NULL index: the value errors are reported all the same, each case holding exactly one error more than
    the one in front of it, so the order is pinned.  ORR_ESTATE for an unsealed index needs a real handle: the GPU file."""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    pool = np.frombuffer(b"abcdeab\0", np.uint8).copy()
    good = np.array([0, 2, 5], np.uint32)                                 # "ab", "cde"
    bitmaps = np.full(64, 0xABABABAB, np.uint32)
    alias = np.full(4, 7, np.uint8)
    info = np.full(4, -5, np.int64)
    p, g, bm, al, nf = pool.ctypes.data, good.ctypes.data, bitmaps.ctypes.data, alias.ctypes.data, info.ctypes.data

    def call(n, terms, off, form, mid, out_bm=bm, out_info=nf):
        r = h.orr_index_keyword_bitmaps(None, n, terms, off, form, mid, 4, out_bm, al, out_info)
        assert NAME.encode() in err()
        return r

    # 1. an output missing wins over everything behind it
    assert call(-1, None, None, 9, 9, out_bm=None) == E and b"is NULL" in err()
    assert call(2, p, g, 0, -1, out_info=None) == E and b"is NULL" in err()
    # 2. the number of terms: 1 .. 4096
    for n in (-1, 0, 4097, 1 << 30):
        assert call(n, None, None, 9, 9) == E and b"n_terms must be in 1 .. 4096" in err()
    # 3. NULL arrays
    assert call(2, None, g, 9, 9) == E and b"is NULL" in err()
    assert call(2, p, None, 9, 9) == E and b"is NULL" in err()
    # 4. form outside -1 .. 1, then mid outside -1 .. 0, with bad offsets behind them
    empty = np.array([0, 2, 2], np.uint32)
    for form in (-2, 2, 64):
        assert call(2, p, empty.ctypes.data, form, 9) == E and b"form must be" in err()
    for mid in (-2, 1, 64):
        for form in (-1, 0, 1):
            assert call(2, p, empty.ctypes.data, form, mid) == E and b"mid must be" in err()
    for form in (-1, 0, 1):
        for mid in (-1, 0):
            # 5. an empty term, offsets that decrease
            assert call(2, p, empty.ctypes.data, form, mid) == E and b"term 1 is empty" in err()
            first_empty = np.array([3, 3, 5], np.uint32)
            assert call(2, p, first_empty.ctypes.data, form, mid) == E and b"term 0 is empty" in err()
            back = np.array([0, 4, 2], np.uint32)
            assert call(2, p, back.ctypes.data, form, mid) == E and b"not monotone at term 1" in err()
            # 6. a term given twice: "ab", "cde", "ab"
            twice = np.array([0, 2, 5, 7], np.uint32)
            assert call(3, p, twice.ctypes.data, form, mid) == E and b"not distinct" in err()
            # 7. then the NULL index: two terms, one term, 4096 terms
            assert call(2, p, g, form, mid) == E and b"null index" in err()
            assert call(1, p, g, form, mid) == E and b"null index" in err()
    many = np.arange(4097, dtype=np.uint32) * 2
    big = np.frombuffer(b"".join(b"%c%c" % (97 + i // 64, 48 + i % 64) for i in range(4096)) + b"\0", np.uint8).copy()
    assert call(4096, big.ctypes.data, many.ctypes.data, -1, -1) == E and b"null index" in err()
    assert (bitmaps == 0xABABABAB).all() and (alias == 7).all() and (info == -5).all()     # nothing was written
