"""CPU checks of the keyword chain's host half (csrc/orr_keyword_plan.h): its selftest -- the distinct terms against a std::map,
the image against one built byte by byte, the lookup tables, the choices and the hit list's rule at their edges -- and that the
driver is made of the header: launch_keyword_side a list of stages without a closure, the overflow rule, the attempt cap and the
bitmap width stated once.  No GPU (the method of tests/test_per_key_cpu.py).  The chain at work is in
tests/test_gpu_keyword_chain.py."""
import os
import re
import subprocess

from helpers import ROOT

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_keyword_plan_selftest")


def run_selftest():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_keyword_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_keyword_plan_selftest: ok"
    return r.stdout


def test_keyword_plan_selftest_passes():
    out = run_selftest()
    m = re.search(r"exhaustive term lists checked: (\d+)", out)
    assert m and int(m.group(1)) == 1093, out                             # every list of 0 .. 6 terms over three: (3^7 - 1) / 2
    m = re.search(r"random batches checked: (\d+) \(repeated terms: (\d+)\)", out)
    assert m and int(m.group(1)) >= 50 and int(m.group(2)) > 10000, out
    m = re.search(r"images compared: (\d+) \((\d+) bytes\)", out)
    assert m and int(m.group(1)) == 10 and int(m.group(2)) > 1000000, out  # two forms x TT of 1, 63, 64, 65 and 3,000
    m = re.search(r"lookup tables checked: (\d+)", out)
    assert m and int(m.group(1)) >= 5, out
    m = re.search(r"forced x env combinations checked: (\d+)", out)
    assert m and int(m.group(1)) == 9, out


def _body(api, name):
    """The text of function `name` of orr_api.hip: from its definition to the first closing brace in column 0."""
    m = re.search(r"^(?:static )?int %s\([^;{]*\)\n\{\n" % name, api, flags=re.M)
    assert m, name
    return api[m.end():].split("\n}\n")[0]


def test_the_driver_is_made_of_the_header():
    header = open(os.path.join(CSRC, "orr_keyword_plan.h")).read()
    kernels_h = open(os.path.join(CSRC, "orr_kernels.h")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_keyword_plan_selftest.cpp")).read()
    assert "hip/hip_runtime.h" not in header and "namespace keyword" in header
    for name in ("words_per_term", "table_size", "distinct_terms", "layout_of", "fill_meta", "short_form", "mid_tokens", "hit_list", "after_run"):
        assert len(re.findall(r"^inline [\w:]+ %s\(" % name, header, flags=re.M)) == 1, name
        assert re.search(r"\b%s\(" % name, selftest), name
    for name in ("distinct_terms", "layout_of", "fill_meta", "short_form", "mid_tokens", "hit_list", "after_run", "words_per_term", "kMaxRuns"):
        assert "keyword::" + name in api, name
    # the structs and the Bloom hash live in the header alone, still in namespace orr; the kernels' header includes it
    for name in ("struct ScanTerm {", "struct MatchTerm {", "struct MatchTerm8 {", "constexpr int kVocabBloomBits", "inline uint32_t vocab_bloom_hash("):
        assert header.count(name) == 1 and name not in kernels_h, name
    assert '#include "orr_keyword_plan.h"' in kernels_h
    assert re.search(r"#if defined\(__HIPCC__\)\n__host__ __device__\n#endif\ninline uint32_t vocab_bloom_hash\(", header)
    assert "static_assert(sizeof(KwHit) == keyword::kHitBytes" in kernels_h
    # launch_keyword_side: the stages in their order, no closure, no getenv
    body = _body(api, "launch_keyword_side")
    stages = ("kw_plan_and_fill(", "kw_reserve(", "kw_upload(", "kw_match_short(", "kw_match_long(", "kw_alias(", "kw_settle_bitmaps(", "kw_expand(",
              "hipEventRecord(idx->ev_kw_done")
    at = [body.index(s) for s in stages]
    assert at == sorted(at) and all(body.count(s) == 1 for s in stages)
    assert "[&]" not in body and "[=]" not in body and "[]" not in body and "getenv" not in body
    assert body.index("n_terms_total == 0) return ORR_OK;") < at[0]       # ... before any voucher is touched
    for name in stages[:-1]:
        stage = _body(api, name[:-1])
        assert "[&]" not in stage and "[=]" not in stage, name
    # the vouchers: one struct, withdrawn behind the bitmaps' reserve, granted by the one cleanup
    reserve = _body(api, "kw_reserve")
    assert reserve.index("ws_bitmaps.reserve(") < reserve.index("kw_clean.withdraw()") < reserve.index("ws_hits.reserve(")
    upload = _body(api, "kw_upload")
    assert upload.index("pin_kwcnt.as<unsigned long long>() = 0ull") < upload.index("hipMemcpyAsync(")
    assert api.count("kw_clean.withdraw()") == 1 and api.count("kw_clean.withdraw_bitmaps()") == 2      # compaction, insertion
    for gone in ("bitmaps_clean_of", "bm_clean_pending", "kw_counters_clean", "kw_counters_of"):
        assert gone not in api, gone
    # one rule, one cap, one width
    csrc_text = {}
    for dirpath, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".h", ".hip", ".cpp", ".inc")) and "selftest" not in f:
                csrc_text[f] = open(os.path.join(dirpath, f)).read()
    assert [f for f, t in csrc_text.items() if "hits / 4 + 1024" in t] == ["orr_keyword_plan.h"] and header.count("hits / 4 + 1024") == 1
    assert [f for f, t in csrc_text.items() if re.search(r"8 << 30\)\).*KwHit|KwHit.*8 << 30", t)] == ["orr_keyword_plan.h"]
    assert "attempt >= 3" not in api and api.count("keyword::kMaxRuns") == 3                             # retry_pass and the two loops
    assert "+ 31) / 32 + 3) / 4 * 4" not in api and header.count("+ 31) / 32 + 3) / 4 * 4") == 1
    assert api.count("keyword::after_run(") == 1 and api.count("check_hit_list(") == 4                   # its definition and three callers
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_keyword_plan_selftest" in makefile.split("all:")[0]                                 # in SELFTEST: build() makes it
    assert "orr_keyword_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]
    assert "host/orr_keyword_plan_selftest: host/orr_keyword_plan_selftest.cpp orr_keyword_plan.h" in makefile
