"""python tools/measure_scope_terms.py [out.txt [repeats]] -- what a term scope (orr_scope_create_terms) costs to make, on one
MI355X: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072) with the int8 shadow and the token bitmaps
built, "mask_screen" = 1.  Five term lists (one whole word; one 2-byte fragment; 8 words ALL; 8 words ANY; 64 words ANY):
scope_terms per call, median (min-max) over the repeats, the share of scope_terms_combine in the call's kernel statistics, and
beside it orr_scope_create from the same rows' ids in host memory -- the only route a host has without this call, once it has
found the ids by its own means.  Then search_in_scope inside the term scope and inside the id-made scope of the same rows at
B in {1, 256}, topk 10, candidate_limit = rows: the two must return identical arrays in every cell (binding); their times are
reported.

MEASURE_PARENT_ROOT=<a built checkout of the parent commit>: the default `bench.py --gpus 1` run of this build and of that one,
alternating, each a child process of this job on the same device, MEASURE_BENCH_RUNS (default 3) runs each; the medians of
ms_per_step must agree within the two builds' min-max spreads taken together (the search's path is unchanged apart from the
moved cleanup).  The first run that does not end with status 0 and a result line ends the section: no further child is started
and the comparison is reported as not taken."""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = ARGS[0] if ARGS else None
REPEATS = int(ARGS[1]) if len(ARGS) > 1 else 15
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
BENCH_RUNS = int(os.environ.get("MEASURE_BENCH_RUNS", 3))
BATCHES = (1, 256)
FRAG = b"ab"
LINES = []


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    LINES.append(line)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(LINES) + "\n")


def stat(ms):
    a = np.sort(np.asarray(ms))
    return float(np.median(a)), float(a[0]), float(a[-1])


def fmt(s):
    return "%.3f (%.3f-%.3f)" % s


def build(P, gen, dev):
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS)
    step = 32768
    for r0 in range(0, ROWS, step):
        m = min(step, ROWS - r0)
        pool, off = gen.contents(r0, m, dev)
        idx.append(gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, ROWS, dev), pool, off)
    del pool, off
    torch.cuda.empty_cache()
    idx.seal()
    idx.set_option("two_stage", 1)
    idx.set_option("mask_screen", 1)
    return idx


def timed_make(make):
    make().close()
    make().close()
    t = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc = make()
        t.append((time.perf_counter() - t0) * 1e3)
        sc.close()
    return stat(t)


def timed(calls):
    for call in calls.values():
        call()
        call()
    t = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stat(v) for k, v in t.items()}


def bench_once(root):
    """one default bench.py run of the build at `root`, a child process: (ms_per_step, queries/s) or an error text"""
    try:
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"], cwd=root, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        return None, "did not end within 600 s and was stopped"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return None, "exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-300:])
    doc = json.loads(lines[-1])
    return (float(doc["ms_per_step"]), float(doc["value"])), None


def main():
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    say("# term scopes (orr_scope_create_terms): what one costs to make, and a search inside it;", torch.cuda.get_device_name(0))
    say("# shard %d x %d, int8 shadow and token bitmaps built, mask_screen 1, %d repeats; ms, median (min-max)" % (ROWS, DIM, REPEATS))
    idx = build(P, gen, dev)
    q1 = gen.query_vectors(0, 1, DIM, ROWS, dev)
    idx.search(q1, [P.text.query_terms(gen.query_texts(0, 1, ROWS)[0])], gen.NOW_TICKS, 10, candidate_limit=ROWS)   # shadow, token bitmaps
    words = [gen.vocab_word(17 + 61 * i) for i in range(64)]
    frag_hits = sum(FRAG in gen.vocab_word(t) for t in range(gen.VOCAB))
    cases = [("one whole word", words[:1], "all"), ("one 2-byte fragment (%d vocabulary hits)" % frag_hits, [FRAG], "any"),
             ("8 words ALL", words[:8], "all"), ("8 words ANY", words[:8], "any"), ("64 words ANY", words, "any")]
    idx.scope(np.arange(8, dtype=np.int64)).close()                  # (the first id scope builds the id table)
    say("")
    kept = []
    for name, terms, mode in cases:
        t_terms = timed_make(lambda: idx.scope_terms(terms, mode))
        idx.set_profiling(1)
        sc = idx.scope_terms(terms, mode)
        st = idx.kernel_stats()
        idx.set_profiling(0)
        total = sum(v["total_ms"] for v in st.values())
        comb = st.get("scope_terms_combine", {"total_ms": 0.0, "algo_bytes": 0.0})
        aliased = st.get("scope_terms_aliased", {"algo_bytes": 0.0})["algo_bytes"]
        ids = sc.row_ids()
        t_ids = timed_make(lambda: idx.scope(ids))
        sc_ids = idx.scope(ids)
        same = sc_ids.rows == sc.rows and np.array_equal(sc_ids.row_ids(), ids)
        say("%-44s %9d rows | scope_terms %s | scope_terms_combine %.4f ms = %4.1f %% of %.4f ms of kernels, %.2f MB read and written, %.2f MB of it stored token bitmaps"
            " | orr_scope_create from the %d ids in host memory %s | same rows: %s"
            % (name + " (" + mode.upper() + ")", sc.rows, fmt(t_terms), comb["total_ms"], 100.0 * comb["total_ms"] / max(total, 1e-9), total,
               comb["algo_bytes"] / 1e6, aliased / 1e6, len(ids), fmt(t_ids), same))
        kept.append((name, sc, sc_ids))
    say("")
    all_same = True
    for B in BATCHES:
        q = gen.query_vectors(0, B, DIM, ROWS, dev)
        terms = P.PackedTerms(P.pack_terms([P.text.query_terms(t) for t in gen.query_texts(0, B, ROWS)]))
        for name, sc, sc_ids in kept:
            calls = {"term scope": lambda: idx.search_in_scope(q, terms, gen.NOW_TICKS, 10, sc, candidate_limit=ROWS),
                     "id scope": lambda: idx.search_in_scope(q, terms, gen.NOW_TICKS, 10, sc_ids, candidate_limit=ROWS)}
            s = timed(calls)
            a, b = calls["term scope"](), calls["id scope"]()
            same = all(np.array_equal(x, y) for x, y in zip(a, b))
            all_same = all_same and same
            say("B = %3d, %-44s search_in_scope: term scope %s | id scope of the same rows %s | identical arrays: %s (pass_mode %d)"
                % (B, name, fmt(s["term scope"]), fmt(s["id scope"]), same, idx.search_stats()["pass_mode"]))
    say("BINDING: the term scope and the id scope return identical arrays in every cell: %s" % ("met" if all_same else "NOT met"))
    for _, sc, sc_ids in kept:
        sc.close()
        sc_ids.close()
    idx.close()
    del idx
    torch.cuda.empty_cache()
    parent = os.environ.get("MEASURE_PARENT_ROOT")
    if parent:
        say("")
        say("# the default bench.py run (--gpus 1) of this build and of a build of the parent commit, alternating, %d runs each, every run a child process of this job on this device" % BENCH_RUNS)
        got = {"this build": [], "parent build": []}
        failed = False
        for i in range(BENCH_RUNS):
            for name, root in (("this build", ROOT), ("parent build", os.path.abspath(parent))):
                r, err = bench_once(root)
                if err:                                              # a child that failed, faulted or hung: nothing more starts on this device
                    say("%-12s run %d: %s" % (name, i + 1, err))
                    failed = True
                    break
                got[name].append(r)
                say("%-12s run %d: %.4f ms per step, %.0f queries/s" % (name, i + 1, r[0], r[1]))
            if failed:
                break
        if failed:
            say("BINDING: not taken -- a bench run did not end with status 0 and a result line; no further run was started")
        else:
            a, b = stat([r[0] for r in got["this build"]]), stat([r[0] for r in got["parent build"]])
            spreads = (a[2] - a[1]) + (b[2] - b[1])
            say("this build   ms per step %s" % fmt(a))
            say("parent build ms per step %s" % fmt(b))
            say("BINDING: |median - median| = %.4f ms against both spreads together %.4f ms: %s"
                % (abs(a[0] - b[0]), spreads, "met" if abs(a[0] - b[0]) <= spreads else "NOT met"))
    say("")
    say("not taken: the figures on a 10M-row shard, and on a large real-text vocabulary.")


if __name__ == "__main__":
    main()
