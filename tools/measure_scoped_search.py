"""python tools/measure_scoped_search.py [out.txt [repeats]] -- what a scoped search (orr_search_batch_scoped) costs next to the unscoped
orr_search_batch of the same batch, on one MI355X: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072;
10,000,000 where the job allows) with the int8 shadow built, B in {1, 256}, per-query scopes of 300, 3,000 and 30,000 rows
drawn as runs of 30 consecutive rows (documents).  Every scoped call alternates with the unscoped call in the same job; the
unscoped path does not change with this feature, so it stands for the code before it.  Reported: ms per call (median, min,
max over the repeats), per-kernel time (orr_index_kernel_stats), the re-score's achieved bytes per second (pairs x 4 x dim over
its kernel time), and the id table's build time and bytes."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft   # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
RESCORE = ("finish_survivors", "rescore_buffer_exact", "scope_rescore")
LINES = []


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    LINES.append(line)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(LINES) + "\n")


def spread(ms):
    a = np.sort(np.asarray(ms))
    return "median %.3f  min %.3f  max %.3f ms" % (float(np.median(a)), float(a[0]), float(a[-1]))


def main():
    P = graft.load_package()
    gen = __import__("importlib").import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    say("# scoped search against the unscoped search of the same batch;", torch.cuda.get_device_name(0))
    say("# shard %d x %d, int8 shadow built, topk 10, candidate_limit = rows, %d repeats, calls alternate" % (ROWS, DIM, REPEATS))
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
    rng = np.random.default_rng(5)

    # the id table: built by the first scoped search
    idx.set_profiling(1)
    t0 = time.perf_counter()
    idx.search_scoped(gen.query_vectors(0, 1, DIM, ROWS, dev), [[b"alpha"]], gen.NOW_TICKS, 10, np.arange(30, dtype=np.int64), candidate_limit=ROWS)
    first = time.perf_counter() - t0
    tab = idx.kernel_stats().get("scope_id_table")
    idx.set_profiling(0)
    say("id table: build %.2f ms (first scoped call %.2f ms in all), %.1f MB = 12 bytes per row" %
        (tab["total_ms"], first * 1e3, tab["algo_bytes"] / 1e6))

    for B in (1, 256):
        q = gen.query_vectors(0, B, DIM, ROWS, dev)
        terms = P.PackedTerms(P.pack_terms([P.text.query_terms(t) for t in gen.query_texts(0, B, ROWS)]))
        for _ in range(3):
            idx.search(q, terms, gen.NOW_TICKS, 10, candidate_limit=ROWS)
        for scope_rows in (300, 3000, 30000):
            runs = scope_rows // 30
            ids = np.concatenate([(rng.choice(ROWS // 30, runs, replace=False)[:, None] * 30 + np.arange(30)[None, :]).ravel() for _ in range(B)]).astype(np.int64)
            off = (np.arange(B + 1, dtype=np.uint64) * np.uint64(scope_rows))
            ids_dev = torch.from_numpy(ids).to(dev)
            for _ in range(2):
                idx.search_scoped(q, terms, gen.NOW_TICKS, 10, ids_dev, candidate_limit=ROWS, scope_off=off)
            t_scoped, t_plain = [], []
            for _ in range(REPEATS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                idx.search_scoped(q, terms, gen.NOW_TICKS, 10, ids_dev, candidate_limit=ROWS, scope_off=off)
                t_scoped.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                idx.search(q, terms, gen.NOW_TICKS, 10, candidate_limit=ROWS)
                t_plain.append((time.perf_counter() - t0) * 1e3)
            say("")
            say("B = %d, %d scoped rows per query (%d pairs)" % (B, scope_rows, B * scope_rows))
            say("  scoped    ", spread(t_scoped))
            say("  unscoped  ", spread(t_plain), "  (spread of the unscoped call: %.3f ms)" % (max(t_plain) - min(t_plain)))
            for label, call in (("unscoped", lambda: idx.search(q, terms, gen.NOW_TICKS, 10, candidate_limit=ROWS)),
                                ("scoped", lambda: idx.search_scoped(q, terms, gen.NOW_TICKS, 10, ids_dev, candidate_limit=ROWS, scope_off=off))):
                idx.set_profiling(1)
                for _ in range(5):
                    call()
                stats = idx.kernel_stats()
                idx.set_profiling(0)
                say("  kernels of the %s call (us per call): " % label +
                    ", ".join("%s %.1f" % (k, v["total_ms"] / 5 * 1e3) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"]) if v["launches"]))
                if label == "scoped":
                    ms = sum(v["total_ms"] for k, v in stats.items() if k in RESCORE) / 5
                    if ms > 0:
                        say("  re-score: %d pairs x %d B in %.1f us = %.2f TB/s" % (B * scope_rows, 4 * DIM, ms * 1e3, B * scope_rows * 4.0 * DIM / (ms * 1e-3) / 1e12))
            st = idx.search_stats(reset=True)
            say("  pass_mode after the last call %d, exact_pass_queries %d, buffer_growths %d" % (st["pass_mode"], st["exact_pass_queries"], st["buffer_growths"]))
    idx.close()


if __name__ == "__main__":
    main()
