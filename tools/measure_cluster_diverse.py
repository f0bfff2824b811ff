"""python tools/measure_cluster_diverse.py [out.txt [repeats]] -- what the diverse search over a cluster
(orr_cluster_search_batch_diverse) costs beside the pool alone, on ONE MI355X in one process: a synthetic cluster of
MEASURE_SHARDS x MEASURE_ROWS x MEASURE_DIM (default 3 x 200,000 x 1024, every shard on device 0), B = MEASURE_B (default 64)
hybrid queries in host memory, topk 10, pool 56, two warm calls first, REPEATS (default 15) repeats, ms, median (min-max).

Reported without a threshold, for collapse at max_cosine 0.95 and MMR at lambda 0.7: the whole call; orr_cluster_search_batch
with topk = 56 on the same cluster (the pool alone: the difference is the price of diversification); from the shards' kernel
statistics, in repeats of their own with profiling on, the rows_gather and pair_dots launches and their times, summed over the
shards; the rows that moved and the bytes that crossed the host (each moved row goes down to pinned memory and up again:
2 x rows x dim x 4).  The claim the numbers are for: the added time is the transport's and the host's, not the kernels'."""
import importlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = ARGS[0] if ARGS and ARGS[0] != "-" else None
REPEATS = int(ARGS[1]) if len(ARGS) > 1 else 15
SHARDS = int(os.environ.get("MEASURE_SHARDS", 3))
ROWS = int(os.environ.get("MEASURE_ROWS", 200_000))
DIM = int(os.environ.get("MEASURE_DIM", 1024))
B = int(os.environ.get("MEASURE_B", 64))
POOL, TOPK = 56, 10
MODES = (("collapse", 0.95), ("mmr", 0.7))
LINES = []


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    LINES.append(line)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(LINES) + "\n")


def stat(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return float(np.median(a)), float(a[0]), float(a[-1])


def fmt(s):
    return "%.3f (%.3f-%.3f)" % tuple(s)


def timed(call):
    import torch
    call()
    call()
    t = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()                                            # (every cluster call ends in a stream synchronise of its own)
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    total = SHARDS * ROWS
    cl = P.RecallCluster([0] * SHARDS, DIM, capacity_rows_per_shard=ROWS)
    step = 32768
    for g in range(SHARDS):
        sh = cl.shard(g)
        for r0 in range(g * ROWS, (g + 1) * ROWS, step):
            m = min(step, (g + 1) * ROWS - r0)
            pool, off = gen.contents(r0, m, dev)
            sh.append(gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, total, dev), pool, off,
                      row_ids=torch.arange(r0, r0 + m, dtype=torch.int64, device=dev))
    del pool, off
    torch.cuda.empty_cache()
    cl.seal()
    q = gen.query_vectors(0, B, DIM, total).numpy()
    terms = [P.text.query_terms(t) for t in gen.query_texts(0, B, total)]
    shards = [cl.shard(g) for g in range(SHARDS)]
    say("# diverse search over a cluster (orr_cluster_search_batch_diverse) on ONE MI355X, one process")
    say("# cluster %d x %d x %d (every shard on device 0), %d hybrid queries in host memory, topk %d, pool %d, %d repeats; ms, median (min-max)"
        % (SHARDS, ROWS, DIM, B, TOPK, POOL, REPEATS))
    plain = stat(timed(lambda: cl.search(q, terms, gen.NOW_TICKS, POOL, candidate_limit=total)))
    say("orr_cluster_search_batch, topk = %d (the pool alone): %s" % (POOL, fmt(plain)))
    for mode, param in MODES:
        call = lambda: cl.search_diverse(q, terms, gen.NOW_TICKS, TOPK, POOL, mode=mode, param=param, candidate_limit=total)
        whole = stat(timed(call))
        gather_ms, pair_ms = [], []
        for _ in range(REPEATS):
            for sh in shards:
                sh.set_profiling(1)
            got = call()
            sts = [sh.kernel_stats() for sh in shards]
            for sh in shards:
                sh.set_profiling(0)
            gather_ms.append(sum(st["rows_gather"]["total_ms"] for st in sts if "rows_gather" in st))
            pair_ms.append(sum(st["pair_dots"]["total_ms"] for st in sts if "pair_dots" in st))
        n_gather = sum(st["rows_gather"]["launches"] for st in sts if "rows_gather" in st)
        n_pair = sum(st["pair_dots"]["launches"] for st in sts if "pair_dots" in st)
        moved = sum(st["rows_gather"]["algo_bytes"] for st in sts if "rows_gather" in st) / (8.0 * DIM)
        say("%-8s %-4s whole call %s | difference to the pool alone %.3f | rows_gather %s in %d launches over the shards | pair_dots %s in %d launches "
            "| both kernels %.3f | %d rows moved of %d pool members (bound %d), %.2f MB across the host (down and up) | %.1f rows kept per query"
            % (mode, param, fmt(whole), whole[0] - plain[0], fmt(stat(gather_ms)), n_gather, fmt(stat(pair_ms)), n_pair,
               stat(gather_ms)[0] + stat(pair_ms)[0], int(moved), B * POOL, B * (POOL - -(-POOL // SHARDS)), 2.0 * moved * DIM * 4 / 1e6,
               float(np.mean(got[2]))))
    cl.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
