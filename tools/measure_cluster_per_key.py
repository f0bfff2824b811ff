"""python tools/measure_cluster_per_key.py [out.txt [repeats]] -- what the per-key search over a cluster
(orr_cluster_search_batch_per_key) costs, on ONE MI355X in one process: a synthetic cluster of MEASURE_SHARDS x MEASURE_ROWS x
MEASURE_DIM (default 3 x 200,000 x 1024, every shard on device 0) and ONE index over the same rows, keys in runs of 40 rows,
topk 10, pool 24, max_per_key 1, B = 1 / 8 / 64 / 256 hybrid queries in host memory, two warm calls first, REPEATS (default 15)
alternating repeats, ms, median (min-max).

Two families.  "spread": the keys as they lie -- nearly every query finishes in round 1.  "concentrated": a second key column in
which every query's best 24 rows (its whole pool) share one key and its next 24 another, so the call needs three rounds.

Reported without a threshold, per family and B: the cluster call; orr_cluster_search_batch with topk = pool on the same cluster
(round 1 alone); the single index's orr_search_batch_per_key on the same rows and keys; the rounds the queries took; and from the
shards' kernel statistics, in repeats of their own with profiling on, the keys_exclude and keys_gather launches and times of every
shard.  Nobody has measured what a cluster round costs: the figures are what the next change is judged against."""
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
BATCHES = tuple(int(b) for b in os.environ.get("MEASURE_B", "1,8,64,256").split(","))
POOL, TOPK, CAP, RUN = 24, 10, 1, 40
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


def alternating(calls):
    """every call twice warm, then REPEATS rounds in which each call runs once, in turn; per call its times in ms"""
    import torch
    for c in calls:
        c()
        c()
    t = [[] for _ in calls]
    for _ in range(REPEATS):
        for i, c in enumerate(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c()                                           # (every call ends in a stream synchronise of its own)
            t[i].append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    total = SHARDS * ROWS
    cl = P.RecallCluster([0] * SHARDS, DIM, capacity_rows_per_shard=ROWS)
    one = P.RecallIndex(dim=DIM, capacity_rows=total)
    step = 32768
    for g in range(SHARDS):
        sh = cl.shard(g)
        for r0 in range(g * ROWS, (g + 1) * ROWS, step):
            m = min(step, (g + 1) * ROWS - r0)
            pool, off = gen.contents(r0, m, dev)
            rows = (gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, total, dev), pool, off)
            ids = torch.arange(r0, r0 + m, dtype=torch.int64, device=dev)
            sh.append(*rows, row_ids=ids)
            one.append(*rows, row_ids=ids)
    del pool, off, rows
    torch.cuda.empty_cache()
    cl.seal()
    one.seal()
    bmax = max(BATCHES)
    q = gen.query_vectors(0, bmax, DIM, total).numpy()
    terms = [P.text.query_terms(t) for t in gen.query_texts(0, bmax, total)]
    ids = np.arange(total, dtype=np.int64)
    spread = ids // RUN
    # the concentrated column: per query (the last query first, so that query 0's plant is whole) its pool one key, the next pool another
    top = one.search(q, terms, gen.NOW_TICKS, 2 * POOL, candidate_limit=total)[0]
    dense = spread.copy()
    for b in range(bmax - 1, -1, -1):
        first, second = top[b, :POOL], top[b, POOL:]
        dense[first[first >= 0]] = 10 ** 9 + 2 * b
        dense[second[second >= 0]] = 10 ** 9 + 2 * b + 1
    columns = {"spread": (cl.keys(ids, spread), one.keys(ids, spread)), "concentrated": (cl.keys(ids, dense), one.keys(ids, dense))}
    shards = [cl.shard(g) for g in range(SHARDS)]
    say("# per-key search over a cluster (orr_cluster_search_batch_per_key) on ONE MI355X, one process")
    say("# cluster %d x %d x %d (every shard on device 0) and one index of %d rows, keys in runs of %d, topk %d, pool %d, max_per_key %d, "
        "hybrid queries in host memory, %d alternating repeats; ms, median (min-max)" % (SHARDS, ROWS, DIM, total, RUN, TOPK, POOL, CAP, REPEATS))
    for family, (ckh, kh) in columns.items():
        for B in BATCHES:
            qb, tb = q[:B], terms[:B]
            plain = lambda: cl.search(qb, tb, gen.NOW_TICKS, POOL, candidate_limit=total)
            clus = lambda: cl.search_per_key(qb, tb, gen.NOW_TICKS, TOPK, ckh, max_per_key=CAP, pool=POOL, candidate_limit=total)
            single = lambda: one.search_per_key(qb, tb, gen.NOW_TICKS, TOPK, kh, max_per_key=CAP, pool=POOL, candidate_limit=total)
            t_plain, t_clus, t_single = (stat(t) for t in alternating((plain, clus, single)))
            got, want = clus(), single()
            same = all(np.array_equal(got[i], want[i]) for i in (0, 2, 3, 4)) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
            rounds = np.bincount(got[4], minlength=4)[1:]
            ex_ms, ga_ms = [[] for _ in shards], [[] for _ in shards]
            for _ in range(REPEATS):
                for sh in shards:
                    sh.set_profiling(1)
                clus()
                sts = [sh.kernel_stats() for sh in shards]
                for sh in shards:
                    sh.set_profiling(0)
                for g, st in enumerate(sts):
                    ex_ms[g].append(st["keys_exclude"]["total_ms"] if "keys_exclude" in st else 0.0)
                    ga_ms[g].append(st["keys_gather"]["total_ms"] if "keys_gather" in st else 0.0)
            n_ex = [st["keys_exclude"]["launches"] if "keys_exclude" in st else 0 for st in sts]
            n_ga = [st["keys_gather"]["launches"] if "keys_gather" in st else 0 for st in sts]
            say("%-12s B %-3d cluster per-key %s | cluster search, topk = pool %s | difference %.3f | one index, per-key %s | rounds 1/2/3+ %s | equal to the one index: %s"
                % (family, B, fmt(t_clus), fmt(t_plain), t_clus[0] - t_plain[0], fmt(t_single), "/".join(str(int(r)) for r in (rounds[0], rounds[1], rounds[2:].sum())), same))
            say("%-12s B %-3d   per shard: keys_exclude %s in %s launches | keys_gather %s in %s launches"
                % (family, B, "; ".join(fmt(stat(t)) for t in ex_ms), "/".join(map(str, n_ex)), "; ".join(fmt(stat(t)) for t in ga_ms), "/".join(map(str, n_ga))))
    for ckh, kh in columns.values():
        ckh.close()
        kh.close()
    cl.close()
    one.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
