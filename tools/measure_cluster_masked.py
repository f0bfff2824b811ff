"""python tools/measure_cluster_masked.py [out.txt [repeats]] -- what a masked search over the shards of a cluster
(orr_cluster_search_batch_masked, "mask_screen" = 1 on every shard) costs next to the cluster's scoped search of the same shared
list (orr_cluster_search_batch_scoped, scope_off NULL) and the unscoped orr_cluster_search_batch of the same batch, on ONE
MI355X: two shards of MEASURE_ROWS x MEASURE_DIM each (default 500,000 x 3072) on that one device, int8 shadows built, topk 10,
candidate_limit = rows, a shared scope of S in {30,000, 100,000, 500,000} rows drawn at random over both shards, B in
{1, 8, 256}.  The three calls alternate in one job.  Reported: ms per call (median, min, max over the repeats), the binding
comparison at B = 256, S = 100,000, the overhead over the unscoped cluster call, the count step alone (every shard's
orr_index_scope_count in turn) and the passes per call from the cluster's and the shards' statistics.  Two shards on one GPU
share its HBM and its queues: the figures say nothing about eight GPUs."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft   # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
ROWS = int(os.environ.get("MEASURE_ROWS", 500_000))       # per shard
DIM = int(os.environ.get("MEASURE_DIM", 3072))
SHARDS = 2
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
SCOPES = tuple(int(s) for s in os.environ.get("MEASURE_SCOPES", "30000,100000,500000").split(","))
BATCHES = tuple(int(b) for b in os.environ.get("MEASURE_BATCHES", "1,8,256").split(","))
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
    return "median %.3f  min %.3f  max %.3f ms" % s


def main():
    P = graft.load_package()
    gen = __import__("importlib").import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    total = ROWS * SHARDS
    say("# cluster masked search against the cluster scoped search of the same shared list and the unscoped cluster search;", torch.cuda.get_device_name(0))
    say("# %d shards of %d x %d on ONE device, int8 shadows built, topk 10, candidate_limit = rows, %d repeats, calls alternate" % (SHARDS, ROWS, DIM, REPEATS))
    cl = P.RecallCluster([0] * SHARDS, DIM, capacity_rows_per_shard=ROWS)
    step = 32768
    for g in range(SHARDS):
        sh = cl.shard(g)
        for r0 in range(g * ROWS, (g + 1) * ROWS, step):
            m = min(step, (g + 1) * ROWS - r0)
            pool, off = gen.contents(r0, m, dev)
            sh.append(gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, total, dev), pool, off,
                      row_ids=np.arange(r0, r0 + m, dtype=np.int64))
    del pool, off
    torch.cuda.empty_cache()
    cl.seal()
    shards = [cl.shard(g) for g in range(SHARDS)]
    for sh in shards:
        sh.set_option("two_stage", 1)
        sh.set_option("mask_screen", 1)
    rng = np.random.default_rng(5)
    table = {}
    for B in BATCHES:
        q = gen.query_vectors(0, B, DIM, total).numpy()
        terms = P.PackedTerms(P.pack_terms([P.text.query_terms(t) for t in gen.query_texts(0, B, total)]))
        for S in SCOPES:
            ids = np.sort(rng.choice(total, S, replace=False)).astype(np.int64)
            calls = {
                "masked": lambda: cl.search_masked(q, terms, gen.NOW_TICKS, 10, ids, candidate_limit=total),
                "scoped": lambda: cl.search_scoped(q, terms, gen.NOW_TICKS, 10, ids, candidate_limit=total),
                "unscoped": lambda: cl.search(q, terms, gen.NOW_TICKS, 10, candidate_limit=total),
            }
            for call in calls.values():
                call()
                call()
            got = calls["masked"](), calls["scoped"]()
            same = all(np.array_equal(a, b) for a, b in zip(*got))
            t = {k: [] for k in calls}
            t["count"] = []
            for _ in range(REPEATS):
                for k, call in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    t[k].append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                live = [int(sh.scope_count(ids)[0]) for sh in shards]          # the count step, one shard after the other
                t["count"].append((time.perf_counter() - t0) * 1e3)
            s = {k: stat(v) for k, v in t.items()}
            table[(B, S)] = s
            say("")
            say("B = %d, shared scope of %d rows, %s live per shard (masked == scoped: %s)" % (B, S, live, same))
            for k in calls:
                say("  %-9s" % k, fmt(s[k]))
            say("  %-9s" % "count", fmt(s["count"]), " (every shard's scope_count in turn, from Python)")
            cl.search_stats(reset=True)
            for sh in shards:
                sh.reset_search_stats()
            for _ in range(5):
                calls["masked"]()
            cst = cl.search_stats(reset=True)
            sst = [sh.search_stats(reset=True) for sh in shards]
            say("  masked: cluster passes per call %.1f, requeried per call %.1f; per shard: pass_mode %s, passes per call %s, survivors per query %s" %
                (cst["passes"] / 5, cst["requeried"] / 5, [x["pass_mode"] for x in sst], ["%.1f" % (x["passes"] / 5) for x in sst],
                 [x["survivors_per_query"] and round(x["survivors_per_query"]) for x in sst]))
            say("  masked - unscoped (medians): %.3f ms; scoped / masked: %.1f x" % (s["masked"][0] - s["unscoped"][0], s["scoped"][0] / s["masked"][0]))
            if B == 256 and S == 100_000:
                m, sc = s["masked"], s["scoped"]
                spreads = (m[2] - m[1]) + (sc[2] - sc[1])
                say("  BINDING: scoped median - masked median = %.3f ms against both spreads together %.3f ms: %s; ratio %.1f x" %
                    (sc[0] - m[0], spreads, "met" if sc[0] - m[0] > spreads else "NOT met", sc[0] / m[0]))
    cl.close()


if __name__ == "__main__":
    main()
