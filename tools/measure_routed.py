"""python tools/measure_routed.py [out.txt [repeats]] -- what the routed search costs (orr_search_batch_routed), on ONE MI355X in
one job: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072), keys in runs of 40 rows (key = position //
40: 25,000 documents), docs from orr_keys_centroid_index, route 10, topk 10, candidate_limit 300; B = 64 distinct queries and
B = 256 with repeated routes (32 vectors x 8); two warm calls first, REPEATS (default 11) repeats with the timed calls
alternating, host clock, median (min-max) in ms.

Timed calls: (a) `search_routed`; (b) the twin route composed by the host through the C ABI: ONE batched search of docs, one
`scope_keys` per query, `search_in_scopes` in slices of 64 scopes, the scopes destroyed.  The answers' bits are compared first.
The one condition: (a)'s median lies below (b)'s; the tool says which it is.  From one profiled call of each: keys_include's
device time beside (b)'s keys_member launches, and the bytes per second of keys_include's algorithmic traffic."""
import importlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

ARGS = sys.argv[1:]
OUT = ARGS[0] if ARGS and ARGS[0] != "-" else None
REPEATS = int(ARGS[1]) if len(ARGS) > 1 else 11
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
RUN, ROUTE, TOPK, LIMIT = 40, 10, 10, 300
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


def main():
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS)
    step = 32768
    for r0 in range(0, ROWS, step):
        m = min(step, ROWS - r0)
        pool, off = gen.contents(r0, m, dev)
        idx.append(gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, ROWS, dev), pool, off)
    del pool, off
    torch.cuda.empty_cache()
    idx.seal()
    ids = torch.arange(ROWS, dtype=torch.int64, device=dev)
    whole = idx.scope_ticks(-(1 << 62), 1 << 62)
    order = whole.row_ids()                              # candidate order: key = position // RUN
    whole.close()
    keys = torch.empty(ROWS, dtype=torch.int64, device=dev)
    keys[torch.from_numpy(order).to(dev)] = torch.arange(ROWS, dtype=torch.int64, device=dev) // RUN
    hk = idx.keys(ids, keys)
    docs = hk.centroid_index()
    n_docs = docs.rows
    now = gen.NOW_TICKS
    q_all = gen.query_vectors(0, 64, DIM, ROWS).numpy()
    t_all = [P.text.query_terms(t) for t in gen.query_texts(0, 64, ROWS)]
    batches = {"B = 64, distinct": (np.ascontiguousarray(q_all), t_all),
               "B = 256, 32 vectors x 8": (np.ascontiguousarray(np.tile(q_all[:32], (8, 1))), t_all[:32] * 8)}

    def routed(q, terms):
        return idx.search_routed(docs, hk, q, terms, now, TOPK, ROUTE, candidate_limit=LIMIT)

    def host(q, terms):
        B = len(terms)
        r = docs.search(q, terms, now, ROUTE, candidate_limit=max(1, n_docs))
        rows, scores, counts = np.full((B, TOPK), -1, np.int64), np.zeros((B, TOPK)), np.zeros(B, np.int32)
        for b0 in range(0, B, 64):
            b1 = min(B, b0 + 64)
            scopes = [idx.scope_keys(hk, r[0][b, :r[2][b]]) for b in range(b0, b1)]
            got = idx.search_in_scopes(q[b0:b1], terms[b0:b1], now, TOPK, scopes, np.arange(b1 - b0, dtype=np.int32), candidate_limit=LIMIT)
            rows[b0:b1], scores[b0:b1], counts[b0:b1] = got
            for sc in scopes:
                sc.close()
        return rows, scores, counts, r[0], r[2]

    say("# routed search on ONE MI355X, one job: shard %d x %d, keys in runs of %d (%d documents), route %d, topk %d, candidate_limit %d, "
        "%d alternating repeats; host clock, ms, median (min-max)" % (ROWS, DIM, RUN, n_docs, ROUTE, TOPK, LIMIT, REPEATS))
    for name, (q, terms) in batches.items():
        a, b = routed(q, terms), host(q, terms)
        same = (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64)) and np.array_equal(a[2], b[2])
                and np.array_equal(a[4], b[4]) and all(np.array_equal(a[3][i, :a[4][i]], b[3][i, :b[4][i]]) for i in range(len(terms))))
        say("%s: the two routes' answers are the same bits: %s; distinct routes: %d" % (name, same, len({tuple(sorted(x)) for x in a[3].tolist()})))
        calls = {"search_routed (a)": routed, "host route (b)": host}
        for c in calls.values():
            c(q, terms)
        ms = {k: [] for k in calls}
        for _ in range(REPEATS):
            for k, c in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c(q, terms)
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for k in calls:
            say("%s: %-18s %s" % (name, k, fmt(stat(ms[k]))))
        sa, sb = stat(ms["search_routed (a)"]), stat(ms["host route (b)"])
        say("%s: the condition, (a)'s median below (b)'s: %s (%.3f against %.3f, %.2f x)"
            % (name, "HOLDS" if sa[0] < sb[0] else "DOES NOT HOLD", sa[0], sb[0], sb[0] / sa[0]))
        st = {}
        for k, c in calls.items():
            idx.set_profiling(1)
            c(q, terms)
            st[k] = idx.kernel_stats()
            idx.set_profiling(0)
            say("%s: %s, kernels on the chunk index: " % (name, k)
                + ", ".join("%s %.3f ms in %d" % (n, v["total_ms"], v["launches"]) for n, v in sorted(st[k].items())))
        ki, km = st["search_routed (a)"].get("keys_include"), st["host route (b)"].get("keys_member")
        if ki and km:
            say("%s: keys_include %.3f ms in %d launch(es), %.1f MB of algorithmic traffic (the key column and every word of the slots' "
                "bitmaps; the base words read are not counted): %.2f TB/s; (b)'s keys_member %.3f ms in %d launches (%.4f ms each)"
                % (name, ki["total_ms"], ki["launches"], ki["algo_bytes"] / 1e6, ki["algo_bytes"] / ki["total_ms"] / 1e9, km["total_ms"],
                   km["launches"], km["total_ms"] / km["launches"]))
    docs.close()
    hk.close()
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
