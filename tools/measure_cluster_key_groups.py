"""python tools/measure_cluster_key_groups.py [out.txt [repeats]] -- what the key groups cost over a cluster
(orr_cluster_keys_groups, orr_cluster_keys_centroids, orr_cluster_scope_centroid), on ONE MI355X in one job, in the set-up of
tools/measure_key_groups.py: synthetic rows MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072), keys in runs of 40 candidates,
two warm calls first, REPEATS (default 11) repeats with the timed calls alternating, median (min-max) in ms.

The yardstick is the single index over the same rows on the same device; the cluster is those rows in four shards on one ordinal,
cut 10, 20 and 30 rows behind the quarters, so that every border falls inside a document (three spanning keys).  Timed (host wall
time, results in host memory): `centroids` of all keys, the scope centroid of the whole corpus, `groups` -- each on the cluster and
on the single index.  Then, from one profiled call: per shard the kernel statistics' times of keys_block_sums and
keys_chain_step, the spanning keys with members there, and the state bytes the chain moved."""
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
RUN = 40
SHARDS = 4
SLICE_BYTES = 64 << 20                                   # key_groups::kSliceBytes
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
    edges = [0] + [ROWS * g // SHARDS + 10 * g for g in range(1, SHARDS)] + [ROWS]
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS)
    cl = P.RecallCluster([0] * SHARDS, DIM, capacity_rows_per_shard=max(edges[g + 1] - edges[g] for g in range(SHARDS)))
    step = 32768
    for g in range(SHARDS):
        for r0 in range(edges[g], edges[g + 1], step):
            m = min(step, edges[g + 1] - r0)
            pool, off = gen.contents(r0, m, dev)
            emb, created = gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, ROWS, dev)
            row_ids = np.arange(r0, r0 + m, dtype=np.int64)
            idx.append(emb, created, pool, off, row_ids=row_ids)
            cl.shard(g).append(emb, created, pool, off, row_ids=row_ids)
    del pool, off, emb, created
    torch.cuda.empty_cache()
    idx.seal()
    cl.seal()
    n_keys = (ROWS + RUN - 1) // RUN
    listed = np.arange(n_keys, dtype=np.int64)
    ids = np.arange(ROWS, dtype=np.int64)
    whole, cwhole = idx.scope_ticks(-(1 << 62), 1 << 62), cl.scope_ticks(-(1 << 62), 1 << 62)

    def keys_by_position(order):                         # key = candidate position // RUN
        keys = np.empty(ROWS, np.int64)
        keys[order] = np.arange(ROWS, dtype=np.int64) // RUN
        return keys

    corder = cwhole.row_ids()
    ckeys = keys_by_position(corder)
    hk, ck = idx.keys(ids, keys_by_position(whole.row_ids())), cl.keys(ids, ckeys)
    live = [cl.shard(g).rows for g in range(SHARDS)]
    base = np.concatenate([[0], np.cumsum(live)])
    on = [set(np.unique(ckeys[corder[base[g]:base[g + 1]]]).tolist()) for g in range(SHARDS)]
    count = {}
    for g in range(SHARDS):
        for k in on[g]:
            count[k] = count.get(k, 0) + 1
    spanning = sorted(k for k, c in count.items() if c > 1)
    calls = {"cluster centroids": lambda: ck.centroids(listed), "index centroids": lambda: hk.centroids(listed),
             "cluster scope_centroid": lambda: cwhole.centroid(), "index scope_centroid": lambda: whole.centroid(),
             "cluster groups": lambda: ck.groups(), "index groups": lambda: hk.groups()}
    say("# cluster key groups on ONE MI355X, one job: %d x %d, keys in runs of %d (%d keys), %d shards on one ordinal (rows %s), %d spanning keys %s;"
        % (ROWS, DIM, RUN, n_keys, SHARDS, live, len(spanning), spanning))
    say("# %d alternating repeats after two warm calls; host wall ms, median (min-max)" % REPEATS)
    for _ in range(2):
        for c in calls.values():
            c()
    t = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, c in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c()
            t[k].append((time.perf_counter() - t0) * 1e3)
    for k in calls:
        say("%-24s %s" % (k, fmt(stat(t[k]))))
    a, b = ck.centroids(listed), hk.centroids(listed)
    assert np.array_equal(a[1], b[1]) and (a[1] == RUN).all() or ROWS % RUN, (a[1][:4], b[1][:4])
    # one profiled call each
    shards = [cl.shard(g) for g in range(SHARDS)]
    per_slice = max(1, min(65536, SLICE_BYTES // (8 * DIM)))
    for name in ("centroids", "scope_centroid", "groups"):
        idx.set_profiling(1)
        calls["index " + name]()
        st = idx.kernel_stats()
        idx.set_profiling(0)
        say("index %s, kernels: " % name + ", ".join("%s %.3f ms in %d launch(es)" % (k, v["total_ms"], v["launches"]) for k, v in sorted(st.items())))
        for sh in shards:
            sh.set_profiling(1)
        calls["cluster " + name]()
        sts = [sh.kernel_stats() for sh in shards]
        for sh in shards:
            sh.set_profiling(0)
        total_sums = 0.0
        for g, s in enumerate(sts):
            here = [k for k in spanning if k in on[g]] if name == "centroids" else ([0] if name == "scope_centroid" else [])
            say("cluster %s, shard %d (%d spanning keys with members): " % (name, g, len(here)) +
                ", ".join("%s %.3f ms in %d launch(es)" % (k, v["total_ms"], v["launches"]) for k, v in sorted(s.items())))
            total_sums += s.get("keys_block_sums", {}).get("total_ms", 0.0)
        if name != "groups":
            chain = sum(s.get("keys_chain_step", {}).get("total_ms", 0.0) for s in sts)
            launches = sum(s.get("keys_chain_step", {}).get("launches", 0) for s in sts)
            single = st["keys_block_sums"]["total_ms"]
            say("  the shards' keys_block_sums sum to %.3f ms against the single index's %.3f ms (%.2f x); keys_chain_step %.3f ms in %d launches = %.3f x one shard's keys_block_sums"
                % (total_sums, single, total_sums / single, chain, launches, chain / max(total_sums / SHARDS, 1e-9)))
            # the state each chain launch moves: the rows of the range of state slots of its slice's spanning keys there, up and down
            moved = 0
            if name == "centroids":
                for s0 in range(0, n_keys, per_slice):
                    span = [k for k in spanning if s0 <= k < s0 + per_slice]
                    for g in range(SHARDS):
                        slots = [i for i, k in enumerate(span) if k in on[g]]
                        if slots:
                            moved += 2 * (max(slots) - min(slots) + 1) * 2 * DIM * 8
            else:
                moved = 2 * SHARDS * 2 * DIM * 8
            say("  state moved through the pinned buffer: %d bytes (%d per spanning key and visit, each way)" % (moved, 2 * DIM * 8))
    for h in (hk, ck, whole, cwhole, idx, cl):
        h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
