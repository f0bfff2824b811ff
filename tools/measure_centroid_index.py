"""python tools/measure_centroid_index.py [out.txt [repeats]] -- what the document index costs (orr_keys_centroid_index), on ONE
MI355X in one job: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072), keys in runs of 40 rows (key =
position // 40: 25,000 keys), two warm calls first, REPEATS (default 11) repeats with the timed calls alternating, median
(min-max) in ms.

Timed calls (host wall time): (a) `centroid_index`, the device route; (b) the host route of the twin rule: groups + centroids +
create + append + seal, the ticks of each key's newest member prepared outside the clock.  (b) contains all of (a)'s device work
plus two bus crossings of the centroids, so (a)'s median must lie below (b)'s: the tool says which it is.  Per-kernel times from
the kernel statistics of one profiled call; keys_centroid_finish is set beside a device-to-device copy of the bytes of the fp64
sums it reads (device events), and (a)'s seal is timed alone on a twin."""
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
    n_keys = (ROWS + RUN - 1) // RUN
    created = gen.created_ticks(0, ROWS, ROWS).numpy()
    first_ticks = created[order[::RUN]]                  # every row participates: a key's first member is its newest
    no_content, no_off = np.zeros(1, np.uint8), np.zeros(n_keys + 1, np.uint64)
    seal_ms = []

    def device_route():
        d = hk.centroid_index()
        assert d.docs == n_keys and d.skipped == 0
        return d

    def host_route():
        gk, _ = hk.groups()
        parts = [hk.centroids(gk[i0:i0 + 65_536]) for i0 in range(0, len(gk), 65_536)]
        cent = np.concatenate([p[0] for p in parts])
        used = np.concatenate([p[1] for p in parts])
        keep = used > 0
        t = P.RecallIndex(dim=DIM, device=0)
        t.append(np.ascontiguousarray(cent[keep]), first_ticks[keep], no_content, no_off[:int(keep.sum()) + 1], row_ids=gk[keep])
        t0 = time.perf_counter()
        t.seal()
        seal_ms.append((time.perf_counter() - t0) * 1e3)
        return t

    calls = {"centroid_index (a)": device_route, "host route (b)": host_route}
    say("# document index on ONE MI355X, one job: shard %d x %d, keys in runs of %d (%d keys), %d alternating repeats; ms, median (min-max)"
        % (ROWS, DIM, RUN, n_keys, REPEATS))
    d, t = device_route(), host_route()
    same = np.array_equal(d.get_rows(np.arange(n_keys))[0].view(np.uint32), t.get_rows(np.arange(n_keys))[0].view(np.uint32))
    say("the two routes' rows are the same bits: %s" % same)
    d.close(); t.close()
    for c in calls.values():
        c().close()
    del seal_ms[:]
    ms = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, c in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = c()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            r.close()
    for k in calls:
        say("%-20s %s" % (k, fmt(stat(ms[k]))))
    a, b = stat(ms["centroid_index (a)"]), stat(ms["host route (b)"])
    say("the condition, (a)'s median below (b)'s: %s (%.3f against %.3f, %.2f x)" % ("HOLDS" if a[0] < b[0] else "DOES NOT HOLD", a[0], b[0], b[0] / a[0]))
    say("orr_index_seal of the %d x %d twin alone (inside (b)): %s" % (n_keys, DIM, fmt(stat(seal_ms))))
    idx.set_profiling(1)
    device_route().close()
    st = idx.kernel_stats()
    idx.set_profiling(0)
    say("centroid_index, kernels of the source's lane: " + ", ".join("%s %.3f ms in %d launch(es)" % (k, v["total_ms"], v["launches"]) for k, v in sorted(st.items())))
    sum_bytes = 8.0 * n_keys * DIM
    src = torch.empty(int(sum_bytes) // 8, dtype=torch.float64, device=dev).normal_()
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cp = []
    for _ in range(2 + REPEATS):
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        cp.append(e0.elapsed_time(e1))
    cp = stat(cp[2:])
    if "keys_centroid_finish" in st:
        f = st["keys_centroid_finish"]
        say("keys_centroid_finish reads %.1f MB of sums and writes %.1f MB of centroids in %.3f ms (%d launches): %.2f TB/s; a device-to-device copy of the sums' %.1f MB takes %s ms (the finish is %.2f x of it)"
            % (sum_bytes / 1e6, sum_bytes / 2e6, f["total_ms"], f["launches"], f["algo_bytes"] / f["total_ms"] / 1e9, sum_bytes / 1e6, fmt(cp), f["total_ms"] / cp[0]))
    hk.close()
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
