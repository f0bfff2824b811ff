"""python tools/measure_key_groups.py [out.txt [repeats]] -- what the key groups cost (orr_keys_groups, orr_keys_centroids,
orr_scope_centroid), on ONE MI355X in one job: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072), keys
in runs of 40 rows (key = position // 40: 25,000 keys), two warm calls first, REPEATS (default 11) repeats with the timed calls
alternating, median (min-max) in ms.

Timed calls (host wall time, results in host memory): `centroids` of all 25,000 keys (float32 centroids only: 307 MB come back),
`scope_centroid` of the whole shard (3,907 blocks through keys_block_fold), `groups`, and a device-to-device copy of a tensor of
the same MEASURE_ROWS x MEASURE_DIM fp32 bytes (the copy moves each byte twice, keys_block_sums reads it once).  Per-kernel times
from the kernel statistics of one profiled call each.  keys_block_sums is set beside the copy of the same bytes and beside the
6.29 TB/s a float4 copy reaches on this chip (the achievable streaming figure)."""
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
STREAM_TBS = 6.29                                        # float4 copy, read + write bytes per second
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
    order = torch.from_numpy(whole.row_ids()).to(dev)    # candidate order: key = position // RUN
    keys = torch.empty(ROWS, dtype=torch.int64, device=dev)
    keys[order] = torch.arange(ROWS, dtype=torch.int64, device=dev) // RUN
    hk = idx.keys(ids, keys)
    n_keys = (ROWS + RUN - 1) // RUN
    listed = np.arange(n_keys, dtype=np.int64)
    src = torch.empty((ROWS, DIM), dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    calls = {"centroids": lambda: hk.centroids(listed), "scope_centroid": lambda: whole.centroid(), "groups": lambda: hk.groups(), "copy": copy}
    say("# key groups on ONE MI355X, one job: shard %d x %d, keys in runs of %d (%d keys), %d alternating repeats; ms, median (min-max)"
        % (ROWS, DIM, RUN, n_keys, REPEATS))
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
    row_bytes = 4.0 * ROWS * DIM
    for k in calls:
        say("%-15s %s" % (k, fmt(stat(t[k]))))
    cp = stat(t["copy"])
    say("device-to-device copy of %.2f GB: %.2f TB/s of read + written bytes" % (row_bytes / 1e9, 2 * row_bytes / cp[0] / 1e9))
    got = hk.centroids(listed)
    assert (got[1] == RUN).all() or ROWS % RUN, got[1][:4]
    for name, call in (("centroids", calls["centroids"]), ("scope_centroid", calls["scope_centroid"]), ("groups", calls["groups"])):
        idx.set_profiling(1)
        call()
        st = idx.kernel_stats()
        idx.set_profiling(0)
        say("%s, kernels: " % name + ", ".join("%s %.3f ms in %d launch(es)" % (k, v["total_ms"], v["launches"]) for k, v in sorted(st.items())))
        if "keys_block_sums" in st:
            ms = st["keys_block_sums"]["total_ms"]
            say("  keys_block_sums reads %.2f GB of rows in %.3f ms: %.2f TB/s = %.0f %% of the %.2f TB/s streaming figure; the copy of the same rows takes %.3f ms (%.2f x)"
                % (row_bytes / 1e9, ms, row_bytes / ms / 1e9, 100 * row_bytes / ms / 1e9 / STREAM_TBS, STREAM_TBS, cp[0], ms / cp[0]))
    hk.close()
    whole.close()
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
