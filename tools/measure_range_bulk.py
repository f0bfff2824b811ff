"""python tools/measure_range_bulk.py [out.txt [repeats]] -- what a bulk cosine range search (orr_search_range_cosine_bulk) costs,
on ONE MI355X in one job: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072), every timed build a child
process of this job on the same device under its own time limit, two warm calls first, REPEATS (default 15) repeats, median
(min-max) in ms.

BINDING 1: the bulk call with 256 queries (this build) against ceil(256 / 64) calls of orr_search_range_cosine on the same queries
on a build of the PARENT commit (MEASURE_PARENT_ROOT=<a built checkout of it>; without it, on this build and said so), the two
children alternated MEASURE_ROUNDS (default 2) times: the bulk median is below the sliced median by more than the two min-max
spreads together.  The ratio is written down.

BINDING 2: the default `bench.py --gpus 1` run of this build and of the parent build, alternating, MEASURE_BENCH_RUNS (default 3)
runs each: the medians of ms_per_step lie apart by less than the spreads together.

Reported without a threshold: the bulk call for 65, 128, 256 and 1024 queries at thresholds that leave about 0, 10 and 1,000 hits
per query, with the screen_tile16_range launch's kernel time, its algorithmic bytes (rows x dim + 24 bytes per row + the query
image) as a share of the HBM roof and its int8 operations as a share of the dense MFMA roof, the pairs the screen kept per query
and the pairs the host decided; beside it the parent's fused screening launches (kernel statistics entry screen_i8_fused) of a
cosine-only 256-query search on the same shard.  The first child that does not end with status 0 and a result line ends the
job: no further child is started on the device.  --no-bench leaves BINDING 2 out, --bench-only runs nothing else."""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(os.environ.get("MEASURE_ROOT", HERE))          # the build a child measures
sys.path.insert(0, ROOT)

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
CHILD = next((a[len("--child="):] for a in sys.argv[1:] if a.startswith("--child=")), None)
OUT = ARGS[0] if ARGS and ARGS[0] != "-" else None
REPEATS = int(ARGS[1]) if len(ARGS) > 1 else 15
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
ROUNDS = int(os.environ.get("MEASURE_ROUNDS", 2))
BENCH_RUNS = int(os.environ.get("MEASURE_BENCH_RUNS", 3))
CHILD_LIMIT = int(os.environ.get("MEASURE_CHILD_SECONDS", 400))
HBM_ROOF, I8_ROOF = 8.0e12, 5.0e15                                    # bytes/s (spec), dense int8 operations/s (spec)
BATCHES = (65, 128, 256, 1024)
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


def build(P, gen, dev):
    import torch
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS)
    step = 32768
    for r0 in range(0, ROWS, step):
        m = min(step, ROWS - r0)
        pool, off = gen.contents(r0, m, dev)
        idx.append(gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, ROWS, dev), pool, off)
    del pool, off
    torch.cuda.empty_cache()
    idx.seal()
    return idx


def queries_and_levels(gen, dev, n):
    """n queries, each a row of the shard plus noise, and per query the thresholds that leave about 0, 10 and 1,000 hits (from
    fp32 cosines on the device: they only place the thresholds)"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(7)
    rows = torch.randint(0, ROWS, (n,), generator=g)
    base = torch.cat([gen.embeddings(int(r), 1, DIM, dev) for r in rows])
    q = (base + 0.6 * (torch.rand((n, DIM), generator=g) * 2 - 1).to(dev)).contiguous()
    qn = q / q.norm(dim=1, keepdim=True)
    top = []
    for r0 in range(0, ROWS, 65536):
        E = gen.embeddings(r0, min(65536, ROWS - r0), DIM, dev)
        top.append(torch.topk((E / E.norm(dim=1, keepdim=True)) @ qn.T, min(1000, E.shape[0]), dim=0).values)
        del E
    kth = torch.sort(torch.cat(top), dim=0, descending=True).values
    levels = {"about 0 hits": np.full(n, 2.0), "about 10 hits": kth[9].double().cpu().numpy(), "about 1,000 hits": kth[min(999, kth.shape[0] - 1)].double().cpu().numpy()}
    return q, levels


def timed(call):
    import torch
    call()
    call()
    t = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def profiled(idx, call):
    idx.set_profiling(1)
    got = call()
    st = idx.kernel_stats()
    idx.set_profiling(0)
    return got, st


def child_sliced():
    """the yardstick in the build at ROOT: 256 queries through orr_search_range_cosine in slices of 64; the fused screening
    launches of a cosine-only 256-query search"""
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    idx = build(P, gen, dev)
    q, levels = queries_and_levels(gen, dev, 256)
    res = {"sliced": {}, "fused": []}

    def sliced(tt):
        return [idx.range_cosine(q[a:a + 64].contiguous(), tt[a:a + 64], 2000) for a in range(0, 256, 64)]

    for what, t in levels.items():
        res["sliced"][what] = timed(lambda: sliced(t))
    search = lambda: idx.search(q, [[] for _ in range(256)], gen.NOW_TICKS, 10, candidate_limit=ROWS)
    search()
    search()
    for _ in range(REPEATS):
        _, st = profiled(idx, search)
        res["fused"].append([st["screen_i8_fused"]["total_ms"], st["screen_i8_fused"]["launches"]] if "screen_i8_fused" in st else [0.0, 0])
    idx.close()
    print("RESULT " + json.dumps(res), flush=True)


def child_bulk():
    """the bulk call in the build at ROOT"""
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    idx = build(P, gen, dev)
    q, levels = queries_and_levels(gen, dev, max(BATCHES))
    res = {"calls": []}
    only = os.environ.get("MEASURE_ONLY_B")
    for B in BATCHES:
        if only and int(only) != B:
            continue
        qq = q[:B].contiguous()
        for what, t in levels.items():
            tt = t[:B]
            call = lambda: idx.range_cosine_bulk(qq, tt, 2000)
            row = dict(B=B, what=what, call=timed(call), launch=[])
            for _ in range(REPEATS):
                got, st = profiled(idx, call)
                row["launch"].append(st["screen_tile16_range"]["total_ms"] / st["screen_tile16_range"]["launches"])
            row.update(hits=int(got[3].sum()), launches=int(st["screen_tile16_range"]["launches"]),
                       survivors=int(st.get("range_screen_pairs", {"algo_bytes": 0})["algo_bytes"] // 16),
                       host_pairs=int(st.get("range_host_pairs", {"algo_bytes": 0})["algo_bytes"] // 32))
            res["calls"].append(row)
    idx.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(kind, root, env_more=None):
    env = dict(os.environ, MEASURE_ROOT=root, **(env_more or {}))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child=" + kind, "-", str(REPEATS)], cwd=root, env=env, capture_output=True, text=True,
                           timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        return None, "did not end within %d s and was stopped" % CHILD_LIMIT
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        return None, "exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-400:])
    return json.loads(lines[-1][7:]), None


def bench_once(root):
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
    parent = os.environ.get("MEASURE_PARENT_ROOT")
    yard_root = os.path.abspath(parent) if parent else HERE
    say("# bulk cosine range search (orr_search_range_cosine_bulk) on ONE MI355X, one job, every timed build a child process on the same device")
    say("# shard %d x %d, %d repeats per child; ms, median (min-max)" % (ROWS, DIM, REPEATS))
    say("# yardstick: ceil(256 / 64) calls of orr_search_range_cosine, from %s" % ("a build of the parent commit" if parent else "THIS build (no parent build was given)"))
    if "--bench-only" not in sys.argv:
        sliced = {}
        bulk256 = {}
        fused = []
        for rnd in range(ROUNDS):
            y, err = run_child("sliced", yard_root)
            if err:
                say("sliced child, round %d: %s -- nothing more is started" % (rnd + 1, err))
                return 1
            b, err = run_child("bulk", HERE, {"MEASURE_ONLY_B": "256"})
            if err:
                say("bulk child, round %d: %s -- nothing more is started" % (rnd + 1, err))
                return 1
            for what, ms in y["sliced"].items():
                sliced.setdefault(what, []).extend(ms)
            for c in b["calls"]:
                bulk256.setdefault(c["what"], []).extend(c["call"])
            fused += y["fused"]
        say("")
        for what in sliced:
            a, b = stat(bulk256[what]), stat(sliced[what])
            spreads = (a[2] - a[1]) + (b[2] - b[1])
            say("256 queries, %-17s bulk call %s | 4 calls of orr_search_range_cosine %s | ratio %.2f" % (what + ":", fmt(a), fmt(b), b[0] / a[0]))
            say("   BINDING 1: %.3f < %.3f - both spreads together %.3f: %s" % (a[0], b[0], spreads, "met" if a[0] < b[0] - spreads else "NOT met"))
        if fused and fused[0][1]:
            say("the parent's fused screening launches (screen_i8_fused) of a cosine-only 256-query search: %s ms in %d launch(es)"
                % (fmt(stat([f[0] for f in fused])), fused[0][1]))
        say("")
        full, err = run_child("bulk", HERE)
        if err:
            say("bulk child: %s -- nothing more is started" % err)
            return 1
        for c in full["calls"]:
            ls = stat(c["launch"])
            tiled = ((c["B"] + 255) // 256) * 256 * DIM
            algo = 1.0 * ROWS * DIM + 24.0 * ROWS + tiled
            ops = 2.0 * ROWS * DIM * ((c["B"] + 255) // 256) * 256
            hbm, mfma = algo / (ls[0] * 1e-3) / HBM_ROOF, ops / (ls[0] * 1e-3) / I8_ROOF
            say("%4d queries, %-17s %8d hits | whole call %s | screen_tile16_range %s per launch, %d launch(es): %.1f MB algorithmic = %.2f of the HBM roof, "
                "%.2f of the dense int8 MFMA roof (%s bounds) | %.1f survivors per query, %d pairs to the host"
                % (c["B"], c["what"] + ":", c["hits"], fmt(stat(c["call"])), fmt(ls), c["launches"], algo / 1e6, hbm, mfma, "HBM" if hbm > mfma else "the MFMA",
                   c["survivors"] / c["B"], c["host_pairs"]))
        say("")
    if parent and "--no-bench" not in sys.argv:
        say("# the default bench.py run (--gpus 1) of this build and of a build of the parent commit, alternating, %d runs each" % BENCH_RUNS)
        got = {"this build": [], "parent build": []}
        for i in range(BENCH_RUNS):
            for name, root in (("this build", HERE), ("parent build", yard_root)):
                r, err = bench_once(root)
                if err:                                  # a child that failed, faulted or hung: nothing more starts on this device
                    say("%-12s run %d: %s" % (name, i + 1, err))
                    say("BINDING 2: not taken -- a bench run did not end with status 0 and a result line; no further run was started")
                    return 1
                got[name].append(r)
                say("%-12s run %d: %.4f ms per step, %.0f queries/s" % (name, i + 1, r[0], r[1]))
        a, b = stat([r[0] for r in got["this build"]]), stat([r[0] for r in got["parent build"]])
        spreads = (a[2] - a[1]) + (b[2] - b[1])
        say("this build   ms per step %s" % fmt(a))
        say("parent build ms per step %s" % fmt(b))
        say("BINDING 2: |median - median| = %.4f ms against both spreads together %.4f ms: %s"
            % (abs(a[0] - b[0]), spreads, "met" if abs(a[0] - b[0]) <= spreads else "NOT met"))
    return 0


if __name__ == "__main__":
    if CHILD == "sliced":
        child_sliced()
    elif CHILD == "bulk":
        child_bulk()
    else:
        sys.exit(main())
