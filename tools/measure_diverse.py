"""python tools/measure_diverse.py [out.txt [repeats]] -- what a diverse search (orr_search_batch_diverse) costs, on ONE MI355X in one
job: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072), every timed build a child process of this job on
the same device under its own time limit, two warm calls first, REPEATS (default 15) repeats, median (min-max) in ms.

Reported without a threshold, for B in {1, 64, 256}, topk 10, pool in {24, 56} and both modes (collapse at max_cosine 0.95, MMR at
lambda 0.7): the whole call; the same build's orr_search_batch with topk = pool (the difference is the price of diversification);
the pair_dots launch alone from the kernel statistics, with its gathered bytes (lists x pool x dim x 4), its products
(lists x pool (pool + 1) / 2 x dim) and the share of the 8 TB/s HBM roof the bytes imply.

BINDING: the default `bench.py --gpus 1` run of this build and of a build of the parent commit (MEASURE_PARENT_ROOT=<a built
checkout of it>), alternating, MEASURE_BENCH_RUNS (default 3) runs each: the medians of ms_per_step lie apart by less than the two
min-max spreads together.  The first child that does not end with status 0 and a result line ends the job: no further child is
started on the device.  --no-bench leaves the binding out, --bench-only runs nothing else."""
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
BENCH_RUNS = int(os.environ.get("MEASURE_BENCH_RUNS", 3))
CHILD_LIMIT = int(os.environ.get("MEASURE_CHILD_SECONDS", 400))
HBM_ROOF = 8.0e12                                                     # bytes/s (spec)
BATCHES = (1, 64, 256)
POOLS = (24, 56)
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


def child_diverse():
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    idx = build(P, gen, dev)
    nq = max(BATCHES)
    q = gen.query_vectors(0, nq, DIM, ROWS, dev)
    terms = [P.text.query_terms(t) for t in gen.query_texts(0, nq, ROWS)]
    res = {"calls": []}
    for B in BATCHES:
        qq, tt = q[:B].contiguous(), terms[:B]
        for pool in POOLS:
            plain = timed(lambda: idx.search(qq, tt, gen.NOW_TICKS, pool, candidate_limit=ROWS))
            for mode, param in MODES:
                call = lambda: idx.search_diverse(qq, tt, gen.NOW_TICKS, 10, pool, mode=mode, param=param, candidate_limit=ROWS)
                row = dict(B=B, pool=pool, mode=mode, param=param, call=timed(call), plain=plain, launch=[])
                for _ in range(REPEATS):
                    idx.set_profiling(1)
                    got = call()
                    st = idx.kernel_stats()
                    idx.set_profiling(0)
                    row["launch"].append(st["pair_dots"]["total_ms"] / st["pair_dots"]["launches"])
                row.update(launches=int(st["pair_dots"]["launches"]), members=int(min(int(c) for c in got[2])), kept=float(np.mean(got[2])))
                res["calls"].append(row)
    idx.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(kind, root):
    env = dict(os.environ, MEASURE_ROOT=root)
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
    say("# diverse search (orr_search_batch_diverse) on ONE MI355X, one job, every timed build a child process on the same device")
    say("# shard %d x %d, topk 10, hybrid queries, %d repeats; ms, median (min-max)" % (ROWS, DIM, REPEATS))
    if "--bench-only" not in sys.argv:
        res, err = run_child("diverse", HERE)
        if err:
            say("diverse child: %s -- nothing more is started" % err)
            return 1
        for c in res["calls"]:
            a, p, ls = stat(c["call"]), stat(c["plain"]), stat(c["launch"])
            gathered = 4.0 * c["B"] * c["pool"] * DIM
            products = 1.0 * c["B"] * c["pool"] * (c["pool"] + 1) / 2 * DIM
            say("%3d queries, pool %2d, %-8s %-4s whole call %s | orr_search_batch with topk = pool %s | difference %.3f | pair_dots %s in %d launch: "
                "%.2f MB gathered, %.1f M products, %.4f of the HBM roof | %.1f rows kept per query"
                % (c["B"], c["pool"], c["mode"], c["param"], fmt(a), fmt(p), a[0] - p[0], fmt(ls), c["launches"], gathered / 1e6, products / 1e6,
                   gathered / (ls[0] * 1e-3) / HBM_ROOF, c["kept"]))
        say("")
    if parent and "--no-bench" not in sys.argv:
        yard_root = os.path.abspath(parent)
        say("# the default bench.py run (--gpus 1) of this build and of a build of the parent commit, alternating, %d runs each" % BENCH_RUNS)
        got = {"this build": [], "parent build": []}
        for i in range(BENCH_RUNS):
            for name, root in (("this build", HERE), ("parent build", yard_root)):
                r, err = bench_once(root)
                if err:                                  # a child that failed, faulted or hung: nothing more starts on this device
                    say("%-12s run %d: %s" % (name, i + 1, err))
                    say("BINDING: not taken -- a bench run did not end with status 0 and a result line; no further run was started")
                    return 1
                got[name].append(r)
                say("%-12s run %d: %.4f ms per step, %.0f queries/s" % (name, i + 1, r[0], r[1]))
        a, b = stat([r[0] for r in got["this build"]]), stat([r[0] for r in got["parent build"]])
        spreads = (a[2] - a[1]) + (b[2] - b[1])
        say("this build   ms per step %s" % fmt(a))
        say("parent build ms per step %s" % fmt(b))
        say("BINDING: |median - median| = %.4f ms against both spreads together %.4f ms: %s"
            % (abs(a[0] - b[0]), spreads, "met" if abs(a[0] - b[0]) <= spreads else "NOT met"))
    return 0


if __name__ == "__main__":
    if CHILD == "diverse":
        child_diverse()
    else:
        sys.exit(main())
