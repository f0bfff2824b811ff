"""python tools/measure_scope_near.py [out.txt [repeats]] -- what a cosine scope (orr_scope_create_near) costs to make, on ONE
MI355X in one job: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072), 1 and 8 probes, every timed
build a child process of this job on the same device, REPEATS (default 15) repeats, median (min-max) in ms.

The yardstick of the walk is launch_dot_exact itself on the same shard with the same number of probes, from a build of the
PARENT commit (MEASURE_PARENT_ROOT=<a built checkout of it>; without it, from this build and said so): the "dot_exact" entry of
the kernel statistics of a search that takes the exact pass ("two_stage" 0; one query with topk 10, and 8 queries with topk 100,
whose large-k form computes its dots with one launch of 8).  scope_near does the same reads and writes 1 bit where that kernel
writes 8 x nq bytes per row.  BINDING: the median of "scope_near" is not above the yardstick's by more than the two min-max
spreads together.  Reported without a threshold: the whole call at thresholds that put about 0, a thousandth and a tenth of the
rows in; the same with 5,000 copies of the probe in the band; orr_scope_create from the same rows' ids beside it; the achieved
bytes per second as a share of what launch_dot_exact reaches.

Then the default `bench.py --gpus 1` run of this build and of the parent build, alternating, MEASURE_BENCH_RUNS (default 3) runs
each: the medians of ms_per_step are to lie apart by less than the spreads together.  The first child that does not end with
status 0 and a result line ends the job: no further child is started on the device."""
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
OUT = ARGS[0] if ARGS else None
REPEATS = int(ARGS[1]) if len(ARGS) > 1 else 15
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
BENCH_RUNS = int(os.environ.get("MEASURE_BENCH_RUNS", 3))
COPIES = 5_000
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


def build(P, gen, dev, copies_of=None):
    import torch
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS)
    step = 32768
    for r0 in range(0, ROWS, step):
        m = min(step, ROWS - r0)
        pool, off = gen.contents(r0, m, dev)
        emb = gen.embeddings(r0, m, DIM, dev)
        if copies_of is not None:                        # COPIES copies of the probe, spread evenly over the shard
            at = torch.arange(r0, r0 + m, device=dev) % (ROWS // COPIES) == 7
            emb[at] = copies_of
        idx.append(emb, gen.created_ticks(r0, m, ROWS, dev), pool, off)
    del pool, off, emb
    torch.cuda.empty_cache()
    idx.seal()
    return idx


def probes_of(gen, dev):
    import torch
    p0 = gen.embeddings(ROWS // 3, 1, DIM, dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    noise = (torch.rand((7, DIM), generator=g) * 2 - 1).to(dev)
    return torch.cat([p0, p0 + 0.6 * noise]).contiguous()


def kernel_ms(idx, name, call):
    """total_ms of one kernel-statistics entry per call, REPEATS times (after two warm calls)"""
    call()
    call()
    out = []
    for _ in range(REPEATS):
        idx.set_profiling(1)
        call()
        st = idx.kernel_stats()
        idx.set_profiling(0)
        out.append(st[name]["total_ms"] / max(1, st[name]["launches"]))
    return out


def child_dot():
    """the yardstick: launch_dot_exact with 1 and with 8 queries over the shard, in the build at ROOT"""
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    idx = build(P, gen, dev)
    idx.set_option("two_stage", 0)
    pr = probes_of(gen, dev)
    res = {}
    for nq, topk in ((1, 10), (8, 100)):
        q = pr[:nq].contiguous()
        res[str(nq)] = kernel_ms(idx, "dot_exact", lambda: idx.search(q, [[] for _ in range(nq)], gen.NOW_TICKS, topk, candidate_limit=ROWS))
    idx.close()
    print("RESULT " + json.dumps(res), flush=True)


def timed_make(make):
    import torch
    make().close()
    make().close()
    t = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc = make()
        t.append((time.perf_counter() - t0) * 1e3)
        sc.close()
    return t


def child_near():
    """scope_near in the build at ROOT: the walk's kernel time, the whole call, and orr_scope_create from the same rows' ids"""
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    res = {"walk": {}, "calls": []}
    for copies in (False, True):
        pr = probes_of(gen, dev)
        idx = build(P, gen, dev, pr[0] if copies else None)
        idx.scope(np.arange(8, dtype=np.int64)).close()              # (the first id scope builds the id table)
        for nq in (1, 8):
            p = pr[:nq].contiguous()
            # thresholds from the cosines themselves: a wide scope read back once, the quantiles of its rows
            E = gen.embeddings(0, 200_000, DIM, dev)
            c = (E @ pr[0]) / (E.norm(dim=1) * pr[0].norm())
            t1000, t10 = float(torch.quantile(c, 0.999)), float(torch.quantile(c, 0.9))
            del E, c
            one = 1.0 if copies else 2.0
            for what, t in (("about 0 rows" if not copies else "the copies (min_cosine 1.0: the band)", one), ("a thousandth", t1000), ("a tenth", t10)):
                if not copies and t == one:
                    res["walk"][str(nq)] = kernel_ms(idx, "scope_near", lambda: idx.scope_near(p, t, "any").close())
                call = timed_make(lambda: idx.scope_near(p, t, "any"))
                idx.set_profiling(1)
                sc = idx.scope_near(p, t, "any")
                st = idx.kernel_stats()
                idx.set_profiling(0)
                ids = sc.row_ids()
                from_ids = timed_make(lambda: idx.scope(ids))
                res["calls"].append(dict(copies=copies, nq=nq, what=what, t=t, rows=int(sc.rows), call=stat(call), from_ids=stat(from_ids),
                                         walks=int(st["scope_near"]["launches"]), band_pairs=int(st.get("scope_near_band_pairs", {"algo_bytes": 0})["algo_bytes"] // 16)))
                sc.close()
        idx.close()
        del idx
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(kind, root):
    env = dict(os.environ, MEASURE_ROOT=root)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child=" + kind, "-", str(REPEATS)], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        return None, "did not end within 900 s and was stopped"
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
    say("# cosine scopes (orr_scope_create_near) on ONE MI355X, one job, every timed build a child process on the same device")
    say("# shard %d x %d, %d repeats; ms, median (min-max)" % (ROWS, DIM, REPEATS))
    say("# yardstick: launch_dot_exact (kernel statistics entry dot_exact) from %s" % ("a build of the parent commit" if parent else "THIS build (no parent build was given)"))
    if "--bench-only" not in sys.argv:
        dot, err = run_child("dot", yard_root)
        if err:
            say("yardstick child: %s -- nothing more is started" % err)
            return 1
        near, err = run_child("near", HERE)
        if err:
            say("scope_near child: %s -- nothing more is started" % err)
            return 1
        say("")
        all_met = True
        for nq in ("1", "8"):
            a, b = stat(near["walk"][nq]), stat(dot[nq])
            spreads = (a[2] - a[1]) + (b[2] - b[1])
            met = a[0] <= b[0] + spreads
            all_met = all_met and met
            read = 4.0 * ROWS * DIM + 8.0 * ROWS
            say("%s probe(s): scope_near kernel %s | launch_dot_exact %s | %.2f and %.2f TB/s of rows and norms read: %.1f %% of what launch_dot_exact reaches"
                % (nq, fmt(a), fmt(b), read / a[0] / 1e9, read / b[0] / 1e9, 100.0 * b[0] / a[0]))
            say("   BINDING: median %.4f <= %.4f + both spreads together %.4f: %s" % (a[0], b[0], spreads, "met" if met else "NOT met"))
        say("")
        for c in near["calls"]:
            say("%-9s %d probe(s), %-40s min_cosine %.6f: %8d rows | whole call %s | %d walk(s), %d band pairs | orr_scope_create from the same ids %s"
                % ("5,000 copies," if c["copies"] else "plain,", c["nq"], c["what"], c["t"], c["rows"], fmt(c["call"]), c["walks"], c["band_pairs"], fmt(c["from_ids"])))
        say("")
    if parent:
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
    say("")
    say("not taken: the figures on a 10M-row shard.")
    return 0


if __name__ == "__main__":
    if CHILD == "dot":
        child_dot()
    elif CHILD == "near":
        child_near()
    else:
        sys.exit(main())
