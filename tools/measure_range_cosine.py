"""python tools/measure_range_cosine.py [out.txt [repeats]] -- what a cosine range search (orr_search_range_cosine) costs, on ONE
MI355X in one job: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072), every timed build a child process
of this job on the same device, REPEATS (default 15) repeats, median (min-max) in ms.

BINDING: the RANGE launch of the streaming int8 screen (kernel statistics entry screen_gemv_i8_range) with 1 and with 4 queries
against the scoring launch of the same kernel (entry screen_gemv_i8) in a 1-query and a 4-query search, from a build of the
PARENT commit (MEASURE_PARENT_ROOT=<a built checkout of it>; without it, from this build and said so).  The RANGE median is not
above the yardstick's by more than the two min-max spreads together: it streams the same bytes with a lighter tail.

Reported without a threshold: the whole call for 1, 4 and 64 queries at thresholds that leave about 0, 10 and 1,000 hits per
query, through the screen ("range_form" 1) and through the exact form (2), with the pairs the screen kept and the pairs the host
decided; orr_scope_create_near + orr_scope_row_ids for the same probes, eight at a time, beside it.

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
OUT = ARGS[0] if ARGS and ARGS[0] != "-" else None
REPEATS = int(ARGS[1]) if len(ARGS) > 1 else 15
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
BENCH_RUNS = int(os.environ.get("MEASURE_BENCH_RUNS", 3))
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


def queries_of(gen, dev, n):
    """n queries, each a row of the shard plus noise: every one has near rows of its own"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(7)
    rows = torch.randint(0, ROWS, (n,), generator=g)
    base = torch.cat([gen.embeddings(int(r), 1, DIM, dev) for r in rows])
    noise = (torch.rand((n, DIM), generator=g) * 2 - 1).to(dev)
    return (base + 0.6 * noise).contiguous()


def kernel_ms(idx, name, call):
    """total_ms of one kernel-statistics entry per launch, REPEATS times (after two warm calls)"""
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


def child_yard():
    """the yardstick: the scoring launch of K2i in a 1-query and a 4-query search, in the build at ROOT"""
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    idx = build(P, gen, dev)
    q = queries_of(gen, dev, 64)
    res = {}
    for nq in (1, 4):
        qq = q[:nq].contiguous()
        res[str(nq)] = kernel_ms(idx, "screen_gemv_i8", lambda: idx.search(qq, [[] for _ in range(nq)], gen.NOW_TICKS, 10, candidate_limit=ROWS))
    idx.close()
    print("RESULT " + json.dumps(res), flush=True)


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


def child_range():
    """the range search in the build at ROOT: the RANGE launch's kernel time, the whole call in both forms, the cosine scope beside it"""
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    idx = build(P, gen, dev)
    q = queries_of(gen, dev, 64)
    # thresholds from the cosines themselves (fp32 on the device: they only place the thresholds): the k-th largest per query
    top = []
    qn = q / q.norm(dim=1, keepdim=True)
    for r0 in range(0, ROWS, 131072):
        E = gen.embeddings(r0, min(131072, ROWS - r0), DIM, dev)
        top.append(torch.topk((E / E.norm(dim=1, keepdim=True)) @ qn.T, 1000, dim=0).values)
        del E
    kth = torch.sort(torch.cat(top), dim=0, descending=True).values
    levels = {"about 0 hits": np.full(64, 2.0), "about 10 hits": kth[9].double().cpu().numpy(), "about 1,000 hits": kth[999].double().cpu().numpy()}
    del top, kth
    res = {"launch": {}, "calls": []}
    idx.set_option("range_form", 1)
    for nq in (1, 4):
        qq, tt = q[:nq].contiguous(), levels["about 10 hits"][:nq]
        res["launch"][str(nq)] = kernel_ms(idx, "screen_gemv_i8_range", lambda: idx.range_cosine(qq, tt, 16))
    for nq in (1, 4, 64):
        qq = q[:nq].contiguous()
        for what, t in levels.items():
            tt = t[:nq]
            row = dict(nq=nq, what=what)
            for form in (1, 2):
                idx.set_option("range_form", form)
                row["form%d" % form] = stat(timed(lambda: idx.range_cosine(qq, tt, 2000)))
                idx.set_profiling(1)
                got = idx.range_cosine(qq, tt, 2000)
                st = idx.kernel_stats()
                idx.set_profiling(0)
                if form == 1:
                    row.update(hits=int(got[3].sum()), survivors=int(st.get("range_screen_pairs", {"algo_bytes": 0})["algo_bytes"] // 16),
                               launches=int(st["screen_gemv_i8_range"]["launches"]))
                row["host_pairs%d" % form] = int(st.get("range_host_pairs", {"algo_bytes": 0})["algo_bytes"] // 32)

            def near():                                 # the same probes as a cosine scope, eight at a time: a set, no cosines
                for b0 in range(0, nq, 8):
                    sc = idx.scope_near(qq[b0:b0 + 8].contiguous(), float(tt[b0:b0 + 8].min()), "any")
                    sc.row_ids()
                    sc.close()
            row["near"] = stat(timed(near))
            res["calls"].append(row)
    idx.close()
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
    say("# cosine range search (orr_search_range_cosine) on ONE MI355X, one job, every timed build a child process on the same device")
    say("# shard %d x %d, %d repeats; ms, median (min-max)" % (ROWS, DIM, REPEATS))
    say("# yardstick: the scoring launch of the streaming int8 screen (kernel statistics entry screen_gemv_i8) in a search, from %s"
        % ("a build of the parent commit" if parent else "THIS build (no parent build was given)"))
    if "--bench-only" not in sys.argv:
        yard, err = run_child("yard", yard_root)
        if err:
            say("yardstick child: %s -- nothing more is started" % err)
            return 1
        rng, err = run_child("range", HERE)
        if err:
            say("range child: %s -- nothing more is started" % err)
            return 1
        say("")
        for nq in ("1", "4"):
            a, b = stat(rng["launch"][nq]), stat(yard[nq])
            spreads = (a[2] - a[1]) + (b[2] - b[1])
            read = 1.0 * ROWS * DIM + 20.0 * ROWS
            say("%s query(ies): screen_gemv_i8_range %s | screen_gemv_i8 of a search %s | %.2f and %.2f TB/s of shadow and row constants read"
                % (nq, fmt(a), fmt(b), read / a[0] / 1e9, (read + 8.0 * ROWS) / b[0] / 1e9))
            say("   BINDING: median %.4f <= %.4f + both spreads together %.4f: %s" % (a[0], b[0], spreads, "met" if a[0] <= b[0] + spreads else "NOT met"))
        say("")
        for c in rng["calls"]:
            say("%2d query(ies), %-17s %7d hits | screen: whole call %s, %d launch(es), %d survivors, %d pairs to the host | exact form: %s, %d pairs to the host | scope_near + row_ids, 8 at a time: %s"
                % (c["nq"], c["what"] + ":", c["hits"], fmt(c["form1"]), c["launches"], c["survivors"], c["host_pairs1"], fmt(c["form2"]), c["host_pairs2"], fmt(c["near"])))
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
    return 0


if __name__ == "__main__":
    if CHILD == "yard":
        child_yard()
    elif CHILD == "range":
        child_range()
    else:
        sys.exit(main())
