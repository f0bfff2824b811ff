"""python tools/measure_cluster_scope_handle.py [out.txt [repeats]] -- what a cluster search inside a scope handle
(orr_cluster_search_batch_in_scope) costs next to the cluster's masked search of the same rows' ids in host memory
(orr_cluster_search_batch_masked), the unscoped orr_cluster_search_batch of the same batch, and what making the scope costs
once (orr_cluster_scope_create), on ONE MI355X: two shards of MEASURE_ROWS x MEASURE_DIM each (default 500,000 x 3072) on that
one device, int8 shadows built, "mask_screen" = 1, topk 10, candidate_limit = rows, ONE scope of S in {30,000, 100,000, 500,000}
rows drawn at random over both shards, B in {1, 8, 256}; the calls alternate, 15 repeats, median (min-max) in ms.

MEASURE_PARENT_ROOT=<a built checkout of the parent commit>: the baseline column.  A child process of this job builds the same
cluster from that build on the same device and answers one orr_cluster_search_batch_masked per request over a pipe, so the
parent build's call alternates with this build's calls inside every repeat.  BINDING at B = 1, S = 100,000: the in-scope call's
median must lie below that baseline's median by more than both calls' min-max spreads together.
MEASURE_BENCH_RUNS (default 3, 0 = skip): the default `bench.py --gpus 1` run of this build and of the parent's, alternating,
each a child process; the medians of ms_per_step must agree within the two builds' min-max spreads taken together.
MEASURE_SEARCH=0 skips the search table (the bench section alone).
Two shards on one GPU share its HBM and its queues: the figures say nothing about eight GPUs."""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

SERVE = "--serve-masked" in sys.argv                # the child's mode: the parent build's cluster masked call, one per request
ROOT = os.environ.get("MEASURE_ROOT") if SERVE else None
ROOT = ROOT or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = ARGS[0] if ARGS else None
REPEATS = int(ARGS[1]) if len(ARGS) > 1 else 15
ROWS = int(os.environ.get("MEASURE_ROWS", 500_000))       # per shard
DIM = int(os.environ.get("MEASURE_DIM", 3072))
SHARDS = 2
TOTAL = ROWS * SHARDS
SCOPES = tuple(int(s) for s in os.environ.get("MEASURE_SCOPES", "30000,100000,500000").split(","))
BATCHES = tuple(int(b) for b in os.environ.get("MEASURE_BATCHES", "1,8,256").split(","))
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
    a = np.sort(np.asarray(ms))
    return float(np.median(a)), float(a[0]), float(a[-1])


def fmt(s):
    return "%.3f (%.3f-%.3f)" % s


def build(P, gen, dev):
    cl = P.RecallCluster([0] * SHARDS, DIM, capacity_rows_per_shard=ROWS)
    step = 32768
    for g in range(SHARDS):
        sh = cl.shard(g)
        for r0 in range(g * ROWS, (g + 1) * ROWS, step):
            m = min(step, (g + 1) * ROWS - r0)
            pool, off = gen.contents(r0, m, dev)
            sh.append(gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, TOTAL, dev), pool, off,
                      row_ids=np.arange(r0, r0 + m, dtype=np.int64))
    torch.cuda.empty_cache()
    cl.seal()
    for g in range(SHARDS):
        cl.shard(g).set_option("two_stage", 1)
        cl.shard(g).set_option("mask_screen", 1)
    return cl


def case(P, gen, B, S):
    """the batch and the scope of one cell: the same in this process and in the child"""
    q = gen.query_vectors(0, B, DIM, TOTAL).numpy()
    terms = P.PackedTerms(P.pack_terms([P.text.query_terms(t) for t in gen.query_texts(0, B, TOTAL)]))
    ids = np.sort(np.random.default_rng(1000 * B + S).choice(TOTAL, S, replace=False)).astype(np.int64)
    return q, terms, ids


def serve():
    """the child: `case B S` prepares a cell and warms it up, `run` times one call and answers its milliseconds"""
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    cl = build(P, gen, torch.device("cuda:0"))
    print("ready", flush=True)
    call = None
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        if word[0] == "case":
            q, terms, ids = case(P, gen, int(word[1]), int(word[2]))
            call = lambda: cl.search_masked(q, terms, gen.NOW_TICKS, 10, ids, candidate_limit=TOTAL)      # noqa: E731
            call()
            call()
            print("ok", flush=True)
        elif word[0] == "run":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            print("%.6f" % ((time.perf_counter() - t0) * 1e3), flush=True)
    cl.close()


class Baseline:
    """the child process with the parent build's cluster; a reply that does not come ends it for the rest of the job"""

    def __init__(self, parent_root):
        env = dict(os.environ, MEASURE_ROOT=parent_root)
        env.pop("ORR_HIP_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve-masked"], env=env, stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, bufsize=1)
        self.ok = self.p.stdout.readline().strip() == "ready"

    def ask(self, text):
        if not self.ok:
            return None
        try:
            self.p.stdin.write(text + "\n")
            self.p.stdin.flush()
            reply = self.p.stdout.readline().strip()
        except OSError:
            reply = ""
        if not reply:
            self.ok = False
            return None
        return reply

    def close(self):
        try:
            if self.p.poll() is None:
                self.p.stdin.write("quit\n")
                self.p.stdin.flush()
            self.p.wait(timeout=60)
        except (OSError, subprocess.TimeoutExpired):
            self.p.kill()


def bench_once(root):
    """one default bench.py run of the build at `root`, a child process: (ms_per_step, queries/s) or an error text"""
    try:
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"], cwd=root, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        return None, "did not end within 600 s and was stopped"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return None, "exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-300:])
    doc = json.loads(lines[-1])
    return (float(doc["ms_per_step"]), float(doc["value"])), None


def search_table(parent):
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    say("# cluster search inside a scope handle against the cluster masked search of the same ids and the unscoped cluster search;", torch.cuda.get_device_name(0))
    say("# %d shards of %d x %d on ONE device, int8 shadows built, mask_screen 1, topk 10, candidate_limit = rows, %d repeats, calls alternate; ms, median (min-max)"
        % (SHARDS, ROWS, DIM, REPEATS))
    cl = build(P, gen, torch.device("cuda:0"))
    base = Baseline(parent) if parent else None
    if base is not None and not base.ok:
        say("# the parent build's child process did not come up: no baseline column")
    shards = [cl.shard(g) for g in range(SHARDS)]
    for B in BATCHES:
        for S in SCOPES:
            q, terms, ids = case(P, gen, B, S)
            sc = cl.scope(ids)
            calls = {
                "in scope": lambda: cl.search_in_scope(q, terms, gen.NOW_TICKS, 10, sc, candidate_limit=TOTAL),
                "masked, host ids": lambda: cl.search_masked(q, terms, gen.NOW_TICKS, 10, ids, candidate_limit=TOTAL),
                "unscoped": lambda: cl.search(q, terms, gen.NOW_TICKS, 10, candidate_limit=TOTAL),
            }
            for call in calls.values():
                call()
                call()
            same = all(np.array_equal(a, b) for a, b in zip(calls["in scope"](), calls["masked, host ids"]()))
            with_base = base is not None and base.ask("case %d %d" % (B, S)) == "ok"
            t = {k: [] for k in calls}
            t["create"], t["parent"] = [], []
            for _ in range(REPEATS):
                for k, call in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    t[k].append((time.perf_counter() - t0) * 1e3)
                if with_base:
                    ms = base.ask("run")
                    if ms is None:
                        with_base = False
                    else:
                        t["parent"].append(float(ms))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                made = cl.scope(ids)
                t["create"].append((time.perf_counter() - t0) * 1e3)
                made.close()
            s = {k: stat(v) for k, v in t.items() if v}
            for sh in shards:
                sh.reset_search_stats()
            calls["in scope"]()
            modes = [sh.search_stats(reset=True)["pass_mode"] for sh in shards]
            say("")
            say("B = %d, S = %d, %s live per shard, pass_mode %s (in scope == masked: %s)" % (B, S, [sc.shard(g).rows for g in range(SHARDS)], modes, same))
            for k in calls:
                say("  %-26s" % k, fmt(s[k]))
            say("  %-26s" % "scope create, once", fmt(s["create"]))
            if "parent" in s:
                say("  %-26s" % "masked, parent build", fmt(s["parent"]))
            say("  masked - in scope (medians, this build): %.3f ms" % (s["masked, host ids"][0] - s["in scope"][0]))
            if B == 1 and S == 100_000:
                if "parent" in s:
                    a, b = s["in scope"], s["parent"]
                    spreads = (a[2] - a[1]) + (b[2] - b[1])
                    say("  BINDING: parent build's masked median - in-scope median = %.3f ms against both spreads together %.3f ms: %s"
                        % (b[0] - a[0], spreads, "met" if b[0] - a[0] > spreads else "NOT met"))
                else:
                    say("  BINDING: not taken -- no parent build's column")
            sc.close()
    if base is not None:
        base.close()
    cl.close()
    say("")
    say("not taken: the figures on several GPUs (two shards on one device share its HBM and its queues).")


def bench_section(parent):
    say("")
    say("# the default bench.py run (--gpus 1) of this build and of a build of the parent commit, alternating, %d runs each, every run a child process of this job on this device" % BENCH_RUNS)
    got = {"this build": [], "parent build": []}
    for i in range(BENCH_RUNS):
        for name, root in (("this build", ROOT), ("parent build", parent)):
            r, err = bench_once(root)
            if err:                                              # a child that failed, faulted or hung: nothing more starts on this device
                say("%-12s run %d: %s" % (name, i + 1, err))
                say("BINDING: not taken -- a bench run did not end with status 0 and a result line; no further run was started")
                return
            got[name].append(r)
            say("%-12s run %d: %.4f ms per step, %.0f queries/s" % (name, i + 1, r[0], r[1]))
    a, b = stat([r[0] for r in got["this build"]]), stat([r[0] for r in got["parent build"]])
    spreads = (a[2] - a[1]) + (b[2] - b[1])
    say("this build   ms per step %s" % fmt(a))
    say("parent build ms per step %s" % fmt(b))
    say("BINDING: |median - median| = %.4f ms against both spreads together %.4f ms: %s"
        % (abs(a[0] - b[0]), spreads, "met" if abs(a[0] - b[0]) <= spreads else "NOT met"))


def main():
    parent = os.environ.get("MEASURE_PARENT_ROOT")
    if os.environ.get("MEASURE_SEARCH", "1") != "0":
        search_table(parent)
    if parent and BENCH_RUNS > 0:
        bench_section(parent)


if __name__ == "__main__":
    serve() if SERVE else main()
