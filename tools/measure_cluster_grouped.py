"""python tools/measure_cluster_grouped.py [out.txt [repeats]] -- what a batch of G tenants costs on a cluster as ONE grouped
call (orr_cluster_search_batch_in_scopes) next to a loop of G in-scope cluster calls (orr_cluster_search_batch_in_scope), each
over the queries that name its scope, on ONE MI355X: two shards of MEASURE_ROWS x MEASURE_DIM each (default 500,000 x 3072) on
that one device, int8 shadows built, "mask_screen" = 1, topk 10, candidate_limit = rows, G disjoint random scopes of S rows each,
queries assigned b % G; B in {8, 256}, G in {2, 8, 64}, S in {30,000, 100,000} (at G = 64: 10,000), and G = 1 for binding 2.
The calls alternate, 15 repeats, median (min-max) in ms; the grouped call must return the loop's arrays in every cell.

MEASURE_PARENT_ROOT=<a built checkout of the parent commit>: a child process of this job builds the same cluster from that build
on the same device and answers one loop of G in-scope calls per request over a pipe, so the parent build's loop alternates with
this build's calls inside every repeat.
BINDING 1: at B = 256, G = 8, S = 100,000 the grouped call's median lies below the parent build's loop by more than both min-max
spreads together.  BINDING 2: with G = 1 the grouped call and the in-scope call differ by less than their spreads.
BINDING 3 (MEASURE_BENCH_RUNS, default 3, 0 = skip): the default `bench.py --gpus 1` run of this build and of the parent's,
alternating, each a child process; the medians of ms_per_step differ by less than both spreads together.
Reported without a threshold: the front of a grouped pass on ONE shard (orr_search_batch_in_scopes on shard 0 with every scope
clipped) -- wall time, and from the kernel statistics group_gather_clip here against mask_clip in the parent build (its copies
are stream operations outside the statistics) -- at G = 8 and 64; and at G = 8 the grouped call under "mask_screen" 0 (the cost
rule), 1 (the grouped pass forced) and 2 (never), which says whether the rule's constants still pick the measured winner.
MEASURE_SEARCH=0 skips everything but the bench section.
Two shards on one GPU share its HBM and its queues: the figures say nothing about eight GPUs."""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

SERVE = "--serve-loop" in sys.argv                  # the child's mode: the parent build's loop of in-scope calls, one per request
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
BATCHES = tuple(int(b) for b in os.environ.get("MEASURE_BATCHES", "8,256").split(","))
# (G, S) per batch size
CELLS = tuple(tuple(int(x) for x in c.split("x")) for c in
              os.environ.get("MEASURE_CELLS", "1x100000,2x30000,2x100000,8x30000,8x100000,64x10000").split(","))
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


def spread(s):
    return s[2] - s[1]


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


class Case:
    """the batch and the scopes of one cell: the same in this process and in the child"""

    def __init__(self, P, gen, cl, B, G, S):
        self.q = gen.query_vectors(0, B, DIM, TOTAL).numpy()
        texts = gen.query_texts(0, B, TOTAL)
        self.term_lists = [P.text.query_terms(t) for t in texts]
        self.terms = P.PackedTerms(P.pack_terms(self.term_lists))
        drawn = np.random.default_rng(1000 * B + 10 * G + S % 7).choice(TOTAL, G * S, replace=False).astype(np.int64)
        self.scopes = [cl.scope(np.sort(drawn[g * S:(g + 1) * S])) for g in range(G)]      # disjoint
        self.qscope = np.arange(B, dtype=np.int32) % G
        self.members = [np.nonzero(self.qscope == g)[0] for g in range(G)]
        self.sub = []
        for g in range(G):
            m = self.members[g]
            self.sub.append(None if len(m) == 0 else
                            (np.ascontiguousarray(self.q[m]), P.PackedTerms(P.pack_terms([self.term_lists[b] for b in m]))))
        self.cl, self.now, self.B, self.G, self.S = cl, gen.NOW_TICKS, B, G, S

    def loop(self, limit=TOTAL):
        """one in-scope cluster call per scope, over the queries that name it; the results in the batch's order"""
        rows, scores, counts = np.full((self.B, 10), -1, np.int64), np.zeros((self.B, 10)), np.zeros(self.B, np.int32)
        for g in range(self.G):
            if self.sub[g] is None:
                continue
            r, s, c = self.cl.search_in_scope(self.sub[g][0], self.sub[g][1], self.now, 10, self.scopes[g], candidate_limit=limit)
            rows[self.members[g]], scores[self.members[g]], counts[self.members[g]] = r, s, c
        return rows, scores, counts

    def grouped(self, limit=TOTAL):
        return self.cl.search_in_scopes(self.q, self.terms, self.now, 10, self.scopes, self.qscope, candidate_limit=limit)

    def shard_grouped(self):
        """the single index's grouped call on shard 0 with every scope clipped: the grouped front at work"""
        sh = self.cl.shard(0)
        parts = [sc.shard(0) for sc in self.scopes]
        limit = max(1, min(p.rows for p in parts) - 1000)
        return sh.search_in_scopes(self.q, self.terms, self.now, 10, parts, self.qscope, candidate_limit=limit)

    def close(self):
        for sc in self.scopes:
            sc.close()


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def front_stats(case):
    """the kernel statistics of one grouped call on shard 0: name -> (launches, total microseconds)"""
    sh = case.cl.shard(0)
    sh.set_profiling(True)
    case.shard_grouped()
    st = sh.kernel_stats()
    sh.set_profiling(False)
    keep = {}
    for k in ("group_gather_clip", "mask_clip"):
        if k in st:
            keep[k] = (int(st[k]["launches"]), round(float(st[k]["total_ms"]) * 1e3, 1))
    return keep


def serve():
    """the child: `case B G S` prepares a cell and warms it up; `run` times one loop, `front` one grouped call on shard 0"""
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    cl = build(P, gen, torch.device("cuda:0"))
    print("ready", flush=True)
    case = None
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        if word[0] == "case":
            if case is not None:
                case.close()
            case = Case(P, gen, cl, int(word[1]), int(word[2]), int(word[3]))
            case.loop()
            case.loop()
            if case.G > 1:
                case.shard_grouped()
            print("ok", flush=True)
        elif word[0] == "run":
            print("%.6f" % timed(case.loop), flush=True)
        elif word[0] == "front":
            print("%.6f" % timed(case.shard_grouped), flush=True)
        elif word[0] == "frontstats":
            print(json.dumps(front_stats(case)), flush=True)
    cl.close()


class Baseline:
    """the child process with the parent build's cluster; a reply that does not come ends it for the rest of the job"""

    def __init__(self, parent_root):
        env = dict(os.environ, MEASURE_ROOT=parent_root)
        env.pop("ORR_HIP_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve-loop"], env=env, stdin=subprocess.PIPE,
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
    say("# a cluster batch of G scopes: one grouped call against a loop of G in-scope calls;", torch.cuda.get_device_name(0))
    say("# %d shards of %d x %d on ONE device, int8 shadows built, mask_screen 1, topk 10, candidate_limit = rows, %d repeats, calls alternate; ms, median (min-max)"
        % (SHARDS, ROWS, DIM, REPEATS))
    cl = build(P, gen, torch.device("cuda:0"))
    base = Baseline(parent) if parent else None
    if base is not None and not base.ok:
        say("# the parent build's child process did not come up: no parent column")
    shards = [cl.shard(g) for g in range(SHARDS)]
    for B in BATCHES:
        for G, S in CELLS:
            if G > B:
                continue
            case = Case(P, gen, cl, B, G, S)
            for call in (case.grouped, case.loop):
                call()
                call()
            same = all(np.array_equal(a, b) for a, b in zip(case.grouped(), case.loop()))
            with_base = base is not None and base.ask("case %d %d %d" % (B, G, S)) == "ok"
            t = {"grouped": [], "loop": [], "parent": []}
            for _ in range(REPEATS):
                t["grouped"].append(timed(case.grouped))
                t["loop"].append(timed(case.loop))
                if with_base:
                    ms = base.ask("run")
                    if ms is None:
                        with_base = False
                    else:
                        t["parent"].append(float(ms))
            s = {k: stat(v) for k, v in t.items() if v}
            for sh in shards:
                sh.reset_search_stats()
            cl.search_stats(reset=True)
            case.grouped()
            modes = [sh.search_stats(reset=True)["pass_mode"] for sh in shards]
            cst = cl.search_stats(reset=True)
            say("")
            say("B = %d, G = %d, S = %d: pass_mode per shard %s, cluster %d, requeried %d (grouped == loop: %s)"
                % (B, G, S, modes, cst["pass_mode"], cst["requeried"], same))
            say("  %-34s" % "grouped call", fmt(s["grouped"]))
            say("  %-34s" % "loop of G in-scope calls", fmt(s["loop"]))
            if "parent" in s:
                say("  %-34s" % "loop of G, parent build", fmt(s["parent"]))
            if not same:
                say("  NOT THE SAME ARRAYS")
            if G == 1:
                d, sp = abs(s["grouped"][0] - s["loop"][0]), spread(s["grouped"]) + spread(s["loop"])
                say("  BINDING 2: |grouped - in-scope| medians = %.3f ms against both spreads together %.3f ms: %s" % (d, sp, "met" if d < sp else "NOT met"))
            if (B, G, S) == (256, 8, 100_000):
                if "parent" in s:
                    d, sp = s["parent"][0] - s["grouped"][0], spread(s["grouped"]) + spread(s["parent"])
                    say("  BINDING 1: parent build's loop median - grouped median = %.3f ms against both spreads together %.3f ms: %s"
                        % (d, sp, "met" if d > sp else "NOT met"))
                else:
                    say("  BINDING 1: not taken -- no parent build's column")
            if G in (8, 64):
                # ---- the grouped front on one shard
                case.shard_grouped()
                tf = {"here": [], "parent": []}
                for _ in range(REPEATS):
                    tf["here"].append(timed(case.shard_grouped))
                    if with_base:
                        ms = base.ask("front")
                        if ms is None:
                            with_base = False
                        else:
                            tf["parent"].append(float(ms))
                say("  one shard, orr_search_batch_in_scopes, every scope clipped: %s" % fmt(stat(tf["here"])),
                    "" if not tf["parent"] else "; parent build %s" % fmt(stat(tf["parent"])))
                say("    kernel statistics (launches, us): here %s" % json.dumps(front_stats(case)),
                    "" if not with_base else "; parent build %s" % (base.ask("frontstats") or "?"))
            if G == 8:
                # ---- the cost rule: mask_screen 0 (the rule), 1 (forced), 2 (never)
                tr = {}
                for opt in (0, 1, 2):
                    for sh in shards:
                        sh.set_option("mask_screen", opt)
                    case.grouped()
                    tr[opt] = stat([timed(case.grouped) for _ in range(REPEATS)])
                    if opt == 0:
                        for sh in shards:
                            sh.reset_search_stats()
                        case.grouped()
                        rule_modes = [sh.search_stats(reset=True)["pass_mode"] for sh in shards]
                for sh in shards:
                    sh.set_option("mask_screen", 1)
                winner = 1 if tr[1][0] <= tr[2][0] else 2
                say("  cost rule: mask_screen 0 %s (pass_mode per shard %s), 1 %s, 2 %s; measured winner: %d"
                    % (fmt(tr[0]), rule_modes, fmt(tr[1]), fmt(tr[2]), winner))
            case.close()
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
                say("BINDING 3: not taken -- a bench run did not end with status 0 and a result line; no further run was started")
                return
            got[name].append(r)
            say("%-12s run %d: %.4f ms per step, %.0f queries/s" % (name, i + 1, r[0], r[1]))
    a, b = stat([r[0] for r in got["this build"]]), stat([r[0] for r in got["parent build"]])
    spreads = spread(a) + spread(b)
    say("this build   ms per step %s" % fmt(a))
    say("parent build ms per step %s" % fmt(b))
    say("BINDING 3: |median - median| = %.4f ms against both spreads together %.4f ms: %s"
        % (abs(a[0] - b[0]), spreads, "met" if abs(a[0] - b[0]) < spreads else "NOT met"))


def main():
    parent = os.environ.get("MEASURE_PARENT_ROOT")
    if os.environ.get("MEASURE_SEARCH", "1") != "0":
        search_table(parent)
    if parent and BENCH_RUNS > 0:
        bench_section(parent)


if __name__ == "__main__":
    serve() if SERVE else main()
