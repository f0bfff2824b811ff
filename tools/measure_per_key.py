"""python tools/measure_per_key.py [out.txt [repeats]] -- what a per-key search (orr_search_batch_per_key) costs, on ONE MI355X in one
job: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072) with its int8 shadow, keys in runs of 40 rows
(key = position // 40), every timed build a child process of this job on the same device under its own time limit, two warm
calls first, REPEATS (default 15) repeats with the timed calls of a child alternating, median (min-max) in ms.

topk 10, pool 24, max_per_key 1, B in {1, 8, 64, 256}, two query families: "spread" (synthetic hybrid queries; they finish in
round 1 unless two of their best 24 rows share a run) and "concentrated" (cosine-only queries; for each query two planted
documents of 30 copies at relative distances 0.05 and 0.25 inside one run of 40 each: round 1 sees only the first document,
round 2 only the second, round 3 the rest -- three rounds; with terms the keyword part, a multiple of 0.2 / terms, lifts rows of
the second document above rows of the first and both close in round 1).  The rounds actually run are reported beside every cell.
Columns: `search` at topk = pool; the same from a build of the PARENT commit (MEASURE_PARENT_ROOT=<a built checkout of it>), a
child of its own; `search_per_key`; the emulation through the parent build's
calls -- per query and round one scope of the ids to leave out, a copy of the candidate scope, one combine and one in-scope
search.  Per-kernel times from the kernel statistics: keys_exclude and keys_gather in the concentrated B = 64 call, keys_remap
inside a compaction (after 1,000 deletes) and inside an insertion of 131 rows.

BINDING 1: this build's plain search agrees with the parent build's within their min-max spreads in every cell.
BINDING 2: concentrated, B = 64: the per-key call's median lies below the emulation's by more than both spreads together.
The first child that does not end with status 0 and a result line ends the job: no further child is started on the device."""
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
CHILD_LIMIT = int(os.environ.get("MEASURE_CHILD_SECONDS", 500))
BATCHES = (1, 8, 64, 256)
TOPK, POOL, CAP, RUN, COPIES = 10, 24, 1, 40, 30
LEVELS = (0.05, 0.25)
NQ = max(BATCHES)
RUN0 = (ROWS // RUN) // 2                                             # the planted documents are runs RUN0 .. RUN0 + 2 NQ - 1
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


def build(P, gen, dev, q_conc):
    """the synthetic shard with the planted documents: document d of query b is rows [RUN * (RUN0 + 2 b + d), + COPIES)"""
    import torch
    g = torch.Generator(device=dev).manual_seed(7)
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS + 1024)
    step = 32768
    for r0 in range(0, ROWS, step):
        m = min(step, ROWS - r0)
        emb = gen.embeddings(r0, m, DIM, dev)
        for run in range(max(RUN0, r0 // RUN), min(RUN0 + 2 * NQ, (r0 + m) // RUN + 1)):
            a = run * RUN
            if a < r0 or a + COPIES > r0 + m:
                continue
            b, d = divmod(run - RUN0, 2)
            v = q_conc[b]
            noise = torch.randn((COPIES, DIM), generator=g, device=dev, dtype=torch.float32)
            emb[a - r0:a - r0 + COPIES] = v[None, :] + noise * (LEVELS[d] * float(v.norm()) / DIM ** 0.5)
        pool, off = gen.contents(r0, m, dev)
        idx.append(emb, gen.created_ticks(r0, m, ROWS, dev), pool, off)
    del pool, off, emb
    torch.cuda.empty_cache()
    idx.seal()
    return idx


def alternating(calls):
    """{name: [ms]}: two warm rounds, then REPEATS rounds in which the calls take turns"""
    import torch
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
    return t


def families(P, gen, dev):
    q_conc = gen.query_vectors(0, NQ, DIM, ROWS, dev)
    q_spread = gen.query_vectors(NQ, NQ, DIM, ROWS, dev)
    terms = lambda b0: [P.text.query_terms(t) for t in gen.query_texts(b0, NQ, ROWS)]
    return {"concentrated": (q_conc, [[] for _ in range(NQ)]), "spread": (q_spread, terms(NQ))}


def emulate(idx, cand, q, terms, now, n_rows):
    """one batch through calls that exist without the feature, query by query; returns the rounds run"""
    rounds = []
    for b in range(len(terms)):
        qb, tb = q[b:b + 1], terms[b:b + 1]
        r = idx.search(qb, tb, now, POOL, candidate_limit=n_rows)
        kept, closed, seen, n_rounds = 0, set(), [], 0
        while True:
            n_rounds += 1
            n = int(r[2][0])
            for j in range(n):
                k = int(r[0][0, j]) // RUN
                if k in closed:
                    continue
                closed.add(k)                            # max_per_key 1: the first row of a key closes it
                kept += 1
                if kept >= TOPK:
                    break
            seen += r[0][0, :n].tolist()
            if kept >= TOPK or n < POOL:
                break
            gone = np.concatenate([np.arange(k * RUN, min(n_rows, k * RUN + RUN), dtype=np.int64) for k in closed] + [np.asarray(seen, np.int64)])
            ex, sc = idx.scope(gone), idx.scope(np.zeros(0, np.int64))
            sc.or_(cand).andnot(ex)
            r = idx.search_in_scope(qb, tb, now, POOL, sc, candidate_limit=n_rows)
            sc.close()
            ex.close()
        rounds.append(n_rounds)
    return rounds


def child(kind):
    import torch
    import __graft_entry__ as graft
    P = graft.load_package()
    gen = importlib.import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    fam = families(P, gen, dev)
    idx = build(P, gen, dev, fam["concentrated"][0])
    idx.set_option("two_stage", 1)
    now = gen.NOW_TICKS
    res = {"cells": []}
    kh = cand = None
    if kind == "this":
        ids = torch.arange(ROWS, dtype=torch.int64, device=dev)
        kh = idx.keys(ids, ids // RUN)
    else:
        cand = idx.scope_ticks(-(1 << 62), 1 << 62)
    for name, (q, terms) in fam.items():
        for B in BATCHES:
            qq, tt = q[:B].contiguous(), terms[:B]
            calls = {"plain": lambda: idx.search(qq, tt, now, POOL, candidate_limit=ROWS)}
            if kind == "this":
                calls["per_key"] = lambda: idx.search_per_key(qq, tt, now, TOPK, kh, max_per_key=CAP, pool=POOL, candidate_limit=ROWS)
            else:
                calls["emulation"] = lambda: emulate(idx, cand, qq, tt, now, ROWS)
            cell = dict(family=name, B=B, t=alternating(calls))
            if kind == "this":
                idx.set_profiling(1)
                got = calls["per_key"]()
                st = idx.kernel_stats()
                idx.set_profiling(0)
                cell.update(rounds=np.bincount(got[4], minlength=6).tolist(), kept=float(np.mean(got[3])),
                            kernels={k: [st[k]["total_ms"], st[k]["launches"]] for k in ("keys_exclude", "keys_clear_seen", "keys_gather", "scope_counts", "mask_clip_slots") if k in st})
            else:
                cell.update(rounds=np.bincount(calls["emulation"](), minlength=6).tolist())
            res["cells"].append(cell)
    if kind == "this":                                   # keys_remap inside a compaction and an insertion
        idx.set_profiling(1)
        idx.delete_rows(np.arange(5, 5 + 997 * 1000, 997, dtype=np.int64))
        t0 = time.perf_counter()
        idx.compact()
        t_compact = (time.perf_counter() - t0) * 1e3
        st = idx.kernel_stats()
        res["remap_compact"] = [st["keys_remap"]["total_ms"], st["keys_remap"]["launches"], t_compact]
        idx.set_profiling(0)
        idx.set_profiling(1)
        m = 131
        pool, off = gen.contents(ROWS, m, dev)
        t0 = time.perf_counter()
        idx.insert_rows(gen.embeddings(ROWS, m, DIM, dev), gen.created_ticks(ROWS // 2, m, ROWS, dev), pool, off,
                        row_ids=torch.arange(ROWS, ROWS + m, dtype=torch.int64, device=dev))
        t_insert = (time.perf_counter() - t0) * 1e3
        st = idx.kernel_stats()
        res["remap_insert"] = [st["keys_remap"]["total_ms"], st["keys_remap"]["launches"], t_insert]
        idx.set_profiling(0)
        kh.close()
    else:
        cand.close()
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
        return None, "exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-600:])
    return json.loads(lines[-1][7:]), None


def main():
    parent = os.environ.get("MEASURE_PARENT_ROOT")
    say("# per-key search (orr_search_batch_per_key) on ONE MI355X, one job, every timed build a child process on the same device")
    say("# shard %d x %d, int8 two-stage pass, keys in runs of %d rows, topk %d, pool %d, max_per_key %d, %d alternating repeats; ms, median (min-max)"
        % (ROWS, DIM, RUN, TOPK, POOL, CAP, REPEATS))
    this, err = run_child("this", HERE)
    if err:
        say("this build's child: %s -- nothing more is started" % err)
        return 1
    old = None
    if parent:
        old, err = run_child("parent", os.path.abspath(parent))
        if err:
            say("the parent build's child: %s -- nothing more is started" % err)
            return 1
    else:
        say("# no parent build was given (MEASURE_PARENT_ROOT): its columns and both bindings are left out")
    ok1, ok2 = True, None
    for i, c in enumerate(this["cells"]):
        plain, pk = stat(c["t"]["plain"]), stat(c["t"]["per_key"])
        line = "%-12s B %3d | search, topk = pool %s" % (c["family"], c["B"], fmt(plain))
        if old:
            o = old["cells"][i]
            pplain, emu = stat(o["t"]["plain"]), stat(o["t"]["emulation"])
            agree = abs(plain[0] - pplain[0]) <= (plain[2] - plain[1]) + (pplain[2] - pplain[1])
            ok1 = ok1 and agree
            line += " | parent build %s%s" % (fmt(pplain), "" if agree else " APART")
        line += " | search_per_key %s" % fmt(pk)
        if old:
            line += " | emulation, parent build %s (rounds 1/2/3/4+: %s)" % (fmt(emu), "/".join(str(x) for x in o["rounds"][1:4] + [sum(o["rounds"][4:])]))
            if c["family"] == "concentrated" and c["B"] == 64:
                ok2 = (emu[0] - pk[0]) > (pk[2] - pk[1]) + (emu[2] - emu[1])
        r = c["rounds"]
        line += " | rounds 1/2/3/4+: %d/%d/%d/%d, %.1f rows kept" % (r[1], r[2], r[3], sum(r[4:]), c["kept"])
        line += " | " + ", ".join("%s %.3f ms in %d launch(es)" % (k, v[0], v[1]) for k, v in sorted(c["kernels"].items()))
        say(line)
    say("keys_remap inside orr_index_compact (1,000 rows deleted): %.3f ms in %d launch; the whole compaction %.1f ms" % tuple(this["remap_compact"]))
    say("keys_remap inside orr_index_insert_rows (131 rows): %.3f ms in %d launch; the whole insertion %.1f ms" % tuple(this["remap_insert"]))
    if old:
        say("BINDING 1 (this build's plain search within the spreads of the parent build's, every cell): %s" % ("met" if ok1 else "NOT met"))
        say("BINDING 2 (concentrated, B = 64: search_per_key below the emulation by more than both spreads together): %s" % ("met" if ok2 else "NOT met"))
    return 0


if __name__ == "__main__":
    if CHILD:
        child(CHILD)
    else:
        sys.exit(main())
