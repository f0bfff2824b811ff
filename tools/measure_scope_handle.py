"""python tools/measure_scope_handle.py [out.txt [repeats]] -- what a search inside a scope handle (orr_search_batch_in_scope) costs
next to the masked search that resolves the same ids on every call (orr_search_batch_masked), on one MI355X: a synthetic shard
of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072) with the int8 shadow built, "mask_screen" = 1, topk 10,
candidate_limit = rows, ONE scope of S in {30,000, 500,000} rows drawn at random over the shard, B in {1, 8, 256}.  Three calls
alternate in one job: search_masked with the ids in HOST memory, the same with the ids already on the device, and
search_in_scope.  Reported: ms per call, median (min-max) over the repeats; what orr_scope_create and orr_scope_create_ticks
cost per S; the time of scope_remap per scope under one orr_index_compact and one orr_index_insert_rows with four scopes
registered; and the one binding ordering (B = 1, S = 500,000).

MEASURE_PARENT_ROOT=<a built checkout of the parent commit>: the host-id search_masked column is also timed from that build,
in a child process of this job on the same device (the yardstick for code this change must not slow down)."""
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.environ.get("MEASURE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
MASKED_ONLY = "--masked-only" in sys.argv          # the child's mode: only the host-id search_masked column
OUT = ARGS[0] if ARGS else None
REPEATS = int(ARGS[1]) if len(ARGS) > 1 else 15
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
SCOPES = (30_000, 500_000)
BATCHES = (1, 8, 256)
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


def build(P, gen, dev, spare=0):
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS + spare)
    step = 32768
    for r0 in range(0, ROWS, step):
        m = min(step, ROWS - r0)
        pool, off = gen.contents(r0, m, dev)
        idx.append(gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, ROWS, dev), pool, off)
    del pool, off
    torch.cuda.empty_cache()
    idx.seal()
    idx.set_option("two_stage", 1)
    idx.set_option("mask_screen", 1)
    return idx


def timed(calls):
    for call in calls.values():
        call()
        call()
    t = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stat(v) for k, v in t.items()}


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    P = graft.load_package()
    gen = __import__("importlib").import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    if MASKED_ONLY:
        say("# search_masked with the ids in host memory, from a build of the parent commit (MEASURE_PARENT_ROOT), a child process of the same job")
    else:
        say("# search inside a scope handle against the masked search that resolves the same ids per call;", torch.cuda.get_device_name(0))
    say("# shard %d x %d, int8 shadow built, mask_screen 1, topk 10, candidate_limit = rows, %d repeats, calls alternate; ms, median (min-max)"
        % (ROWS, DIM, REPEATS))
    idx = build(P, gen, dev, spare=0 if MASKED_ONLY else 4096)
    rng = np.random.default_rng(5)
    scope_ids = {S: np.sort(rng.choice(ROWS, S, replace=False)).astype(np.int64) for S in SCOPES}      # (row ids are positions here)
    table = {}
    handles = {}
    if not MASKED_ONLY:
        say("")
        for S in SCOPES:
            ids = scope_ids[S]
            idx.scope(ids).close()                                   # (the first call builds the id table)
            t_create = []
            for _ in range(5):
                sc, ms = once(lambda: idx.scope(ids))
                t_create.append(ms)
                sc.close()
            created = gen.created_ticks(0, ROWS, ROWS).numpy()
            t0, t1 = int(created[(ROWS + S) // 2]), int(created[(ROWS - S) // 2])
            t_ticks = []
            for _ in range(5):
                sc, ms = once(lambda: idx.scope_ticks(t0, t1))
                t_ticks.append(ms)
                rows_ticks = sc.rows
                sc.close()
            handles[S] = idx.scope(ids)
            say("S = %7d: orr_scope_create (ids in host memory) %s; orr_scope_create_ticks of a window of %d rows %s"
                % (S, fmt(stat(t_create)), rows_ticks, fmt(stat(t_ticks))))
    for B in BATCHES:
        q = gen.query_vectors(0, B, DIM, ROWS, dev)
        terms = P.PackedTerms(P.pack_terms([P.text.query_terms(t) for t in gen.query_texts(0, B, ROWS)]))
        for S in SCOPES:
            ids_host = scope_ids[S]
            calls = {"masked, host ids": lambda: idx.search_masked(q, terms, gen.NOW_TICKS, 10, ids_host, candidate_limit=ROWS)}
            if not MASKED_ONLY:
                ids_dev = torch.from_numpy(ids_host).to(dev)
                sc = handles[S]
                calls["masked, device ids"] = lambda: idx.search_masked(q, terms, gen.NOW_TICKS, 10, ids_dev, candidate_limit=ROWS)
                calls["in scope"] = lambda: idx.search_in_scope(q, terms, gen.NOW_TICKS, 10, sc, candidate_limit=ROWS)
            s = timed(calls)
            table[(B, S)] = s
            same = ""
            if not MASKED_ONLY:
                got = calls["masked, host ids"](), calls["in scope"]()
                same = " (in scope == masked: %s, pass_mode %d)" % (all(np.array_equal(a, b) for a, b in zip(*got)), idx.search_stats()["pass_mode"])
            say("")
            say("B = %d, S = %d%s" % (B, S, same))
            for k in calls:
                say("  %-19s" % k, fmt(s[k]))
            if not MASKED_ONLY and B == 1 and S == 500_000:
                m, h = s["masked, host ids"], s["in scope"]
                spreads = (m[2] - m[1]) + (h[2] - h[1])
                say("  BINDING: masked (host ids) median - in-scope median = %.3f ms against both spreads together %.3f ms: %s; ratio %.1f x"
                    % (m[0] - h[0], spreads, "met" if m[0] - h[0] > spreads else "NOT met", m[0] / h[0]))
    if MASKED_ONLY:
        idx.close()
        return
    # ---- scope_remap under one compact and one insert, four scopes registered
    say("")
    more = [idx.scope_ticks(int(created[ROWS // 2]), int(created[0]) + 1), idx.scope(scope_ids[30_000][::2])]
    n_scopes = len(handles) + len(more)
    before = {S: handles[S].rows for S in SCOPES}
    gone = scope_ids[500_000][::500]
    assert idx.delete_rows(gone) == len(gone)
    idx.set_profiling(1)
    _, ms = once(idx.compact)
    st = idx.kernel_stats().get("scope_remap")
    say("orr_index_compact after %d deletes: %.1f ms in all; scope_remap for %d scopes %.3f ms = %.3f ms per scope"
        % (len(gone), ms, n_scopes, st["total_ms"], st["total_ms"] / n_scopes))
    assert handles[500_000].rows == before[500_000] - len(gone)
    m = 1024
    pool, off = gen.contents(ROWS, m, dev)
    new_ticks = torch.from_numpy(created[rng.choice(ROWS, m, replace=False)].copy())
    idx.set_profiling(1)
    _, ms = once(lambda: idx.insert_rows(gen.embeddings(ROWS, m, DIM, dev), new_ticks, pool, off,
                                         row_ids=np.arange(ROWS, ROWS + m, dtype=np.int64)))
    st = idx.kernel_stats().get("scope_remap")
    idx.set_profiling(0)
    say("orr_index_insert_rows of %d rows spread over the shard: %.1f ms in all; scope_remap for %d scopes %.3f ms = %.3f ms per scope"
        % (m, ms, n_scopes, st["total_ms"], st["total_ms"] / n_scopes))
    assert handles[500_000].rows == before[500_000] - len(gone)
    for sc in list(handles.values()) + more:
        sc.close()
    idx.close()
    parent = os.environ.get("MEASURE_PARENT_ROOT")
    if parent:                                                       # a fresh process: its own library, its own shard, this device
        say("")
        env = dict(os.environ, MEASURE_ROOT=parent)
        torch.cuda.empty_cache()
        try:                                                         # (one shard build and 6 x REPEATS searches: minutes at the most)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--masked-only", "/dev/null", str(REPEATS)], env=env,
                               capture_output=True, text=True, timeout=420)
            out = r.stdout + (r.stderr if r.returncode else "")
        except subprocess.TimeoutExpired as e:
            out = (e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode("utf-8", "replace")) + "\nthe parent build's run did not end within 420 s and was stopped"
        for line in out.splitlines():
            say("parent |", line)
    say("")
    say("not taken: the figures on a 10M-row shard, and scopes of 5M rows.")


if __name__ == "__main__":
    main()
