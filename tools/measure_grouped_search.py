"""python tools/measure_grouped_search.py [out.txt [repeats]] -- what a grouped masked search (orr_search_batch_masked_groups)
costs next to the loop of G masked searches (orr_search_batch_masked, one per group with that group's queries: what the library
offered before), on one MI355X: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072) with the int8 shadow
built, topk 10, candidate_limit = rows, G disjoint random groups of S rows each, the B queries assigned to the groups in turn.
Cells: G in {2, 8} x S in {3,000, 30,000, 100,000} x B in {8, 256}, and G = 1 (S = 100,000, B = 256).  In each cell three arms
alternate: the loop ("mask_screen" = 0: each masked call picks its own pass), the grouped call forced onto the grouped screen
("mask_screen" = 1) and the grouped call under the cost rule ("mask_screen" = 0).  MEASURE_CELLS="G:S:B,..." restricts the
cells.  Reported: ms per call (median, min, max over the repeats), whether grouped and looped calls returned identical arrays,
what the rule chose (pass_mode) beside the measured winner, the kernels of the forced grouped call (orr_index_kernel_stats) with the two new kernels and the sample stages singled
out, and the survivors per query in front of and behind the filter.

MEASURE_LOOP_ONLY=1 runs only the loop arm, through nothing but search_masked -- so that MEASURE_TREE=<a checkout of the parent
commit, built> gives the yardstick from code without this call (the figures of both trees belong side by side)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.environ.get("MEASURE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft   # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
LOOP_ONLY = os.environ.get("MEASURE_LOOP_ONLY") == "1"
CELLS = [(1, 100_000, 256)] + [(G, S, B) for B in (8, 256) for G in (2, 8) for S in (3_000, 30_000, 100_000)]
if LOOP_ONLY:
    CELLS = [(1, 100_000, 256), (8, 100_000, 256)]
if os.environ.get("MEASURE_CELLS"):                      # "G:S:B,G:S:B": only these cells
    CELLS = [tuple(int(x) for x in c.split(":")) for c in os.environ["MEASURE_CELLS"].split(",")]
SAMPLE = ("mask_sample_compact", "mask_sample_rescore", "mask_sample_floor")
NEW = ("row_consts_grouped", "mask_survivors_grouped")
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
    return "median %.3f  min %.3f  max %.3f ms" % s


def kernel_stats(P, idx):
    return {k: (v["launches"], v["total_ms"], v["algo_bytes"]) for k, v in idx.kernel_stats().items()}


def main():
    P = graft.load_package()
    gen = __import__("importlib").import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    say("# grouped masked search against the loop of one masked search per group;", torch.cuda.get_device_name(0), "; tree", "parent" if LOOP_ONLY else "this")
    say("# shard %d x %d, int8 shadow built, topk 10, candidate_limit = rows, %d repeats, arms alternate" % (ROWS, DIM, REPEATS))
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS)
    step = 32768
    for r0 in range(0, ROWS, step):
        m = min(step, ROWS - r0)
        pool, off = gen.contents(r0, m, dev)
        idx.append(gen.embeddings(r0, m, DIM, dev), gen.created_ticks(r0, m, ROWS, dev), pool, off)
    del pool, off
    torch.cuda.empty_cache()
    idx.seal()
    idx.set_option("two_stage", 1)
    rng = np.random.default_rng(5)
    agree = []
    for G, S, B in CELLS:
        q = gen.query_vectors(0, B, DIM, ROWS, dev)
        texts = gen.query_texts(0, B, ROWS)
        all_terms = [P.text.query_terms(t) for t in texts]
        terms = P.PackedTerms(P.pack_terms(all_terms))
        qg = (np.arange(B) % G).astype(np.int32)
        perm = rng.permutation(ROWS)[: G * S].astype(np.int64)
        groups = [np.sort(perm[g * S:(g + 1) * S]) for g in range(G)]
        flat = torch.from_numpy(np.concatenate(groups)).to(dev)
        off = (np.arange(G + 1) * S).astype(np.uint64)
        ids_dev = [flat[g * S:(g + 1) * S] for g in range(G)]
        members = [np.nonzero(qg == g)[0] for g in range(G)]
        sub_q = [q[torch.from_numpy(m).to(dev)].contiguous() for m in members]
        sub_terms = [P.PackedTerms(P.pack_terms([all_terms[b] for b in m])) for m in members]

        def loop():
            idx.set_option("mask_screen", 0)
            return [idx.search_masked(sub_q[g], sub_terms[g], gen.NOW_TICKS, 10, ids_dev[g], candidate_limit=ROWS) for g in range(G) if len(members[g])]

        def grouped(mode):
            idx.set_option("mask_screen", mode)
            return idx.search_masked_groups(q, terms, gen.NOW_TICKS, 10, flat, qg, candidate_limit=ROWS, group_off=off)

        calls = {"loop": loop} if LOOP_ONLY else {"loop": loop, "grouped forced": lambda: grouped(1), "grouped by rule": lambda: grouped(0)}
        for call in calls.values():
            call()
            call()
        same = None
        if not LOOP_ONLY:
            lo, gf, gr = calls["loop"](), calls["grouped forced"](), calls["grouped by rule"]()
            used = [g for g in range(G) if len(members[g])]
            same = all(np.array_equal(got[i][members[g]], lo[j][i]) for got in (gf, gr) for j, g in enumerate(used) for i in range(3))
        t = {k: [] for k in calls}
        for _ in range(REPEATS):
            for k, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                t[k].append((time.perf_counter() - t0) * 1e3)
        s = {k: stat(v) for k, v in t.items()}
        say("")
        say("G = %d groups of %d rows, B = %d (%s queries per group)%s" % (G, S, B, "/".join(str(len(m)) for m in members[:2]) + ("/.." if G > 2 else ""),
                                                                        "" if same is None else " (grouped == looped: %s)" % same))
        for k in calls:
            say("  %-16s" % k, fmt(s[k]))
        if LOOP_ONLY:
            continue
        idx.reset_search_stats()
        grouped(0)
        mode = idx.search_stats(reset=True)["pass_mode"]
        chose = mode == 6
        lo_s, gf_s = s["loop"], s["grouped forced"]
        winner = gf_s[0] < lo_s[0]
        if G > 1:
            agree.append((G, S, B, chose, winner, gf_s[0], lo_s[0]))
            say("  the rule (mask_screen = 0) %s the grouped screen (pass_mode %d); measured winner: %s (%.3f against %.3f ms)%s" %
                ("chose" if chose else "did not choose", mode, "grouped" if winner else "loop", gf_s[0], lo_s[0], "" if chose == winner else "  <-- DISAGREE"))
        idx.set_profiling(1)
        for _ in range(5):
            grouped(1)
        stats = kernel_stats(P, idx)
        idx.set_profiling(0)
        st = idx.search_stats(reset=True)
        us = {k: v[1] / 5 * 1e3 for k, v in stats.items() if v[0] and k != "grouped_screen_pairs"}
        say("  kernels of the forced grouped call (us per call): " + ", ".join("%s %.1f" % kv for kv in sorted(us.items(), key=lambda kv: -kv[1])))
        before = stats["grouped_screen_pairs"][2] / 16.0 / st["survivor_samples"] if "grouped_screen_pairs" in stats and st["survivor_samples"] else None
        say("  in-scope sample %.1f us (%s); the two new kernels %s; survivors per query in front of the filter %s, behind it %s; pass_mode %d, passes per call %.1f" %
            (sum(us.get(k, 0.0) for k in SAMPLE), ", ".join("%s %.1f" % (k, us.get(k, 0.0)) for k in SAMPLE), ", ".join("%s %.1f" % (k, us.get(k, 0.0)) for k in NEW),
             "%.0f" % before if before is not None else "-", st["survivors_per_query"], st["pass_mode"], st["passes"] / 5))
        spreads = (gf_s[2] - gf_s[1]) + (lo_s[2] - lo_s[1])
        if (G, S, B) == (8, 100_000, 256):
            say("  BINDING 1: loop median - grouped median = %.3f ms against both spreads together %.3f ms: %s; ratio %.1f x" %
                (lo_s[0] - gf_s[0], spreads, "met" if lo_s[0] - gf_s[0] > spreads else "NOT met", lo_s[0] / gf_s[0]))
        if G == 1:
            say("  BINDING 2: |grouped - masked| (medians) = %.3f ms against both spreads together %.3f ms: %s" %
                (abs(gf_s[0] - lo_s[0]), spreads, "met" if abs(gf_s[0] - lo_s[0]) <= spreads else "NOT met"))
    if agree:
        say("")
        say("cost rule (sum over the screen groups of max(max(4 B_g, 128) x took_g, 2^19) >= n_clip) against the measured winner:")
        for G, S, B, chose, winner, gm, lm in agree:
            say("  G = %d, S = %6d, B = %3d: rule %-7s measured %-7s (grouped %.3f, loop %.3f ms) %s" %
                (G, S, B, "grouped" if chose else "loop", "grouped" if winner else "loop", gm, lm, "agree" if chose == winner else "DISAGREE"))
    idx.close()


if __name__ == "__main__":
    main()
