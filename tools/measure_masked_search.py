"""python tools/measure_masked_search.py [out.txt [repeats]] -- what a masked search (orr_search_batch_masked, "mask_screen" = 1)
costs next to the scoped search of the same shared list (orr_search_batch_scoped, scope_off NULL) and the unscoped
orr_search_batch of the same batch, on one MI355X: a synthetic shard of MEASURE_ROWS x MEASURE_DIM (default 1,000,000 x 3072)
with the int8 shadow built, topk 10, candidate_limit = rows, a shared scope of S in {3,000, 30,000, 100,000, 500,000} rows
drawn at random over the shard, B in {1, 8, 256}.  The three calls alternate in one job.  Reported: ms per call (median, min,
max over the repeats), the kernels of the masked call (orr_index_kernel_stats) with the in-scope sample and the three new
kernels singled out, survivors per query behind the mask, the two binding comparisons, and the measured crossover of masked
against scoped next to the cost rule's (4 B S >= rows)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft   # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
ROWS = int(os.environ.get("MEASURE_ROWS", 1_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
SCOPES = (3_000, 30_000, 100_000, 500_000)
BATCHES = (1, 8, 256)
SAMPLE = ("mask_sample_compact", "mask_sample_rescore", "mask_sample_floor")
NEW = ("mask_clip", "row_consts_masked", "mask_survivors")
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


def main():
    P = graft.load_package()
    gen = __import__("importlib").import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    say("# masked search against the scoped search of the same shared list and the unscoped search;", torch.cuda.get_device_name(0))
    say("# shard %d x %d, int8 shadow built, topk 10, candidate_limit = rows, %d repeats, calls alternate" % (ROWS, DIM, REPEATS))
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
    idx.set_option("mask_screen", 1)
    rng = np.random.default_rng(5)
    table = {}
    for B in BATCHES:
        q = gen.query_vectors(0, B, DIM, ROWS, dev)
        terms = P.PackedTerms(P.pack_terms([P.text.query_terms(t) for t in gen.query_texts(0, B, ROWS)]))
        for S in SCOPES:
            ids_dev = torch.from_numpy(np.sort(rng.choice(ROWS, S, replace=False)).astype(np.int64)).to(dev)
            calls = {
                "masked": lambda: idx.search_masked(q, terms, gen.NOW_TICKS, 10, ids_dev, candidate_limit=ROWS),
                "scoped": lambda: idx.search_scoped(q, terms, gen.NOW_TICKS, 10, ids_dev, candidate_limit=ROWS),
                "unscoped": lambda: idx.search(q, terms, gen.NOW_TICKS, 10, candidate_limit=ROWS),
            }
            for call in calls.values():
                call()
                call()
            got = calls["masked"](), calls["scoped"]()
            same = all(np.array_equal(a, b) for a, b in zip(*got))
            t = {k: [] for k in calls}
            for _ in range(REPEATS):
                for k, call in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    t[k].append((time.perf_counter() - t0) * 1e3)
            s = {k: stat(v) for k, v in t.items()}
            table[(B, S)] = s
            say("")
            say("B = %d, shared scope of %d rows (masked == scoped: %s)" % (B, S, same))
            for k in calls:
                say("  %-9s" % k, fmt(s[k]))
            idx.reset_search_stats()
            idx.set_profiling(1)
            for _ in range(5):
                calls["masked"]()
            stats = idx.kernel_stats()
            idx.set_profiling(0)
            st = idx.search_stats(reset=True)
            us = {k: v["total_ms"] / 5 * 1e3 for k, v in stats.items() if v["launches"]}
            say("  kernels of the masked call (us per call): " + ", ".join("%s %.1f" % kv for kv in sorted(us.items(), key=lambda kv: -kv[1])))
            say("  in-scope sample %.1f us, the three new kernels %.1f us (%s); survivors per query %s, pass_mode %d, passes per call %.1f" %
                (sum(us.get(k, 0.0) for k in SAMPLE), sum(us.get(k, 0.0) for k in NEW), ", ".join("%s %.1f" % (k, us.get(k, 0.0)) for k in NEW),
                 st["survivors_per_query"], st["pass_mode"], st["passes"] / 5))
            if B == 256:
                gap = s["masked"][0] - s["unscoped"][0]
                say("  masked - unscoped (medians): %.3f ms; sample + new kernels: %.3f ms" %
                    (gap, (sum(us.get(k, 0.0) for k in SAMPLE) + sum(us.get(k, 0.0) for k in NEW)) / 1e3))
            if B == 256 and S == 100_000:
                m, sc = s["masked"], s["scoped"]
                spreads = (m[2] - m[1]) + (sc[2] - sc[1])
                say("  BINDING: scoped median - masked median = %.3f ms against both spreads together %.3f ms: %s; ratio %.1f x" %
                    (sc[0] - m[0], spreads, "met" if sc[0] - m[0] > spreads else "NOT met", sc[0] / m[0]))
    say("")
    say("crossover of masked against scoped (medians), beside the cost rule 4 B S >= rows:")
    for B in BATCHES:
        wins = [S for S in SCOPES if table[(B, S)]["masked"][0] < table[(B, S)]["scoped"][0]]
        rule = [S for S in SCOPES if 4 * B * S >= ROWS]
        say("  B = %3d: masked faster at S in %s; the rule takes the screen at S in %s (S >= %d)" % (B, wins, rule, -(-ROWS // (4 * B))))
    idx.close()


if __name__ == "__main__":
    main()
