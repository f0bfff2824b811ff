"""python tools/measure_insert_rows.py [out.json] -- measurements for orr_index_insert_rows on a 10M x 3072 shard (int8 shadow built, capacity reserved): 1,000 and 100,000
rows, all in front and all behind, split into phases; the rebuild (append + seal + shadow) in the same job; the merge kernel's
bytes per second against hipMemcpyAsync device-to-device."""
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft   # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None            # where the results go as JSON, besides the lines printed
ROWS = int(os.environ.get("MEASURE_ROWS", 10_000_000))
DIM = int(os.environ.get("MEASURE_DIM", 3072))


def main():
    P = graft.load_package()
    gen = __import__("importlib").import_module(graft.PKG_NAME + ".synthetic")
    dev = torch.device("cuda:0")
    res = {"rows": ROWS, "dim": DIM, "device": torch.cuda.get_device_name(0)}

    def dump():
        if OUT:
            with open(OUT, "w") as f:
                json.dump(res, f, indent=1)

    # ---- the yardstick: append + seal + int8 shadow of the same shard
    extra = 1000 + 1000 + 100_000 + 100_000
    idx = P.RecallIndex(dim=DIM, device=0, capacity_rows=ROWS + extra)
    t_append = 0.0
    step = 32768
    for r0 in range(0, ROWS, step):
        m = min(step, ROWS - r0)
        pool, off = gen.contents(r0, m, dev)
        emb = gen.embeddings(r0, m, DIM, dev)
        created = gen.created_ticks(r0, m, ROWS, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx.append(emb, created, pool, off)
        t_append += time.perf_counter() - t0
        if (r0 // step) % 32 == 0:
            print('appended', r0 + m, flush=True)
    del pool, off, emb, created
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    idx.seal()
    t_seal = time.perf_counter() - t0
    t0 = time.perf_counter()
    idx.set_option("two_stage", 1)
    t_shadow = time.perf_counter() - t0
    res["rebuild_s"] = {"append": t_append, "seal": t_seal, "shadow": t_shadow, "total": t_append + t_seal + t_shadow}
    print("rebuild", res["rebuild_s"], flush=True)
    dump()

    B = 8
    q = gen.query_vectors(0, B, DIM, ROWS, dev)
    terms = [P.text.query_terms(t) for t in gen.query_texts(0, B, ROWS)]
    idx.search(q, terms, gen.NOW_TICKS, 10, candidate_limit=ROWS)
    res["pass_mode_before"] = idx.search_stats()["pass_mode"]
    oldest = int(gen.created_ticks(ROWS - 1, 1, ROWS, "cpu")[0])

    # ---- the inserts
    res["inserts"] = []
    next_id = ROWS
    for n_new, where in ((1000, "front"), (1000, "behind"), (100_000, "front"), (100_000, "behind")):
        emb = gen.embeddings(next_id, n_new, DIM, dev)
        pool, off = gen.contents(next_id, n_new, dev)
        ar = torch.arange(n_new, dtype=torch.int64, device=dev)
        created = (gen.NOW_TICKS + 10**9 * (1 + len(res["inserts"])) - ar) if where == "front" else (oldest - 10**9 * (1 + len(res["inserts"])) - ar)
        ids = next_id + ar
        torch.cuda.synchronize()
        idx.set_profiling(1)                                      # (resets the counters)
        rows_before = idx.rows
        t0 = time.perf_counter()
        done = idx.insert_rows(emb, created.contiguous(), pool, off, row_ids=ids.contiguous())
        wall = time.perf_counter() - t0
        stats = idx.kernel_stats()
        idx.set_profiling(0)
        assert done == n_new and idx.rows == rows_before + n_new
        t0 = time.perf_counter()
        rows, scores, counts = idx.search(q, terms, gen.NOW_TICKS, 10, candidate_limit=idx.rows)
        first_search = time.perf_counter() - t0
        entry = {"rows": n_new, "where": where, "wall_s": wall, "first_search_s": first_search,
                 "pass_mode_after": idx.search_stats()["pass_mode"], "phases": stats}
        for name in ("merge_rows_f32_direct", "merge_rows_f32_bounce"):
            if name in stats and stats[name]["total_ms"] > 0:
                entry[name + "_TBps"] = stats[name]["algo_bytes"] / (stats[name]["total_ms"] * 1e-3) / 1e12
        res["inserts"].append(entry)
        print(json.dumps(entry), flush=True)
        dump()
        next_id += n_new
        del emb, pool, off, created, ids
        torch.cuda.empty_cache()

    # ---- hipMemcpyAsync device to device in the same job: chunks of 256 MiB like the merge kernel's launches, and one copy
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    chunk = (256 << 20) // (4 * DIM) * (4 * DIM)
    n_chunks = 32
    src = torch.empty(chunk * n_chunks, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    memcpy = {}
    for label, pieces in (("chunks_256MiB", n_chunks), ("one_copy", 1)):
        size = chunk * n_chunks // pieces
        best = None
        for rep in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream = torch.cuda.current_stream().cuda_stream
            e0.record()
            for i in range(pieces):
                rc = hip.hipMemcpyAsync(dst.data_ptr() + i * size, src.data_ptr() + i * size, size, 3, stream)
                assert rc == 0
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        memcpy[label] = {"bytes_read_plus_written": 2 * chunk * n_chunks, "best_ms": best, "TBps": 2 * chunk * n_chunks / (best * 1e-3) / 1e12}
    res["memcpy_d2d"] = memcpy
    print("memcpy", json.dumps(memcpy), flush=True)
    dump()
    idx.close()


if __name__ == "__main__":
    main()
