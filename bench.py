#!/usr/bin/env python3
"""bench.py -- queries/sec of the hybrid recall-search hot path on MI355X.

One GPU (`python bench.py [--gpus 1]`), headline = BASELINE.json configs[2], "C3":
10M chunks x 3072-d fp32 resident on one MI355X, 256 queries per step, top-k = 10, full hybrid
score (cosine + keyword + recency fused 0.7/0.2/0.1), candidate_limit = whole corpus.

A plain run does what the headline figure needs and nothing else: it builds the corpus, runs the warm-up
and the timed steps, writes --dump-outputs and prints the line.  `--full` adds the rest: the legs
(configs[1] "C2": 1M chunks, one query per step, and the robustness legs on one GPU; C4, cluster and
strong-scaling legs on several), two steps in flight, the per-kernel table, roofline.traffic measured by
rocprofv3 child runs, the host probe, the parity block (HIP path against the oracle on a candidate_limit
prefix of the headline corpus) and the CPU baseline.  The --no-* options trim a --full run.

N > 1 GPUs (`--gpus N`; started plainly it spawns `python -m torch.distributed.run` as a CHILD before
anything touches a GPU, started under torch.distributed.run it is one rank): 12.5M rows per GPU (the
per-GPU shape of configs[3]/[4], 100M rows over 8 GPUs), row-sharded, one process per GPU.  Rank 0
originates a batch of 1024 queries per step (C5, full hybrid), broadcasts it, every rank scores all of
them against its shard, ONE all-gather of per-shard top-k' records over RCCL, host merge.  Legs: C4
(cosine only) with 1 and 256 queries per step.  Weak scaling: rows per GPU and queries per step are
fixed, the corpus grows with N; value = queries answered per second by the whole job.

A step is one pass of the hot path over one batch.  Inputs are resident in HBM before the timed
region; results land in host memory inside it.  Results are exact (the reference's arithmetic): the
library screens the corpus through an int8 shadow with a rigorous per-pair bound and re-scores the
survivors from the fp32 master in f32 x f32 -> f64.  The oracle is used here ONLY for
the `cpu_baseline` / `parity` leg of a --full run, never inside a timed GPU region.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# Peaks the roofline fractions are priced against (MI355X_MICROARCH.md, chip-level parameters; dense, no
# sparsity).  host_probe() re-reads what the box reports (CUs, max clock) and records it beside them.
HBM_PEAK_GBS = 8000.0            # HBM3E spec; 6.29 TB/s is the measured copy ceiling
MFMA_BF16_PEAK_TFLOPS = 2500.0
MFMA_I8_PEAK_TOPS = 5000.0
# What the matrix cores of a whole MI355X sustain on v_mfma_i32_32x32x32_i8 with NOTHING else going on (tools/mfma_rate.hip, one
# wave per SIMD on all 256 CUs, profiles/r02_mfma_rate_microbench.txt): 32.1 cycles per MFMA, but the chip holds 1.60 GHz
# under that load, not 2.4 -- 65536 ops x 1024 SIMDs / (32.1 / 1.60e9 s).  The dense peak above is never reachable for a
# full-chip launch of a millisecond or more; reported beside it, not instead of it.
MFMA_I8_SUSTAINED_TOPS = 65536.0 * 1024.0 / (32.1 / 1.60e9) / 1e12       # ~3345
I8_CROSSOVER_B = MFMA_I8_PEAK_TOPS * 1e12 / (HBM_PEAK_GBS * 1e9) / 2.0     # queries per int8 row byte: 312.5


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows-per-gpu", type=int, default=0, help="0 = 10,000,000 on one GPU (C3), 12,500,000 per GPU on several (C4/C5)")
    ap.add_argument("--dim", type=int, default=3072)
    ap.add_argument("--batch", type=int, default=0, help="queries per step of the whole job; 0 = 256 on one GPU (C3), 1024 on several (C5)")
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beside the headline as well: legs, two steps in flight, the kernel table, "
                         "roofline.traffic from rocprofv3, the host probe, parity and the CPU baseline (the --no-* options trim it)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the oracle leg (cpu_baseline + parity)")
    ap.add_argument("--cpu-sample-rows", type=int, default=262144)
    ap.add_argument("--cpu-sample-queries", type=int, default=96)
    ap.add_argument("--no-pmc", action="store_true",
                    help="do not measure roofline.traffic in this run (two rocprofv3 --pmc child runs of the headline shape, FETCH_SIZE and "
                         "WRITE_SIZE, before this process touches the GPU); the committed figure of the same shape is quoted instead")
    ap.add_argument("--no-legs", action="store_true", help="headline only: skip the C2 leg (one GPU) / the C4 legs (several)")
    ap.add_argument("--no-overlap-leg", action="store_true", help="skip the two-steps-in-flight measurements (headline and C2 leg: reported beside `value`, never as it)")
    ap.add_argument("--no-robustness-legs", action="store_true",
                    help="skip the two 1M-row legs on unfriendly data: a clustered corpus (64 centroids + 0.1 noise: thousands of "
                         "survivors per query) and a keyword-heavy one (2^18 Zipf-distributed tokens of mixed length, substring terms)")
    ap.add_argument("--no-terms", action="store_true", help="headline without keyword terms (cosine + recency only)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend of a multi-GPU run: nccl (= RCCL, the product path) or gloo (a rehearsal of the same "
                         "code with several ranks on ONE card, which RCCL refuses; ranks then share cuda:0)")
    ap.add_argument("--mode", default="ranks", choices=["ranks", "cluster"],
                    help="several GPUs: 'ranks' = one process per GPU + RCCL (torch.distributed; what the driver launches); 'cluster' = ONE "
                         "process driving all --gpus devices through orr_cluster_search_batch (the form a C# host loads, INTEGRATION.md 5a)")
    ap.add_argument("--cluster-exchange", default="host", choices=["host", "rccl"],
                    help="--mode cluster: how the per-shard records reach the merge: pinned host memory (default) or ONE RCCL all-gather "
                         "(orr_cluster_set_option exchange=1)")
    ap.add_argument("--cluster-oversubscribe", action="store_true",
                    help="rehearsal only: --mode cluster with more shards than visible devices (shards share cards, device g %% visible)")
    ap.add_argument("--dist-rehearsal", action="store_true",
                    help="rehearsal only: take the multi-rank branch (torch.distributed, the sharded front end, its legs) with the ranks "
                         "there are -- with --gpus 1 under torch.distributed.run that is RCCL itself with one rank on a one-GPU box")
    ap.add_argument("--strong-rows", type=int, default=10_000_000, help="total rows of the fixed-N (strong-scaling) leg of a multi-GPU run; 0 = skip")
    ap.add_argument("--cluster-leg-rows", type=int, default=1_000_000, help="rows per device of the in-process orr_cluster leg of a multi-GPU run; 0 = skip")
    ap.add_argument("--set-option", action="append", default=[], metavar="NAME=VALUE",
                    help="orr_index_set_option on every shard before the run (e.g. two_stage=0)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the headline's last timed step returned (rows, scores, counts of every "
                         "query) as DIR/<name>.npy in float64; the inputs are a pure function of the arguments, so two builds "
                         "run with the same arguments can be compared output for output")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:          # a plain run: the headline alone
        args.no_legs = args.no_overlap_leg = args.no_cpu_baseline = args.no_pmc = True
    return args


# ------------------------------------------------------------------------------------------------
# host probes: all of them child processes, all before this process touches the GPU
# ------------------------------------------------------------------------------------------------
def _run_quiet(cmd, timeout=30):
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
        return p.returncode, p.stdout.decode(errors="replace")
    except FileNotFoundError:
        return None, ""
    except Exception as exc:                       # timeouts, permissions
        return -1, repr(exc)


def host_probe():
    """dotnet, core counts, and what rocminfo says about the GPU."""
    out = {"os_cpu_count": os.cpu_count()}
    try:
        out["cpus_in_affinity_mask"] = len(os.sched_getaffinity(0))
    except Exception:
        pass
    out["cpu_quota"] = cgroup_cpu_quota()
    rc, txt = _run_quiet(["dotnet", "--version"])
    out["dotnet"] = txt.strip().splitlines()[0] if rc == 0 and txt.strip() else "unavailable"
    rc, txt = _run_quiet(["/opt/rocm/bin/rocminfo"])
    if rc == 0:
        agents = txt.split("*******")
        for a in agents:
            if "gfx950" in a and "Compute Unit" in a:
                m_cu = re.search(r"Compute Unit:\s+(\d+)", a)
                m_clk = re.search(r"Max Clock Freq\. \(MHz\):\s+(\d+)", a)
                m_name = re.search(r"Marketing Name:[ \t]+(\S.*)", a)
                out["gpu"] = {"name": m_name.group(1).strip() if m_name else None,
                              "compute_units": int(m_cu.group(1)) if m_cu else None,
                              "max_clock_mhz": int(m_clk.group(1)) if m_clk else None}
                break
    gpu = out.get("gpu") or {}
    if gpu.get("compute_units") and gpu.get("max_clock_mhz"):
        # dense int8 MFMA: 32x32x32 x 2 ops per 32 cycles per SIMD, 4 SIMDs per CU
        gpu["mfma_i8_peak_tops_at_max_clock"] = gpu["compute_units"] * 4 * 2048 * gpu["max_clock_mhz"] * 1e6 / 1e12
    return out


def cgroup_cpu_quota():
    """CPUs the container may actually use (cgroup v2 `cpu.max`, v1 `cpu.cfs_quota_us / cpu.cfs_period_us`); None = no limit
    set.  Reported beside os_cpu_count: a 256-CPU box hands a one-GPU container about 16 cores."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        return None if quota == "max" else round(int(quota) / int(period), 2)
    except Exception:
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            quota = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            period = int(f.read())
        return None if quota <= 0 else round(quota / period, 2)
    except Exception:
        return None


PMC_KERNEL_SYMBOLS = {"screen_i8_fused": ("screen_tile16_kernel", "screen_tile4_kernel", "screen_bf16_kernel<true, true"),
                      "screen_gemv_i8": ("screen_gemv_i8_kernel",), "screen_gemv_bf16": ("screen_gemv_bf16_kernel",),
                      "screen_bf16_fused": ("screen_bf16_kernel<true, false",), "dot_exact": ("dot_exact_tiled",)}


def measure_traffic(args):
    """roofline.traffic measured IN THIS RUN: HBM bytes per launch of the headline's kernels from the PMC counters, collected as
    MI355X_MICROARCH.md (HBM / rocprofv3) prescribes -- FETCH_SIZE and WRITE_SIZE in SEPARATE passes (they do not fit one), with
    --kernel-trace only; both counters read in KiB; on gfx950 FETCH_SIZE reports half the bytes of a wide coalesced stream, so
    bytes = 2 x FETCH_SIZE + WRITE_SIZE.  Two child runs of the headline shape (3 steps each) BEFORE this process touches the GPU.
    Returns {kernel name: {bytes_per_launch, launches, ...}} or {"error": ...}."""
    import csv
    import glob
    import shutil
    import tempfile
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return {"error": "rocprofv3 not found"}
    child = [sys.executable if os.path.basename(sys.executable).startswith("python") else "python3", os.path.abspath(__file__),
             "--gpus", "1", "--full", "--no-legs", "--no-overlap-leg", "--no-cpu-baseline", "--no-pmc", "--steps", "3", "--warmup", "2",
             "--dim", str(args.dim), "--topk", str(args.topk), "--rows-per-gpu", str(args.rows_per_gpu), "--batch", str(args.batch)]
    for o in args.set_option:
        child += ["--set-option", o]
    if args.no_terms:
        child.append("--no-terms")
    out, t0 = {}, time.perf_counter()
    sums = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        tmp = tempfile.mkdtemp(prefix="orr_pmc_")
        try:
            cmd = [rocprof, "--output-format", "csv", "--kernel-trace", "--pmc", counter, "-d", tmp, "--"] + child
            env = dict(os.environ, TMPDIR="/tmp")
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240, env=env, cwd="/tmp")
            files = glob.glob(os.path.join(tmp, "**", "*_counter_collection.csv"), recursive=True)
            if p.returncode != 0 or not files:
                return {"error": "rocprofv3 --pmc %s: rc %d, %d csv file(s): %s" % (counter, p.returncode, len(files), p.stderr.decode(errors="replace")[-160:])}
            for f in files:
                with open(f, newline="") as fh:
                    for r in csv.DictReader(fh):
                        if r.get("Counter_Name") != counter:
                            continue
                        for name, symbols in PMC_KERNEL_SYMBOLS.items():
                            if any(sym in r["Kernel_Name"] for sym in symbols):
                                e = sums.setdefault(name, {}).setdefault(counter, [0.0, 0])
                                e[0] += float(r["Counter_Value"])
                                e[1] += 1
        except Exception as exc:                       # a timeout, a refused profiler: the committed figure is quoted instead
            return {"error": "%s: %s" % (type(exc).__name__, str(exc)[:160])}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    for name, cs in sums.items():
        if "FETCH_SIZE" in cs and cs["FETCH_SIZE"][1]:
            fetch = cs["FETCH_SIZE"][0] / cs["FETCH_SIZE"][1] * 1024.0
            write = (cs["WRITE_SIZE"][0] / cs["WRITE_SIZE"][1] * 1024.0) if cs.get("WRITE_SIZE", [0, 0])[1] else 0.0
            out[name] = {"hbm_bytes_per_launch": 2.0 * fetch + write, "fetch_size_bytes_avg": fetch, "write_size_bytes_avg": write,
                         "launches_seen": cs["FETCH_SIZE"][1]}
    out["seconds"] = round(time.perf_counter() - t0, 1)
    out["how"] = ("this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate child runs of the headline shape, 3 steps), "
                  "bytes = 2 x FETCH_SIZE + WRITE_SIZE per launch, counters in KiB (MI355X_MICROARCH.md, HBM)")
    return out


def spawn_ranks(args, argv):
    """`--gpus N` started without a launcher: run torch.distributed.run as a CHILD (this process has not touched
    the GPU and never will) and relay its output."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run(cmd, env=env)
    raise SystemExit(p.returncode)


# ------------------------------------------------------------------------------------------------
# corpus and legs
# ------------------------------------------------------------------------------------------------
def build_shard(P, gen, torch, rank, rows, dim, n_total, dev, options=()):
    idx = P.RecallIndex(dim=dim, device=dev.index or 0, capacity_rows=rows, row_base=rank * rows)
    step = 32768
    for r0 in range(0, rows, step):
        m = min(step, rows - r0)
        g0 = rank * rows + r0
        pool, off = gen.contents(g0, m, dev)
        emb = gen.embeddings(g0, m, dim, dev)
        created = gen.created_ticks(g0, m, n_total, dev)
        torch.cuda.current_stream().synchronize()         # the library reads the tensors on its own stream
        idx.append(emb, created, pool, off)
    idx.seal()
    for opt in options:
        name, _, value = opt.partition("=")
        idx.set_option(name, int(value or 1))
    return idx


class Leg:
    """One timed workload: W warm-up steps, then exactly K steps between barrier + synchronize."""

    def __init__(self, name, workload, rows_per_gpu, n_total, batch, terms=True):
        self.name, self.workload = name, workload
        self.rows_per_gpu, self.n_total, self.batch, self.terms = rows_per_gpu, n_total, batch, terms


def leg_steps(args):
    """Steps run_leg issues through the handle: warm-up, timed, and in a --full run up to five untimed ones for the kernel table."""
    return args.warmup + args.steps + (min(5, args.steps) if args.full else 0)


def run_leg(leg, args, env, idx, front, gen, overlap=False, outputs=None):
    """Returns the leg's result dict on every rank (timings are the max over ranks).  `outputs` (a dict): receives what the
    last timed step returned."""
    P, torch, dist, dev, world, rank = env["P"], env["torch"], env["dist"], env["dev"], env["world"], env["rank"]
    k, dim, B = args.topk, args.dim, leg.batch
    n_steps_total = args.warmup + args.steps
    origin = rank == 0
    # queries for every step, generated up front and resident in HBM; the tokenisation of the query texts (the host
    # half of KeywordScore, RecallSearchService.cs:95-108) is timed separately and reported, not inside the steps
    q_steps, term_steps = [], []
    tok_s = 0.0
    if origin or front is None:
        for s in range(n_steps_total):
            b0 = s * B
            q_steps.append(gen.query_vectors(b0, B, dim, leg.n_total, dev))
            texts = gen.query_texts(b0, B, leg.n_total)
            t0 = time.perf_counter()
            terms = [[] if not leg.terms else P.text.query_terms(t) for t in texts]
            packed = P.PackedTerms(P.pack_terms(terms))
            tok_s += time.perf_counter() - t0
            term_steps.append(packed)
    torch.cuda.synchronize()

    def step(s, lane=None):
        if front is not None:
            return front.search_from(0, q_steps[s] if origin else None, term_steps[s] if origin else None,
                                     gen.NOW_TICKS, k, leg.n_total)
        return (lane or idx).search(q_steps[s], term_steps[s], gen.NOW_TICKS, k, candidate_limit=leg.n_total)

    for s in range(args.warmup):
        step(s)
    # timed region: HIP events around the one launch per step that streams every row (the kernel the roofline is quoted on);
    # an event pair around each of the ~10 small kernels as well costs a one-query step several percent, so the rest of
    # the kernel table comes from a few untimed steps afterwards
    idx.set_profiling(2)
    idx.reset_search_stats()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for s in range(args.warmup, n_steps_total):
        last = step(s)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if outputs is not None:
        outputs.update(zip(OUTPUT_NAMES, last))
    stats = idx.kernel_stats()
    sstats = idx.search_stats()
    if args.full:
        idx.set_profiling(1)
        for s in range(args.warmup, args.warmup + min(5, args.steps)):
            step(s)
        torch.cuda.synchronize()
        stats_all = idx.kernel_stats()
        for name, v in stats_all.items():
            stats.setdefault(name, v)
    idx.set_profiling(0)

    two = None
    if overlap and front is None:
        import threading
        lane2 = None
        try:
            both = [idx, idx]                    # ONE handle from two threads: the library gives each search a lane of its own
            errors = []

            def run2(lane):
                try:
                    for s in range(args.warmup + lane, n_steps_total, 2):
                        both[lane].search(q_steps[s], term_steps[s], gen.NOW_TICKS, k, candidate_limit=leg.n_total)
                except Exception as exc:         # e.g. no room for a second set of workspaces
                    errors.append(repr(exc))

            for _ in range(2):                   # the first round warms the view's workspaces
                threads = [threading.Thread(target=run2, args=(ln,)) for ln in range(2)]
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for t in threads:
                    t.start()
                for t in threads:
                    t.join()
                torch.cuda.synchronize()
                dt2 = time.perf_counter() - t1
            two = ({"steps_in_flight": 2, "value": args.steps * B / dt2, "unit": "queries/s", "ms_per_step": 1e3 * dt2 / args.steps}
                   if not errors else {"steps_in_flight": 2, "error": errors[0]})
        except Exception as exc:
            two = {"steps_in_flight": 2, "error": repr(exc)}
        finally:
            if lane2 is not None:
                lane2.close()

    # sanity inside the bench: the planted row of every query of the last step must be rank 1
    planted = gen.planted_rows((n_steps_total - 1) * B, B, leg.n_total)
    ok = [int(r) for r in last[0][:, 0]] == planted
    if not getattr(gen, "PLANTED_WINS", True):        # clustered corpus: a newer row of the cluster may legitimately outrank it
        ok = True
    if world > 1:
        cdev = dev if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        okt = torch.tensor([1 if ok else 0], dtype=torch.int32, device=cdev)
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        ok = bool(okt.item())
    queries = args.steps * B
    res = {
        "workload": leg.workload, "value": queries / elapsed, "unit": "queries/s", "ms_per_step": 1e3 * elapsed / args.steps,
        "queries_per_step": B, "corpus_rows": leg.n_total, "row_scores_per_sec": queries * leg.n_total / elapsed,
        "rank1_is_planted_row": ok if getattr(gen, "PLANTED_WINS", True) else None,
        "query_tokenisation_ms_per_step": 1e3 * tok_s / max(1, n_steps_total),
        "query_tokenisation": "host half of KeywordScore (split / lower / distinct / stop words, then packed into the ABI arrays) "
                              "done before the timed region; its cost per step is this field",
        "roofline": roofline_of(stats, leg.rows_per_gpu, dim, B, args.steps),
        "search_stats": sstats,
        "kernels": {n: {"launches": v["launches"], "avg_ms": v["total_ms"] / max(1, v["launches"])} for n, v in stats.items()},
        "kernels_source": "the kernel that streams every row: HIP events over the timed steps"
                          + ("; the others: HIP events over 5 untimed steps after them" if args.full else ""),
    }
    if two is not None:
        res["two_steps_in_flight"] = two
    return res


def _committed_traffic(kernel, rows, dim, B):
    """HBM bytes per launch from this round's committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate
    runs, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950), only where the shape matches."""
    path = os.path.join(ROOT, "profiles", "r03_pmc_hbm_traffic.json")
    if not os.path.exists(path):
        return None, None, 1
    try:
        with open(path) as f:
            doc = json.load(f)
        for e in doc.get("entries", []):
            if e.get("kernel") == kernel and e.get("rows") == rows and e.get("dim") == dim and e.get("batch") == B:
                return (e.get("hbm_bytes_per_launch_corrected"), "profiles/r03_pmc_hbm_traffic.json (" + e.get("command", "") + ")",
                        int(e.get("launches_per_step", 1)))
    except Exception:
        pass
    return None, None, 1


MEASURED_TRAFFIC = {}        # kernel name -> measure_traffic()'s entry, set by run() for the headline leg only


def _traffic(kernel, rows, dim, B):
    """HBM bytes per launch: measured in this run where that was done (the headline), else this round's committed PMC passes."""
    m = MEASURED_TRAFFIC.get(kernel)
    if m:
        return m["hbm_bytes_per_launch"], MEASURED_TRAFFIC.get("how"), None
    return _committed_traffic(kernel, rows, dim, B)


def roofline_of(stats, rows, dim, B, steps):
    """The dominant kernel of the leg against its roofline.  `achieved` is priced on the bytes / operations the kernel
    really performs (it streams the int8 shadow: N*D bytes); `frac_survey_8d` prices the same launch on SURVEY.md
    §8(d)'s fp32 figure 4*N*D, which this kernel does not read -- a value > 1 there says exactly that."""
    def avg(name):
        v = stats.get(name)
        return (v["total_ms"] / v["launches"], v["algo_bytes"] / v["launches"]) if v and v["launches"] else None
    survey_bytes = 4.0 * rows * dim + 4.0 * B * dim + 16.0 * rows + 16.0 * B * 10
    for name in ("screen_gemv_i8", "screen_gemv_bf16", "dot_exact"):
        a = avg(name)
        if a:
            ms, bytes_per_launch = a
            achieved = bytes_per_launch / (ms * 1e-3) / 1e9
            traffic, src, _ = _traffic(name, rows, dim, B)
            return {"bound": "hbm", "kernel": name, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": src, "avg_launch_ms": ms,
                    "algo_bytes_per_launch": bytes_per_launch,
                    "basis": "bytes this kernel streams per launch (int8 shadow N*D + 28*N of per-row constants + queries; fp32 4*N*D for dot_exact)",
                    "frac_survey_8d": survey_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "survey_8d_bytes_per_launch": survey_bytes}
    for name in ("screen_i8_fused", "screen_bf16_fused"):
        a = avg(name)
        if a:
            ms, bytes_per_launch = a
            i8 = name == "screen_i8_fused"
            # large shards take the screening GEMM in several row ranges, one launch each (orr_api.hip): everything below is per
            # LAUNCH, as the contract asks -- rows, operations and the committed PMC traffic of a step divided by its launches
            per_step = max(1, int(round(stats[name]["launches"] / max(1, steps))))
            ops = 2.0 * B * rows * dim / per_step
            mfma_peak = MFMA_I8_PEAK_TOPS if i8 else MFMA_BF16_PEAK_TFLOPS
            crossover = I8_CROSSOVER_B if i8 else I8_CROSSOVER_B / 2.0 * (MFMA_BF16_PEAK_TFLOPS / MFMA_I8_PEAK_TOPS) * 2.0
            gbs = bytes_per_launch / (ms * 1e-3) / 1e9
            tops = ops / (ms * 1e-3) / 1e12
            traffic, src, committed_per_step = _traffic(name, rows, dim, B)
            if traffic is not None and committed_per_step:
                traffic *= committed_per_step / per_step          # (the committed figure is per launch of ITS run)
            hbm_bound = B < crossover
            r = {"bound": "hbm" if hbm_bound else "mfma", "kernel": name,
                 "achieved": gbs if hbm_bound else tops, "peak": HBM_PEAK_GBS if hbm_bound else mfma_peak,
                 "unit": "GB/s" if hbm_bound else ("TOP/s" if i8 else "TFLOP/s"),
                 "frac": (gbs / HBM_PEAK_GBS) if hbm_bound else (tops / mfma_peak),
                 "traffic": traffic, "traffic_source": src, "avg_launch_ms": ms,
                 "algo_bytes_per_launch": bytes_per_launch, "algo_ops_per_launch": ops, "launches_per_step": per_step,
                 "avg_ms_per_step_in_this_kernel": ms * per_step,
                 "basis": ("rows of the %s shadow streamed once per launch (N*D%s bytes) + the query image; bound chosen from the batch "
                           "against the dtype's crossover (%.0f queries)" % ("int8" if i8 else "bf16", "" if i8 else "*2", crossover)),
                 "hbm": {"achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS},
                 "mfma": dict({"achieved": tops, "peak": mfma_peak, "unit": "TOP/s" if i8 else "TFLOP/s", "frac": tops / mfma_peak},
                              **({"sustained_peak": MFMA_I8_SUSTAINED_TOPS, "frac_of_sustained": tops / MFMA_I8_SUSTAINED_TOPS,
                                  "sustained_peak_source": "tools/mfma_rate.hip on this chip: MFMA-only, one wave per SIMD, all CUs "
                                                           "(profiles/r02_mfma_rate_microbench.txt): 32.1 cycles per MFMA at the 1.60 GHz "
                                                           "the chip holds under that load"} if i8 else {})),
                 "frac_survey_8d": survey_bytes / per_step / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                 "survey_8d_bytes_per_launch": survey_bytes / per_step}
            return r
    return None


def oracle_leg(args, env, idx, gen, n_total, B_headline, probe):
    """cpu_baseline + parity: the C oracle (kind "port", reference arithmetic) over a candidate_limit prefix of the
    HEADLINE corpus, timed on the host cores, and the HIP path's answers for the same queries over the same prefix
    compared with it: rank identity and max |score delta|."""
    import numpy as np
    from oracle import oracle_py as orc           # checker / baseline only
    P, torch, dev = env["P"], env["torch"], env["dev"]
    m = min(args.cpu_sample_rows, n_total)
    nq = min(args.cpu_sample_queries, B_headline)
    threads = max(1, min(probe.get("cpus_in_affinity_mask") or probe["os_cpu_count"] or 1, 256))   # every CPU in the affinity mask
    emb = torch.cat([gen.embeddings(r0, min(32768, m - r0), args.dim, dev).cpu() for r0 in range(0, m, 32768)]).numpy()
    created = gen.created_ticks(0, m, n_total, dev).cpu().numpy()
    pool, off = gen.contents(0, m, dev)
    corpus = orc.OracleCorpus(emb, created, (pool.cpu().numpy(), off.cpu().numpy()))
    # the HIP path: ONE batch of B_headline queries (the headline's batch size) over the prefix; the first nq are checked
    q = gen.query_vectors(0, B_headline, args.dim, n_total, dev)
    texts = gen.query_texts(0, B_headline, n_total)
    terms = [P.text.query_terms(t) for t in texts]
    torch.cuda.synchronize()
    g_rows, g_scores, g_counts = idx.search(q, terms, gen.NOW_TICKS, args.topk, candidate_limit=m)
    qs = q[:nq].cpu().numpy()
    rank_identical, max_delta, checked = True, 0.0, 0
    t0 = time.perf_counter()
    oracle_out = [corpus.search(qs[b], texts[b], gen.NOW_TICKS, args.topk, candidate_limit=m, threads=threads) for b in range(nq)]
    dt = time.perf_counter() - t0
    for b, (orow, osc, ornd) in enumerate(oracle_out):
        kk = int(g_counts[b])
        if kk != len(orow) or list(g_rows[b, :kk]) != list(orow):
            rank_identical = False
            continue
        checked += kk
        d = np.abs(g_scores[b, :kk] - osc)
        max_delta = max(max_delta, float(d.max()) if kk else 0.0)
    t1 = time.perf_counter()
    corpus.search(qs[0], texts[0], gen.NOW_TICKS, args.topk, candidate_limit=m, threads=1)
    dt1 = time.perf_counter() - t1
    rows_per_s = m * nq / dt
    # an optimised CPU variant beside the reference-faithful one, labelled as such -- cosine part only,
    # fp32 BLAS GEMM over the same sample with precomputed norms (NOT the reference arithmetic), top-k by partition
    norms = np.concatenate([np.sqrt(np.square(emb[i:i + 8192], dtype=np.float64).sum(axis=1)) for i in range(0, m, 8192)]).astype(np.float32)
    qn = np.sqrt(np.square(qs, dtype=np.float64).sum(axis=1)).astype(np.float32)
    t2 = time.perf_counter()
    cos = (emb @ qs.T) / (norms[:, None] * qn[None, :] + np.float32(1e-30))
    top = np.argpartition(-cos, args.topk, axis=0)[: args.topk]
    dt2 = time.perf_counter() - t2
    del cos, top
    cpu = {
        "value": rows_per_s / n_total, "unit": "queries/s", "cores": threads, "kind": "port",
        "sample": f"{nq} queries x newest {m} of {n_total} rows, C oracle, {threads} threads, {dt:.2f}s; value linear in rows",
        "sample_note": f"{nq} queries x the newest {m} of {n_total} rows x {args.dim}-d scored by the C oracle (reference arithmetic, "
                       f"full hybrid, candidate_limit = {m}) on {threads} threads in {dt:.2f}s; value = row-rate / rows per query of the "
                       f"headline corpus (linear extrapolation in rows)",
        "os_cpu_count": probe["os_cpu_count"], "cpus_in_affinity_mask": probe.get("cpus_in_affinity_mask"), "cpu_quota": probe.get("cpu_quota"),
        "threads_used": threads, "parallel_speedup_over_one_thread": (m * nq / dt) / (m / dt1),
        "single_thread_value": (m / dt1) / n_total,
        "dotnet": probe["dotnet"],
        "csharp_reference": ("C# runtime unavailable on this box (`dotnet --version` failed): the baseline is the C restatement "
                             "of RecallSearchService.cs, not the .NET build") if probe["dotnet"] == "unavailable"
        else "dotnet present; the reference itself is not shipped to this box (it cannot travel), baseline stays the C restatement",
        "optimised_variant": {"value": (m * nq / dt2) / n_total, "unit": "queries/s",
                              "what": "cosine part only: fp32 BLAS GEMM with precomputed norms + argpartition (numpy), "
                                      "not the reference arithmetic, no keyword or recency term"},
    }
    parity = {"rank_identical": rank_identical, "max_abs_score_delta": max_delta, "rows_checked": checked,
              "queries_checked": nq, "candidate_limit": m,
              "what": f"orr_search_batch with {B_headline} queries over the newest {m} rows of the headline corpus "
                      f"(same kernels as the timed steps) against the oracle's ranked row ids and unrounded fp64 scores for the first {nq}"}
    return cpu, parity



def cluster_child(args, n_dev):
    """`bench.py --mode cluster --cluster-exchange rccl` over the same devices as a child process; its compact line comes back as the leg."""
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(n_dev), "--mode", "cluster", "--cluster-exchange", "rccl",
           "--rows-per-gpu", str(args.cluster_leg_rows), "--batch", "256", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--dim", str(args.dim), "--topk", str(args.topk), "--no-legs", "--no-cpu-baseline"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=150)
    lines = [ln for ln in p.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
    if not lines:
        raise RuntimeError("child rc %d: %s" % (p.returncode, p.stderr.decode(errors="replace")[-200:]))
    doc = json.loads(lines[-1])
    if doc.get("error") or p.returncode != 0:
        raise RuntimeError("child rc %d: %s" % (p.returncode, doc.get("error")))
    return {"workload": doc["config"]["workload"], "value": doc["value"], "unit": "queries/s", "ms_per_step": doc["ms_per_step"],
            "rank1_is_planted_row": doc.get("rank1_is_planted_row"), "rccl_exchanges": doc.get("rccl_exchanges"), "child_total_s": doc.get("total_s")}


def run_cluster_leg(args, env, gen, devices, rows_per_dev, B, terms=True, workload=None, exchange="host", outputs=None):
    """ONE process, every device: orr_cluster (one shard per device, a host thread per shard, records through pinned host
    memory, host merge) -- the multi-GPU form of the C ABI that a C# host binds.  Queries are host-resident by contract."""
    P, torch = env["P"], env["torch"]
    G, dim, k = len(devices), args.dim, args.topk
    n_total = rows_per_dev * G
    t0 = time.perf_counter()
    cl = P.RecallCluster(devices, dim, capacity_rows_per_shard=rows_per_dev)
    step = 32768
    for g, d in enumerate(devices):
        dev = torch.device("cuda", d)
        sh = cl.shard(g)
        with torch.cuda.device(dev):
            for r0 in range(0, rows_per_dev, step):
                m = min(step, rows_per_dev - r0)
                g0 = g * rows_per_dev + r0
                pool, off = gen.contents(g0, m, dev)
                emb = gen.embeddings(g0, m, dim, dev)
                created = gen.created_ticks(g0, m, n_total, dev)
                ids = torch.arange(g0, g0 + m, dtype=torch.int64, device=dev)
                torch.cuda.current_stream().synchronize()
                sh.append(emb, created, pool, off, row_ids=ids)
    cl.seal()
    if exchange == "rccl":
        cl.set_option("exchange", 1)
    setup = time.perf_counter() - t0
    n_steps_total = args.warmup + args.steps
    q_steps, term_steps = [], []
    for s_ in range(n_steps_total):
        b0 = s_ * B
        q_steps.append(gen.query_vectors(b0, B, dim, n_total, "cpu").numpy())
        texts = gen.query_texts(b0, B, n_total)
        term_steps.append(P.PackedTerms(P.pack_terms([P.text.query_terms(t) if terms else [] for t in texts])))
    for s_ in range(args.warmup):
        cl.search(q_steps[s_], term_steps[s_], gen.NOW_TICKS, k, candidate_limit=n_total)
    cl.search_stats(reset=True)
    t1 = time.perf_counter()
    last = None
    for s_ in range(args.warmup, n_steps_total):
        last = cl.search(q_steps[s_], term_steps[s_], gen.NOW_TICKS, k, candidate_limit=n_total)
    dt = time.perf_counter() - t1
    if outputs is not None:
        outputs.update(zip(OUTPUT_NAMES, last))
    planted = gen.planted_rows((n_steps_total - 1) * B, B, n_total)
    res = {"workload": workload or ("orr_cluster (one process, %d devices): %d chunks x %d-d, %d per device, batch=%d, top-k=%d, %s" %
                                    (G, n_total, dim, rows_per_dev, B, k, "full hybrid" if terms else "cosine + recency")),
           "value": args.steps * B / dt, "unit": "queries/s", "ms_per_step": 1e3 * dt / args.steps, "queries_per_step": B,
           "corpus_rows": n_total, "devices": G, "rank1_is_planted_row": [int(r) for r in last[0][:, 0]] == planted,
           "search_stats": cl.search_stats(), "setup_s": round(setup, 2),
           "exchange": ("ONE ncclAllGather (RCCL over xGMI) of the per-shard [B][k'+1] candidate records per pass, merge from device 0's copy"
                        if exchange == "rccl" else
                        "per-shard [B][k'+1] candidate records through pinned host memory, host merge (no collective: one address space)")}
    res["rccl_exchanges"] = res["search_stats"].get("rccl_exchanges", 0)
    cl.close()
    return res


# what a search returns: rows [B, k] int64 (-1 past the count), scores [B, k] fp64, counts [B] int32
OUTPUT_NAMES = ("rows", "scores", "counts")


def dump_outputs(path, outputs):
    """--dump-outputs: one float64 .npy per returned array (row ids stay exact below 2^53; a few KB for any batch)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name in OUTPUT_NAMES:
        np.save(os.path.join(path, name + ".npy"), np.asarray(outputs[name], dtype=np.float64))


# ------------------------------------------------------------------------------------------------
# the driver's record: ONE short last line on stdout; the whole document goes to a file
# ------------------------------------------------------------------------------------------------
COMPACT_LIMIT = 1800       # bytes; the driver keeps ~2,000 characters of stdout (round 2's 21 KB line could not be parsed)


def _r(x, digits=4):
    """Numbers to `digits` significant digits: a 17-digit double is 20 bytes of a 1.8 KB line."""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        if x != x or x in (float("inf"), float("-inf")):
            return None
        return float(f"{x:.{digits}g}")
    return x


def _pick(d, keys, digits=4):
    return {k: _r(d[k], digits) for k in keys if d is not None and k in d}


def compact_line(out, full_path=None):
    """The contract's JSON line (task statement + tier section (4)), from the full document: every key the driver and
    the judge read, numbers rounded, no prose beyond `config.workload` and `cpu_baseline.sample`.  Anything that would
    push it past COMPACT_LIMIT is dropped in a fixed order (legs first), never the contract keys."""
    c = {k: _r(out.get(k), 6) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                        "scaling", "vs_baseline", "dtype", "data")}
    cfg = out.get("config") or {}
    c["config"] = _pick(cfg, ("workload", "name", "corpus_rows", "queries_per_step") + (("rows_per_gpu", "parallelism") if (out.get("n_gpus") or 1) > 1 else ()))
    rf = out.get("roofline")
    if rf:
        c["roofline"] = _pick(rf, ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "launches_per_step",
                                   "algo_bytes_per_launch", "frac_survey_8d"), 5)
        if "mfma" in rf:
            c["roofline"]["mfma_frac"] = _r(rf["mfma"].get("frac"))
        if "traffic_measured_in_this_run" in rf:
            c["roofline"]["traffic_in_run"] = rf["traffic_measured_in_this_run"]
        if "step_hbm_frac" in rf:
            c["roofline"]["step_hbm_frac"] = _r(rf["step_hbm_frac"])
    else:
        c["roofline"] = None
    cpu = out.get("cpu_baseline")
    if cpu:
        c["cpu_baseline"] = _pick(cpu, ("value", "unit", "cores", "kind", "sample", "threads_used", "os_cpu_count", "cpu_quota", "dotnet"))
    elif "cpu_baseline" in out:
        c["cpu_baseline"] = None
    if out.get("parity"):
        c["parity"] = _pick(out["parity"], ("rank_identical", "max_abs_score_delta", "rows_checked", "queries_checked", "candidate_limit"))
    for k in ("rank1_is_planted_row", "rccl_ranks_seen", "collectives_per_step", "backend", "exchange_mode", "rccl_exchanges", "error"):
        if k in out:
            c[k] = _r(out[k])
    if isinstance(out.get("two_steps_in_flight"), dict) and "value" in out["two_steps_in_flight"]:
        c["two_in_flight_qps"] = _r(out["two_steps_in_flight"]["value"])
    if out.get("leg_errors"):
        c["leg_errors"] = {kk: str(v)[:80] for kk, v in out["leg_errors"].items()}
    ss = out.get("search_stats") or {}
    if ss:
        c["search_stats"] = _pick(ss, ("passes", "requeried", "overflowed_queries", "exact_pass_queries", "survivors_per_query", "pass_mode"))
    legs = {}
    for name, leg in (out.get("legs") or {}).items():
        if not isinstance(leg, dict) or "value" not in leg:
            continue
        lr = leg.get("roofline") or {}
        short = name.replace("_rows", "").replace("_queries", "q").replace("_query", "q").replace("cosine_only", "cos")
        legs[short] = [_r(leg["value"], 3), _r(leg.get("ms_per_step"), 3), _r(lr.get("avg_launch_ms"), 3), _r(lr.get("frac"), 3)]
    if legs:
        c["legs_qps_ms_kernelms_frac"] = legs
    c["total_s"] = out.get("total_s")
    if full_path:
        c["full"] = full_path
    # shrink in a fixed order if needed; the contract keys stay
    for drop in ("legs_qps_ms_kernelms_frac", "search_stats", "two_in_flight_qps", "leg_errors", "full"):
        if len(json.dumps(c, separators=(",", ":"))) <= COMPACT_LIMIT:
            break
        c.pop(drop, None)
    line = json.dumps(c, separators=(",", ":"))
    if len(line) > COMPACT_LIMIT:                      # a runaway string (an error text, a path): cut the prose, keep the numbers
        for holder, key in ((c.get("cpu_baseline") or {}, "sample"), (c, "error"), (c.get("config") or {}, "parallelism")):
            if isinstance(holder.get(key), str):
                holder[key] = holder[key][:120]
        line = json.dumps(c, separators=(",", ":"))
    return line


def emit(out):
    """Full document -> bench_full.json (and gpurun_out/ when that exists); compact line -> the LAST line of stdout."""
    full_path = None
    for d in (os.path.join(ROOT, "gpurun_out"), ROOT):
        try:
            if os.path.isdir(d):
                with open(os.path.join(d, "bench_full.json"), "w") as f:
                    json.dump(out, f, indent=1)
                full_path = full_path or os.path.relpath(os.path.join(d, "bench_full.json"), ROOT)
        except OSError:
            pass
    sys.stdout.flush()
    print(compact_line(out, full_path), flush=True)

# ------------------------------------------------------------------------------------------------
def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    launched = "WORLD_SIZE" in os.environ
    if (args.gpus > 1 or args.dist_rehearsal) and args.mode == "ranks" and not launched:
        spawn_ranks(args, argv)                    # never returns
    cluster_mode = args.mode == "cluster"          # (one device too: a one-shard cluster, e.g. to rehearse the RCCL exchange on a one-GPU box)
    world = 1 if cluster_mode else int(os.environ.get("WORLD_SIZE", "1"))
    rank = 0 if cluster_mode else int(os.environ.get("RANK", "0"))
    if not cluster_mode and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    probe = host_probe() if rank == 0 and args.full else {}     # child processes only; before the first GPU call of this process
    if rank == 0 and world == 1 and not cluster_mode and not args.no_pmc and not args.dist_rehearsal:
        try:
            probe["pmc"] = measure_traffic(args)       # (children too: the profiler must not meet a process that already holds the GPU)
        except Exception as exc:
            probe["pmc"] = {"error": repr(exc)[:200]}
    state = {"t_start": time.perf_counter(), "out": None, "dist": None}
    try:
        run(args, probe, state, cluster_mode, world, rank)
    except BaseException as exc:                   # a collective that raised, a rank that died, no memory: say so in the ONE line
        if isinstance(exc, SystemExit) and exc.code in (0, None):
            raise
        import traceback
        traceback.print_exc()
        if rank == 0:
            out = state["out"] or {
                "metric": METRIC, "value": None, "unit": "queries/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": None, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": DTYPE, "data": "synthetic",
                "config": {"workload": "not reached"}, "roofline": None, "cpu_baseline": None}
            out["error"] = ("%s: %s" % (type(exc).__name__, exc))[:400]
            out["total_s"] = round(time.perf_counter() - state["t_start"], 2)
            emit(out)
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)                                # (no destructor of a half-dead process group gets to hang the job)


METRIC = "queries/sec at top-k=10 over N x 3072-d chunks; score delta vs C# reference in `parity`"
DTYPE = "i8 screen + f32*f32->f64 exact re-score"


def run(args, probe, state, cluster_mode, world, rank):
    t_start = state["t_start"]
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if not cluster_mode else 0
    import datetime
    import torch
    import torch.distributed as dist
    import __graft_entry__ as graft
    P = graft.load_package()
    syn = importlib.import_module(graft.PKG_NAME + ".synthetic")
    sharded = importlib.import_module(graft.PKG_NAME + ".sharded")
    n_visible = torch.cuda.device_count()
    if cluster_mode and n_visible < args.gpus and not args.cluster_oversubscribe:
        raise SystemExit(f"--mode cluster --gpus {args.gpus} needs {args.gpus} visible GPUs, found {n_visible}")
    if world > 1 and args.backend == "nccl" and n_visible < world:
        raise SystemExit(f"--gpus {world} with the nccl (RCCL) backend needs {world} visible GPUs, found {n_visible}")
    dev_index = local_rank if args.backend == "nccl" else local_rank % max(1, n_visible)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1 or args.dist_rehearsal:
        # (a collective that cannot complete -- a rank died -- raises after five minutes instead of the default ten, and the
        # survivors report it in the JSON line)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=300))
        else:
            dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=300))
        state["dist"] = dist
    env = {"P": P, "torch": torch, "dist": dist, "dev": dev, "world": world, "rank": rank}

    dim, k = args.dim, args.topk
    legs_out = {}
    setup_s = {}
    leg_errors = {}

    def optional_leg(name, fn):
        """A leg beside the headline must not take the headline down with it: its failure is recorded and the run goes on.
        (Collective legs: a failure on ONE rank desynchronises the job -- those are not optional and propagate.)"""
        try:
            r = fn()
            if r is not None:
                legs_out[name] = r
        except Exception as exc:
            leg_errors[name] = ("%s: %s" % (type(exc).__name__, exc))[:300]

    head_out = {}                                  # what the headline's last timed step returned

    def dump_head():
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, head_out)

    if cluster_mode:
        # ---- ONE process, all devices, through orr_cluster: the C5 per-GPU shape on every device
        rows = args.rows_per_gpu or 12_500_000
        B = args.batch or 1024
        n_total = rows * args.gpus
        head = run_cluster_leg(args, env, syn, [g % max(1, n_visible) for g in range(args.gpus)], rows, B, terms=not args.no_terms,
                               workload=workload_label(rows, dim, B, k, not args.no_terms, args.gpus).replace("row-sharded over", "orr_cluster, one process, over"),
                               exchange=args.cluster_exchange, outputs=head_out)
        dump_head()
        head["exchange_mode"] = args.cluster_exchange
        head["row_scores_per_sec"] = head["value"] * n_total
        if n_visible < args.gpus:
            head["workload"] += " [REHEARSAL: %d shards on %d card(s)]" % (args.gpus, n_visible)
        head["roofline"] = None
        head["kernels"] = {}
        head["query_tokenisation_ms_per_step"] = None
        front, idx = None, None
    elif world == 1 and not args.dist_rehearsal:
        rows = args.rows_per_gpu or 10_000_000
        B = args.batch or 256
        # ---- leg: C2 (configs[1]) on its own 1M-row shard
        if not args.no_legs:
            t0 = time.perf_counter()
            idx2 = build_shard(P, syn, torch, 0, 1_000_000, dim, 1_000_000, dev, args.set_option)
            setup_s["c2_corpus"] = time.perf_counter() - t0
            leg = Leg("c2", workload_label(1_000_000, dim, 1, k, True, 1), 1_000_000, 1_000_000, 1)
            legs_out["C2_1M_rows_1_query"] = run_leg(leg, args, env, idx2, None, syn, overlap=not args.no_overlap_leg)
            idx2.close()
            del idx2
        if not args.no_legs and not args.no_robustness_legs:
            for tag, modname, what in (("clustered", "synthetic_clustered", "clustered corpus (64 centroids + 0.1 noise)"),
                                       ("keyword_heavy", "synthetic_zipf", "keyword-heavy corpus (2^18 Zipf tokens of 3..24 bytes, substring terms)")):
                gen = importlib.import_module(graft.PKG_NAME + "." + modname)
                t0 = time.perf_counter()
                idxc = build_shard(P, gen, torch, 0, 1_000_000, dim, 1_000_000, dev, args.set_option)
                setup_s[tag + "_corpus"] = time.perf_counter() - t0
                for bq in (1, 256):
                    leg = Leg(tag, what + ": " + workload_label(1_000_000, dim, bq, k, True, 1), 1_000_000, 1_000_000, bq)
                    legs_out[f"{tag}_1M_rows_{bq}_queries"] = run_leg(leg, args, env, idxc, None, gen)
                if tag == "clustered":       # without keyword steps in the scores the screen keeps thousands of pairs per query
                    leg = Leg(tag, what + ": " + workload_label(1_000_000, dim, 256, k, False, 1), 1_000_000, 1_000_000, 256, terms=False)
                    legs_out["clustered_1M_rows_256_queries_cosine_only"] = run_leg(leg, args, env, idxc, None, gen)
                idxc.close()
                del idxc
        torch.cuda.empty_cache()
        # ---- headline: C3 (configs[2])
        t0 = time.perf_counter()
        idx = build_shard(P, syn, torch, 0, rows, dim, rows, dev, args.set_option)
        setup_s["headline_corpus"] = time.perf_counter() - t0
        head_leg = Leg("headline", workload_label(rows, dim, B, k, not args.no_terms, 1), rows, rows, B, terms=not args.no_terms)
        pmc = probe.get("pmc") or {}
        if "error" not in pmc:
            MEASURED_TRAFFIC.update(pmc)                # (the children ran the headline's shape: only this leg may quote them)
        head = run_leg(head_leg, args, env, idx, None, syn, overlap=not args.no_overlap_leg, outputs=head_out)
        dump_head()
        MEASURED_TRAFFIC.clear()
        if head.get("roofline") is not None:
            head["roofline"]["traffic_measured_in_this_run"] = bool(pmc) and "error" not in pmc and head["roofline"].get("traffic") is not None
            if pmc.get("error"):
                head["roofline"]["traffic_pmc_error"] = pmc["error"]
        n_total, front = rows, None
    else:
        rows = args.rows_per_gpu or 12_500_000
        B = args.batch or 1024
        n_total = rows * world
        coll_dev = dev if args.backend == "nccl" else "cpu"
        t0 = time.perf_counter()
        idx = build_shard(P, syn, torch, rank, rows, dim, n_total, dev, args.set_option)
        setup_s["headline_corpus"] = time.perf_counter() - t0
        front = sharded.ShardedRecallSearch(idx, dim, coll_dev)
        front.always_collect = bool(args.dist_rehearsal)
        ranks_seen = front.rccl_ranks_seen()
        head_leg = Leg("headline", workload_label(rows, dim, B, k, not args.no_terms, world), rows, n_total, B, terms=not args.no_terms)
        head = run_leg(head_leg, args, env, idx, front, syn, outputs=head_out)
        dump_head()
        head["rccl_ranks_seen"] = ranks_seen if args.backend == "nccl" else 0
        head["backend"] = args.backend + (" (RCCL over xGMI)" if args.backend == "nccl" else f" (rehearsal: {world} ranks, {n_visible} card(s))")
        head["collectives_per_step"] = front.collectives / max(1, leg_steps(args))
        head["escalated_queries"] = front.escalated_queries
        if rank == 0:                              # the headline is in hand from here on: a later failure still reports it
            state["out"] = assemble(args, probe, head, {}, setup_s, None, None, rows, n_total, B, world, t_start, leg_errors)
        def keep():                                # whatever is in hand goes into the line a later failure prints
            if rank == 0:
                state["out"] = assemble(args, probe, head, legs_out, setup_s, None, None, rows, n_total, B, world, t_start, leg_errors)
        if not args.no_legs:
            for bq in (1, 256):
                leg = Leg(f"c4_b{bq}", workload_label(rows, dim, bq, k, False, world), rows, n_total, bq, terms=False)
                legs_out[f"C4_cosine_only_{bq}_queries"] = run_leg(leg, args, env, idx, front, syn)
                keep()
        # ---- leg: the same devices from ONE process through orr_cluster (rank 0 drives every device; the other ranks wait).  Small
        # shards: every device already holds its rank's 12.5M rows.
        if not args.no_legs and args.cluster_leg_rows > 0 and args.backend == "nccl":
            if rank == 0:
                tag = "cluster_one_process_%dM_rows_per_device_256_queries" % max(1, args.cluster_leg_rows // 1_000_000)
                optional_leg(tag, lambda: run_cluster_leg(args, env, syn, list(range(world)), args.cluster_leg_rows, 256))
                torch.cuda.set_device(dev_index)
                # the same with the records exchanged by ONE RCCL all-gather (orr_cluster "exchange" = 1) -- in a CHILD process: that
                # path has never run on more than one device, and whatever it does must not take this job's record down with it
                optional_leg(tag + "_rccl_exchange", lambda: cluster_child(args, world))
                keep()
            dist.barrier()

        # ---- leg: FIXED corpus split over the ranks (strong scaling: the curve 1 -> N shows what sharding buys one batch),
        # C3's corpus and batch: 10M rows in all, 256 hybrid queries per step.  LAST: the headline shard is closed first (on up to four
        # GPUs the two do not fit side by side), and whatever happens here the headline is already in hand.
        if not args.no_legs and args.strong_rows >= world:
            idx.close()
            idx = None
            torch.cuda.empty_cache()
            rows_s = args.strong_rows // world
            t0 = time.perf_counter()
            idx_s = build_shard(P, syn, torch, rank, rows_s, dim, rows_s * world, dev, args.set_option)
            setup_s["strong_corpus"] = time.perf_counter() - t0
            front_s = sharded.ShardedRecallSearch(idx_s, dim, coll_dev)
            front_s.always_collect = bool(args.dist_rehearsal)
            leg = Leg("strong", "fixed corpus (strong scaling): " + workload_label(rows_s, dim, 256, k, True, world), rows_s, rows_s * world, 256)
            r = run_leg(leg, args, env, idx_s, front_s, syn)
            r["scaling"] = "strong"
            r["collectives_per_step"] = front_s.collectives / max(1, leg_steps(args))
            legs_out[f"strong_{args.strong_rows // 1_000_000}M_rows_total_256_queries"] = r
            idx_s.close()
            del idx_s, front_s
            torch.cuda.empty_cache()

    cpu = parity = None
    if rank == 0 and world == 1 and not cluster_mode and not args.no_cpu_baseline and not args.dist_rehearsal:
        t0 = time.perf_counter()
        cpu, parity = oracle_leg(args, env, idx, syn, n_total, B, probe)
        setup_s["oracle_leg"] = time.perf_counter() - t0

    if rank == 0:
        out = assemble(args, probe, head, legs_out, setup_s, cpu, parity, rows, n_total, B, args.gpus if cluster_mode else world, t_start, leg_errors,
                       cluster_mode=cluster_mode)
        state["out"] = out
        emit(out)
    if world > 1 or args.dist_rehearsal:
        dist.barrier()
        dist.destroy_process_group()
    if idx is not None:
        idx.close()


def assemble(args, probe, head, legs_out, setup_s, cpu, parity, rows, n_total, B, world, t_start, leg_errors, cluster_mode=False):
    dim = args.dim
    cfg_name = config_name(rows, dim, B, world, not args.no_terms)
    out = {
        "metric": METRIC,
        "value": head["value"], "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": DTYPE,
        "dtype_note": "int8 screen with a rigorous per-pair bound over all rows, then f32 x f32 -> f64 re-score of the survivors in the reference's arithmetic",
        "data": "synthetic",
        "config": {"workload": head["workload"], "name": cfg_name, "corpus_rows": n_total, "rows_per_gpu": rows,
                   "queries_per_step": B, "options": args.set_option, "steps_in_flight": 1,
                   "parallelism": ("one process, orr_cluster over %d devices: per-shard top-k' records through pinned host memory, host merge" % world) if cluster_mode
                   else (f"row-sharded x{world}: broadcast of the batch from rank 0, one all-gather of per-shard top-k' "
                         f"records (RCCL), host merge on every rank") if world > 1 else "single GPU"},
        "row_scores_per_sec": head.get("row_scores_per_sec"),
        "rank1_is_planted_row": head.get("rank1_is_planted_row"),
        "roofline": head.get("roofline"),
        "search_stats": head.get("search_stats"),
        "kernels": head.get("kernels"),
        "query_tokenisation_ms_per_step": head.get("query_tokenisation_ms_per_step"),
        "query_tokenisation": head.get("query_tokenisation"),
        "legs": legs_out,
        "peaks": {"hbm_gbs": HBM_PEAK_GBS, "mfma_i8_tops_dense": MFMA_I8_PEAK_TOPS, "mfma_bf16_tflops_dense": MFMA_BF16_PEAK_TFLOPS,
                  "source": "MI355X_MICROARCH.md chip-level parameters (spec, dense)", "read_on_this_box": probe.get("gpu")},
        "setup_s": {kk: round(v, 2) for kk, v in setup_s.items()},
        "total_s": round(time.perf_counter() - t_start, 2),
    }
    for extra in ("rccl_ranks_seen", "collectives_per_step", "backend", "two_steps_in_flight", "escalated_queries", "exchange_mode", "rccl_exchanges"):
        if extra in head:
            out[extra] = head[extra]
    if leg_errors:
        out["leg_errors"] = dict(leg_errors)
    if parity is not None:
        out["parity"] = parity
    if cpu is not None:
        out["cpu_baseline"] = cpu
    else:
        out["cpu_baseline"] = None
    return out


def config_name(rows, dim, B, world, terms):
    if dim == 3072 and world == 1 and rows == 1_000_000 and B == 1:
        return "C2"
    if dim == 3072 and world == 1 and rows == 10_000_000 and B == 256:
        return "C3"
    if dim == 3072 and world == 8 and rows == 12_500_000:
        return "C5" if terms and B == 1024 else ("C4" if not terms and B in (1, 256) else "C4/C5 shape, other batch")
    if dim == 3072 and rows == 12_500_000:
        return f"C4/C5 per-GPU shape on {world} GPU(s)"
    return "custom"


def workload_label(rows, dim, B, k, terms, world):
    name = config_name(rows, dim, B, world, terms)
    total = rows * world
    return (f"{name}: {total} chunks x {dim}-d fp32" + (f" row-sharded over {world} GPUs ({rows} per GPU)" if world > 1 else " on one GPU")
            + f", batch={B} queries per step, top-k={k}, "
            + ("full hybrid (cosine+keyword+recency)" if terms else "cosine + recency only (no query terms)")
            + ", candidate_limit=corpus")


if __name__ == "__main__":
    main()
