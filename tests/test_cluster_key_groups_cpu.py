"""CPU checks of the cluster key groups (orr_cluster_keys_groups, orr_cluster_keys_centroids, orr_cluster_scope_centroid): the
rules of csrc/orr_cluster_key_groups_plan.h through their selftest; the plan plus its host executor (records_of, run_records)
compiled for the host and held against this file's own numpy restatement of the blocked sum over the CONCATENATED members, on
data cut into 1 to 5 parts; the kernel and the driver made of the shared rules; the three symbols declared, exported, bound and
documented; every argument error on NULL handles in the documented order with the outputs untouched -- so on a machine without a
GPU (the method of tests/test_key_groups_cpu.py).  The calls at work are in tests/test_gpu_cluster_key_groups.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_cluster_key_groups_plan_selftest")
NAMES = ("orr_cluster_keys_groups", "orr_cluster_keys_centroids", "orr_cluster_scope_centroid")
N_ARGS = (7, 8, 5)
SHARED = ("keys_pairs_count", "keys_pairs", "keys_pairs_scan", "keys_pairs_sort", "keys_runs", "keys_block_sums", "keys_block_fold")
BLOCK = 256


def test_cluster_key_groups_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_cluster_key_groups_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_cluster_key_groups_plan_selftest: ok"
    m = re.search(r"cuts checked: (\d+)", r.stdout)
    assert m and int(m.group(1)) == 7 * 7 * 3, r.stdout          # before x count x (total equal to, one above, 300 above before + count)
    m = re.search(r"chained cases checked: (\d+) \(chain records run: (\d+), told apart from both wrong orders: (\d+)\)", r.stdout)
    assert m and int(m.group(1)) == 6 * 5 * 12 and int(m.group(2)) > 300 and int(m.group(3)) > 50, r.stdout


# ---- this file's own restatement -----------------------------------------------------------------------------------------------

def _sum_blocked(E):
    S = np.zeros(E.shape[1], np.float64)
    with np.errstate(all="ignore"):
        for b0 in range(0, E.shape[0], BLOCK):
            P = np.zeros(E.shape[1], np.float64)
            for row in E[b0:b0 + BLOCK].astype(np.float64):
                P = P + row
            S = S + P
    return S


def _restarted(parts):
    S = np.zeros(parts[0].shape[1], np.float64)
    with np.errstate(all="ignore"):
        for E in parts:
            for b0 in range(0, len(E), BLOCK):
                S = S + _sum_blocked(E[b0:b0 + BLOCK])
    return S


def _added(parts):
    S = np.zeros(parts[0].shape[1], np.float64)
    with np.errstate(all="ignore"):
        for E in parts:
            if len(E):
                S = S + _sum_blocked(E)
    return S


def _same64(a, b):
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


RUNNER = '#include "orr_cluster_key_groups_plan.h"\n#include <cstdio>\n#include <vector>\n' + """
// in: dim, rows, cases; emb; per case: mutation, n_shards, then per shard its member count and members.  One key per case, slot 0.
// mutation 0: the rule.  1: the head starts from +0.0, not the seed.  2: `before` ignored (blocks restart at the border).
// 3: the open block folded early.  4: S seeded with +0.0 on a later shard.
int main(int argc, char **argv)
{
    namespace ckg = cluster_key_groups;
    FILE *f = fopen(argv[1], "rb");
    int32_t dim = 0, rows = 0, cases = 0;
    if (!f || fread(&dim, 4, 1, f) != 1 || fread(&rows, 4, 1, f) != 1 || fread(&cases, 4, 1, f) != 1) return 2;
    std::vector<float> emb((size_t)rows * dim);
    if (fread(emb.data(), 4, emb.size(), f) != emb.size()) return 2;
    FILE *o = fopen(argv[2], "wb");
    for (int c = 0; c < cases; ++c) {
        int32_t mutation = 0, G = 0;
        if (fread(&mutation, 4, 1, f) != 1 || fread(&G, 4, 1, f) != 1) return 2;
        std::vector<std::vector<uint32_t>> pos((size_t)G);
        int64_t total = 0;
        for (int g = 0; g < G; ++g) {
            int64_t n = 0;
            if (fread(&n, 8, 1, f) != 1) return 2;
            std::vector<int64_t> m((size_t)n);
            if (n && fread(m.data(), 8, (size_t)n, f) != (size_t)n) return 2;
            for (int64_t v : m) pos[(size_t)g].push_back((uint32_t)v);
            total += n;
        }
        std::vector<double> state((size_t)2 * dim, 7.0), answer((size_t)dim, 0.0);
        bool spanning = false;
        for (int g = 0; g < G; ++g) spanning = spanning || ckg::spans((int64_t)pos[(size_t)g].size(), total);
        int64_t before = 0;
        for (int g = 0; g < G; ++g) {
            const int64_t count = (int64_t)pos[(size_t)g].size(), first = 0, b = mutation == 2 ? 0 : before;
            const int32_t slot = 0;
            ckg::Records r;
            ckg::records_of(1, &count, &first, &b, &total, &slot, nullptr, r);
            for (ckg::Chain &ch : r.chains) {
                if (mutation == 1) ch.flags &= ~ckg::kSeedP;
                if (mutation == 2 && before > 0) ch.flags |= ckg::kSeedS;                  // (the chain of S itself goes on)
                if (mutation == 3 && ckg::chain_open(ch.flags) == ckg::kOpenFree) ch.n_close += 1;
                if (mutation == 3 && ckg::chain_open(ch.flags) == ckg::kOpenHead) ch.flags |= ckg::kHeadCloses;
                if (mutation == 4) ch.flags &= ~ckg::kSeedS;
            }
            std::vector<double> sums((size_t)dim, 0.0), parts((size_t)(r.n_parts + 1) * dim, -3.0);
            ckg::run_records(r, emb.data(), dim, pos[(size_t)g].data(), sums.data(), parts.data(), state.data());
            if (count == total && count > 0) answer = sums;
            before += count;
        }
        if (spanning) answer.assign(state.begin(), state.begin() + dim);
        std::vector<float> cen((size_t)dim, 7.f);
        key_groups::finish(answer.data(), total, dim, cen.data());
        fwrite(answer.data(), 8, answer.size(), o);
        fwrite(cen.data(), 4, cen.size(), o);
    }
    fclose(o);
    return 0;
}
"""


def test_the_plan_and_run_records_compiled_for_the_host_equal_the_numpy_restatement_over_the_concatenated_members(tmp_path):
    """random rows over 30 decades with mixed signs, an infinity, a NaN and signed zeros; members picked through their positions,
    out of order of storage, cut into 1 to 5 parts (empty parts, cuts on block edges and right behind them included): the sums'
    uint64 bits and the centroids' uint32 bits.  Both wrong orders differ from the rule in at least one case, and each of the
    four mutations of the chain that the CPU can show gives other bits in at least one case."""
    src = tmp_path / "chain.cpp"
    src.write_text(RUNNER)
    exe = tmp_path / "chain"
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=120)
    rng = np.random.default_rng(6)
    dim, rows = 9, 1_200
    emb = (rng.standard_normal((rows, dim)) * 10.0 ** rng.uniform(-15, 15, (rows, dim))).astype(np.float32)
    emb[17, 2] = np.inf
    emb[23, 4] = np.nan
    emb[30:40, 5] = -0.0
    cases = []
    for n in (1, 40, 255, 256, 257, 300, 513, 600, 1_000):
        for g in (1, 2, 3, 4, 5):
            for style in range(3):
                members = rng.permutation(rows)[:n].astype(np.int64)
                if n >= 40:
                    members[:3] = (17, 23, 35)          # the special rows lead the first block
                cuts = np.sort(rng.integers(0, n + 1, g - 1))
                if style == 1:
                    cuts = cuts // BLOCK * BLOCK        # on block edges (0 included: an empty first part)
                if style == 2 and g > 2:
                    cuts[1:] = np.minimum(n, cuts[0] + np.arange(1, g - 1) * 3)      # parts of three members: heads that stay open
                cases.append((members, np.sort(cuts)))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([dim, rows, len(cases) * 5], np.int32).tobytes())
        f.write(emb.tobytes())
        for mutation in range(5):
            for members, cuts in cases:
                parts = np.split(members, cuts)
                f.write(np.array([mutation, len(parts)], np.int32).tobytes())
                for p in parts:
                    f.write(np.int64(len(p)).tobytes())
                    f.write(p.tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    raw = open(tmp_path / "out.bin", "rb").read()
    at, restarted, added, mutated = 0, 0, 0, [0] * 5
    for mutation in range(5):
        for members, cuts in cases:
            S = np.frombuffer(raw, np.float64, dim, at); at += 8 * dim
            c = np.frombuffer(raw, np.float32, dim, at); at += 4 * dim
            want = _sum_blocked(emb[members])
            if mutation:
                mutated[mutation] += int(not _same64(S, want))
                continue
            assert _same64(S, want), (len(members), cuts)
            with np.errstate(all="ignore"):
                wc = (want / np.float64(len(members))).astype(np.float32)
            assert bool(((c.view(np.uint32) == wc.view(np.uint32)) | (np.isnan(c) & np.isnan(wc))).all()), (len(members), cuts)
            parts = [emb[p] for p in np.split(members, cuts)]
            a, b = not _same64(_restarted(parts), want), not _same64(_added(parts), want)
            if all(int(x) % BLOCK == 0 or int(x) == len(members) for x in cuts):
                assert not a, (len(members), cuts)      # every cut on a block edge: the restarted blocks ARE the blocks
            restarted += int(a)
            added += int(b)
    assert at == len(raw)
    assert restarted >= 1 and added >= 1                # the data tell both wrong orders from the rule
    assert all(m >= 1 for m in mutated[1:]), mutated    # ... and each mutated chain


def test_the_kernel_and_the_driver_share_the_rules():
    header = open(os.path.join(CSRC, "orr_cluster_key_groups_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_cluster_key_groups_plan_selftest.cpp")).read()
    for name in ("first_invalid_groups", "first_invalid_centroids", "first_invalid_scope_centroid", "merge_groups", "cut", "records_of", "run_records", "spans"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert re.search(r"\b%s\(" % name, selftest), name
    assert "namespace cluster_key_groups" in header and "using key_groups::kBlock" in header
    # the kernel: the seed loads, the adds in the rule's order, no atomics, no FMA; the two older kernels textually as they were
    chain = kernels.split("void key_groups_chain_kernel(")[1].split("hipError_t launch_keys_chain_step(")[0]
    order = ["if (cluster_key_groups::chain_seed_p(c.flags)) load_row(p_row, p0, p1, p2, p3)", "p0 = p0 + (double)v[j].x",
             "if (cluster_key_groups::chain_seed_s(c.flags)) load_row(s_row, s0, s1, s2, s3)", "s0 = s0 + p0", "s0 = s0 + w[j][0]",
             "store_row(s_row, s0, s1, s2, s3)", "store_row(p_row, p0, p1, p2, p3)"]
    at = [chain.index(piece) for piece in order]
    assert at == sorted(at), at
    for piece in ("__shared__ uint32_t sh_pos[key_groups::kBlock]", "reinterpret_cast<const float4 *>(row)", "reinterpret_cast<const double2 *>(row)",
                  "double p0 = +0.0", "double s0 = +0.0", "cluster_key_groups::chain_head_closes(c.flags)", "cluster_key_groups::kOpenFree"):
        assert piece in chain, piece
    assert "atomic" not in chain and "fma" not in chain.lower()
    assert "dim3 grid((unsigned)n_chains, (unsigned)tiles)" in kernels
    # the driver
    for k in SHARED + ("keys_chain_step",):
        assert api.count('Timed t(lane, "%s"' % k) == 1, k          # the cluster driver calls the single index's helpers
    section = api.split("// ---- cluster key groups (")[1]
    for helper in ("key_groups_pairs(", "key_groups_runs(", "key_groups_slice_launch(", "ckg::records_of(",
                   "cluster_key_groups::merge_groups(", "key_groups::finish(", "key_groups::slice_keys(dim, lanes[0].lane->opt_key_groups_slice)", "work.pin"):
        assert helper in section, helper
    assert "sstats" not in section
    hold = section.split("int cluster_key_groups_hold(")[1].split("\n}\n")[0]
    assert hold.index("acquire_in_order(") < hold.index("sc->parts[g]->mu") < hold.index("k->parts[g]->mu")
    for name, rule in zip(NAMES, ("first_invalid_groups(", "first_invalid_centroids(", "first_invalid_scope_centroid(")):
        entry = api.split("\nint %s(" % name)[1].split("\n}\n")[0]
        owner = "cluster_scope_owner(" if name == "orr_cluster_scope_centroid" else "cluster_keys_owner("
        assert entry.index("cluster_key_groups::" + rule) < entry.index(owner) < entry.index("std::shared_lock") < entry.index("cluster_key_groups_hold("), name
        work = "for_each_shard(" if name == "orr_cluster_keys_groups" else "cluster_key_groups_sums("
        assert entry.index("cluster_key_groups_hold(") < entry.index(work), name          # every lane before any shard starts
        assert "sstats" not in entry, name
    sums = section.split("int cluster_key_groups_sums(")[1].split("\n}\n")[0]
    assert sums.index("for_each_shard(") < sums.index('"keys_chain_step"') and "for (int32_t g = 0; g < G && n_span; ++g)" in sums
    assert "if (r.chains.empty()) continue;" in sums     # a shard without a member of a spanning key is skipped
    single = api.split("\nint orr_keys_centroids(")[1].split("\n}\n")[0]
    assert "key_groups_slice_sums(" in single            # the single-index call is what it was
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_cluster_key_groups_plan_selftest" in makefile.split("all:")[0]
    assert "orr_cluster_key_groups_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]
    rule = makefile.split("host/orr_cluster_key_groups_plan_selftest: host/orr_cluster_key_groups_plan_selftest.cpp orr_cluster_key_groups_plan.h orr_key_groups_plan.h\n")[1]
    assert "-ffp-contract=off" in rule.split("\n")[0]


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entry_points_are_declared_exported_bound_and_documented():
    P = pkg()
    decl = _declared("omnirecall_hip.h")
    for name, n_args in zip(NAMES, N_ARGS):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, decl)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, m.group(1)
        assert name in P.native.EXPORTED_HIP_SYMBOLS
        f = getattr(P.native.hip, name)
        assert len(f.argtypes) == n_args and f.restype is C.c_int, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    assert P.native.hip.orr_abi_version() == 1              # adding functions is compatible
    for name in ("groups", "centroids"):
        assert callable(getattr(P.RecallClusterKeys, name)), name
    assert callable(P.RecallClusterScope.centroid)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    section = design.split("### 8w.")[1].split("\n## 9.")[0]
    assert "keys_chain_step" in section and "orr_cluster_key_groups_plan.h" in section
    part = full.split("---- cluster key groups:")[1]
    for piece in ("BIT FOR BIT", "COUNTED FROM THE KEY'S FIRST MEMBER ANYWHERE", "carry P", "keys_chain_step", "pinned host buffer",
                  "The search statistics do not move"):
        assert piece in part, piece
    for out_of_scope in ("sharded.py", "record (shard) form", "service mirror", "micro-batcher", "keys in the shard file", "device-side finish",
                         "pinned return path", "ranks documents by centroid", "every key on every shard"):
        assert out_of_scope in part or out_of_scope in section, out_of_scope
        assert out_of_scope in section, out_of_scope
    # the single index's texts keep their phrases, in the house style
    old = full.split("---- key groups:")[1].split("#define ORR_KEY_GROUPS_BLOCK")[0]
    assert "the cluster forms (built since: §8w" in old and "ARE NOT the single index's bits" in old
    assert "cluster forms (built since: §8w" in design.split("### 8v.")[1].split("### 8w.")[0]


def test_argument_errors_in_their_order_before_the_handle_with_the_outputs_untouched():
    """every case passes NULL handles (or a handle that is never looked at), each holding exactly one error more than the one behind it"""
    P = pkg()
    h, E = P.native.hip, P.native.ORR_EINVAL
    err = h.orr_last_error
    keys = np.full(4, 7, np.int64)
    rows = np.full(4, 7, np.int64)
    n, total = C.c_int64(7), C.c_int64(7)
    pn, pt = C.cast(C.byref(n), C.c_void_p), C.cast(C.byref(total), C.c_void_p)
    kp, rp = keys.ctypes.data, rows.ctypes.data

    assert h.orr_cluster_keys_groups(None, None, -1, None, None, None, None) == E and b"orr_cluster_keys_groups: cap is negative" in err()
    assert h.orr_cluster_keys_groups(None, None, 4, None, None, None, pt) == E and b"out_n or out_total is NULL" in err()
    assert h.orr_cluster_keys_groups(None, None, 4, None, None, pn, None) == E and b"out_n or out_total is NULL" in err()
    assert h.orr_cluster_keys_groups(None, None, 4, None, rp, pn, pt) == E and b"out_keys or out_rows is NULL" in err()
    assert h.orr_cluster_keys_groups(None, None, 4, kp, None, pn, pt) == E and b"out_keys or out_rows is NULL" in err()
    assert h.orr_cluster_keys_groups(None, None, 4, kp, rp, pn, pt) == E and b"null keys" in err()
    assert h.orr_cluster_keys_groups(None, None, 0, None, None, pn, pt) == E and b"null keys" in err()
    assert (keys == 7).all() and (rows == 7).all() and n.value == 7 and total.value == 7

    cent = np.full((4, 8), 7, np.float32)
    sums = np.full((4, 8), 7.0)
    used = np.full(4, 7, np.int64)
    cp, sp, up = cent.ctypes.data, sums.ctypes.data, used.ctypes.data
    for bad in (-1, 65_537, 1 << 30):
        assert h.orr_cluster_keys_centroids(None, None, bad, None, 8, cp, sp, None) == E and b"n_keys must be in 0 .. 65536" in err()
    assert h.orr_cluster_keys_centroids(None, None, 4, None, 8, cp, sp, None) == E and b"keys is NULL with 4 keys" in err()
    assert h.orr_cluster_keys_centroids(None, None, 4, kp, 8, cp, sp, None) == E and b"out_used is NULL with 4 keys" in err()
    assert h.orr_cluster_keys_centroids(None, None, 4, kp, 8, cp, sp, up) == E and b"orr_cluster_keys_centroids: null keys" in err()
    assert h.orr_cluster_keys_centroids(None, None, 4, kp, 0, None, None, up) == E and b"null keys" in err()    # (dim is looked at with the handle)
    assert h.orr_cluster_keys_centroids(None, None, 0, None, 8, None, None, None) == E and b"null keys" in err()
    assert h.orr_cluster_keys_centroids(None, None, 65_536, kp, 8, None, None, up) == E and b"null keys" in err()
    assert (cent == 7).all() and (sums == 7.0).all() and (used == 7).all()

    u = C.c_int64(7)
    pu = C.cast(C.byref(u), C.c_void_p)
    assert h.orr_cluster_scope_centroid(None, 8, cp, sp, None) == E and b"orr_cluster_scope_centroid: out_used is NULL" in err()
    assert h.orr_cluster_scope_centroid(None, 8, cp, sp, pu) == E and b"null scope" in err()
    assert h.orr_cluster_scope_centroid(None, 0, None, None, pu) == E and b"null scope" in err()
    assert u.value == 7 and (cent == 7).all() and (sums == 7.0).all()
