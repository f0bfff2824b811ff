"""CPU checks of the key groups (orr_keys_groups, orr_keys_centroids, orr_scope_centroid): the rules of
csrc/orr_key_groups_plan.h through their selftest (the argument order, the sort key, the blocks of a run, the slice rule, the
finish, the blocked order against the sequential and the reversed one), sum_blocked and finish compiled for the host against
this file's own numpy restatement on random data, the kernels and the driver made of the shared inlines, the three symbols
declared, exported, bound and documented, and every argument error on NULL handles in the documented order with the outputs
untouched -- so on a machine without a GPU (the method of tests/test_per_key_cpu.py).  The calls at work are in
tests/test_gpu_key_groups.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from helpers import ROOT, pkg

CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_key_groups_plan_selftest")
NAMES = ("orr_keys_groups", "orr_keys_centroids", "orr_scope_centroid")
N_ARGS = (7, 8, 5)
KERNELS = ("keys_pairs_count", "keys_pairs", "keys_pairs_scan", "keys_pairs_sort", "keys_runs", "keys_block_sums", "keys_block_fold")


def test_key_groups_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_key_groups_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_key_groups_plan_selftest: ok"
    m = re.search(r"block records checked: (\d+)", r.stdout)
    assert m and int(m.group(1)) == 1 + 1 + 1 + 2 + 2 + 3 + 391, r.stdout      # n = 1, 255, 256, 257, 512, 513, 100,000


def _sum_blocked(E):
    S = np.zeros(E.shape[1], np.float64)
    with np.errstate(all="ignore"):
        for b0 in range(0, E.shape[0], 256):
            P = np.zeros(E.shape[1], np.float64)
            for row in E[b0:b0 + 256].astype(np.float64):
                P = P + row
            S = S + P
    return S


def test_sum_blocked_and_finish_compiled_for_the_host_equal_the_numpy_restatement(tmp_path):
    """random rows over 30 decades with mixed signs, an infinity and signed zeros; members picked through their positions, out of
    order of storage; n in {0, 1, 255, 256, 257, 700}: the sums' uint64 bits and the centroids' uint32 bits"""
    src = tmp_path / "sum.cpp"
    src.write_text('#include "orr_key_groups_plan.h"\n#include <cstdio>\n#include <vector>\n' + """
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int32_t dim = 0, rows = 0, cases = 0;
    if (!f || fread(&dim, 4, 1, f) != 1 || fread(&rows, 4, 1, f) != 1 || fread(&cases, 4, 1, f) != 1) return 2;
    std::vector<float> emb((size_t)rows * dim);
    if (fread(emb.data(), 4, emb.size(), f) != emb.size()) return 2;
    FILE *o = fopen(argv[2], "wb");
    for (int c = 0; c < cases; ++c) {
        int64_t n = 0;
        if (fread(&n, 8, 1, f) != 1) return 2;
        std::vector<int64_t> member((size_t)n);
        if (n && fread(member.data(), 8, (size_t)n, f) != (size_t)n) return 2;
        std::vector<double> S((size_t)dim, 7.0);
        std::vector<float> cen((size_t)dim, 7.f);
        key_groups::sum_blocked(emb.data(), dim, member.data(), n, S.data());
        key_groups::finish(S.data(), n, dim, cen.data());
        fwrite(S.data(), 8, S.size(), o);
        fwrite(cen.data(), 4, cen.size(), o);
    }
    fclose(o);
    return 0;
}
""")
    exe = tmp_path / "sum"
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=120)
    rng = np.random.default_rng(5)
    dim, rows = 9, 900
    emb = (rng.standard_normal((rows, dim)) * 10.0 ** rng.uniform(-15, 15, (rows, dim))).astype(np.float32)
    emb[17, 2] = np.inf
    emb[30:40, 5] = -0.0
    members = [rng.permutation(rows)[:n].astype(np.int64) for n in (0, 1, 255, 256, 257, 700)]
    members.append(np.arange(30, 40, dtype=np.int64))   # every value of coordinate 5 is -0.0: the sum is +0.0
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([dim, rows, len(members)], np.int32).tobytes())
        f.write(emb.tobytes())
        for m in members:
            f.write(np.int64(len(m)).tobytes())
            f.write(m.tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=60)
    raw = open(tmp_path / "out.bin", "rb").read()
    at, differs = 0, 0
    for m in members:
        S = np.frombuffer(raw, np.float64, dim, at); at += 8 * dim
        c = np.frombuffer(raw, np.float32, dim, at); at += 4 * dim
        want = _sum_blocked(emb[m])
        assert np.array_equal(S.view(np.uint64), want.view(np.uint64)), len(m)
        with np.errstate(all="ignore"):
            wc = (want / np.float64(len(m))).astype(np.float32) if len(m) else np.zeros(dim, np.float32)
        assert np.array_equal(c.view(np.uint32), wc.view(np.uint32)), len(m)
        plain = np.zeros(dim, np.float64)
        with np.errstate(all="ignore"):
            for row in emb[m].astype(np.float64):
                plain = plain + row
        differs += int((plain.view(np.uint64) != want.view(np.uint64)).any())
    assert at == len(raw) and differs >= 1              # (the 700-member case tells the blocked order from the plain one)
    assert S.view(np.uint64)[5] == 0                    # the last case: ten times -0.0 from +0.0 is +0.0


def test_the_kernels_and_the_driver_share_the_rules():
    header = open(os.path.join(CSRC, "orr_key_groups_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_key_groups_plan_selftest.cpp")).read()
    for name in ("first_invalid_groups", "first_invalid_centroids", "first_invalid_scope_centroid", "sort_key", "key_of_sort", "participates",
                 "blocks_of", "slice_keys", "sum_blocked", "finish", "table_bits", "n_blocks_of"):
        assert len(re.findall(r"inline [\w:<>]+ %s\(" % name, header)) == 1, name
        assert re.search(r"\b%s\(" % name, selftest), name
    assert "kBlock = 256" in header and "kSliceBytes = (int64_t)64 << 20" in header
    pairs = kernels.split("void key_groups_pairs_kernel(")[1].split("hipError_t launch_keys_pairs(")[0]
    for piece in ("per_key::table_find(tk, n_tab, key[r])", "key_groups::participates(norm_b[r])", "key_groups::sort_key(k)", "__ballot(sel)",
                  "k != per_key::kNone", "r < n_rows", "at < cap"):
        assert piece in pairs, piece
    assert "atomic" not in pairs
    sums = kernels.split("void key_groups_block_sums_kernel(")[1].split("hipError_t launch_keys_block_sums(")[0]
    for piece in ("__shared__ uint32_t sh_pos[key_groups::kBlock]", "reinterpret_cast<const float4 *>(row)", "a0 = a0 + (double)v[j].x",
                  "b.part == key_groups::kDirect", "double a0 = +0.0"):
        assert piece in sums, piece
    assert "atomic" not in sums and "fma" not in sums.lower()
    fold = kernels.split("void key_groups_block_fold_kernel(")[1].split("hipError_t launch_keys_block_fold(")[0]
    assert "s = s + v[j]" in fold and "double s = +0.0" in fold and "atomic" not in fold
    assert "hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, key_in, key_out, pos_in, pos_out" in kernels
    assert "hipcub::DeviceRunLengthEncode::Encode(" in kernels and "hipcub::DeviceScan::ExclusiveSum(" in kernels
    # the driver: every launch timed under its own name; the entry points check their arguments through the header, in its order,
    # before a handle is looked at
    for k in KERNELS:
        assert api.count('Timed t(lane, "%s"' % k) == 1, k
    for name, rule in zip(NAMES, ("first_invalid_groups(", "first_invalid_centroids(", "first_invalid_scope_centroid(")):
        entry = api.split("\nint %s(" % name)[1].split("\n}\n")[0]
        owner = "scope_owner(" if name == "orr_scope_centroid" else "keys_owner("
        assert entry.index("key_groups::" + rule) < entry.index(owner) < entry.index("acquire_lane(") < entry.index("std::shared_lock"), name
        assert "sstats" not in entry, name
    cent = api.split("\nint orr_keys_centroids(")[1].split("\n}\n")[0]
    for piece in ("key_groups::slice_keys(dim, lane->opt_key_groups_slice)", "key_groups::blocks_of(", "key_groups::finish(", "per_key::member_table(keys, n_keys)"):
        assert piece in cent, piece
    assert '"key_groups_slice"' in api and "to->opt_key_groups_slice = from->opt_key_groups_slice" in api
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_key_groups_plan_selftest" in makefile.split("all:")[0]                      # in SELFTEST: build() makes it
    assert "orr_key_groups_plan.h" in makefile.split("%.o: %.hip")[1].split("\n")[0]
    assert "host/orr_key_groups_plan_selftest: host/orr_key_groups_plan_selftest.cpp orr_key_groups_plan.h" in makefile


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
    assert re.search(r"#define ORR_KEY_GROUPS_BLOCK 256\b", decl)
    for name in ("groups", "centroids"):
        assert callable(getattr(P.RecallKeys, name)), name
    assert callable(P.RecallScope.centroid)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    full = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    assert "8v" in design and all(k in design for k in KERNELS)
    part = full.split("---- key groups:")[1].split("#define ORR_KEY_GROUPS_BLOCK")[0]
    for piece in ("BLOCKS OF 256", "normB > 0.0", "round to nearest even", "key_groups_slice", "ARE NOT the single index's bits"):
        assert piece in part, piece
    for out_of_scope in ("cluster forms", "unit-normalised", "weighted mean", "sharded.py", "service mirror", "micro-batcher",
                         "keys in the shard file", "ranks documents by centroid"):
        assert out_of_scope in part, out_of_scope
        assert out_of_scope in design.split("### 8v.")[1].split("\n## 9.")[0], out_of_scope


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

    # orr_keys_groups: cap negative; out_n or out_total NULL; an array NULL with cap > 0; the keys handle NULL
    assert h.orr_keys_groups(None, None, -1, None, None, None, None) == E and b"orr_keys_groups: cap is negative" in err()
    assert h.orr_keys_groups(None, None, 4, None, None, None, pt) == E and b"out_n or out_total is NULL" in err()
    assert h.orr_keys_groups(None, None, 4, None, None, pn, None) == E and b"out_n or out_total is NULL" in err()
    assert h.orr_keys_groups(None, None, 4, None, rp, pn, pt) == E and b"out_keys or out_rows is NULL" in err()
    assert h.orr_keys_groups(None, None, 4, kp, None, pn, pt) == E and b"out_keys or out_rows is NULL" in err()
    assert h.orr_keys_groups(None, None, 4, kp, rp, pn, pt) == E and b"null keys" in err()
    assert h.orr_keys_groups(None, None, 0, None, None, pn, pt) == E and b"null keys" in err()
    assert (keys == 7).all() and (rows == 7).all() and n.value == 7 and total.value == 7

    # orr_keys_centroids: n_keys outside 0 .. 65,536; keys NULL; out_used NULL; the keys handle NULL
    cent = np.full((4, 8), 7, np.float32)
    sums = np.full((4, 8), 7.0)
    used = np.full(4, 7, np.int64)
    cp, sp, up = cent.ctypes.data, sums.ctypes.data, used.ctypes.data
    for bad in (-1, 65_537, 1 << 30):
        assert h.orr_keys_centroids(None, None, bad, None, 8, cp, sp, None) == E and b"n_keys must be in 0 .. 65536" in err()
    assert h.orr_keys_centroids(None, None, 4, None, 8, cp, sp, None) == E and b"keys is NULL with 4 keys" in err()
    assert h.orr_keys_centroids(None, None, 4, kp, 8, cp, sp, None) == E and b"out_used is NULL with 4 keys" in err()
    assert h.orr_keys_centroids(None, None, 4, kp, 8, cp, sp, up) == E and b"null keys" in err()
    assert h.orr_keys_centroids(None, None, 4, kp, 0, None, None, up) == E and b"null keys" in err()    # (dim is looked at with the handle)
    assert h.orr_keys_centroids(None, None, 0, None, 8, None, None, None) == E and b"null keys" in err()
    assert h.orr_keys_centroids(None, None, 65_536, kp, 8, None, None, up) == E and b"null keys" in err()
    assert (cent == 7).all() and (sums == 7.0).all() and (used == 7).all()

    # orr_scope_centroid: out_used NULL; the scope NULL
    u = C.c_int64(7)
    pu = C.cast(C.byref(u), C.c_void_p)
    assert h.orr_scope_centroid(None, 8, cp, sp, None) == E and b"orr_scope_centroid: out_used is NULL" in err()
    assert h.orr_scope_centroid(None, 8, cp, sp, pu) == E and b"null scope" in err()
    assert h.orr_scope_centroid(None, 0, None, None, pu) == E and b"null scope" in err()
    assert u.value == 7 and (cent == 7).all() and (sums == 7.0).all()

    # the option
    assert h.orr_index_set_option(None, b"key_groups_slice", 1) == E
