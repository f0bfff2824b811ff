"""The diverse search over a cluster's shards (orr_cluster_search_batch_diverse) and its diagnostic (orr_cluster_pair_dots).

The contract is one sentence: the answers of orr_search_batch_diverse on ONE index holding all the cluster's rows.  So the model
is tests/test_gpu_diverse.py's own -- its restatement (_want, _pair_dots), its corpora D1 (4,099 x 70) and D2 (4,099 x 128) with
their planted near-duplicate families, its queries -- and the twin is that module's single index.  The clusters hold the same
rows cut into three shards on ordinal 0 at uneven cuts; the families were planted at random positions, so they lie across the
shard borders (test_the_planted_families_span_the_shards).  Every comparison is exact: rows, counts and ranks with
np.array_equal, scores and sums bit for bit (NaN = NaN).

What only a cluster has is the pair step's plan (csrc/orr_cluster_diverse_plan.h): _plan restates it -- home = the shard holding
most of a pool, a tie to the lowest; the rest is gathered on its shard -- and the shards' kernel statistics are held against it
(rows_gather: algorithmic bytes 8 * dim * rows)."""
import threading

import numpy as np
import pytest

import test_gpu_diverse as dbase
import test_gpu_scope_terms as tbase
from helpers import pkg

pytestmark = pytest.mark.gpu

INF = dbase.INF
CUTS = {"D1": (211, 2_905), "D2": (150, 1_733), "D4": (100_000,)}        # uneven; the first below 300: a candidate_limit of 300 spans two shards
_syn, _terms, _same_bits, _diverse, _check, _batch = dbase._syn, dbase._terms, dbase._same_bits, dbase._diverse, dbase._check, dbase._batch


# ---- clusters ----------------------------------------------------------------------------------------------------------------

def _cluster_of(emb, created, rowbytes, ids, cuts, capacity=0):
    P, syn = pkg(), _syn()
    n, dim = emb.shape
    edges = (0,) + tuple(cuts) + (n,)
    cl = P.RecallCluster([0] * (len(edges) - 1), dim, capacity_rows_per_shard=capacity)
    for g in range(len(edges) - 1):
        r0, r1 = edges[g], edges[g + 1]
        off = np.arange(r1 - r0 + 1, dtype=np.int64) * syn.ROW_BYTES
        for c0 in range(r0, r1, 50_000):
            c1 = min(r1, c0 + 50_000)
            cl.shard(g).append(emb[c0:c1], created[c0:c1], rowbytes[c0:c1].reshape(-1), off[: c1 - c0 + 1], row_ids=ids[c0:c1])
    cl.seal()
    return cl


_CLUSTERS = {}


def _cluster(name):
    """(the module's shard `name` -- twin index, model, queries --, the cluster over the same rows, its edges)"""
    s = dbase._shard(name)
    if name not in _CLUSTERS:
        m = s["model"]
        _CLUSTERS[name] = _cluster_of(m.emb, m.created, m.rowbytes, m.ids, CUTS[name])
    return s, _CLUSTERS[name], (0,) + CUTS[name] + (s["n"],)


def _cstats(cl, fn):
    """fn() and every shard's kernel statistics of it alone"""
    shards = [cl.shard(g) for g in range(cl.n_shards)]
    for sh in shards:
        sh.set_profiling(True)
    try:
        r = fn()
        return r, [sh.kernel_stats() for sh in shards]
    finally:
        for sh in shards:
            sh.set_profiling(False)


def _n(st, name):
    return st[name]["launches"] if name in st else 0


def _gathered(st, dim):
    rows = st["rows_gather"]["algo_bytes"] / (8.0 * dim) if "rows_gather" in st else 0.0
    assert rows == int(rows), rows
    return int(rows)


def _plan(pools, edges):
    """the pair step of these pools (global order keys each; only pools that read a cosine): per shard how many lists are at
    home there and how many rows it sends away, and the bound sum(n - ceil(n / G))"""
    G = len(edges) - 1
    homes, sent, bound = [0] * G, [0] * G, 0
    for keys in pools:
        held = np.bincount(np.searchsorted(np.asarray(edges[1:]), np.asarray(keys), side="right"), minlength=G)
        h = int(np.argmax(held))                            # the first of the largest: a tie goes to the lowest shard
        homes[h] += 1
        for g in range(G):
            if g != h:
                sent[g] += int(held[g])
        bound += len(keys) - -(-len(keys) // G)
    return homes, sent, bound


def _held_against_the_plan(sts, pools, edges, dim, what):
    """one group: at most one launch of each kernel a shard, exactly where and as much as the plan says"""
    homes, sent, bound = _plan(pools, edges)
    for g, st in enumerate(sts):
        assert _n(st, "pair_dots") == (1 if homes[g] else 0), (what, g, homes, st.get("pair_dots"))
        assert _n(st, "rows_gather") == (1 if sent[g] else 0), (what, g, sent, st.get("rows_gather"))
        assert _gathered(st, dim) == sent[g], (what, g, sent, st.get("rows_gather"))
    assert sum(sent) <= bound, (what, sent, bound)
    return homes, sent


def test_the_planted_families_span_the_shards():
    for name in ("D1", "D2"):
        s, cl, edges = _cluster(name)
        assert cl.n_shards == 3 and cl.rows == s["n"] and [cl.shard(g).rows for g in range(3)] == [edges[g + 1] - edges[g] for g in range(3)]
        for a, rows in s["fam"].items():
            assert len(set(np.searchsorted(edges[1:], rows, side="right").tolist())) >= 2, (name, a)


# ---- 1. pair_dots ------------------------------------------------------------------------------------------------------------

def _check_cluster_pairs(cl, twin, emb, edges, lists, what):
    got, sts = _cstats(cl, lambda: cl.pair_dots(lists))
    want = twin.pair_dots(lists)                            # the twin's row_base is 0: a position is the global order key
    assert got.shape == want.shape and _same_bits(got, want), what
    for l, keys in enumerate(lists):
        m = len(keys)
        if m:
            assert _same_bits(got[l, :m, :m], dbase._pair_dots(emb[np.asarray(keys)])), (what, l)
        assert np.isnan(got[l, m:, :]).all() and np.isnan(got[l, :, m:]).all()      # beyond a list's length nothing is written
    dim = emb.shape[1]
    return _held_against_the_plan(sts, [k for k in lists if len(k)], edges, dim, what)


def _pair_lists(edges, rng):
    e0, e1, e2, e3 = edges
    on = lambda g, m: (edges[g] + rng.choice(edges[g + 1] - edges[g], m, replace=False)).tolist()
    return {
        "one shard": [on(1, 56)],
        "one foreign member": [on(2, 23) + on(0, 1)],
        "the borders": [[e0, e1 - 1, e1, e2 - 1, e2, e3 - 1]],
        "56 spread evenly": [[edges[i % 3] + i // 3 for i in range(56)]],
        "a home tie": [on(2, 2) + on(1, 2)],
        "a three-way tie": [on(2, 5) + on(0, 5) + on(1, 5)],
        "the same row twice": [[e1 + 7, e0 + 3, e1 + 7, e0 + 3, e1 + 9, e2 + 1, e2 + 1]],
        "one member": [[e2 + 5]],
        "mixed": [on(0, 9) + on(2, 4), [], on(1, 1), on(2, 30) + on(1, 26), on(0, 2), []],
    }


@pytest.mark.parametrize("name", ["D1", "D2"])
def test_cluster_pair_dots_are_the_twins_and_the_restatements(name):
    s, cl, edges = _cluster(name)
    emb = s["model"].emb
    for what, lists in _pair_lists(edges, np.random.default_rng(31)).items():
        homes, sent = _check_cluster_pairs(cl, s["idx"], emb, edges, lists, (name, what))
        if what == "one shard":
            assert homes == [0, 1, 0] and sent == [0, 0, 0]
        if what == "a home tie":                             # 2 : 2 between shards 1 and 2: shard 1 is home, shard 2 sends
            assert homes == [0, 1, 0] and sent == [0, 0, 2]
        if what == "a three-way tie":
            assert homes == [1, 0, 0] and sent == [0, 5, 5]
        if what == "56 spread evenly":
            assert homes == [1, 0, 0] and sum(sent) == 56 - 19
        if what == "the same row twice":                     # no de-duplication: the row wanted twice is gathered twice
            assert homes == [0, 1, 0] and sent == [2, 0, 2]


def test_cluster_pair_dots_over_four_slabs():
    """3 x 700 x 1024 built here: 16-byte staging, four slabs, rows from all three shards in one list"""
    n, dim, cuts = 2_100, 1024, (700, 1_400)
    rng = np.random.default_rng(9)
    emb = rng.standard_normal((n, dim), dtype=np.float32)
    emb[800] = emb[100]                                      # an exact copy on another shard
    _, created, rowbytes = tbase._rows(n, 64)
    ids = np.arange(n, dtype=np.int64) + 5
    cl = _cluster_of(emb, created, rowbytes, ids, cuts)
    twin = tbase._build(emb, created, rowbytes, ids, n)
    try:
        edges = (0,) + cuts + (n,)
        lists = _pair_lists(edges, rng)
        for what in ("56 spread evenly", "one foreign member", "a home tie", "mixed", "one shard"):
            _check_cluster_pairs(cl, twin, emb, edges, lists[what], what)
        got = cl.pair_dots([[100, 800, 1_500]])
        assert got[0, 0, 1] == got[0, 0, 0] == got[0, 1, 1]  # the copy: the same sum whichever source a row is read from
    finally:
        cl.close()
        twin.close()


def test_cluster_pair_dots_argument_errors_come_from_the_host_before_any_launch():
    P = pkg()
    s, cl, edges = _cluster("D2")
    n = s["n"]
    h, E = P.native.hip, P.native.ORR_EINVAL

    def refused(lists, what):
        def call():
            with pytest.raises(P.native.OrrError) as e:
                cl.pair_dots(lists)
            assert what in str(e.value), str(e.value)
        _, sts = _cstats(cl, call)
        assert all("pair_dots" not in st and "rows_gather" not in st for st in sts)

    refused([[0, n]], "is outside every shard")
    refused([[1, 2], [5, -1]], "is outside every shard")
    refused([list(range(57))], "stride must be in 1 .. 56")
    off, keys, out = np.array([0, 5], np.uint32), np.arange(5, dtype=np.int64) * 900, np.full((1, 4, 4), 7.0)
    fp, kp, op = off.ctypes.data, keys.ctypes.data, out.ctypes.data

    def raw():
        assert h.orr_cluster_pair_dots(cl._h, 1, fp, kp, 4, op) == E and b"holds 5 order keys, stride is 4" in h.orr_last_error()
        assert h.orr_cluster_pair_dots(cl._h, 1, fp, kp, 5, None) == E and b"out is NULL" in h.orr_last_error()
        assert h.orr_cluster_pair_dots(cl._h, -1, fp, kp, 5, op) == E and b"n_lists is negative" in h.orr_last_error()
        assert h.orr_cluster_pair_dots(cl._h, 1, None, kp, 5, op) == E and b"list_off is NULL" in h.orr_last_error()
        assert h.orr_cluster_pair_dots(cl._h, 1, fp, None, 5, op) == E and b"order_keys is NULL" in h.orr_last_error()
        assert h.orr_cluster_pair_dots(None, 1, fp, kp, 5, op) == E and b"null cluster" in h.orr_last_error()
        assert h.orr_cluster_pair_dots(cl._h, 0, fp, kp, 5, op) == 0
    _, sts = _cstats(cl, raw)
    assert all("pair_dots" not in st and "rows_gather" not in st for st in sts) and (out == 7.0).all()


# ---- 2. the search -----------------------------------------------------------------------------------------------------------

def _reads(pool, mode, param):
    return pool >= 2 and not (mode == "collapse" and param == INF) and not (mode == "mmr" and param == 1.0)


@pytest.mark.parametrize("name,B,limit", [("D1", 1, 300), ("D1", 64, 4_099), ("D1", 130, 300), ("D2", 5, 4_099), ("D2", 64, 300),
                                          ("D2", 130, 4_099)])
def test_rows_score_bits_counts_and_pool_ranks_are_one_indexs(name, B, limit):
    s, cl, edges = _cluster(name)
    twin = s["idx"]
    qis, q, texts = _batch(s, B)
    n_diff = n_moved = 0
    for topk, pool in ((1, 2), (4, 24), (10, 56)):
        plain = cl.search(q, _terms(texts), _syn().NOW_TICKS, topk, candidate_limit=limit)
        for mode, params in (("collapse", dbase.MAX_COSINES), ("mmr", dbase.LAMBDAS)):
            for param in params:
                what = (name, B, limit, topk, pool, mode, param)
                got, sts = _cstats(cl, lambda: _diverse(cl, q, texts, topk, pool, mode, param, limit))
                want = _diverse(twin, q, texts, topk, pool, mode, param, limit)
                assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]), what
                assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what
                _check(got, s, qis, topk, pool, mode, param, limit, what=what)
                if not _reads(pool, mode, param):           # nothing beyond the pool's search, and the cluster's plain search bit for bit
                    assert all(_n(st, "pair_dots") == 0 and _n(st, "rows_gather") == 0 for st in sts), what
                    assert np.array_equal(got[0], plain[0]) and _same_bits(got[1], plain[1]) and np.array_equal(got[2], plain[2]), what
                    assert all(list(got[3][b, :got[2][b]]) == list(range(got[2][b])) for b in range(B))
                    continue
                pools = [dbase._pool(s, qi, limit)[0][:pool] for qi in qis]
                homes, sent = _held_against_the_plan(sts, [p for p in pools if len(p) >= 2], edges, s["dim"], what)
                n_moved += sum(sent)
                if topk > 1 and param in (0.95, 0.5, 0.3):
                    n_diff += int((got[0][:5] != plain[0][:5]).any())
    assert n_moved > 0, (name, B, limit)                    # the pools did span shards
    if limit >= s["n"]:
        assert n_diff > 0, (name, B, limit)                 # the planted families take part: the feature did something


def test_the_planted_queries_lose_near_duplicates_that_sit_on_other_shards():
    s, cl, edges = _cluster("D2")
    n, model = s["n"], s["model"]
    qis, q, texts = _batch(s, 5)
    plain = cl.search(q, _terms(texts), _syn().NOW_TICKS, 4, candidate_limit=n)
    got = _diverse(cl, q, texts, 4, 56, "collapse", 0.95, n)
    _check(got, s, qis, 4, 56, "collapse", 0.95, n)
    for b in range(4):
        fam = set(model.ids[s["fam"][s["anchors"][b]]].tolist())
        assert set(plain[0][b].tolist()) <= fam and not np.array_equal(got[0][b], plain[0][b])
        assert got[0][b, 0] == plain[0][b, 0] and got[2][b] == 4
        shard_of = lambda ids: np.searchsorted(edges[1:], model.rows_of_ids(ids), side="right")
        dropped = np.setdiff1d(plain[0][b], got[0][b])
        assert len(dropped) and len(set(shard_of(plain[0][b]).tolist())) >= 2, (b, shard_of(plain[0][b]))     # the copies it lost span shards
        c = dbase._pair_cos(model.emb[model.rows_of_ids(got[0][b])])
        assert all(c[i][j] < 0.95 for i in range(4) for j in range(4) if i != j), c
    big = _diverse(cl, q[4:5], texts[4:5], 10, 56, "collapse", 0.99, n)     # the family of 61: the collapse runs out of pool
    _check(big, s, [4], 10, 56, "collapse", 0.99, n)
    assert big[2][0] == 1


def test_a_foreign_query_dimension_and_an_empty_batch():
    s, cl, edges = _cluster("D2")
    rng = np.random.default_rng(3)
    qf = rng.standard_normal((3, 64)).astype(np.float32)
    texts = [s["texts"][20], s["texts"][21], ""]
    for mode, param in (("collapse", 0.5), ("mmr", 0.3)):
        got = _diverse(cl, qf, texts, 4, 24, mode, param, 300)
        want = _diverse(s["idx"], qf, texts, 4, 24, mode, param, 300)
        assert all(np.array_equal(got[i], want[i]) for i in (0, 2, 3)) and _same_bits(got[1], want[1])
        for b in range(3):
            _check(tuple(x[b:b + 1] for x in got), s, [b], 4, 24, mode, param, 300, qvec=qf[b], text=texts[b], tag=("cluster foreign", b))
    h = pkg().native.hip
    qoff = np.zeros(1, np.uint32)
    out = np.full(4, 7, np.int64)
    assert h.orr_cluster_search_batch_diverse(cl._h, 0, 128, None, None, None, qoff.ctypes.data, 0, 4, 300, None, 24, 0, 0.5, out.ctypes.data,
                                              out.ctypes.data, out.ctypes.data, None) == 0
    assert (out == 7).all()


# ---- 3. within cluster scopes ------------------------------------------------------------------------------------------------

def test_within_cluster_scopes():
    s, cl, edges = _cluster("D2")
    twin, n, model = s["idx"], s["n"], s["model"]
    qis, q, texts = _batch(s, 12)
    rng = np.random.default_rng(8)
    fam_ids = model.ids[sorted(set(sum(s["fam"].values(), [])))]
    all_shards = np.unique(np.concatenate([fam_ids, model.ids[rng.choice(n, 700, replace=False)]]))
    one_shard = model.ids[edges[1] + np.sort(rng.choice(edges[2] - edges[1], 600, replace=False))]
    for what, ids in (("all shards", all_shards), ("one shard", one_shard), ("empty", np.zeros(0, np.int64))):
        sc, tsc = cl.scope(ids), twin.scope(ids)
        try:
            assert sc.rows == len(ids) == tsc.rows, what
            for mode, param, topk, pool in (("collapse", 0.95, 4, 24), ("mmr", 0.3, 10, 56), ("collapse", INF, 4, 4)):
                got, sts = _cstats(cl, lambda: _diverse(cl, q, texts, topk, pool, mode, param, n, within=sc))
                want = _diverse(twin, q, texts, topk, pool, mode, param, n, within=tsc)
                assert all(np.array_equal(got[i], want[i]) for i in (0, 2, 3)) and _same_bits(got[1], want[1]), (what, mode)
                _check(got, s, qis, topk, pool, mode, param, n, scope_ids=ids, what=(what, mode))
                if what == "empty":
                    assert (got[2] == 0).all()
                if param == INF:
                    inside = cl.search_in_scope(q, _terms(texts), _syn().NOW_TICKS, topk, sc, candidate_limit=n)
                    assert np.array_equal(got[0], inside[0]) and _same_bits(got[1], inside[1]) and np.array_equal(got[2], inside[2])
                if what == "empty" or param == INF:
                    assert all(_n(st, "pair_dots") == 0 and _n(st, "rows_gather") == 0 for st in sts), (what, mode)
                elif what == "one shard":                    # every pool at home on shard 1: nothing moves, one launch there
                    assert [_n(st, "rows_gather") for st in sts] == [0, 0, 0] and [_n(st, "pair_dots") for st in sts] == [0, 1, 0], (what, mode)
                else:
                    pools = [dbase._pool(s, qi, n, ids)[0][:pool] for qi in qis]
                    homes, sent = _held_against_the_plan(sts, [p for p in pools if len(p) >= 2], edges, s["dim"], (what, mode))
                    assert sum(sent) > 0
        finally:
            sc.close()
            tsc.close()


# ---- 5. maintenance ----------------------------------------------------------------------------------------------------------

def test_after_maintenance_the_updated_vector_is_compared_and_moved_row_bases_are_followed():
    n = dbase.SHAPES["D2"][0]
    s = dbase._build_shard("D2", capacity=n + 64)           # a twin of its own, rebuilt here from the same rows
    twin, model = s["idx"], s["model"]
    cl = _cluster_of(model.emb, model.created, model.rowbytes, model.ids, CUTS["D2"], capacity=n + 64)
    edges = (0,) + CUTS["D2"] + (n,)
    shard_of = {int(i): g for g in range(3) for i in model.ids[edges[g]:edges[g + 1]]}
    qis, q, texts = _batch(s, 10)

    def check(what):
        s["cache"].clear()                                   # the model moved
        for mode, param in (("collapse", 0.95), ("mmr", 0.3)):
            got = _diverse(cl, q, texts, 4, 24, mode, param, len(model.ids))
            want = _diverse(twin, q, texts, 4, 24, mode, param, len(model.ids))
            assert all(np.array_equal(got[i], want[i]) for i in (0, 2, 3)) and _same_bits(got[1], want[1]), (what, mode)
            _check(got, s, qis, 4, 24, mode, param, len(model.ids), what=(what, mode))

    def on_shards(ids, fn):
        done = 0
        for g in range(3):
            mine = [k for k, i in enumerate(ids) if shard_of[int(i)] == g]
            if mine:
                done += fn(cl.shard(g), mine)
        return done

    try:
        check("fresh")
        # update through ONE shard: an old row far from every query (shard 2) becomes an exact copy of anchor 1 (another shard)
        far = model.ids[[n - 5]]
        a1 = s["anchors"][1]
        assert shard_of[int(far[0])] == 2
        new = model.emb[a1][None, :].copy()
        assert cl.shard(2).update_rows(far, new) == 1 and twin.update_rows(far, new) == 1
        model.update(far, new)
        check("updated")
        far_pos = int(np.nonzero(model.ids == far[0])[0][0])
        assert far_pos in dbase._pool(s, 1, len(model.ids))[0][:24].tolist()      # it stands in query 1's pool: its NEW vector was compared
        d = cl.pair_dots([[a1, far_pos]])
        assert d[0, 0, 1] == d[0, 0, 0] == d[0, 1, 1]
        # deletes on every shard (the best near-copies of family 0 among them), then the row bases move
        fam = s["fam"][s["anchors"][0]]
        gone = np.unique(np.concatenate([model.ids[fam[1:3]], model.ids[np.random.default_rng(6).choice(n - 10, 300, replace=False)]]))
        gone = gone[gone != model.ids[a1]]
        assert on_shards(gone, lambda sh, mine: sh.delete_rows(gone[mine])) == len(gone) and twin.delete_rows(gone) == len(gone)
        model.delete(gone)
        check("deleted")
        assert cl.compact() == len(gone) and twin.compact() == len(gone)
        model.compact()
        assert cl.rows == len(model.ids) == twin.rows          # every shard lost rows: the bases behind shard 0 moved
        check("compacted")
        m = 32
        _, c2, b2 = tbase._rows(m, 64, row0=n, n_total=n + m)                      # older than every row: they belong to the last shard
        e2 = np.random.default_rng(4).standard_normal((m, s["dim"]), dtype=np.float32)
        e2[0] = model.emb[0]                                                      # an exact copy of a row of shard 0
        e2[1] = dbase._noisy(np.random.default_rng(2), s["q"][2], 0.02)           # lands in query 2's pool
        ids2 = np.arange(m, dtype=np.int64) + 10_000_000
        off2 = np.arange(m + 1, dtype=np.int64) * b2.shape[1]
        assert cl.insert_rows(2, e2, c2, b2.reshape(-1), off2, row_ids=ids2) == m
        twin.insert_rows(e2, c2, b2.reshape(-1), off2, row_ids=ids2)
        model.insert(e2, c2, b2, ids2)
        check("inserted")
        # ... and into the FIRST shard's neighbourhood: rows as new as shard 1's newest, so every base behind shard 1 moves
        first1 = cl.shard(0).rows
        c3 = np.full(3, model.created[first1], np.int64)
        e3 = np.stack([dbase._noisy(np.random.default_rng(5 + i), s["q"][3], 0.02) for i in range(3)])
        ids3 = np.arange(3, dtype=np.int64) + 20_000_000
        off3 = np.arange(4, dtype=np.int64) * b2.shape[1]
        assert cl.insert_rows(1, e3, c3, b2[:3].reshape(-1), off3, row_ids=ids3) == 3
        twin.insert_rows(e3, c3, b2[:3].reshape(-1), off3, row_ids=ids3)
        model.insert(e3, c3, b2[:3], ids3)
        check("inserted in the middle")
    finally:
        cl.close()
        twin.close()


# ---- 6. refusals and lifetime ------------------------------------------------------------------------------------------------

def _tiny(seal=True, dim=64, n_per=300):
    P, syn = pkg(), _syn()
    n = 2 * n_per
    emb, created, rowbytes = tbase._rows(n, dim)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    off = np.arange(n_per + 1, dtype=np.int64) * syn.ROW_BYTES
    cl = P.RecallCluster([0, 0], dim)
    for g in range(2):
        r0, r1 = g * n_per, (g + 1) * n_per
        cl.shard(g).append(emb[r0:r1], created[r0:r1], rowbytes[r0:r1].reshape(-1), off, row_ids=ids[r0:r1])
    if seal:
        cl.seal()
    return cl, ids


def _raises(code, call, what):
    P = pkg()
    with pytest.raises(P.native.OrrError) as e:
        call()
    assert e.value.code == code and what in str(e.value), (e.value.code, str(e.value))


def test_refusals_an_unsealed_cluster_foreign_and_orphaned_scopes_device_queries():
    import torch
    P = pkg()
    N = P.native
    q, terms = np.ones((2, 64), np.float32), [[b"abc"], []]
    cl, ids = _tiny(seal=False)
    _raises(N.ORR_ESTATE, lambda: cl.search_diverse(q, terms, 0, 4, 24), "not sealed")
    _raises(N.ORR_ESTATE, lambda: cl.pair_dots([[0, 1]]), "not sealed")
    _raises(N.ORR_EINVAL, lambda: cl.search_diverse(q, terms, 0, 4, 3), "exceeds the pool")       # the arguments come first
    cl.seal()
    other, _ = _tiny()
    theirs, mine = other.scope(ids[:100]), cl.scope(ids[:100])
    _raises(N.ORR_EINVAL, lambda: cl.search_diverse(q, terms, 0, 4, 24, within=theirs), "belongs to another cluster")
    assert cl.search_diverse(q, terms, 0, 4, 24, within=mine)[2].tolist() == [4, 4]
    other.close()                                            # its scope is orphaned now
    _raises(N.ORR_ESTATE, lambda: cl.search_diverse(q, terms, 0, 4, 24, within=theirs), "orphaned")
    dq = torch.from_numpy(q).cuda()
    import omni_recall_rag_amd.index as index
    pool, toff, qoff = index.pack_terms(terms)
    rows, scores, counts, ranks = np.full((2, 4), 7, np.int64), np.full((2, 4), 7.0), np.full(2, 7, np.int32), np.full((2, 4), 7, np.int32)
    for within in (None, mine._h):
        r = N.hip.orr_cluster_search_batch_diverse(cl._h, 2, 64, dq.data_ptr(), pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, 0, 4, 300, within,
                                                   24, 0, 0.5, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data, ranks.ctypes.data)
        assert r == N.ORR_EINVAL and b"host memory" in N.hip.orr_last_error()
    r = N.hip.orr_cluster_search_batch_diverse(None, 2, 64, q.ctypes.data, pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, 0, 4, 300, None,
                                               24, 0, 0.5, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data, ranks.ctypes.data)
    assert r == N.ORR_EINVAL and b"null cluster" in N.hip.orr_last_error()
    assert (rows == 7).all() and (scores == 7.0).all() and (counts == 7).all() and (ranks == 7).all()
    theirs.close()
    mine.close()
    cl.close()


def test_four_threads_on_one_cluster_each_get_the_single_thread_answer():
    s, cl, edges = _cluster("D2")
    n = s["n"]
    qis, q, texts = _batch(s, 16)
    cases = (("collapse", 0.95), ("mmr", 0.3), ("collapse", 0.5), ("mmr", 0.7))
    alone = [_diverse(cl, q, texts, 10, 56, mode, param, n) for mode, param in cases]
    cl.search_stats(reset=True)
    results, errors = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                results[i] = _diverse(cl, q, texts, 10, 56, *cases[i], n)
        except Exception as e:                               # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, (mode, param) in enumerate(cases):
        assert all(np.array_equal(results[i][k], alone[i][k]) for k in (0, 2, 3)) and _same_bits(results[i][1], alone[i][1]), (mode, param)
        _check(results[i], s, qis, 10, 56, mode, param, n, what=("threads", mode, param))
    st = cl.search_stats()
    assert st["searches"] == 12 and st["queries"] == 12 * 16, st      # each call one search of B queries


# ---- 7. the two-stage pool ---------------------------------------------------------------------------------------------------

def test_the_pool_of_a_two_stage_pass_over_two_shards():
    """2 x 100,000 x 128 with 130 queries against the twin of 200,000 rows, whose pool is the two-stage pass's"""
    s, cl, edges = _cluster("D4")                            # 2 x 100,000 x 128
    twin, n = s["idx"], s["n"]
    for sh in [twin] + [cl.shard(g) for g in range(2)]:
        sh.set_option("two_stage", 1)
    qis = [b % dbase.NQ if b % dbase.NQ != 8 else 9 for b in range(130)]      # (without the NaN query, as the single index's test)
    q, texts = s["q"][qis], [s["texts"][i] for i in qis]
    cl.search_stats(reset=True)
    got, sts = _cstats(cl, lambda: _diverse(cl, q, texts, 10, 56, "collapse", 0.95, n))
    stats = cl.search_stats()
    assert stats["searches"] == 1 and stats["queries"] == 130, stats
    twin.search_stats(reset=True)
    want = _diverse(twin, q, texts, 10, 56, "collapse", 0.95, n)
    # the twin's pool comes from the two-stage int8 pass; a shard of 100,000 rows is below the 48 selection segments that pass
    # asks for, so the cluster's pool comes from the split pass of each shard: the two must agree all the same
    assert twin.search_stats()["pass_mode"] == 1, twin.search_stats()
    assert all(np.array_equal(got[i], want[i]) for i in (0, 2, 3)) and _same_bits(got[1], want[1])
    assert all(_n(st, "pair_dots") <= 1 and _n(st, "rows_gather") <= 1 for st in sts) and sum(_n(st, "pair_dots") for st in sts) >= 1
    assert sum(_gathered(st, s["dim"]) for st in sts) <= 130 * (56 - 28)
    got = _diverse(cl, q, texts, 10, 24, "mmr", 0.3, n)
    want = _diverse(twin, q, texts, 10, 24, "mmr", 0.3, n)
    assert all(np.array_equal(got[i], want[i]) for i in (0, 2, 3)) and _same_bits(got[1], want[1])
