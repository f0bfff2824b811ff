"""Row keys and the per-key search over a cluster's shards (orr_cluster_keys_*, orr_cluster_scope_create_keys,
orr_cluster_search_batch_per_key).

The contract is one sentence: the answers of orr_search_batch_per_key on ONE index holding all the cluster's rows.  So the model
is tests/test_gpu_per_key.py's own -- its restatement (_want, _check), its corpora K1 (4,099 x 70) and K3 (70,001 x 64) with their
planted documents, its queries and key assignment -- and the twin is that module's single index.  The K1 cluster holds the same
rows in three shards on ordinal 0, cut at (211, 3804): a candidate_limit of 300 ends inside the second shard, the second cut
lies inside the second of target A's five planted documents (rows 3,769 .. 3,838), so the key that closes in round 2 has rows on
both sides of a border, and SPREAD_KEY lies on two shards (test_the_cuts_put_a_document_and_a_key_across_the_borders).  Every
comparison is exact: rows, keys, counts and rounds with np.array_equal, scores bit for bit (NaN = NaN).

What only a cluster has is held against the shards' kernel statistics: which shard gathers (one keys_gather where a pool member
lies, none elsewhere), one keys_exclude / scope_counts / mask_clip_slots per slice on EVERY shard (a key closes cluster-wide),
keys_clear_seen only where a seen row lies."""
import threading

import numpy as np
import pytest

import test_gpu_cluster_diverse as cbase
import test_gpu_cluster_scope as sbase
import test_gpu_per_key as kbase
import test_gpu_scope_terms as tbase
from helpers import pkg

pytestmark = pytest.mark.gpu

NONE = kbase.NONE
CUTS = {"K1": (211, 3_804), "K3": (20_011, 50_003)}
_syn, _terms, _same_bits, _check, _batch = kbase._syn, kbase._terms, kbase._same_bits, kbase._check, kbase._batch
_cluster_of, _cstats, _n, _raises = cbase._cluster_of, cbase._cstats, cbase._n, cbase._raises
KEYS_KERNELS = kbase.KERNELS


def _per_key(target, kh, q, texts, topk, cap, pool, limit, within=None):
    return target.search_per_key(np.ascontiguousarray(q, np.float32), _terms(texts), _syn().NOW_TICKS, topk, kh, max_per_key=cap, pool=pool,
                                 within=within, candidate_limit=limit)


def _equal(got, want):
    return all(np.array_equal(got[i], want[i]) for i in (0, 2, 3, 4)) and _same_bits(got[1], want[1])


_K1 = {}


def _k1():
    """(test_gpu_per_key's shard K1 -- twin index, model, keys, queries --, the cluster over the same rows, its keys, its edges)"""
    s = kbase._shard("K1")
    if not _K1:
        m = s["model"]
        cl = _cluster_of(m.emb, m.created, m.rowbytes, m.ids, CUTS["K1"])
        _K1["v"] = (cl, cl.keys(m.ids, m.keys), (0,) + CUTS["K1"] + (s["n"],))
    return (s,) + _K1["v"]


def _shard_of(edges, positions):
    return np.searchsorted(np.asarray(edges[1:]), np.asarray(positions), side="right")


def _pos(ids):
    return (np.asarray(ids, np.int64) - 11) // 3            # (K1's and K3's ids are 3 r + 11)


def _scope_cases(s, cl, edges):
    """name -> (the cluster's scope, the twin's, its ids)"""
    model, idx, n = s["model"], s["idx"], s["n"]
    hi, lo = int(model.created[100]), int(model.created[1_500])      # candidate order is newest first: rows ~100 .. 1,500, across the first border
    tick_ids = model.ids[(model.created >= lo) & (model.created < hi) & ~model.dead]
    word = _syn().vocab_word(17)
    rng = np.random.default_rng(17)
    one = model.ids[edges[1] + np.sort(rng.choice(edges[2] - edges[1], 600, replace=False))]
    tiny = model.ids[[3, 4, 5, n - 300, n - 299, n - 1]]
    none = np.zeros(0, np.int64)
    return {"ticks": (lambda: cl.scope_ticks(lo, hi), lambda: idx.scope_ticks(lo, hi), tick_ids),
            "terms": (lambda: cl.scope_terms([word], "all"), lambda: idx.scope_terms([word], "all"), model.term_ids([word], "all")),
            "one shard": (lambda: cl.scope(one), lambda: idx.scope(one), one),
            "tiny": (lambda: cl.scope(tiny), lambda: idx.scope(tiny), tiny),
            "empty": (lambda: cl.scope(none), lambda: idx.scope(none), none)}


# ---- the placement -----------------------------------------------------------------------------------------------------------

def test_the_cuts_put_a_document_and_a_key_across_the_borders():
    s, cl, ckh, edges = _k1()
    model, n = s["model"], s["n"]
    assert cl.n_shards == 3 and cl.rows == n and [cl.shard(g).rows for g in range(3)] == [edges[g + 1] - edges[g] for g in range(3)]
    assert edges[1] < 300 < edges[2]                        # a candidate_limit of 300 ends inside the second shard
    second = np.nonzero(model.keys == 9_000_001)[0]         # the key that query 0 closes in round 2
    assert second[0] == 3_769 and second[-1] == 3_838 and set(_shard_of(edges, second).tolist()) == {1, 2}
    assert set(_shard_of(edges, np.nonzero(model.keys == 9_000_000)[0]).tolist()) == {1}
    assert set(_shard_of(edges, np.nonzero(model.keys == kbase.SPREAD_KEY)[0]).tolist()) == {0, 1}
    cases = _scope_cases(s, cl, edges)
    assert set(_shard_of(edges, _pos(cases["ticks"][2])).tolist()) == {0, 1}        # the ticks window crosses the first border
    assert set(_shard_of(edges, _pos(cases["one shard"][2])).tolist()) == {1}
    assert len(cases["tiny"][2]) < 10 and len(cases["terms"][2]) > 56


# ---- the keys themselves -----------------------------------------------------------------------------------------------------

def test_cluster_keys_set_get_and_rows_against_the_twins_handle():
    s, cl, ckh, edges = _k1()
    idx, model, n = s["idx"], s["model"], s["n"]
    live = ~model.dead
    assert np.array_equal(ckh.get(model.ids), s["kh"].get(model.ids)) and ckh.rows == s["kh"].rows == int((model.keys[live] != NONE).sum())
    assert [ckh.shard(g).rows for g in range(3)] == [int((model.keys[edges[g]:edges[g + 1]] != NONE).sum()) for g in range(3)]
    kh, tk = cl.keys(np.zeros(0, np.int64), np.zeros(0, np.int64)), idx.keys(np.zeros(0, np.int64), np.zeros(0, np.int64))
    try:
        assert kh.rows == 0 and (kh.get(model.ids[:50]) == NONE).all()
        unknown = np.array([1, 2, -5, 10 ** 12], np.int64)                          # ids are 3 r + 11: these name no row
        ids = np.concatenate([model.ids[[0, 210, 211, 3_803, 3_804, n - 1]], unknown])      # both sides of both borders
        vals = np.array([0, -1, kbase.I64_MAX, kbase.I64_MIN + 1, 42, 43, 5, 6, 7, 8], np.int64)
        (done, sts) = _cstats(cl, lambda: kh.set(ids, vals))
        assert done == 6 == tk.set(ids, vals) and [_n(st, "keys_scatter") for st in sts] == [1, 1, 1]      # the whole list goes to every shard
        probe = np.concatenate([ids, model.ids[[1, 2]]])
        assert np.array_equal(kh.get(probe), tk.get(probe)) and list(kh.get(probe)[:6]) == [0, -1, kbase.I64_MAX, kbase.I64_MIN + 1, 42, 43]
        assert kh.rows == 6 == tk.rows and [kh.shard(g).rows for g in range(3)] == [2, 2, 2]
        assert kh.set(model.ids[[3_804]], np.array([NONE], np.int64)) == 1 and kh.rows == 5           # an explicit ORR_KEY_NONE takes a key away
        assert kh.set(model.ids, model.keys) == n and np.array_equal(kh.get(model.ids), model.keys)
        assert kh.get(np.zeros(0, np.int64)).shape == (0,) and kh.set(np.zeros(0, np.int64), np.zeros(0, np.int64)) == 0
    finally:
        kh.close()
        tk.close()


def test_an_id_carried_by_rows_of_two_shards_counts_twice_and_reads_the_lower_shards_key():
    P, syn = pkg(), _syn()
    n_per, dim = 300, 16
    emb, created, rowbytes = tbase._rows(2 * n_per, dim)
    ids = np.arange(2 * n_per, dtype=np.int64) * 3 + 11
    ids[n_per + 7] = ids[5]                                  # one id on both shards
    cl = _cluster_of(emb, created, rowbytes, ids, (n_per,))
    try:
        kh = cl.keys(np.zeros(0, np.int64), np.zeros(0, np.int64))
        assert kh.set(ids[[5, 6]], np.array([70, 80], np.int64)) == 3       # id[5] names a live row on each shard
        assert kh.rows == 3 and [kh.shard(g).rows for g in range(2)] == [2, 1]
        assert list(kh.get(ids[[5, 6, n_per + 7]])) == [70, 80, 70]
        # the two rows of the id get different keys through the shards' own parts: get answers with the LOWER shard's
        assert kh.shard(1).set(ids[[5]], np.array([99], np.int64)) == 1
        assert list(kh.get(ids[[5]])) == [70] and list(kh.shard(1).get(ids[[5]])) == [99]
        assert kh.shard(0).set(ids[[5]], np.array([NONE], np.int64)) == 1   # the lower shard has none: the next one's
        assert list(kh.get(ids[[5]])) == [99]
        assert list(kh.get(np.array([-4, 7, 10 ** 15], np.int64))) == [NONE] * 3
        kh.close()
    finally:
        cl.close()


def test_cluster_scope_keys_is_the_twins_scope_keys():
    s, cl, ckh, edges = _k1()
    idx, model, kh, n = s["idx"], s["model"], s["kh"], s["n"]
    present = np.unique(model.keys[model.keys != NONE])
    many = np.concatenate([present[:100], np.arange(5_000_000, 5_004_900)])
    last_key = int(model.keys[n - 1])
    cases = {"none": [], "one": [last_key], "one absent": [123_456_789], "across a border": [9_000_001], "spread": [kbase.SPREAD_KEY, kbase.SPREAD_KEY],
             "no key": [NONE], "extremes": [0, -1, kbase.I64_MAX, kbase.I64_MIN + 1, NONE], "5000": many.tolist()}
    for what, listed in cases.items():
        listed = np.asarray(listed, np.int64)
        (sc, sts), tsc = _cstats(cl, lambda: cl.scope_keys(ckh, listed)), idx.scope_keys(kh, listed)
        try:
            assert sc.rows == tsc.rows == int((np.isin(model.keys, listed) & ~model.dead).sum()), what
            assert np.array_equal(sc.row_ids(), tsc.row_ids()), what
            assert [_n(st, "keys_member") for st in sts] == [1 if len(listed) else 0] * 3, what
        finally:
            sc.close()
            tsc.close()
    sc, tsc = cl.scope_keys(ckh, [9_000_001, 9_100_002, kbase.SPREAD_KEY]), idx.scope_keys(kh, [9_000_001, 9_100_002, kbase.SPREAD_KEY])
    try:
        qis, q, texts = _batch(s, 4)                         # an ordinary cluster scope from then on
        a = cl.search_in_scope(q, _terms(texts), _syn().NOW_TICKS, 10, sc, candidate_limit=n)
        assert tbase._equal(a, tbase._in_scope(idx, q, texts, 10, n, tsc)) and sc.rows == 70 + 12 + 5
    finally:
        sc.close()
        tsc.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------

def _cases(n):
    out, i = [], 0
    for topk in (1, 10, 56):
        for cap in (1, 2, 56):
            for pool in sorted({max(1, topk), 16, 56}):
                if pool < max(1, topk):
                    continue
                out.append((topk, cap, pool, (300, n)[i % 2]))
                i += 1
    return out


@pytest.mark.parametrize("within", [None, "ticks", "terms", "one shard", "tiny", "empty"])
@pytest.mark.parametrize("B", [1, 8, 70, 130])
def test_rows_score_bits_keys_counts_and_rounds_are_one_indexs(B, within):
    s, cl, ckh, edges = _k1()
    idx, kh, n = s["idx"], s["kh"], s["n"]
    qis, q, texts = _batch(s, B)
    make, make_twin, scope_ids = _scope_cases(s, cl, edges)[within] if within else (None, None, None)
    sc, tsc = (make(), make_twin()) if make else (None, None)
    multi = 0
    try:
        for topk, cap, pool, limit in _cases(n):
            what = (B, within, topk, cap, pool, limit)
            got = _per_key(cl, ckh, q, texts, topk, cap, pool, limit, within=sc)
            want = _per_key(idx, kh, q, texts, topk, cap, pool, limit, within=tsc)
            assert _equal(got, want), what
            _check(got, s, qis, topk, cap, pool, limit, scope_ids=scope_ids, what=what)
            multi += int((got[4] > 1).sum())
            if within == "tiny":
                assert (got[3] <= 6).all() and (got[4] == 1).all()
            if within == "empty":
                assert (got[3] == 0).all() and (got[0] == -1).all() and (got[2] == NONE).all()
    finally:
        if sc:
            sc.close()
            tsc.close()
    if within not in ("tiny", "empty"):
        assert multi > 0, (B, within)                       # the rounds beyond the first did run


def test_the_planted_query_needs_exactly_six_rounds_as_on_the_twin():
    s, cl, ckh, edges = _k1()
    idx, kh, n = s["idx"], s["kh"], s["n"]
    got = _per_key(cl, ckh, s["q"][:2], s["texts"][:2], 10, 1, 16, n)
    assert _equal(got, _per_key(idx, kh, s["q"][:2], s["texts"][:2], 10, 1, 16, n))
    _check(got, s, [0, 1], 10, 1, 16, n, what="planted")
    assert int(got[4][0]) == 6 and int(got[3][0]) == 10 and list(got[2][0, :5]) == [9_000_000 + d for d in range(5)]
    assert _shard_of(edges, _pos(got[0][0, :2])).tolist() == [1, 1]      # the second document's best row lies in front of the border ...
    assert list(got[2][1, :4]) == [9_100_000 + d for d in range(4)] and int(got[4][1]) == 3
    got = _per_key(cl, ckh, s["q"][:2], s["texts"][:2], 10, 2, 16, n)
    _check(got, s, [0, 1], 10, 2, 16, n, what="planted, two per key")
    assert list(got[2][0]) == [9_000_000 + d for d in range(5) for _ in range(2)]


def test_the_rows_on_both_sides_of_every_border_report_their_own_keys():
    """every row a key of its own (its position): a member gathered from the wrong shard, or at the wrong position, shows in out_keys"""
    s, cl, ckh, edges = _k1()
    idx, model, n = s["idx"], s["model"], s["n"]
    own = np.arange(n, dtype=np.int64) + 1_000
    kh, tk = cl.keys(model.ids, own), idx.keys(model.ids, own)
    try:
        at = [edges[1] - 1, edges[1], edges[2] - 1, edges[2], 0, n - 1]
        rng = np.random.default_rng(23)
        q = np.ascontiguousarray(model.emb[at] + np.float32(0.01) * rng.standard_normal((len(at), s["dim"])).astype(np.float32))
        (got, sts) = _cstats(cl, lambda: _per_key(cl, kh, q, [""] * len(at), 10, 1, 16, n))
        assert _equal(got, _per_key(idx, tk, q, [""] * len(at), 10, 1, 16, n))
        for b, r in enumerate(at):
            assert got[0][b, 0] == model.ids[r] and got[2][b, 0] == own[r], (b, r, got[0][b, :3], got[2][b, :3])       # the row itself ranks first
        assert np.array_equal(got[2], _pos(got[0]) + 1_000) and (got[4] == 1).all()
        assert [_n(st, "keys_gather") for st in sts] == [1, 1, 1]
    finally:
        kh.close()
        tk.close()


def test_the_nan_query_a_foreign_dimension_dim_zero_and_an_empty_batch():
    P = pkg()
    s, cl, ckh, edges = _k1()
    idx, kh, n = s["idx"], s["kh"], s["n"]
    got = _per_key(cl, ckh, s["q"][6:7], s["texts"][6:7], 10, 1, 16, n)  # the NaN coordinate
    assert _equal(got, _per_key(idx, kh, s["q"][6:7], s["texts"][6:7], 10, 1, 16, n))
    _check(got, s, [6], 10, 1, 16, n, what="nan")
    rng = np.random.default_rng(3)
    qf = rng.standard_normal((3, 64)).astype(np.float32)                 # a foreign dim: every cosine is 0, keyword and recency only
    texts = [s["texts"][20], s["texts"][21], ""]
    got = _per_key(cl, ckh, qf, texts, 10, 1, 16, n)
    assert _equal(got, _per_key(idx, kh, qf, texts, 10, 1, 16, n))
    for b in range(3):
        _check(tuple(x[b:b + 1] for x in got), s, [b], 10, 1, 16, n, qvec=qf[b], text=texts[b], tag=("foreign", b), what=("foreign", b))
    got = cl.search_per_key(None, _terms(texts), _syn().NOW_TICKS, 10, ckh, max_per_key=2, pool=24, candidate_limit=n)      # dim 0
    assert _equal(got, idx.search_per_key(None, _terms(texts), _syn().NOW_TICKS, 10, kh, max_per_key=2, pool=24, candidate_limit=n))
    assert (got[4] > 1).any()                               # recency alone ranks whole documents on top: more than one round
    h = P.native.hip
    qoff = np.zeros(1, np.uint32)
    out = np.full(4, 7, np.int64)
    o = out.ctypes.data
    assert h.orr_cluster_search_batch_per_key(cl._h, 0, 70, None, None, None, qoff.ctypes.data, 0, 4, 300, None, ckh._h, 1, 24, o, o, o, o, o) == 0
    assert (out == 7).all()
    B, k = 2, 10                                            # out_rounds may be NULL
    q = np.ascontiguousarray(s["q"][:B])
    tpool, toff, qoff = P.pack_terms(_terms(s["texts"][:B]))
    rows, scores, keys, counts = np.zeros((B, k), np.int64), np.zeros((B, k)), np.zeros((B, k), np.int64), np.zeros(B, np.int32)
    assert h.orr_cluster_search_batch_per_key(cl._h, B, 70, q.ctypes.data, tpool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, _syn().NOW_TICKS, k, n,
                                              None, ckh._h, 1, 16, rows.ctypes.data, scores.ctypes.data, keys.ctypes.data, counts.ctypes.data, None) == 0
    _check((rows, scores, keys, counts, _per_key(cl, ckh, q, s["texts"][:B], k, 1, 16, n)[4]), s, [0, 1], k, 1, 16, n, what="no out_rounds")


# ---- launch counts -----------------------------------------------------------------------------------------------------------

def test_a_batch_that_ends_in_round_one_gathers_once_where_a_member_lies_and_launches_no_other_keys_kernel():
    s, cl, ckh, edges = _k1()
    n = s["n"]
    for qis, limit in (([0, 1], n), ([7, 8, 9, 10], 300), ([2], 150)):
        q, texts = s["q"][qis], [s["texts"][i] for i in qis]
        cl.search(q, _terms(texts), _syn().NOW_TICKS, 16, candidate_limit=limit)           # (what a lane adapts to a batch has settled)
        plain, st_plain = _cstats(cl, lambda: cl.search(q, _terms(texts), _syn().NOW_TICKS, 16, candidate_limit=limit))
        got, sts = _cstats(cl, lambda: _per_key(cl, ckh, q, texts, 16, 16, 16, limit))      # max_per_key >= take = pool: the pool itself comes back
        assert (got[4] == 1).all() and np.array_equal(got[0], plain[0]) and _same_bits(got[1], plain[1]) and np.array_equal(got[3], plain[2])
        holds = set(_shard_of(edges, _pos(got[0][got[0] >= 0])).tolist())
        if limit == 150:
            assert holds == {0}                             # the whole candidate set lies on the first shard
        for g, st in enumerate(sts):
            assert _n(st, "keys_gather") == (1 if g in holds else 0), (qis, g, holds)
            assert not any(name in st for name in KEYS_KERNELS if name != "keys_gather"), (qis, g, sorted(st))
            assert not any(name in st for name in ("scope_counts", "mask_clip_slots", "mask_clip", "scope_fill_range")), (qis, g, sorted(st))
            mine = {name: v["launches"] for name, v in st.items() if not name.startswith("keys_")}
            assert mine == {name: v["launches"] for name, v in st_plain[g].items()}, (qis, g)


def _round_ranks(keys, take, cap, pool):
    """the ranks each round sees, by the round rule (test_gpu_per_key._walk_rounds with its rounds kept)"""
    kept, count, closed, seen, out = 0, {}, set(), set(), []
    finished = False
    while not finished:
        rnd = [r for r, k in enumerate(keys) if r not in seen and not (int(k) != NONE and int(k) in closed)][:pool]
        for r in rnd:
            k = int(keys[r])
            if k != NONE:
                if k in closed:
                    continue
                count[k] = count.get(k, 0) + 1
                if count[k] >= cap:
                    closed.add(k)
            kept += 1
            if kept >= take:
                finished = True
                break
        seen.update(rnd)
        out.append(rnd)
        finished = finished or len(rnd) < pool
    return out


def test_a_later_round_launches_once_per_slice_on_every_shard_and_clears_seen_rows_only_where_they_lie():
    s, cl, ckh, edges = _k1()
    n = s["n"]
    # query 0 alone: six rounds over documents that lie on shards 1 and 2; shard 0 holds none of their rows
    ids, _, keys, _ = kbase._ranking(s, 0, n)
    rounds = _round_ranks(keys, 10, 1, 16)
    assert len(rounds) == 6
    where = [set(_shard_of(edges, _pos(ids[r])).tolist()) for r in rounds]
    got, sts = _cstats(cl, lambda: _per_key(cl, ckh, s["q"][:1], s["texts"][:1], 10, 1, 16, n))
    assert int(got[4][0]) == 6
    for g, st in enumerate(sts):
        assert _n(st, "keys_exclude") == 5 and _n(st, "scope_counts") == 5 and _n(st, "mask_clip_slots") == 5, (g, sorted(st))      # a key closes cluster-wide
        seen_here = [any(g in where[j] for j in range(r)) for r in range(1, 6)]       # round r + 1 has seen the rows of rounds 1 .. r
        assert _n(st, "keys_clear_seen") == sum(seen_here), (g, seen_here, st.get("keys_clear_seen"))
        assert _n(st, "keys_gather") == sum(1 for w in where if g in w), (g, where)
        assert _n(st, "scope_fill_range") >= 1              # the frozen set is built on every shard
    assert all(0 not in w for w in where[:5]) and _n(sts[0], "keys_clear_seen") == 0 and _n(sts[1], "keys_clear_seen") == 5
    assert 2 not in where[0] and 1 <= _n(sts[2], "keys_clear_seen") <= 4     # round 2 has seen rows of shard 1 only
    # 130 queries: per round beyond the first one launch per slice of 64 unfinished queries, on every shard
    qis, q, texts = _batch(s, 130)
    cl.search_stats(reset=True)
    got, sts = _cstats(cl, lambda: _per_key(cl, ckh, q, texts, 10, 1, 16, n))
    stats = cl.search_stats()
    r = got[4]
    slices = sum(-(-int((r >= k).sum()) // 64) for k in range(2, int(r.max()) + 1))
    assert slices >= 3 and all(_n(st, "keys_exclude") == slices and _n(st, "mask_clip_slots") == slices and _n(st, "scope_counts") == slices for st in sts)
    assert all(_n(st, "keys_clear_seen") <= slices for st in sts)
    # the cluster's statistics: one search of B queries for round 1, one of S queries per slice and round after that
    assert stats["searches"] == 1 + slices and stats["queries"] == 130 + sum(int((r >= k).sum()) for k in range(2, int(r.max()) + 1)), stats


# ---- the grouped screen ------------------------------------------------------------------------------------------------------

def test_seventy_queries_through_the_grouped_screen_of_two_large_shards():
    """tests/test_gpu_cluster_scope.py's 2 x 200,000 x 128 cluster and its twin (only read); keys in runs of 40, and planted
    documents: the best 16 rows of each of queries 0 .. 7 share one key, so with pool 16 they need a second round, and query 0's
    next 16 rows share another, so it needs a third"""
    cl, one, model, texts, fam, plants, _, _ = sbase._big()
    q = np.ascontiguousarray(plants["random 10 %"][0], np.float32)
    n = sbase.N
    qis = [b % sbase.POOL_Q for b in range(70)]
    qq, tt = q[qis], [texts[i] for i in qis]
    keys = np.arange(n, dtype=np.int64) // 40
    top = one.search(q[:8], _terms(texts[:8]), _syn().NOW_TICKS, 32, candidate_limit=n)[0]
    assert (top >= 0).all()                                 # (a row two queries share gets one of their keys; query 0's are set last)
    for b in range(7, -1, -1):
        keys[_pos(top[b, :16])] = 50_000_000 + 2 * b
    keys[_pos(top[0, 16:])] = 50_000_001
    keys[_pos(top[0, :16])] = 50_000_000
    ckh, tkh = cl.keys(model.ids, keys), one.keys(model.ids, keys)
    try:
        assert ckh.rows == n == tkh.rows
        cl.search_stats(reset=True)
        got = _per_key(cl, ckh, qq, tt, 10, 1, 16, n)
        stats = cl.search_stats()
        want = _per_key(one, tkh, qq, tt, 10, 1, 16, n)
        assert _equal(got, want)
        assert int(got[4][0]) >= 3 and list(got[2][0, :2]) == [50_000_000, 50_000_001] and (got[3] == 10).all()
        assert (got[4] > 1).sum() >= 16 and stats["searches"] == 3       # sixteen unfinished queries shared round 2, two shared round 3
        # a call whose last search is round 2's grouped cluster search over 14 temporary scopes: the grouped screen ran
        sub = [b for b in range(70) if 1 <= b % sbase.POOL_Q <= 7]
        cl.search_stats(reset=True)
        again = _per_key(cl, ckh, qq[sub], [tt[b] for b in sub], 10, 1, 16, n)
        assert all(np.array_equal(again[i], got[i][sub]) for i in (0, 2, 3, 4)) and _same_bits(again[1], got[1][sub]) and (again[4] == 2).all()
        stats = cl.search_stats()
        assert stats["searches"] == 2 and stats["pass_mode"] == 6, stats
        sc, tsc = cl.scope(model.ids[fam["older half of each shard"]]), one.scope(model.ids[fam["older half of each shard"]])
        try:
            got = _per_key(cl, ckh, qq[:9], tt[:9], 10, 2, 24, 150_000, within=sc)      # the limit ends inside the second shard's part
            assert _equal(got, _per_key(one, tkh, qq[:9], tt[:9], 10, 2, 24, 150_000, within=tsc))
        finally:
            sc.close()
            tsc.close()
    finally:
        ckh.close()
        tkh.close()


# ---- maintenance -------------------------------------------------------------------------------------------------------------

def test_maintenance_on_the_shards_carries_the_cluster_keys():
    n, dim = kbase.SHAPES["K3"]
    s = kbase._build_shard("K3", capacity=n + 1_000)         # a twin of its own, rebuilt here from the same rows
    twin, model, tkh = s["idx"], s["model"], s["kh"]
    cl = _cluster_of(model.emb, model.created, model.rowbytes, model.ids, CUTS["K3"], capacity=n + 1_000)
    edges = (0,) + CUTS["K3"] + (n,)
    ckh = cl.keys(model.ids, model.keys)
    qis, q, texts = _batch(s, 8)
    all_ids = [model.ids.copy()]

    def check(what):
        ids = np.concatenate(all_ids)
        assert np.array_equal(ckh.get(ids), tkh.get(ids)) and ckh.rows == tkh.rows, what
        total = cl.rows
        assert total == twin.rows
        for topk, cap, pool, limit in ((10, 1, 16, total), (10, 2, 24, total), (10, 1, 16, 30_000)):
            got = _per_key(cl, ckh, q, texts, topk, cap, pool, limit)
            assert _equal(got, _per_key(twin, tkh, q, texts, topk, cap, pool, limit)), (what, topk, cap, pool, limit)
        return got

    try:
        assert int(check("fresh")[4][0]) >= 1
        got = _per_key(cl, ckh, q, texts, 10, 1, 16, n)
        assert int(got[4][0]) >= 3
        # 1. deletes on two shards: the first document of target A (shard 2) and 3,000 rows of shard 0
        rng = np.random.default_rng(4)
        gone0 = model.ids[np.sort(rng.choice(edges[1], 3_000, replace=False))]
        gone2 = model.ids[n - 400:n - 330]
        assert cl.shard(0).delete_rows(gone0) == 3_000 and cl.shard(2).delete_rows(gone2) == 70
        assert twin.delete_rows(np.concatenate([gone0, gone2])) == 3_070
        assert (ckh.get(gone2[:10]) == NONE).all()
        got = check("deleted")
        assert 9_000_000 not in got[2][0]
        # 2. update: the rows move nowhere, the keys stay
        far, new = model.ids[[n - 5]], model.emb[n - 100][None, :].copy()
        assert cl.shard(2).update_rows(far, new) == 1 and twin.update_rows(far, new) == 1
        check("updated")
        # 3. compaction: every base behind shard 0 moves
        assert cl.compact() == 3_070 == twin.compact()
        check("compacted")
        # 4. two insertions that move the row bases; the new rows read ORR_KEY_NONE until the host sets them
        width = model.rowbytes.shape[1]
        for shard, m, first_id, key in ((1, 131, 10_000_000, 8_000_000), (0, 17, 20_000_000, 8_000_001)):
            at = sum(cl.shard(g).rows for g in range(shard))
            created = twin_created(model, gone0, gone2)[at]    # as new as the shard's newest row
            c2 = np.full(m, created, np.int64)
            e2 = np.random.default_rng(5 + shard).standard_normal((m, dim)).astype(np.float32)
            e2[:20 if m > 20 else 5] = kbase._copies(np.random.default_rng(6), s["q"][0], 0.01, 20 if m > 20 else 5)       # nearer to v than every planted document
            b2 = model.rowbytes[:m]
            ids2 = np.arange(m, dtype=np.int64) + first_id
            off2 = np.arange(m + 1, dtype=np.int64) * width
            assert cl.insert_rows(shard, e2, c2, b2.reshape(-1), off2, row_ids=ids2) == m
            twin.insert_rows(e2, c2, b2.reshape(-1), off2, row_ids=ids2)
            all_ids.append(ids2)
            assert (ckh.get(ids2) == NONE).all()
            got = check(("inserted", shard))
            assert (got[2][0] == NONE).sum() >= 5           # rows without a key: no cap applies to them
            assert ckh.set(ids2, np.full(m, key, np.int64)) == m == tkh.set(ids2, np.full(m, key, np.int64))
            got = check(("inserted and set", shard))
            assert list(got[2][0]).count(key) == 1
        one = cl.scope_keys(ckh, [8_000_000, 8_000_001])
        assert one.rows == 131 + 17
        one.close()
    finally:
        ckh.close()
        cl.close()
        tkh.close()
        twin.close()


def twin_created(model, *gone):
    """the created ticks of the rows that are left, in candidate order"""
    keep = ~np.isin(model.ids, np.concatenate(gone))
    return model.created[keep]


# ---- refusals, threads, destroy orders ---------------------------------------------------------------------------------------

def test_refusals_foreign_and_orphaned_handles_device_queries_and_both_destroy_orders():
    import torch
    P = pkg()
    N = P.native
    q, terms = np.ones((2, 64), np.float32), [[b"abc"], []]
    cl, ids = cbase._tiny(seal=False)
    _raises(N.ORR_ESTATE, lambda: cl.keys(ids, ids // 7), "not sealed")
    cl.seal()
    other, _ = cbase._tiny()
    mine, theirs = cl.keys(ids, ids // 7), other.keys(ids, ids // 7)
    my_scope, their_scope = cl.scope(ids[:100]), other.scope(ids[:100])
    assert cl.search_per_key(q, terms, 0, 4, mine, pool=24, within=my_scope)[3].tolist() == [4, 4]
    _raises(N.ORR_EINVAL, lambda: cl.search_per_key(q, terms, 0, 4, mine, pool=3), "exceeds the pool")         # the arguments come first
    _raises(N.ORR_EINVAL, lambda: cl.search_per_key(q, terms, 0, 4, theirs, pool=24), "keys belong to another cluster")
    _raises(N.ORR_EINVAL, lambda: cl.search_per_key(q, terms, 0, 4, mine, pool=24, within=their_scope), "scope belongs to another cluster")
    _raises(N.ORR_EINVAL, lambda: cl.scope_keys(theirs, [1]), "another cluster")
    dq = torch.from_numpy(q).cuda()
    pool, toff, qoff = P.pack_terms(terms)
    rows, scores, keys, counts = np.full((2, 4), 7, np.int64), np.full((2, 4), 7.0), np.full((2, 4), 7, np.int64), np.full(2, 7, np.int32)
    for within in (None, my_scope._h):
        r = N.hip.orr_cluster_search_batch_per_key(cl._h, 2, 64, dq.data_ptr(), pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, 0, 4, 300, within,
                                                   mine._h, 1, 24, rows.ctypes.data, scores.ctypes.data, keys.ctypes.data, counts.ctypes.data, None)
        assert r == N.ORR_EINVAL and b"host memory" in N.hip.orr_last_error()
    assert (rows == 7).all() and (scores == 7.0).all() and (keys == 7).all() and (counts == 7).all()
    dk = torch.from_numpy(ids[:4].copy()).cuda()
    done = np.zeros(1, np.int64)
    assert N.hip.orr_cluster_keys_set(mine._h, 4, dk.data_ptr(), dk.data_ptr(), done.ctypes.data) == N.ORR_EINVAL and b"host memory" in N.hip.orr_last_error()
    # the cluster first: its keys and scopes are orphaned; then the handles
    other.close()
    assert theirs.rows == -1
    _raises(N.ORR_ESTATE, lambda: cl.search_per_key(q, terms, 0, 4, theirs, pool=24), "orphaned")
    _raises(N.ORR_ESTATE, lambda: cl.search_per_key(q, terms, 0, 4, mine, pool=24, within=their_scope), "orphaned")
    _raises(N.ORR_ESTATE, lambda: theirs.set(ids[:3], ids[:3]), "orphaned")
    _raises(N.ORR_ESTATE, lambda: theirs.get(ids[:3]), "orphaned")
    theirs.close()
    their_scope.close()
    # the handles first: the cluster goes on working
    mine.close()
    my_scope.close()
    again = cl.keys(ids, ids // 7)
    assert cl.search_per_key(q, terms, 0, 4, again, pool=24)[3].tolist() == [4, 4] and again.rows == len(ids)
    cl.close()
    assert again.rows == -1
    again.close()


def test_six_threads_on_three_shards_each_get_the_single_thread_answer():
    s, cl, ckh, edges = _k1()
    n = s["n"]
    qis, q, texts = _batch(s, 16)
    cases = [(10, 1, 16, n), (10, 2, 24, n), (10, 1, 16, 300), (56, 1, 56, n), (1, 1, 16, n), (10, 1, 24, n)]
    sc = cl.scope_ticks(*[int(s["model"].created[i]) for i in (1_500, 100)])
    alone = [_per_key(cl, ckh, q, texts, *c, within=sc if i % 2 else None) for i, c in enumerate(cases)]
    results, errors = [None] * 6, []

    def work(i):
        try:
            for _ in range(2):
                results[i] = _per_key(cl, ckh, q, texts, *cases[i], within=sc if i % 2 else None)
        except Exception as e:                              # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(6)]      # more threads than lanes
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    try:
        assert not any(t.is_alive() for t in threads), "a search did not come back: the lanes or the holds deadlocked"
        assert not errors, errors
        for i in range(6):
            assert _equal(results[i], alone[i]), cases[i]
    finally:
        sc.close()
