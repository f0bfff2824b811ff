"""The routed search (orr_search_batch_routed): the top `route` documents of a document index, then the best chunks inside them.

The expected answer is ALWAYS the twin the header states, composed per query through bindings that exist without the feature
(_twin_one): docs.search at topk = route over every row of docs gives D_b; idx.scope_keys(keys, D_b without ORR_KEY_NONE),
.and_(within) where a scope is given; idx.search_in_scope.  It is never a second call of the routed function.  Every check is
exact equality of rows, order, fp64 score BITS, counts, route keys and route counts (_check).  Where the whole routed scope is
returned (topk = every row) the row set is also compared with the model's own membership: every bit of keys_include's bitmaps.

Shards are tests/test_gpu_per_key.py's (built once per process, only read): R1 = K1 4,099 x 70 (n_rows no multiple of 64, two
workgroups of keys_include and a tail, the small-scope paths), R2 = K2 200,000 x 128 with two_stage 1 and the shadow warmed (the
grouped screening pass), and a fresh K3 70,001 x 64 for maintenance.  Keys are that file's: runs of 1 .. 40 rows, a key spread
over distant rows, the keys 0, -1, INT64_MAX and INT64_MIN + 1, rows at ORR_KEY_NONE; R1 gets a key column of its own with a key
that straddles row 2,048 and a key on the last three rows (the last, partial bitmap word)."""
import threading

import numpy as np
import pytest

import test_gpu_per_key as kbase
import test_gpu_scope_terms as tbase
from helpers import pkg

pytestmark = pytest.mark.gpu

NONE = kbase.NONE
STRADDLE, TAIL = 5_555_555, 6_666_666
_syn, _stats, _terms, _same_bits = tbase._syn, tbase._stats, tbase._terms, kbase._same_bits
_R = {}


def _r1():
    """R1 with its own key column (straddle and tail keys), the document index, and three planted cosine-only queries"""
    if "R1" not in _R:
        s = dict(kbase._shard("K1"))
        n, model = s["n"], s["model"]
        keys = model.keys.copy()
        keys[2_040:2_056] = STRADDLE
        keys[n - 3:] = TAIL
        s["keys"] = keys
        s["kh"] = s["idx"].keys(s["ids"], keys)
        s["docs"] = s["kh"].centroid_index()
        q = s["q"].copy()
        for b, k in ((2, STRADDLE), (3, kbase.SPREAD_KEY), (4, TAIL)):
            q[b] = model.emb[keys == k].astype(np.float64).mean(axis=0).astype(np.float32)
        s["q"], s["cache"] = q, {}
        _R["R1"] = s
    return _R["R1"]


def _r2():
    if "R2" not in _R:
        s = dict(kbase._shard("K2"))
        s["keys"] = s["model"].keys
        s["docs"] = s["kh"].centroid_index()
        rng = np.random.default_rng(77)
        # 130 queries: the shard's 24, then cosine-only ones near rows of 106 further documents
        first = np.flatnonzero((s["keys"][1:] != s["keys"][:-1]) & (s["keys"][1:] != NONE))[::60][:106] + 1
        assert len(first) == 106
        extra = s["model"].emb[first] + np.float32(0.2) * rng.standard_normal((106, s["dim"])).astype(np.float32)
        s["q"] = np.ascontiguousarray(np.concatenate([s["q"], extra]), np.float32)
        s["texts"] = list(s["texts"]) + [""] * 106
        s["cache"] = {}
        # A second, host-built document index whose routes are spread over the whole shard and disjoint between queries (the
        # centroid index's routes are not: recency is part of the score, so every query's route leans to the young end of the
        # shard and the routes overlap): one row per key, all of one age, document j near the unit vector e_(j mod 64); query
        # b = e_b then routes to documents of class b only.
        P = pkg()
        uniq = np.unique(s["keys"][s["keys"] != NONE])
        emb = np.float32(0.3) * rng.standard_normal((len(uniq), s["dim"])).astype(np.float32) / np.float32(np.sqrt(s["dim"]))
        emb[np.arange(len(uniq)), np.arange(len(uniq)) % 64] += np.float32(1.0)
        flat = P.RecallIndex(dim=s["dim"], capacity_rows=len(uniq))
        flat.append(emb, np.full(len(uniq), int(s["model"].created.max()), np.int64), np.zeros(0, np.uint8), np.zeros(len(uniq) + 1, np.int64),
                    row_ids=uniq)
        flat.seal()
        s["flat"], s["q_flat"] = flat, np.eye(64, s["dim"], dtype=np.float32)
        _R["R2"] = s
    return _R["R2"]


def _routed(idx, docs, kh, q, texts, topk, route, limit, within=None):
    return idx.search_routed(docs, kh, None if q is None else np.ascontiguousarray(q, np.float32), _terms(texts), _syn().NOW_TICKS, topk, route,
                             within=within, candidate_limit=limit)


def _twin_one(idx, docs, kh, qv, text, topk, route, limit, within=None):
    """the header's three steps for ONE query, through calls that exist without the feature"""
    q1, t1, now = (None if qv is None else np.ascontiguousarray(qv[None, :], np.float32)), _terms([text]), _syn().NOW_TICKS
    r = docs.search(q1, t1, now, route, candidate_limit=max(1, docs.rows))
    n = int(r[2][0])
    D = r[0][0, :n].copy()
    sc = idx.scope_keys(kh, D[D != NONE])
    try:
        if within is not None:
            sc.and_(within)
        got = idx.search_in_scope(q1, t1, now, topk, sc, candidate_limit=limit)
    finally:
        sc.close()
    route_keys = np.full(route, NONE, np.int64)
    route_keys[:n] = D
    return got[0][0], got[1][0], int(got[2][0]), route_keys, n


def _check(got, s, q, texts, topk, route, limit, within=None, tag=None, docs=None, kh=None, what=None):
    rows, scores, counts, rkeys, rn = got
    B, k = len(texts), max(1, topk)
    assert rows.shape == scores.shape == (B, k) and counts.shape == rn.shape == (B,) and rkeys.shape == (B, route)
    docs, kh = docs or s["docs"], kh or s["kh"]
    for b in range(B):
        qv = None if q is None else q[b]
        key = (tag, id(docs), id(kh), None if qv is None else qv.tobytes(), texts[b], topk, route, limit)
        if tag is None or key not in s["cache"]:
            s["cache"][key] = _twin_one(s["idx"], docs, kh, qv, texts[b], topk, route, limit, within)
        w_rows, w_scores, w_c, w_rk, w_rn = s["cache"][key]
        assert int(rn[b]) == w_rn and np.array_equal(rkeys[b], w_rk), (what, b, rkeys[b], w_rk)
        assert int(counts[b]) == w_c, (what, b, int(counts[b]), w_c)
        assert np.array_equal(rows[b], w_rows), (what, b, rows[b, :8], w_rows[:8])
        assert _same_bits(scores[b], w_scores), (what, b)
        assert (rows[b, w_c:] == -1).all() and (scores[b, w_c:] == 0.0).all() and (rkeys[b, w_rn:] == NONE).all(), (what, b)


# ---- 1: R1, every bit of the bitmaps ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 24])
@pytest.mark.parametrize("route", [1, 3, 40])
def test_r1_the_whole_routed_scope_comes_back_bit_for_bit(B, route):
    s = _r1()
    idx, n, keys, model = s["idx"], s["n"], s["keys"], s["model"]
    qis = [2] if B == 1 else list(range(24))             # 0 .. 5 cosine-only (2, 3, 4 planted), 6 holds a NaN, the rest hybrid
    q, texts = s["q"][qis], [s["texts"][i] for i in qis]
    got, st = _stats(idx, lambda: _routed(idx, s["docs"], s["kh"], q, texts, n, route, n))
    _check(got, s, q, texts, n, route, n, tag="r1", what=("r1", B, route))
    rows, _, counts, rkeys, rn = got
    for b in range(B):                                  # topk and the limit reach every row: the row SET is the routed scope
        D = rkeys[b, :rn[b]]
        want = model.ids[np.isin(keys, D[D != NONE]) & ~model.dead]
        assert int(counts[b]) == len(want) and np.array_equal(np.sort(rows[b, :counts[b]]), want), (b, counts[b], len(want))
    planted = {2: STRADDLE, 3: kbase.SPREAD_KEY, 4: TAIL}
    if route >= 3:                                      # the planted documents are routed to: a key across row 2,048 (two
        for b, qi in enumerate(qis):                    # workgroups), the spread key, rows in the last partial word
            if qi in planted:
                assert planted[qi] in rkeys[b], (qi, rkeys[b])
                assert set(model.ids[keys == planted[qi]]) <= set(rows[b, :counts[b]])
    assert st["keys_include"]["launches"] == 1 and "keys_member" not in st and "keys_exclude" not in st


# ---- 2 .. 4: R2 against the twin, launch counts, the grouped pass ----------------------------------------------------------------

def _scopes(s):
    if "scopes" not in s:
        cases = kbase._scope_cases(s)
        s["scopes"] = {"ticks": cases["ticks"][0](), "terms": cases["terms"][0](), "empty": s["idx"].scope(np.zeros(0, np.int64)), None: None}
    return s["scopes"]


R2_CASES = [(1, 1, 300, None), (1, 40, None, "ticks"), (24, 8, 300, "terms"), (24, 40, None, None), (24, 1, None, "empty"), (24, 8, None, "ticks"),
            (130, 8, None, None), (130, 40, 300, "ticks"), (130, 1, 300, None), (130, 8, 300, "terms"), (24, 40, 300, None), (130, 1, None, "empty")]


@pytest.mark.parametrize("B,route,limit,within", R2_CASES)
def test_r2_equals_the_twin_with_one_keys_include_per_slice_and_no_keys_member(B, route, limit, within):
    s = _r2()
    idx, n = s["idx"], s["n"]
    limit = n if limit is None else limit
    sc = _scopes(s)[within]
    q, texts = s["q"][:B], s["texts"][:B]
    idx.search_stats(reset=True)
    got, st = _stats(idx, lambda: _routed(idx, s["docs"], s["kh"], q, texts, 10, route, limit, within=sc))
    stats = idx.search_stats()
    _check(got, s, q, texts, 10, route, limit, within=sc, tag=("r2", within), what=(B, route, limit, within))
    rkeys, rn = got[3], got[4]
    sets = {tuple(sorted(set(rkeys[b, :rn[b]].tolist()) - {NONE})) for b in range(B)} - {()}
    if B == 130 and route > 1:
        assert len(sets) > 128                          # distinct routes: three slices
    slices = -(-len(sets) // 64) if within != "empty" else 0           # (an empty `within` ends the call before any launch)
    assert st.get("keys_include", {"launches": 0})["launches"] == slices, (st.get("keys_include"), len(sets))
    assert "keys_member" not in st and "keys_exclude" not in st
    if slices:
        assert st["mask_clip_slots"]["launches"] == slices
    assert stats["searches"] == 1 and stats["queries"] == B             # counted as one grouped call


def test_large_routes_spread_over_the_shard_share_the_grouped_screening_pass():
    s = _r2()
    idx, n = s["idx"], s["n"]
    q, texts = s["q_flat"][:24], [""] * 24
    idx.search_stats(reset=True)
    got, st = _stats(idx, lambda: _routed(idx, s["flat"], s["kh"], q, texts, 10, 40, n))
    stats = idx.search_stats()
    assert stats["pass_mode"] == 6, stats["pass_mode"]                  # 24 scopes of 40 documents each: ONE grouped screening pass
    assert st["keys_include"]["launches"] == 1 and (got[4] == 40).all()
    _check(got, s, q, texts, 10, 40, n, docs=s["flat"], tag=("flat", None), what="grouped pass")


def test_slot_dedupe_sixty_four_queries_of_four_vectors_share_four_slots():
    """How the number of groups is read from statistics the project already exposes: keys_include is timed with
    8 n_rows + 4 words S algorithmic bytes, S the slots of the slice -- so its algo_bytes minus the 8 n_rows of the key column
    are, for this call, 4 / 64 of those of a call with 64 distinct routes.  One temporary scope per slot is what the grouped pass
    receives as its groups."""
    s = _r2()
    idx, n = s["idx"], s["n"]
    q4, t4 = np.tile(s["q"][7:11], (16, 1)), s["texts"][7:11] * 16
    got, st = _stats(idx, lambda: _routed(idx, s["docs"], s["kh"], q4, t4, 10, 8, n))
    _check(got, s, q4, t4, 10, 8, n, tag=("r2", None), what="4 vectors x 16")
    q64, t64 = s["q"][24:88], s["texts"][24:88]
    got64, st64 = _stats(idx, lambda: _routed(idx, s["docs"], s["kh"], q64, t64, 10, 8, n))
    _check(got64, s, q64, t64, 10, 8, n, tag=("r2", None), what="64 distinct")
    assert len({tuple(sorted(got64[3][b])) for b in range(64)}) == 64
    assert st["keys_include"]["launches"] == 1 and st64["keys_include"]["launches"] == 1
    assert (st["keys_include"]["algo_bytes"] - 8.0 * n) * 16 == st64["keys_include"]["algo_bytes"] - 8.0 * n
    # 130 queries with 60 distinct routes: one slice, not three
    q130, t130 = np.concatenate([s["q"][24:84], s["q"][24:84], s["q"][24:34]]), [""] * 130
    got, st = _stats(idx, lambda: _routed(idx, s["docs"], s["kh"], q130, t130, 10, 8, n))
    _check(got, s, q130, t130, 10, 8, n, tag=("r2", None), what="130 queries, 60 routes")
    assert st["keys_include"]["launches"] == 1


def test_a_union_table_beyond_the_lds_cut_over_goes_through_global_memory():
    s = _r2()
    idx, n = s["idx"], s["n"]
    q, texts = s["q_flat"], [""] * 64                   # 64 disjoint routes of 40 documents
    got, st = _stats(idx, lambda: _routed(idx, s["flat"], s["kh"], q, texts, 10, 40, n))
    union = set(got[3].reshape(-1).tolist()) - {NONE}
    assert len(union) > 2_048, len(union)               # ONE slice whose table lies beyond per_key::kLdsTable
    assert st["keys_include"]["launches"] == 1
    _check(got, s, q, texts, 10, 40, n, docs=s["flat"], tag=("flat", None), what="global table")


# ---- 6: maintenance -----------------------------------------------------------------------------------------------------------------

def test_maintenance_with_the_document_index_kept_as_the_old_snapshot():
    n, dim = kbase.SHAPES["K3"]
    s = kbase._build_shard("K3", capacity=n + 1_000)
    idx, model, kh = s["idx"], s["model"], s["kh"]
    docs = kh.centroid_index()
    s["docs"] = docs
    q, texts = s["q"][:8], s["texts"][:8]

    def check(what):
        for route, limit in ((3, 300), (40, len(model.ids))):
            got = _routed(idx, docs, kh, q, texts, 10, route, limit)
            _check(got, s, q, texts, 10, route, limit, what=(what, route))
        return got

    try:
        got = check("fresh")
        routed = got[3][0, :got[4][0]]                   # query 0's documents: delete half of their rows, and 5,000 others
        rows_of = model.ids[np.isin(model.keys, routed[routed != NONE])]
        rng = np.random.default_rng(14)
        gone = np.unique(np.concatenate([rows_of[::2], model.ids[rng.choice(n - 500, 5_000, replace=False)]]))
        assert idx.delete_rows(gone) == len(gone)
        got = check("deleted")
        assert not set(got[0][0, :got[2][0]].tolist()) & set(gone.tolist())
        idx.compact()
        check("compacted")
        m = 131
        _, c2, b2 = tbase._rows(m, dim, row0=n, n_total=n + m)
        e2 = kbase._copies(np.random.default_rng(6), q[0], 0.01, m)
        ids2 = np.arange(m, dtype=np.int64) + 10_000_000
        idx.insert_rows(e2, c2, b2.reshape(-1), np.arange(m + 1, dtype=np.int64) * b2.shape[1], row_ids=ids2)
        got = check("inserted")                         # new rows have no key: no route reaches them
        assert not set(got[0].reshape(-1).tolist()) & set(ids2.tolist())
        first = int(got[3][0, 0])
        assert kh.set(ids2, np.full(m, first, np.int64)) == m
        got = check("inserted and set")                 # now they belong to query 0's first document, and are nearest
        assert set(got[0][0].tolist()) <= set(ids2.tolist())
    finally:
        docs.close()
        kh.close()
        idx.close()


# ---- 7: a host-built document index ---------------------------------------------------------------------------------------------

def test_a_host_built_docs_with_titles_a_view_docs_is_idx_and_a_document_without_a_key():
    P = pkg()
    s = _r1()
    idx, n, dim, keys, model = s["idx"], s["n"], s["dim"], s["keys"], s["model"]
    uniq = [int(k) for k in np.unique(keys) if k != NONE][:150]
    emb = np.stack([model.emb[keys == k].astype(np.float64).mean(axis=0).astype(np.float32) for k in uniq])
    first = [int(np.flatnonzero(keys == k)[0]) for k in uniq]
    emb = np.concatenate([emb, emb[:1]])                 # one more document whose id is ORR_KEY_NONE, a copy of document 0
    ids = np.array(uniq + [NONE], np.int64)
    first.append(first[0])
    titles = model.rowbytes[first]                       # a document's title: the content of its first chunk
    docs = P.RecallIndex(dim=dim, capacity_rows=len(ids))
    bare = P.RecallIndex(dim=dim, capacity_rows=len(ids))
    view = None
    try:
        off = np.arange(len(ids) + 1, dtype=np.int64) * titles.shape[1]
        docs.append(emb, model.created[first], titles.reshape(-1), off, row_ids=ids)
        docs.seal()
        bare.append(emb, model.created[first], np.zeros(0, np.uint8), np.zeros(len(ids) + 1, np.int64), row_ids=ids)
        bare.seal()
        q, texts = s["q"][7:19], s["texts"][7:19]        # hybrid queries
        q = np.concatenate([q, emb[:1]])                 # and document 0 itself: ORR_KEY_NONE ranks beside it
        texts = texts + [""]
        got = _routed(idx, docs, s["kh"], q, texts, 10, 5, n)
        _check(got, s, q, texts, 10, 5, n, docs=docs, what="titles")
        assert NONE in got[3][12, :got[4][12]].tolist()   # reported, and selects no row (the twin drops it)
        plain = _routed(idx, bare, s["kh"], q, texts, 10, 5, n)
        _check(plain, s, q, texts, 10, 5, n, docs=bare, what="no content")
        assert not np.array_equal(got[3][:12], plain[3][:12])           # the titles took part in the route
        view = docs.view()
        on_view = _routed(idx, view, s["kh"], q, texts, 10, 5, n)
        for a, b in zip(got, on_view):
            assert np.array_equal(a, b) or _same_bits(a, b)
        # docs is idx: the chunk rows rank themselves, each row a document of its own (a key column of the row ids)
        own = idx.keys(s["ids"], s["ids"])
        try:
            got = _routed(idx, idx, own, q[:12], texts[:12], 10, 7, n)
            _check(got, s, q[:12], texts[:12], 10, 7, n, docs=idx, kh=own, what="docs is idx")
            assert (got[2] == 7).all() and np.array_equal(np.sort(got[0][:, :7], axis=1), np.sort(got[3], axis=1))
        finally:
            own.close()
    finally:
        if view is not None:
            view.close()
        docs.close()
        bare.close()


# ---- 8: query kinds -----------------------------------------------------------------------------------------------------------------

def _raw(docs, idx, kh, B, q, texts, route, topk, limit, within=None, fill=7):
    """the C entry with outputs pre-filled: (code, rows, scores, counts, route_keys, route_n)"""
    P = pkg()
    k = max(1, topk)
    tpool, toff, qoff = P.pack_terms(_terms(texts))
    rows, scores, counts = np.full((max(B, 1), k), fill, np.int64), np.full((max(B, 1), k), float(fill)), np.full(max(B, 1), fill, np.int32)
    rk, rn = np.full((max(B, 1), max(route, 1)), fill, np.int64), np.full(max(B, 1), fill, np.int32)
    p = lambda a: a.ctypes.data if a is not None and a.size else None
    dim = 0 if q is None else q.shape[1]
    code = P.native.hip.orr_search_batch_routed(docs._h if docs is not None else None, idx._h, kh._h if kh is not None else None, B, dim, p(q),
                                                p(tpool), p(toff), qoff.ctypes.data, _syn().NOW_TICKS, route, topk, limit,
                                                within._h if within is not None else None, rows.ctypes.data, scores.ctypes.data,
                                                counts.ctypes.data, rk.ctypes.data, rn.ctypes.data)
    return code, rows, scores, counts, rk, rn


def _untouched(r, fill=7):
    return all((a == fill).all() for a in r[1:])


def test_query_kinds_dim_zero_a_foreign_dimension_an_empty_batch_and_an_empty_docs():
    P = pkg()
    s = _r1()
    idx, n, docs, kh = s["idx"], s["n"], s["docs"], s["kh"]
    texts = [s["texts"][20], s["texts"][21], ""]
    got = _routed(idx, docs, kh, None, texts, 10, 5, n)                     # dim 0: keyword and recency only, in both steps
    _check(got, s, None, texts, 10, 5, n, what="dim 0")
    assert (got[4] == 5).all() and (got[2] > 0).all()
    qf = np.random.default_rng(3).standard_normal((3, 64)).astype(np.float32)
    got = _routed(idx, docs, kh, qf, texts, 10, 5, n)                       # a foreign dimension: every cosine is 0
    _check(got, s, qf, texts, 10, 5, n, what="foreign dim")
    r = _raw(docs, idx, kh, 0, None, [], 5, 10, n)
    assert r[0] == 0 and _untouched(r)                                      # B == 0: ORR_OK, nothing written
    empty = P.RecallIndex(dim=s["dim"], capacity_rows=0)
    try:
        empty.seal()
        q = s["q"][:4]
        got, st = _stats(idx, lambda: _routed(idx, empty, kh, q, s["texts"][:4], 10, 5, n))
        assert (got[2] == 0).all() and (got[4] == 0).all() and (got[0] == -1).all() and (got[3] == NONE).all()
        assert not st, st                                                   # nothing launched on idx
    finally:
        empty.close()


# ---- 9: threads and refusals --------------------------------------------------------------------------------------------------------

def test_two_threads_on_one_pair_of_handles_and_the_refusals():
    P = pkg()
    s, other = _r1(), _r2()
    idx, n, docs, kh = s["idx"], s["n"], s["docs"], s["kh"]
    q, texts = s["q"][:16], s["texts"][:16]
    results, errors = [None] * 2, []

    def work(i):
        try:
            for _ in range(3):
                results[i] = _routed(idx, docs, kh, q, texts, 10, 3 + 5 * i, n)
        except Exception as e:                          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, got in enumerate(results):
        _check(got, s, q, texts, 10, 3 + 5 * i, n, what=("threads", i))
    E, S = P.native.ORR_EINVAL, P.native.ORR_ESTATE
    err = P.native.hip.orr_last_error
    q2, t2 = np.ascontiguousarray(q[:2]), texts[:2]
    r = _raw(docs, idx, other["kh"], 2, q2, t2, 3, 10, n)
    assert r[0] == E and b"another shard" in err() and _untouched(r)
    osc = other["idx"].scope(other["ids"][:10])
    try:
        r = _raw(docs, idx, kh, 2, q2, t2, 3, 10, n, within=osc)
        assert r[0] == E and b"another shard" in err() and _untouched(r)
    finally:
        osc.close()
    for route in (0, 1_025):
        r = _raw(docs, idx, kh, 2, q2, t2, route, 10, n)
        assert r[0] == E and b"route must be in 1 .. 1024" in err() and _untouched(r)
    r = _raw(None, idx, kh, 2, q2, t2, 3, 10, n)
    assert r[0] == E and b"null document index" in err() and _untouched(r)
    r = _raw(docs, idx, None, 2, q2, t2, 3, 10, n)
    assert r[0] == E and b"null keys" in err() and _untouched(r)
    emb, created, rowbytes = tbase._rows(500, 16)
    ids = np.arange(500, dtype=np.int64)
    small = tbase._build(emb, created, rowbytes, ids, 500)
    k2 = small.keys(ids, ids // 7)
    d2 = k2.centroid_index()
    try:
        qs = np.ascontiguousarray(emb[:2])
        assert _raw(d2, small, k2, 2, qs, ["", ""], 3, 10, 500)[0] == 0
        small.close()                                   # the keys are orphaned: ORR_ESTATE, nothing written
        r = _raw(d2, d2, k2, 2, qs, ["", ""], 3, 10, 500)
        assert r[0] == S and b"orphaned" in err() and _untouched(r)
    finally:
        d2.close()
        k2.close()
