"""The document index on the device (orr_keys_centroid_index) and the read-back of stored rows (orr_index_get_rows).

Every comparison is on raw bits.  Three yardsticks:
  * the test's OWN host copy of the vectors (get_rows on an ordinary index, through maintenance and a view);
  * the numpy restatement of tests/test_gpu_key_groups.py (Model: members in candidate order, participating rows, the blocked
    fp64 sum, float32(S / n)) and RecallKeys.centroids, the host's division and cast;
  * THE TWIN: the index a host builds on the same device from groups + centroids + create + append + seal, with the ticks of each
    key's first participating member taken from the test's own data.  Derived index and twin must answer alike: row ids, score
    bits, counts and order.

Shards (those of tests/test_gpu_key_groups.py, built once and only read; a second key column on G1 adds a key none of whose
members participates):
    G1   4,099 x 70     the scalar form of keys_centroid_finish; keys INT64_MIN + 1, -1, 0, INT64_MAX, ORR_KEY_NONE; rows without
                        an embedding, a zero vector, a NaN coordinate, a +inf, deleted rows; skipped >= 1
    G2  20,000 x 128    the vector form; planted keys of 1, 255, 256, 257 and 1,000 members
    G3  70,001 x 8      one key per row: more keys than one orr_keys_centroids call lists, two slices of 65,536"""
import copy
import ctypes as C
import threading

import numpy as np
import pytest

import test_gpu_key_groups as kg
import test_gpu_scope_terms as tbase
from helpers import pkg

pytestmark = pytest.mark.gpu

NONE = kg.NONE
ALL_OUT, LATE = -5, -7                                  # G1: the key of four rows without an embedding; a key whose newest member has none
_syn, _stats, _bits32, _same32 = kg._syn, kg._stats, kg._bits32, kg._same32
_F = {}


def _same_bits64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the shards --------------------------------------------------------------------------------------------------------------

def _g1():
    """G1 with a second key column.  Four rows without an embedding carry a key of their own (ALL_OUT, below -1: kept keys follow
    it, so a gap left for it would shift them); the fifth shares the key LATE with one OLDER ordinary row, so LATE's first member
    in candidate order does not participate and its ticks are not those of the first member that does"""
    if "g1" not in _F:
        idx, _, model, ids = kg._g1()
        _, created, _ = tbase._rows(kg.N1, kg.D1)
        m2 = copy.copy(model)
        m2.key = dict(model.key)
        for r in (10, 11, 4_000, 4_098):
            assert not m2.emb[int(ids[r])].any()
            m2.key[int(ids[r])] = ALL_OUT
        x = 500
        assert not m2.emb[int(ids[x])].any()
        older = [r for r in range(kg.N1) if int(ids[r]) in m2.key and created[r] < created[x] and r not in (77, 1_203, 2_950)
                 and kg._participates(m2.emb[int(ids[r])][None, :])[0]]
        y = min(older, key=lambda r: created[r])
        m2.key[int(ids[x])] = m2.key[int(ids[y])] = LATE
        live = np.fromiter(m2.key.keys(), np.int64)
        hk = idx.keys(live, np.array([m2.key[int(i)] for i in live], np.int64))
        _F["g1"] = (idx, hk, m2, ids, dict(zip(ids.tolist(), created.tolist())))
        _F["late"] = (int(created[x]), int(created[y]))
    return _F["g1"]


def _g2():
    if "g2" not in _F:
        idx, hk, model, ids, created = kg._g2()
        _F["g2"] = (idx, hk, model, ids, dict(zip(ids.tolist(), created.tolist())))
    return _F["g2"]


def _expected(model, ticks_of, within=None):
    """(kept keys ascending, their first participating member's ticks, all keys, the rows) from the test's own data"""
    order = np.asarray(model.order(within), np.int64)
    rows = model.rows(order)
    ks, E = rows
    part = kg._participates(E) & (ks != NONE) if len(ks) else np.zeros(0, bool)
    kept, first = np.unique(ks[part], return_index=True)               # (the index of a key's FIRST occurrence)
    ticks = np.array([ticks_of[int(i)] for i in order[part][first]], np.int64)
    every = np.unique(ks[ks != NONE])
    return kept, ticks, every, rows


def _twin(P, hk, dim, kept_ticks, within=None):
    """the host route of the header's twin rule, on the same device; kept_ticks: key -> ticks from the test's own data"""
    gk, _ = hk.groups(within)
    cents, used = [], []
    for i0 in range(0, len(gk), 65_536):
        c, u = hk.centroids(gk[i0:i0 + 65_536], within)
        cents.append(c)
        used.append(u)
    cent = np.concatenate(cents) if cents else np.zeros((0, dim), np.float32)
    used = np.concatenate(used) if used else np.zeros(0, np.int64)
    keep = used > 0
    keys = gk[keep]
    twin = P.RecallIndex(dim=dim)
    if len(keys):
        ticks = np.array([kept_ticks[int(k)] for k in keys], np.int64)
        twin.append(np.ascontiguousarray(cent[keep]), ticks, np.zeros(1, np.uint8), np.zeros(len(keys) + 1, np.uint64), row_ids=keys)
    twin.seal()
    return twin, keys, int((~keep).sum())


def _answers(ix, dim, n_docs, cosines=(0.0, 0.05, 0.1, 0.2), near=0.05):
    """what the comparisons of check 3 look at, in one list"""
    syn, P = _syn(), pkg()
    q = syn.query_vectors(0, 64, dim, max(n_docs, 64)).numpy()
    terms = [P.text.query_terms(t) for t in syn.query_texts(0, 64, max(n_docs, 64))]
    out = []
    for B in (1, 64):
        for tt in (terms[:B], [[] for _ in range(B)]):
            for limit in (300, max(n_docs, 1)):
                out.append(ix.search(q[:B], tt, syn.NOW_TICKS, 10, candidate_limit=limit))
    rows, keys, cos, totals = ix.range_cosine(q[:4], list(cosines), 50)
    sc = ix.scope_near(q[:2], near, "any")
    near = sc.row_ids()
    sc.close()
    return out, (rows, keys, cos, totals), near


def _alike(a, b, what):
    (sa, ra, na), (sb, rb, nb) = a, b
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert np.array_equal(x[2], y[2]), (what, "counts", i)
        assert np.array_equal(x[0], y[0]), (what, "rows", i, x[0][0, :5], y[0][0, :5])
        assert _same_bits64(x[1], y[1]), (what, "scores", i)
    assert np.array_equal(ra[3], rb[3]), (what, "range totals")
    for b_ in range(len(ra[0])):
        assert np.array_equal(ra[0][b_], rb[0][b_]) and np.array_equal(ra[1][b_], rb[1][b_]) and _same_bits64(ra[2][b_], rb[2][b_]), (what, "range", b_)
    assert np.array_equal(na, nb), (what, "near")


def _derive(hk, within=None):
    d = hk.centroid_index(within)
    assert d.rows == d.docs, (d.rows, d.docs)
    return d


# ---- 1. get_rows on an ordinary index ----------------------------------------------------------------------------------------

def test_get_rows_on_an_ordinary_index_through_maintenance_and_a_view():
    P = pkg()
    rng = np.random.default_rng(901)
    n, dim = 3_001, 36
    _, created, rowbytes = tbase._rows(n, dim)
    emb = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-6, 6, (n, dim))).astype(np.float32)
    emb[5, 3] = np.nan
    emb[6] = 0.0
    ids = np.arange(n, dtype=np.int64) * 7 + 2
    idx = tbase._build(emb, created, rowbytes, ids, n + 400)
    host = {int(i): emb[r] for r, i in enumerate(ids)}
    UNKNOWN = 1_000_000_007
    dead = []                                           # every id deleted so far: asked for in every check

    def check(ix, what):
        live = np.fromiter(host.keys(), np.int64)
        ask = np.concatenate([live, [UNKNOWN], rng.permutation(live)[:257], np.array(dead, np.int64), [UNKNOWN, int(ids[0]) - 1]])
        got, found = ix.get_rows(ask)
        want = np.stack([host.get(int(i), np.zeros(dim, np.float32)) for i in ask])
        assert np.array_equal(_bits32(got), _bits32(want)), (what, np.nonzero((_bits32(got) != _bits32(want)).any(axis=1))[0][:6])
        assert np.array_equal(found, np.array([int(i) in host for i in ask])), what

    check(idx, "made")
    got, found = idx.get_rows(np.zeros(0, np.int64))
    assert got.shape == (0, dim) and found.shape == (0,)
    gone = rng.choice(ids, 300, replace=False)
    assert idx.delete_rows(gone) == 300
    for i in gone:
        del host[int(i)]
    dead.extend(int(i) for i in gone)
    check(idx, "deleted")                               # a deleted id reads zeros and found 0
    live = np.fromiter(host.keys(), np.int64)
    upd = rng.choice(live, 64, replace=False)
    new = rng.standard_normal((64, dim)).astype(np.float32)
    assert idx.update_rows(upd, new) == 64
    for r, i in enumerate(upd):
        host[int(i)] = new[r]
    lost = np.setdiff1d(live, upd)[:9]
    assert idx.update_rows(lost, None) == 9             # rows without an embedding: the stored zeros, found 1
    for i in lost:
        host[int(i)] = np.zeros(dim, np.float32)
    check(idx, "updated")
    assert idx.compact() == 300
    check(idx, "compacted")
    m = 130
    e2 = rng.standard_normal((m, dim)).astype(np.float32)
    _, _, rb2 = tbase._rows(m, dim, row0=9_000_000)
    c2 = rng.choice(created, m).astype(np.int64) + rng.integers(-2, 3, m)
    new_ids = 80_000_000 + np.arange(m, dtype=np.int64)
    assert idx.insert_rows(e2, c2, rb2.reshape(-1), np.arange(m + 1, dtype=np.uint64) * rb2.shape[1], row_ids=new_ids) == m
    for r, i in enumerate(new_ids):
        host[int(i)] = e2[r]
    check(idx, "inserted")
    view = idx.view()
    check(view, "a view")
    h = P.native.hip
    out = np.full((1, dim + 1), 7, np.float32)
    one = np.array([int(new_ids[0])], np.int64)
    for bad in (dim + 1, dim - 1, 0, -2):
        assert h.orr_index_get_rows(idx._h, 1, one.ctypes.data, bad, out.ctypes.data, None) == P.native.ORR_EDIM
    assert (out == 7).all()
    view.close()
    idx.close()


# ---- 2. the derived index against the restatement ----------------------------------------------------------------------------

def _check_against_the_restatement(idx, hk, model, ticks_of, dim, what):
    kept, ticks, every, rows = _expected(model, ticks_of)
    d = _derive(hk)
    try:
        assert d.docs == len(kept) and d.skipped == len(every) - len(kept), (what, d.docs, len(kept), d.skipped)
        got, found = d.get_rows(kept)
        assert found.all()
        cent, used = hk.centroids(kept)
        assert (used > 0).all()
        assert _same32(got, cent), (what, "the device's division or cast differs from the host's")
        for i, k in enumerate(kept):
            c, _, n = model.centroid(rows, int(k))
            assert n == int(used[i]) and _same32(got[i], c), (what, int(k), n)
        _, absent = d.get_rows(np.setdiff1d(every, kept))
        assert not absent.any()
        # the ticks: a query that returns every document, as records
        syn = _syn()
        q = syn.query_vectors(0, 1, dim, 64).numpy()
        rec = d.search_shard(q, [[]], syn.NOW_TICKS, d.docs, d.docs)[0]
        assert int(rec[d.docs]["matches"]) == d.docs, (what, int(rec[d.docs]["matches"]))          # the trailer: the valid records
        rec = rec[:d.docs]
        assert sorted(rec["row_id"].tolist()) == kept.tolist(), what
        by_key = dict(zip(kept.tolist(), ticks.tolist()))
        assert [int(t) for t in rec["created_ticks"]] == [by_key[int(k)] for k in rec["row_id"]], what
    finally:
        d.close()
    return kept, every


def test_g1_the_derived_index_equals_the_restatement_and_the_hosts_centroids():
    idx, hk, model, ids, ticks_of = _g1()
    kept, every = _check_against_the_restatement(idx, hk, model, ticks_of, kg.D1, "g1")
    assert ALL_OUT in every and ALL_OUT not in kept and len(every) - len(kept) >= 1
    assert (kept > ALL_OUT).sum() > 100 and kept[0] < ALL_OUT         # kept keys on both sides of the skipped one
    t_first, t_part = _F["late"]
    assert LATE in kept and t_first > t_part                          # LATE's newest member takes no part ...
    assert {kg.I64_MIN + 1, -1, 0, kg.I64_MAX} <= set(kept.tolist()) and kept[0] == kg.I64_MIN + 1 and kept[-1] == kg.I64_MAX
    d = _derive(hk)
    k_inf = model.key[int(ids[2_950])]
    assert np.isposinf(d.get_rows([k_inf])[0][0, 3])    # the +inf row takes part
    rec = d.search_shard(_syn().query_vectors(0, 1, kg.D1, 64).numpy(), [[]], _syn().NOW_TICKS, d.docs, d.docs)[0, :d.docs]
    assert int(rec["created_ticks"][rec["row_id"] == LATE][0]) == t_part      # ... and its ticks are the first participating member's
    d.close()


def test_g2_the_derived_index_equals_the_restatement_and_the_hosts_centroids():
    idx, hk, model, ids, ticks_of = _g2()
    kept, every = _check_against_the_restatement(idx, hk, model, ticks_of, kg.D2, "g2")
    assert set(kg.PLANTED) <= set(kept.tolist()) and len(kept) == len(every) > 800


# ---- 3. the derived index against the twin -----------------------------------------------------------------------------------

def _scopes_g2(idx, model, ids, created_of):
    created = np.array([created_of[int(i)] for i in ids], np.int64)
    lo, hi = np.sort(created)[[kg.N2 // 4, 3 * kg.N2 // 4]]
    k255 = np.array([int(i) for i in ids if model.key[int(i)] == 9_000_255], np.int64)
    return {"none": None, "ticks": idx.scope_ticks(int(lo), int(hi)), "terms": idx.scope_terms([tbase.FRAG], "any"),
            "rest": idx.scope(np.setdiff1d(ids, k255)), "empty": idx.scope(np.zeros(0, np.int64))}


def _check_against_the_twin(P, hk, model, ticks_of, dim, within, what):
    kept, ticks, every, _ = _expected(model, ticks_of, within)
    twin, tkeys, tskipped = _twin(P, hk, dim, dict(zip(kept.tolist(), ticks.tolist())), within)
    d = _derive(hk, within)
    try:
        assert np.array_equal(tkeys, kept) and d.docs == twin.rows == len(kept) and d.skipped == tskipped, (what, d.docs, twin.rows, d.skipped, tskipped)
        if d.docs:
            _alike(_answers(d, dim, d.docs), _answers(twin, dim, d.docs), what)
    finally:
        d.close()
        twin.close()
    return len(kept)


def test_g1_the_derived_index_answers_like_the_twin():
    idx, hk, model, ids, ticks_of = _g1()
    assert _check_against_the_twin(pkg(), hk, model, ticks_of, kg.D1, None, "g1") > 100
    sc = idx.scope(ids[::3])
    _check_against_the_twin(pkg(), hk, model, ticks_of, kg.D1, sc, "g1 every third id")
    sc.close()


@pytest.mark.parametrize("name", ["none", "ticks", "terms", "rest", "empty"])
def test_g2_the_derived_index_answers_like_the_twin(name):
    idx, hk, model, ids, ticks_of = _g2()
    scopes = _scopes_g2(idx, model, ids, ticks_of)
    try:
        n = _check_against_the_twin(pkg(), hk, model, ticks_of, kg.D2, scopes[name], "g2 " + name)
        if name == "empty":
            assert n == 0                               # both sides have 0 rows
        else:
            assert n > 100
        if name == "rest":
            d = _derive(hk, scopes[name])
            assert not d.get_rows([9_000_255])[1][0]    # the scope empties this key: it has no row at all
            d.close()
    finally:
        for sc in scopes.values():
            if sc is not None:
                sc.close()


# ---- 4. slices ---------------------------------------------------------------------------------------------------------------

def _slices_with_a_kept_key(every, kept, per_slice):
    is_kept = np.isin(every, kept)
    return sum(1 for s0 in range(0, len(every), per_slice) if is_kept[s0:s0 + per_slice].any())


def _check_slices(idx, hk, model, ticks_of, within, what):
    kept, _, every, _ = _expected(model, ticks_of, within)
    base = _derive(hk, within)
    want, _ = base.get_rows(kept)
    base.close()
    try:
        for per_slice in (7, 1):
            idx.set_option("key_groups_slice", per_slice)
            d, stats = _stats(idx, lambda: _derive(hk, within))
            got, found = d.get_rows(kept)
            rec = d.docs
            d.close()
            assert found.all() and rec == len(kept) and np.array_equal(_bits32(got), _bits32(want)), (what, per_slice)
            n = _slices_with_a_kept_key(every, kept, per_slice)
            assert stats["keys_centroid_finish"]["launches"] == n, (what, per_slice, stats["keys_centroid_finish"], n)
            assert stats["keys_block_sums"]["launches"] == n, (what, per_slice, stats["keys_block_sums"], n)
            assert stats["keys_centroid_finish"]["algo_bytes"] == 12.0 * model.dim * len(kept)
            assert stats["keys_pairs_sort"]["launches"] == 2 and stats["keys_runs"]["launches"] == 2      # all members; the participating ones
    finally:
        idx.set_option("key_groups_slice", 0)
    d, stats = _stats(idx, lambda: _derive(hk, within))
    d.close()
    assert stats["keys_centroid_finish"]["launches"] == 1 and stats["keys_block_sums"]["launches"] == 1
    return kept, every


def test_g1_the_slice_option_changes_no_bit_and_a_slice_without_a_kept_key_launches_nothing():
    idx, hk, model, ids, ticks_of = _g1()
    kept, every = _check_slices(idx, hk, model, ticks_of, None, "g1")
    assert _slices_with_a_kept_key(every, kept, 1) == len(kept) < len(every)      # at one key per slice the skipped keys launch nothing


def test_g2_the_slice_option_changes_no_bit_with_keys_of_several_blocks():
    idx, hk, model, ids, ticks_of = _g2()
    some = set(list(kg.PLANTED) + list(range(1_000, 1_040)))
    sc = idx.scope(np.array([int(i) for i in ids if model.key[int(i)] in some], np.int64))
    kept, every = _check_slices(idx, hk, model, ticks_of, sc, "g2 some keys")
    sc.close()
    assert set(kg.PLANTED) <= set(kept.tolist())


def test_an_index_appended_slice_by_slice_answers_like_the_twins_single_append():
    """"key_groups_slice" = 7: the derived index is filled by one append per slice with a kept key (G1: some 30 of them, a skipped
    key among the slices; G2 inside a ticks scope: some 70), the twin by ONE append -- search, range and scope_near answers alike"""
    P = pkg()
    idx1, hk1, model1, ids1, ticks1 = _g1()
    idx2, hk2, model2, ids2, ticks2 = _g2()
    sc = _scopes_g2(idx2, model2, ids2, ticks2)
    try:
        for idx in (idx1, idx2):
            idx.set_option("key_groups_slice", 7)
        d, stats = _stats(idx1, lambda: _derive(hk1))
        d.close()
        assert stats["keys_centroid_finish"]["launches"] > 20
        assert _check_against_the_twin(P, hk1, model1, ticks1, kg.D1, None, "g1 in slices of 7") > 100
        assert _check_against_the_twin(P, hk2, model2, ticks2, kg.D2, sc["ticks"], "g2 ticks in slices of 7") > 100
    finally:
        for idx in (idx1, idx2):
            idx.set_option("key_groups_slice", 0)
        for s in sc.values():
            if s is not None:
                s.close()


# ---- 5. more than 65,536 keys ------------------------------------------------------------------------------------------------

def test_g3_one_key_per_row_beyond_the_limit_of_one_centroids_call():
    n, dim = 70_001, 8
    emb, created, rowbytes = tbase._rows(n, dim)
    assert not (np.signbit(emb) & (emb == 0)).any() and (emb != 0).any(axis=1).all()       # no -0.0 (the sum starts at +0.0), no zero row
    ids = np.arange(n, dtype=np.int64) * 3 + 5
    keys = ids * 11 - 400_000                          # one key per row, some negative
    idx = tbase._build(emb, created, rowbytes, ids, n)
    hk = idx.keys(ids, keys)
    d, stats = _stats(idx, lambda: _derive(hk))
    assert d.docs == n and d.skipped == 0
    assert stats["keys_centroid_finish"]["launches"] == 2 and stats["keys_block_sums"]["launches"] == 2      # slices of 65,536 and 4,465 keys
    got, found = d.get_rows(keys)
    assert found.all() and np.array_equal(_bits32(got), _bits32(emb))          # a one-member centroid is the row itself
    r = int(np.argmax(created))                         # the newest row: no other row is ahead of it in cosine or in recency
    rows, _, counts = d.search(emb[r:r + 1], [[]], _syn().NOW_TICKS, 1, candidate_limit=n)
    assert counts[0] == 1 and rows[0, 0] == keys[r]
    sc = d.scope_near(emb[65_536:65_537], 0.999999, "all")
    assert int(keys[65_536]) in sc.row_ids().tolist()   # the first key of the second slice landed on its own row
    sc.close()
    # two appends here, one on the twin (built from two centroids calls): the answers alike
    twin, tkeys, tskipped = _twin(pkg(), hk, dim, dict(zip(keys.tolist(), created.tolist())))
    assert np.array_equal(tkeys, np.sort(keys)) and tskipped == 0 and twin.rows == n
    high = dict(cosines=(0.9, 0.93, 0.95, 0.97), near=0.95)      # (dim 8: a low threshold would list a third of the shard)
    _alike(_answers(d, dim, n, **high), _answers(twin, dim, n, **high), "g3 against the twin")
    twin.close()
    d.close()
    hk.close()
    idx.close()


# ---- 6. independence ---------------------------------------------------------------------------------------------------------

def _small(seed):
    rng = np.random.default_rng(seed)
    n, dim = 3_000, 36
    _, created, rowbytes = tbase._rows(n, dim)
    emb = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-3, 3, (n, dim))).astype(np.float32)
    ids = np.arange(n, dtype=np.int64) + 50
    keys = (np.arange(n) // 6).astype(np.int64)         # 500 documents of six chunks
    idx = tbase._build(emb, created, rowbytes, ids, n)
    return idx, idx.keys(ids, keys), kg.Model(idx, emb, ids, keys), dict(zip(ids.tolist(), created.tolist())), dim


def test_the_derived_index_outlives_its_source_in_both_destroy_orders_and_takes_maintenance():
    P = pkg()
    idx, hk, model, ticks_of, dim = _small(905)
    kept, ticks, _, _ = _expected(model, ticks_of)
    by_key = dict(zip(kept.tolist(), ticks.tolist()))
    twin, _, _ = _twin(P, hk, dim, by_key)
    twin2, _, _ = _twin(P, hk, dim, by_key)
    d1, d2 = _derive(hk), _derive(hk)
    want = _answers(twin, dim, twin.rows)
    hk.close()                                          # the keys first, then the index ...
    _alike(_answers(d1, dim, d1.docs), want, "after orr_keys_destroy")
    idx.close()
    _alike(_answers(d1, dim, d1.docs), want, "after the source index is destroyed")
    # maintenance on the derived index, then a twin treated alike
    rng = np.random.default_rng(7)
    gone = rng.choice(kept, 40, replace=False)
    upd = np.setdiff1d(kept, gone)[:25]
    new = rng.standard_normal((25, dim)).astype(np.float32)
    for ix in (d2, twin2):
        assert ix.delete_rows(gone) == 40 and ix.update_rows(upd, new) == 25
    _alike(_answers(d2, dim, d2.docs), _answers(twin2, dim, d2.docs), "deleted and updated alike")
    got, found = d2.get_rows(np.concatenate([upd, gone]))
    assert np.array_equal(_bits32(got[:25]), _bits32(new)) and found[:25].all() and not found[25:].any() and not got[25:].any()
    for ix in (d1, d2, twin, twin2):
        ix.close()
    # ... and the index first: the keys are orphaned, a derived index made before still answers
    idx, hk, model, ticks_of, dim = _small(906)
    d = _derive(hk)
    before = _answers(d, dim, d.docs)
    idx.close()
    with pytest.raises(P.native.OrrError) as e:
        hk.centroid_index()
    assert e.value.code == P.native.ORR_ESTATE
    _alike(_answers(d, dim, d.docs), before, "the index went first")
    hk.close()
    d.close()


def test_two_threads_build_at_once_and_a_view_builds_the_same():
    idx, hk, model, ticks_of, dim = _small(907)
    kept, _, _, _ = _expected(model, ticks_of)
    base = _derive(hk)
    want, _ = base.get_rows(kept)
    base.close()
    errors = []

    def work():
        try:
            for _ in range(3):
                d = _derive(hk)
                got, found = d.get_rows(kept)
                d.close()
                assert found.all() and np.array_equal(_bits32(got), _bits32(want))
        except BaseException as e:                      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    view = idx.view()
    sc = view.scope(np.fromiter(model.emb.keys(), np.int64)[:1_500])    # a scope made through a view
    kept_sc, _, _, rows = _expected(model, ticks_of, sc)
    d = _derive(hk, sc)
    got, _ = d.get_rows(kept_sc)
    for i, k in enumerate(kept_sc):
        assert _same32(got[i], model.centroid(rows, int(k))[0]), int(k)
    d.close()
    sc.close()
    view.close()
    hk.close()
    idx.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_out_pointer_untouched():
    P = pkg()
    h = P.native.hip
    idx, hk, model, ticks_of, dim = _small(908)
    out = C.c_void_p(0x7777)
    docs = C.c_int64(7)
    pd = C.cast(C.byref(docs), C.c_void_p)
    emb, created, rowbytes = tbase._rows(64, dim)
    ids = np.arange(64, dtype=np.int64) + 50
    other = tbase._build(emb, created, rowbytes, ids, 64)
    foreign = other.scope(ids[:10])
    assert h.orr_keys_centroid_index(hk._h, foreign._h, C.byref(out), pd, None) == P.native.ORR_EINVAL      # a scope of another shard
    assert out.value == 0x7777 and docs.value == 7
    foreign.close()
    other.close()
    # a source without embeddings
    syn = _syn()
    idx0 = P.RecallIndex(dim=0)
    idx0.append(None, created, rowbytes.reshape(-1), np.arange(65, dtype=np.int64) * syn.ROW_BYTES, row_ids=ids)
    idx0.seal()
    hk0 = idx0.keys(ids, np.arange(64, dtype=np.int64) // 4)
    assert h.orr_keys_centroid_index(hk0._h, None, C.byref(out), pd, None) == P.native.ORR_EDIM
    assert out.value == 0x7777 and docs.value == 7
    hk0.close()
    idx0.close()
    # an orphaned keys handle
    idx.close()
    assert h.orr_keys_centroid_index(hk._h, None, C.byref(out), pd, None) == P.native.ORR_ESTATE
    assert out.value == 0x7777 and docs.value == 7
    hk.close()
