"""Term scopes (orr_scope_create_terms): the scope of the live rows whose content contains all, or any, of a list of terms.

Membership is restated here in Python: for every live row, all / any of `term in content` over the row's lowercased bytes; the
expected row_ids() are the ids of those rows in candidate order (Model.has compares the rows' bytes on the device with tensors,
which test_the_two_restatements_agree holds against bytes.find).  Every check is exact.  Behind the handle nothing is new, so a
search inside a term scope is compared array for array with search_masked on the restated ids, and a stated subset with the
oracle on that sub-corpus (the method of tests/test_gpu_scope_handle.py, whose Model / _rows / _build are restated below).

Shard A, 200,000 x 128, built once: the smallest shard with stored token bitmaps (196,608 rows) and a masked screen; one hybrid
search runs first so that the int8 shadow and the token bitmaps exist.  On its corpus every token's posting list is longer than
N / 64, so a whole vocabulary word is the ALIAS path (the fold reads a stored token bitmap) and a 2-byte fragment, a substring
of many words, the EXPANSION path.  Shard B, 70,001 x 64, built fresh per test with capacity reserved: three bitmap chunks with
the last one partial, a row count that is no multiple of 32, no stored token bitmaps, and planted tokens of 20 and 40 bytes in
the first word, the last full word, the partial last word and row 70,000."""
import importlib
import threading

import numpy as np
import pytest

from helpers import orc, pkg

pytestmark = pytest.mark.gpu

NA, DIM_A = 200_000, 128
NB, DIM_B = 70_001, 64
POOL_Q = 40
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FRAG = b"ab"                                            # a substring of dozens of the 4096 vocabulary words
NOTHING = b"qqqqqqq"                                    # longer than any word of shard A: matches nothing


def _syn():
    pkg()                                               # (registers the package under its importable name)
    return importlib.import_module("omni_recall_rag_amd.synthetic")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


class Model:
    """The shard as the test knows it: rows in candidate order with their ids and bytes; deletes, compaction and insertion
    restated; and the restatement of a term scope."""

    def __init__(self, emb, created, rowbytes, ids):
        self.emb, self.created, self.rowbytes = emb.copy(), np.asarray(created, np.int64).copy(), rowbytes.copy()
        self.ids = np.asarray(ids, np.int64).copy()
        self.dead = np.zeros(len(self.ids), bool)
        self._has = {}

    def _changed(self):
        self._has = {}

    def has_by_find(self, term):
        """per row: the row's bytes contain the term -- `term in content`, with bytes.find over the rows laid end to end"""
        term = bytes(term)
        blob, (n, width) = self.rowbytes.tobytes(), self.rowbytes.shape
        m = np.zeros(n, bool)
        pos = blob.find(term)
        while pos >= 0:
            row = pos // width
            if pos + len(term) <= (row + 1) * width:                # (a match across two rows is no match)
                m[row] = True
                pos = blob.find(term, (row + 1) * width)            # on with the next row
            else:
                pos = blob.find(term, pos + 1)
        return m

    def has(self, term):
        """the same, byte for byte, as tensor comparisons on the device (a hundred terms over 200,000 rows take seconds with
        bytes.find): position p of a row matches when byte p + j equals term[j] for every j; cached until the rows move.
        test_the_two_restatements_agree holds the two against each other."""
        import torch
        term = bytes(term)
        if term not in self._has:
            if "dev" not in self._has:
                self._has["dev"] = torch.from_numpy(self.rowbytes).to("cuda:0")
            x = self._has["dev"]
            span = x.shape[1] - len(term) + 1
            if span <= 0:
                self._has[term] = np.zeros(x.shape[0], bool)
            else:
                m = x[:, 0:span] == term[0]
                for j in range(1, len(term)):
                    m &= x[:, j:j + span] == term[j]
                self._has[term] = m.any(dim=1).cpu().numpy()
        return self._has[term]

    def term_ids(self, terms, mode):
        """the ids of the live rows that contain all / any of the terms, in candidate order"""
        n = len(self.ids)
        if not terms:
            return np.zeros(0, np.int64)
        m = np.ones(n, bool) if mode == "all" else np.zeros(n, bool)
        for t in terms:
            m = (m & self.has(t)) if mode == "all" else (m | self.has(t))
        return self.ids[m & ~self.dead]

    def rows_of_ids(self, ids):
        return np.nonzero(np.isin(self.ids, np.asarray(ids, np.int64)) & ~self.dead)[0]

    def ordered(self, id_set):
        """the ids of the set's live rows in candidate order: what row_ids() of a scope holding them must return"""
        return self.ids[np.isin(self.ids, np.fromiter(id_set, np.int64, len(id_set))) & ~self.dead]

    def sub(self, ids):
        keep = self.rows_of_ids(ids)
        if len(keep) == 0:
            return keep, None
        width = self.rowbytes.shape[1]
        off = np.arange(len(keep) + 1, dtype=np.int64) * width
        return keep, orc.OracleCorpus(np.ascontiguousarray(self.emb[keep]), self.created[keep], (np.ascontiguousarray(self.rowbytes[keep]).reshape(-1), off))

    def delete(self, ids):
        self.dead |= np.isin(self.ids, np.asarray(ids, np.int64))

    def compact(self):
        keep = ~self.dead
        self.emb, self.created, self.rowbytes, self.ids = self.emb[keep], self.created[keep], self.rowbytes[keep], self.ids[keep]
        self.dead = np.zeros(len(self.ids), bool)
        self._changed()

    def insert(self, emb, created, rowbytes, ids):
        """a STABLE descending order by ticks: at equal ticks the rows that were there stay in front"""
        c = np.concatenate([self.created, np.asarray(created, np.int64)])
        order = np.argsort(np.negative(c), kind="stable")
        self.emb = np.concatenate([self.emb, emb])[order]
        self.rowbytes = np.concatenate([self.rowbytes, rowbytes])[order]
        self.ids = np.concatenate([self.ids, np.asarray(ids, np.int64)])[order]
        self.dead = np.concatenate([self.dead, np.zeros(len(ids), bool)])[order]
        self.created = c[order]
        self._changed()


def _rows(n, dim, row0=0, n_total=None):
    """synthetic rows row0 .. row0 + n: (emb, created, rowbytes) as numpy"""
    syn = _syn()
    emb = syn.embeddings(row0, n, dim, "cuda:0").cpu().numpy()
    created = syn.created_ticks(row0, n, n_total or n).numpy()
    pool, _ = syn.contents(row0, n, "cuda:0")
    return emb, created, pool.reshape(n, syn.ROW_BYTES).cpu().numpy()


def _build(emb, created, rowbytes, ids, capacity):
    import torch
    P, syn = pkg(), _syn()
    n, dim = emb.shape
    idx = P.RecallIndex(dim=dim, capacity_rows=capacity)
    off = np.arange(n + 1, dtype=np.int64) * syn.ROW_BYTES
    for r0 in range(0, n, 50_000):
        r1 = min(n, r0 + 50_000)
        idx.append(emb[r0:r1], created[r0:r1], rowbytes[r0:r1].reshape(-1), off[: r1 - r0 + 1], row_ids=ids[r0:r1])
    idx.seal()
    torch.cuda.synchronize()
    return idx


def _queries(dim, n):
    syn = _syn()
    return syn.query_vectors(0, POOL_Q, dim, n).numpy(), syn.query_texts(0, POOL_Q, n)


def _terms(texts):
    P = pkg()
    return [P.text.query_terms(t) for t in texts]


def _search(idx, q, texts, topk, limit):
    return idx.search(np.ascontiguousarray(q, dtype=np.float32), _terms(texts), _syn().NOW_TICKS, topk, candidate_limit=limit)


def _in_scope(idx, q, texts, topk, limit, sc):
    return idx.search_in_scope(np.ascontiguousarray(q, dtype=np.float32), _terms(texts), _syn().NOW_TICKS, topk, sc, candidate_limit=limit)


def _masked(idx, q, texts, topk, limit, ids):
    return idx.search_masked(np.ascontiguousarray(q, dtype=np.float32), _terms(texts), _syn().NOW_TICKS, topk, ids, candidate_limit=limit)


def _equal(x, y):
    return np.array_equal(x[0], y[0]) and _same(x[1], y[1]) and np.array_equal(x[2], y[2])


def _against_oracle(model, ids, got, q, texts, topk, limit, checked, what):
    """the results `got` of a search inside the live rows of `ids` against the oracle on that sub-corpus"""
    keep, corpus = model.sub(ids)
    rows, scores, counts = got
    took = min(len(keep), max(1, limit))
    assert (counts == min(max(1, topk), took)).all(), (what, counts[:8], took)
    for b in checked:
        orow, osc, _ = corpus.search(q[b], texts[b], _syn().NOW_TICKS, topk, candidate_limit=limit, threads=16)
        k = int(counts[b])
        assert list(rows[b, :k]) == [int(model.ids[keep[r]]) for r in orow], (what, b, list(rows[b, :6]))
        assert _same(scores[b, :k], np.asarray(osc)), (what, b)


def _check(sc, model, terms, mode, what=None):
    want = model.term_ids(terms, mode)
    assert sc.rows == len(want), (what or terms, mode, sc.rows, len(want))
    assert np.array_equal(sc.row_ids(), want), (what or terms, mode)
    return want


def _stats(idx, fn):
    """the kernel statistics of fn() alone"""
    idx.set_profiling(True)
    try:
        r = fn()
        return r, idx.kernel_stats()
    finally:
        idx.set_profiling(False)


# ---- shard A -----------------------------------------------------------------------------------------------------------------

_A = {}


def _shard_a():
    if _A:
        return _A
    syn = _syn()
    emb, created, rowbytes = _rows(NA, DIM_A)
    ids = np.arange(NA, dtype=np.int64) * 3 + 11
    idx = _build(emb, created, rowbytes, ids, NA)
    model = Model(emb, created, rowbytes, ids)
    q, texts = _queries(DIM_A, NA)
    idx.set_option("two_stage", 1)
    _search(idx, q[:8], texts[:8], 10, NA)              # a search with terms first: the int8 shadow and the token bitmaps exist
    words = [syn.vocab_word(t) for t in (17, 1500, 4000, 2222)]
    assert all(NOTHING not in w and len(w) == 6 for w in words)
    _A.update(idx=idx, model=model, q=q, texts=texts, words=words, words_per_bitmap=((NA + 31) // 32 + 3) // 4 * 4)
    return _A


CASES_A = {
    "one whole word": lambda w: [w[0]],
    "three whole words": lambda w: [w[0], w[1], w[2]],
    "a 2-byte fragment": lambda w: [FRAG],
    "a whole word with a fragment": lambda w: [w[1], FRAG],
    "a term matching nothing": lambda w: [NOTHING],
    "nothing beside a word": lambda w: [w[0], NOTHING],
    "the same term three times": lambda w: [w[2], w[2], w[2]],
    "no terms": lambda w: [],
}


@pytest.mark.parametrize("mode", ["all", "any"])
@pytest.mark.parametrize("case", list(CASES_A))
def test_membership_equals_the_restatement(case, mode):
    a = _shard_a()
    idx, model = a["idx"], a["model"]
    terms = CASES_A[case](a["words"])
    sc, st = _stats(idx, lambda: idx.scope_terms(terms, mode))
    want = _check(sc, model, terms, mode, case)
    sc.close()
    bitmap_bytes = 4.0 * a["words_per_bitmap"]
    if case == "no terms":
        assert len(want) == 0 and "scope_terms_combine" not in st
        return
    n_distinct = len(set(terms))
    assert st["scope_terms_combine"]["launches"] == 1 and st["scope_terms_combine"]["algo_bytes"] == bitmap_bytes * (n_distinct + 1), st
    assert st["expand_hits"]["launches"] == 1                              # the search's chain, once
    # the alias path: what the fold read from STORED token bitmaps -- every whole word, and nothing else
    n_whole = len(set(t for t in terms if t in a["words"]))
    assert st["scope_terms_aliased"]["algo_bytes"] == bitmap_bytes * n_whole, (case, st["scope_terms_aliased"])
    if case == "one whole word":
        assert 0.02 * NA < len(want) < 0.04 * NA                          # 120 of 4096 words per row
    if case == "three whole words":
        assert (len(want) > 0.08 * NA) if mode == "any" else (len(want) < 100)
    if case == "a 2-byte fragment":
        assert len(want) > NA // 2                                        # dozens of words hold it
        assert len(set(w for w in (_syn().vocab_word(t) for t in range(4096)) if FRAG in w)) >= 30
    if case in ("a term matching nothing", "nothing beside a word"):
        assert len(want) == (0 if mode == "all" or case == "a term matching nothing" else len(model.term_ids(terms[:1], "any")))
    if case == "the same term three times":
        assert np.array_equal(want, model.term_ids(terms[:1], mode)) and len(want) > 0


def test_the_two_restatements_agree():
    a = _shard_a()
    model, w = a["model"], a["words"]
    for term in (w[0], FRAG, NOTHING, w[1][1:5], w[2][5:] + b" ", b"f " + w[3][:1]):     # (the last two cross a word border: rows' bytes, not tokens)
        assert np.array_equal(model.has(term), model.has_by_find(term)), term
    assert model.has(w[0]).sum() > 0 and model.has(FRAG).sum() > NA // 2 and model.has(NOTHING).sum() == 0


ROW_MANY = 123_457


def test_more_than_64_terms():
    """65 .. 256 distinct terms: the alias stage counts the hits per term with many workgroups instead of one, and the fold loops
    over up to 256 bitmaps.  The terms are the distinct words of ONE row (and of its neighbours, for 256), so ALL of them is not
    empty: it holds that row."""
    a = _shard_a()
    idx, model = a["idx"], a["model"]
    bitmap_bytes = 4.0 * a["words_per_bitmap"]
    words_of = lambda r: model.rowbytes[r].tobytes().split(b" ")
    one_row = list(dict.fromkeys(words_of(ROW_MANY)))
    assert len(one_row) >= 100 and all(len(x) == 6 for x in one_row)
    hundred = one_row[:100] + [one_row[0][:2], one_row[1][2:5]]          # 100 whole words and two fragments of the same row
    three_rows = list(dict.fromkeys(words_of(ROW_MANY) + words_of(ROW_MANY + 1) + words_of(ROW_MANY + 2)))
    assert len(three_rows) >= 256
    vocab = [bytes(v) for v in _syn()._vocab_table("cpu")[:, :6].numpy()]
    for terms, n_whole in ((hundred, 100), (three_rows[:256], 256), (one_row[:65], 65)):
        # a term is read from a stored token bitmap when exactly one vocabulary word holds it: every whole word, and a fragment by chance
        n_alias = sum(1 for t in terms if sum(t in v for v in vocab) == 1)
        assert n_alias >= n_whole
        for mode in ("all", "any"):
            sc, st = _stats(idx, lambda: idx.scope_terms(terms, mode))
            want = _check(sc, model, terms, mode, (len(terms), "terms"))
            sc.close()
            assert st["scope_terms_combine"]["launches"] == 1 and st["scope_terms_combine"]["algo_bytes"] == bitmap_bytes * (len(terms) + 1)
            assert st["scope_terms_aliased"]["algo_bytes"] == bitmap_bytes * n_alias
            if mode == "any":
                # a row's 120 words are drawn from 4096: it holds none of n words with probability (1 - n / 4096) ** 120
                assert len(want) > 0.98 * NA * (1.0 - (1.0 - n_whole / 4096.0) ** 120)
            elif len(terms) == 256:
                assert len(want) == 0                                      # no row holds three rows' words
            else:
                assert model.ids[ROW_MANY] in want and len(want) < 10
    with pytest.raises(pkg().native.OrrError) as e:                        # 257 terms: refused
        idx.scope_terms(three_rows[:256] + [FRAG], "any")
    assert e.value.code == pkg().native.ORR_EINVAL


@pytest.mark.parametrize("B", [1, 8, 40])
def test_search_in_a_term_scope_equals_search_masked_and_the_oracle(B):
    a = _shard_a()
    idx, model, w = a["idx"], a["model"], a["words"]
    q, texts = a["q"][:B], a["texts"][:B]
    large_terms, small_terms = [FRAG, w[0]], [w[0], w[1]]
    large, small = idx.scope_terms(large_terms, "any"), idx.scope_terms(small_terms, "all")
    ids_large, ids_small = _check(large, model, large_terms, "any"), _check(small, model, small_terms, "all")
    assert len(ids_large) > NA // 2 and 20 < len(ids_small) < 1000
    try:
        for screen, sc, ids, what in ((1, large, ids_large, "large ANY"), (2, small, ids_small, "small ALL")):
            idx.set_option("mask_screen", screen)
            for topk in (1, 10, 64):
                for limit in (300, NA):
                    got = _in_scope(idx, q, texts, topk, limit, sc)
                    idx.reset_search_stats()
                    want = _masked(idx, q, texts, topk, limit, ids)
                    mode = idx.search_stats()["pass_mode"]
                    assert _equal(got, want), (what, B, topk, limit)
                    if screen == 1 and topk == 10 and limit == NA:
                        assert mode == 5, (what, B, mode)                  # the masked screen did run
                        _against_oracle(model, ids, got, q, texts, topk, limit, (0, B - 1) if B > 1 else (0,), what)
                    if screen == 2:
                        assert mode == 4, (what, B, topk, limit, mode)
                        if topk == 10:
                            _against_oracle(model, ids, got, q, texts, topk, limit, range(min(B, 8)), what)
    finally:
        idx.set_option("mask_screen", 0)
        large.close()
        small.close()


def test_search_in_scopes_with_four_term_scopes_and_one_id_scope():
    a = _shard_a()
    idx, model, w = a["idx"], a["model"], a["words"]
    B = 40
    q, texts = a["q"][:B], a["texts"][:B]
    rng = np.random.default_rng(91)
    listed = model.ids[np.sort(rng.choice(NA, 20_000, replace=False))]
    made = [([FRAG], "any"), ([w[0], w[1], w[2]], "any"), ([w[3]], "all"), ([FRAG, w[2]], "all")]
    scopes = [idx.scope_terms(t, m) for t, m in made] + [idx.scope(listed)]
    ids = [model.term_ids(t, m) for t, m in made] + [listed]
    assert [s.rows for s in scopes] == [len(i) for i in ids]
    qs = np.arange(B, dtype=np.int32) % 5
    idx.set_option("mask_screen", 1)
    try:
        idx.reset_search_stats()
        rows, scores, counts = idx.search_in_scopes(q, _terms(texts), _syn().NOW_TICKS, 10, scopes, qs, candidate_limit=NA)
        assert idx.search_stats()["pass_mode"] == 6                        # ONE grouped screening pass
        for g in range(5):
            members = np.nonzero(qs == g)[0]
            own = _in_scope(idx, q[members], [texts[b] for b in members], 10, NA, scopes[g])
            assert _equal((rows[members], scores[members], counts[members]), own), g
            assert _equal(own, _masked(idx, q[members], [texts[b] for b in members], 10, NA, ids[g])), g
    finally:
        idx.set_option("mask_screen", 0)
        for s in scopes:
            s.close()


def test_combine_with_term_scopes():
    a = _shard_a()
    idx, model, w = a["idx"], a["model"], a["words"]
    # "contains none of": all rows ANDNOT ANY(terms)
    terms = [w[0], w[3], FRAG]
    none_of = idx.scope_ticks(I64_MIN, I64_MAX)
    assert none_of.rows == NA
    any_of = idx.scope_terms(terms, "any")
    none_of.andnot(any_of)
    held = ~(model.has(terms[0]) | model.has(terms[1]) | model.has(terms[2])) & ~model.dead
    assert 0 < held.sum() < NA // 2 and np.array_equal(none_of.row_ids(), model.ids[held])
    assert any_of.rows + none_of.rows == NA
    # ALL(a, b) == ALL(a) AND ALL(b); ANY(a, b) == ANY(a) OR ANY(b)
    for x, y in (([w[0]], [w[1]]), ([w[2]], [FRAG]), ([w[0], w[1]], [FRAG, w[0]])):
        both_all, both_any = idx.scope_terms(x + y, "all"), idx.scope_terms(x + y, "any")
        sx, sy = idx.scope_terms(x, "all"), idx.scope_terms(y, "all")
        sx.and_(sy)
        assert np.array_equal(both_all.row_ids(), sx.row_ids()) and np.array_equal(sx.row_ids(), model.term_ids(x + y, "all"))
        ox, oy = idx.scope_terms(x, "any"), idx.scope_terms(y, "any")
        ox.or_(oy)
        assert np.array_equal(both_any.row_ids(), ox.row_ids()) and np.array_equal(ox.row_ids(), model.term_ids(x + y, "any"))
        for s in (both_all, both_any, sx, sy, ox, oy):
            s.close()
    none_of.close()
    any_of.close()


def _one_lane_index(a):
    idx = _build(a["model"].emb, a["model"].created, a["model"].rowbytes, a["model"].ids, NA)
    idx.set_option("max_lanes", 1)                      # every call uses the index's own workspaces
    idx.set_option("two_stage", 1)
    return idx


def test_a_term_scope_leaves_the_lane_as_a_search_leaves_it():
    """The keyword chain ORs postings into term bitmaps that must start out zero, and counts into counters that must start out
    zero; a search cleans both up behind itself for the next one.  A term scope runs the same chain on the same lane: made from
    a fragment, it dirties dozens of postings' worth of bitmap -- the hybrid search behind it must return what it returns on
    an index that never made a scope, and so must the search after a search-scope-search sequence.  Every query of the search
    carries a 2-byte fragment in front of its three words: a whole word is read from its stored token bitmap, so only a term
    that EXPANDS meets what an earlier chain left in the batch's own bitmaps."""
    a = _shard_a()
    model, w = a["model"], a["words"]
    q = np.ascontiguousarray(a["q"], dtype=np.float32)
    frags = [bytes([ord("a"), d]) for d in b"bcdefghijklm"]
    kw = [[frags[b % len(frags)]] + list(t) for b, t in enumerate(_terms(a["texts"]))]      # 40 queries, a fragment and three words each
    now = _syn().NOW_TICKS

    def hybrid(idx, n=POOL_Q):
        return idx.search(q[:n], kw[:n], now, 10, candidate_limit=NA)

    fresh = _one_lane_index(a)
    want = hybrid(fresh)
    assert _equal(want, hybrid(fresh))
    fresh.close()
    assert (want[2] == 10).all()
    # scope, search: the scope's fragment is NOT the search's first one, and lands in the bitmap the search's first term expands into
    idx = _one_lane_index(a)
    sc = idx.scope_terms([b"cd"], "any")
    got = hybrid(idx)
    assert _equal(got, want)
    _check(sc, model, [b"cd"], "any")
    sc.close()
    idx.close()
    # search, scope, search -- scopes of more and of fewer distinct terms than the search in front of them
    idx = _one_lane_index(a)
    assert _equal(hybrid(idx, 2), tuple(x[:2] for x in want))
    s1 = idx.scope_terms(frags[::-1] + [w[0]], "any")
    s2 = idx.scope_terms([b"cd", w[1]], "all")
    assert _equal(hybrid(idx), want)
    _check(s1, model, frags + [w[0]], "any")
    _check(s2, model, [b"cd", w[1]], "all")
    s3 = idx.scope_terms([w[2]], "all")                 # ... and a scope behind a scope behind a search
    _check(s3, model, [w[2]], "all")
    assert _equal(hybrid(idx), want)
    for s in (s1, s2, s3):
        s.close()
    idx.close()


def test_hit_list_overflow_grows_the_list_and_runs_the_chain_again():
    a = _shard_a()
    model = a["model"]
    idx = _one_lane_index(a)
    idx.set_option("kw_hits_cap", 16)                   # the fragment matches dozens of vocabulary tokens
    idx.reset_search_stats()
    sc, st = _stats(idx, lambda: idx.scope_terms([FRAG], "any"))
    _check(sc, model, [FRAG], "any")                    # never a scope of a truncated hit list
    assert st["expand_hits"]["launches"] >= 2 and st["scope_terms_combine"]["launches"] >= 2, st      # the chain ran again
    ss = idx.search_stats()
    assert ss["kw_passes"] == 0 and ss["kw_hits_total"] == 0 and ss["passes"] == 0 and ss["searches"] == 0      # no search statistic moved
    # the list has grown and stays grown: the same scope again, and a SEARCH with the fragment as a term, need no second chain
    again, st = _stats(idx, lambda: idx.scope_terms([FRAG], "any"))
    assert st["expand_hits"]["launches"] == 1, st
    assert np.array_equal(again.row_ids(), sc.row_ids())
    idx.reset_search_stats()
    idx.search(np.ascontiguousarray(a["q"][:1], dtype=np.float32), [[FRAG]], _syn().NOW_TICKS, 10, candidate_limit=NA)
    assert idx.search_stats()["passes"] == 1            # with a 16-entry list it would have been 2
    sc.close()
    again.close()
    idx.close()


# ---- shard B -----------------------------------------------------------------------------------------------------------------

T20 = b"http://a.io/q?zq=123"
T40 = b"https://example.org/zq9/path?id=77&k=zzq"
ROWS_T20 = (5, 69_983, 69_990, 70_000)                  # the first word, the last full word, the partial last word, the last row
ROWS_T40 = (31, 69_952, 69_984, 70_000)
SHARED3 = b"://"                                        # in both planted tokens and in no vocabulary word
TERMS_B = {"3 bytes": SHARED3, "20 bytes": T20, "36 of 40 bytes": T40[2:38], "41 bytes": T40 + b"x"}


def _plant(rowbytes, rows20, rows40):
    """T20 over the row's first three words (bytes 0 .. 19, the space at 20 stays); T40 from byte 21 (a word's start) to 60, a
    space at 61, and a letter at 62 that joins the next word: single spaces throughout, no whitespace in a token"""
    assert len(T20) == 20 and len(T40) == 40 and rowbytes[0, 20] == 32 and rowbytes[0, 62] == 32 and rowbytes[0, 69] == 32
    for r in rows20:
        rowbytes[r, 0:20] = np.frombuffer(T20, np.uint8)
    for r in rows40:
        rowbytes[r, 21:61] = np.frombuffer(T40, np.uint8)
        rowbytes[r, 61], rowbytes[r, 62] = 32, ord("x")


def _shard_b(capacity=NB + 1000):
    emb, created, rowbytes = _rows(NB, DIM_B)
    _plant(rowbytes, ROWS_T20, ROWS_T40)
    ids = np.arange(NB, dtype=np.int64) * 3 + 11
    idx = _build(emb, created, rowbytes, ids, capacity)
    q, texts = _queries(DIM_B, NB)
    return idx, Model(emb, created, rowbytes, ids), q[:8], texts[:8]


def test_planted_tokens_at_the_borders_of_the_bitmap():
    assert NB % 32 == 17 and (NB - 1) // 32 == 2187 and 69_983 // 32 == 2186 and 69_984 // 32 == 2187
    idx, model, q, texts = _shard_b()
    ids = model.ids
    want = {"3 bytes": sorted(set(ROWS_T20) | set(ROWS_T40)), "20 bytes": sorted(ROWS_T20), "36 of 40 bytes": sorted(ROWS_T40), "41 bytes": []}
    for name, term in TERMS_B.items():
        for mode in ("all", "any"):
            sc, st = _stats(idx, lambda: idx.scope_terms([term], mode))
            got = _check(sc, model, [term], mode, name)
            assert np.array_equal(got, ids[want[name]]), name
            assert st["scope_terms_aliased"]["algo_bytes"] == 0           # no stored token bitmaps on this shard: every term expands
            sc.close()
    # which kernel found the long ones: tokens of 17 .. 32 bytes one lane each, longer ones by the wave-per-token scan
    _, st = _stats(idx, lambda: idx.scope_terms([T20, T40[2:38]], "any").close())
    assert st.get("vocab_match_mid", {}).get("launches", 0) == 1 and st.get("vocab_scan", {}).get("launches", 0) == 1, sorted(st)
    both = idx.scope_terms([T20, T40[2:38]], "all")
    assert np.array_equal(both.row_ids(), ids[[70_000]])                   # the last row, in the partial last word
    either = idx.scope_terms([T20, T40[2:38]], "any")
    assert np.array_equal(either.row_ids(), ids[want["3 bytes"]])
    # with words of the corpus: the tail of ALL's identity and the padding words must be clear -- rows() counts every set bit
    w = _syn().vocab_word(900)
    for terms, mode in (([w], "all"), ([w], "any"), ([w, FRAG], "any"), ([FRAG], "all")):
        sc = idx.scope_terms(terms, mode)
        _check(sc, model, terms, mode)
        sc.close()
    # searched: the scope of 7 rows, every query against the oracle on those rows
    got = _in_scope(idx, q, texts, 10, NB, either)
    _against_oracle(model, ids[want["3 bytes"]], got, q, texts, 10, NB, range(len(texts)), "planted")
    both.close()
    either.close()
    idx.close()


def test_maintenance_carries_a_term_scope():
    idx, model, q, texts = _shard_b()
    rng = np.random.default_rng(35)
    w = _syn().vocab_word(900)
    made = {"word": ([w], "all"), "planted": ([SHARED3], "any"), "fragment": ([FRAG, w], "all")}
    scopes = {k: idx.scope_terms(t, m) for k, (t, m) in made.items()}
    sets = {k: set(model.term_ids(t, m).tolist()) for k, (t, m) in made.items()}
    assert len(sets["word"]) > 1000 and len(sets["planted"]) == 7

    def check(what):
        for k, sc in scopes.items():
            want = model.ordered(sets[k])               # the rows that were in it and are still alive, in present order
            assert sc.rows == len(want) and np.array_equal(sc.row_ids(), want), (what, k)

    check("made")
    # delete some members and some non-members (planted rows at both ends among them)
    members = np.fromiter(sets["word"], np.int64)
    gone = np.unique(np.concatenate([members[:150], model.ids[[5, 70_000]], rng.choice(model.ids, 400, replace=False)]))
    assert idx.delete_rows(gone) == len(gone)
    model.delete(gone)
    check("deleted")
    assert scopes["planted"].rows == len(model.ordered(sets["planted"])) <= 5
    # a term scope made now, before compaction, holds no deleted row: the posting lists still do
    fresh = idx.scope_terms([w], "all")
    assert np.array_equal(fresh.row_ids(), model.term_ids([w], "all")) and fresh.rows == scopes["word"].rows
    assert not np.isin(gone, fresh.row_ids()).any()
    fresh.close()
    # compact after 9,000 deletes in all
    more = rng.choice(model.ids[~model.dead], 9_000 - len(gone), replace=False)
    assert idx.delete_rows(more) == len(more)
    model.delete(more)
    check("deleted more")
    assert idx.compact() == 9_000
    model.compact()
    check("compacted")
    # update_rows touches nothing
    before = {k: s.row_ids() for k, s in scopes.items()}
    target = int(before["word"][len(before["word"]) // 2])
    assert idx.update_rows([target], np.ascontiguousarray(q[:1] * np.float32(0.5))) == 1
    model.emb[int(np.nonzero(model.ids == target)[0][0])] = q[0] * np.float32(0.5)
    for k, s in scopes.items():
        assert np.array_equal(s.row_ids(), before[k]), k
    # insert 131 rows whose text contains the terms: NOT in the old scopes; a NEW scope_terms holds them
    emb, _, rowbytes = _rows(131, DIM_B, row0=5_000_000)
    _plant(rowbytes, range(131), ())
    rowbytes[:, 21:27] = np.frombuffer(w, np.uint8)     # the fourth word of every new row, behind the planted token
    c = model.created
    mid = c[rng.choice(len(c), 51, replace=False)].copy()
    mid[::2] -= 3
    created = np.concatenate([c[0] + 1 + np.arange(40), mid, c[-1] - 1 - np.arange(40)]).astype(np.int64)
    new_ids = 10_000_000 + np.arange(131, dtype=np.int64)
    width = rowbytes.shape[1]
    assert idx.insert_rows(emb, created, rowbytes.reshape(-1), np.arange(132, dtype=np.uint64) * width, row_ids=new_ids) == 131
    model.insert(emb, created, rowbytes, new_ids)
    check("inserted")
    for k, sc in scopes.items():
        assert not np.isin(new_ids, sc.row_ids()).any(), k
    for k, (t, m) in made.items():
        if k == "fragment":
            continue
        new = idx.scope_terms(t, m)
        got = _check(new, model, t, m, ("made after the insert", k))
        assert np.isin(new_ids, got).all() and len(got) == len(model.ordered(sets[k])) + 131, k
        if k == "word":                                 # ... and it is searched like any other, against the oracle
            _against_oracle(model, got, _in_scope(idx, q, texts, 10, NB + 1000, new), q, texts, 10, NB + 1000, (0, 5), k)
        new.close()
    got = _in_scope(idx, q, texts, 10, NB + 1000, scopes["word"])
    assert _equal(got, _masked(idx, q, texts, 10, NB + 1000, model.ordered(sets["word"])))
    for s in scopes.values():
        s.close()
    idx.close()


def test_views_orphans_and_an_unsealed_index():
    P = pkg()
    idx, model, q, texts = _shard_b()
    w = _syn().vocab_word(900)
    want_ids = model.term_ids([w], "all")
    view = idx.view()
    on_owner, on_view = idx.scope_terms([w], "all"), view.scope_terms([w], "all")
    assert np.array_equal(on_view.row_ids(), want_ids) and np.array_equal(on_owner.row_ids(), want_ids)
    want = _masked(idx, q, texts, 10, NB, want_ids)
    for handle, sc in ((idx, on_view), (view, on_owner), (view, on_view), (idx, on_owner)):
        assert _equal(_in_scope(handle, q, texts, 10, NB, sc), want)
    on_view.close()
    view.close()
    idx.close()                                         # the index goes first: the scope is orphaned
    assert on_owner.rows == -1
    for call in (lambda: on_owner.row_ids(), lambda: on_owner.and_(on_owner)):
        with pytest.raises(P.native.OrrError) as e:
            call()
        assert e.value.code == P.native.ORR_ESTATE
    on_owner.close()
    # an index that is not sealed: ORR_ESTATE, after every argument error
    emb, created, rowbytes = _rows(64, DIM_B)
    raw = P.RecallIndex(dim=DIM_B, capacity_rows=64)
    raw.append(emb, created, rowbytes.reshape(-1), np.arange(65, dtype=np.int64) * rowbytes.shape[1], row_ids=np.arange(64, dtype=np.int64))
    with pytest.raises(P.native.OrrError) as e:
        raw.scope_terms([w], "all")
    assert e.value.code == P.native.ORR_ESTATE
    with pytest.raises(P.native.OrrError) as e:
        raw.scope_terms([w, b""], "all")
    assert e.value.code == P.native.ORR_EINVAL
    with pytest.raises(ValueError):
        raw.scope_terms([w], "both")
    raw.close()


def test_four_threads_create_and_search_term_scopes_on_one_handle():
    idx, model, q, texts = _shard_b()
    syn = _syn()
    jobs = [([syn.vocab_word(900 + 7 * i)], "all") for i in range(2)] + [([FRAG, syn.vocab_word(33)], "any"), ([SHARED3], "any")]
    want_ids = [model.term_ids(t, m) for t, m in jobs]
    want = [_masked(idx, q, texts, 10, NB, ids) for ids in want_ids]
    bad = []

    def work(i):
        terms, mode = jobs[i]
        for _ in range(4):
            sc = idx.scope_terms(terms, mode)
            if not np.array_equal(sc.row_ids(), want_ids[i]) or not _equal(_in_scope(idx, q, texts, 10, NB, sc), want[i]):
                bad.append(i)
            sc.close()

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not bad
    assert _equal(_search(idx, q, texts, 10, NB), _search(idx, q, texts, 10, NB))
    idx.close()
