"""Cluster scope handles (orr_cluster_scope) at work: one orr_scope per shard behind one handle, the search inside one
(orr_cluster_search_batch_in_scope) and the shard form it drives (orr_search_shard_in_scope).  The contract: what
orr_search_batch_in_scope returns on ONE index that holds all the cluster's rows with the same set of rows as its scope -- so
every result is compared with search_in_scope of the twin scope on one RecallIndex built from the same rows, with the id-list
cluster call (search_masked with scope.row_ids()) where the scope's ids are distinct, and a stated subset with the oracle on
the sub-corpus.  Every comparison is exact: rows and counts with np.array_equal, fp64 scores bit for bit, NaN = NaN.

Shards are several "devices" on ordinal 0.  The small cluster (1,000 / 2,700 / 2,300 rows x 64, 200 rows deleted, one id on two
shards) and the large one (2 x 200,000 x 128, "mask_screen" = 1, the planted tie and mass of the ladder test) are
tests/test_gpu_cluster_scope.py's own fixtures, built once per session and only read here; the maintenance and lifetime tests
build their own clusters, which they change."""
import threading

import numpy as np
import pytest

import test_gpu_cluster_scope as base
import test_gpu_scope_handle as hbase
from helpers import NOW, orc, pkg

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
TEXTS, CUTS = base.TEXTS, base.CUTS
TWO_STAGE = base.TWO_STAGE
_same, _equal = base._same, base._same_results


def _terms(texts):
    P = pkg()
    return [P.text.query_terms(t) for t in texts]


def _raises(code, call):
    P = pkg()
    with pytest.raises(P.native.OrrError) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


# ---- 1. semantics: three small shards -----------------------------------------------------------------------------------------

class SmallRows:
    """The small fixture by ROWS: which live positions a scope holds, restated with numpy."""

    def __init__(self, model):
        P = pkg()
        self.m = model
        n = len(model.ids)
        self.live = np.ones(n, bool)
        self.live[np.fromiter(model.deleted, np.int64)] = False
        lower = [P.text.lower_invariant(s) for s in model.contents]
        self.lower = [x if isinstance(x, bytes) else x.encode("utf-8") for x in lower]

    def of_ids(self, ids):
        return np.nonzero(np.isin(self.m.ids, np.asarray(ids, np.int64)) & self.live)[0]

    def of_ticks(self, t0, t1):
        if t0 >= t1:
            return np.zeros(0, np.int64)
        upper = np.ones(len(self.live), bool) if t1 == I64_MAX else self.m.created < t1
        return np.nonzero((self.m.created >= t0) & upper & self.live)[0]

    def of_terms(self, terms, mode):
        if not terms:
            return np.zeros(0, np.int64)
        fold = all if mode == "all" else any
        hit = np.array([len(c) > 0 and fold(t in c for t in terms) for c in self.lower])
        return np.nonzero(hit & self.live)[0]

    def corpus(self, keep):
        m = self.m
        return orc.OracleCorpus([m.emb[r] for r in keep], m.created[keep], [m.contents[r] for r in keep])


_S = {}


def _small():
    """(cluster, single index, SmallRows, query vectors, cases); a case: (name, kind, argument)."""
    if _S:
        return _S["v"]
    cl, one, model, id_scopes, qs = base._small()
    c = model.created
    cases = [(name, "ids", ids) for name, ids in id_scopes.items()]
    cases += [
        ("window inside shard 1", "ticks", (int(c[3000]), int(c[1500]) + 1)),
        ("window = shard 1 exactly", "ticks", (int(c[CUTS[2] - 1]), int(c[CUTS[1]]) + 1)),
        ("window ending at the first shard border", "ticks", (int(c[CUTS[1] - 1]), int(c[500]) + 1)),
        ("window across both borders", "ticks", (int(c[4000]), int(c[800]) + 1)),
        ("both ends open", "ticks", (I64_MIN, I64_MAX)),
        ("open towards the old", "ticks", (I64_MIN, int(c[2000]))),
        ("open towards the new", "ticks", (int(c[2000]), I64_MAX)),
        ("inverted window", "ticks", (int(c[100]), int(c[200]))),
        ("all of two terms", "terms", ([b"kubernetes", b"helm"], "all")),
        ("any of three terms", "terms", ([b"azure", b"cosmos", "été".encode("utf-8")], "any")),
        ("a term matching nothing", "terms", ([b"qqqqzz"], "any")),
        ("all with a term matching nothing", "terms", ([b"azure", b"qqqqzz"], "all")),
        ("no terms", "terms", ([], "all")),
    ]
    _S["v"] = (cl, one, SmallRows(model), qs, cases)
    return _S["v"]


def _make(target, kind, arg):
    if kind == "ids":
        return target.scope(arg)
    if kind == "ticks":
        return target.scope_ticks(*arg)
    return target.scope_terms(*arg)


def _positions(rows, kind, arg):
    return {"ids": rows.of_ids, "ticks": lambda a: rows.of_ticks(*a), "terms": lambda a: rows.of_terms(*a)}[kind](arg)


def test_rows_and_row_ids_of_every_small_scope():
    P = pkg()
    cl, one, rows, qs, cases = _small()
    for name, kind, arg in cases:
        sc, twin = _make(cl, kind, arg), _make(one, kind, arg)
        keep = _positions(rows, kind, arg)
        want = rows.m.ids[keep]
        assert sc.rows == len(keep) == twin.rows, (name, sc.rows, len(keep))
        parts = [sc.shard(g) for g in range(3)]
        assert sc.rows == sum(p.rows for p in parts), name
        assert [p.rows for p in parts] == [int(((keep >= CUTS[g]) & (keep < CUTS[g + 1])).sum()) for g in range(3)], name
        got = sc.row_ids()
        assert np.array_equal(got, want) and np.array_equal(got, twin.row_ids()), name
        assert np.array_equal(np.concatenate([p.row_ids() for p in parts]), want), name     # shard 0's, then shard 1's, ...
        if len(keep) > 0:                                                    # a cap one too small
            buf = np.full(len(keep) + 4, 7, np.int64)
            n = P.native.C.c_int64(-5)
            r = P.native.hip.orr_cluster_scope_row_ids(sc._h, len(keep) - 1, buf.ctypes.data, P.native.C.cast(P.native.C.byref(n), P.native.C.c_void_p))
            assert r == P.native.ORR_EINVAL and n.value == len(keep), (name, r, n.value)
            assert (buf[len(keep) - 1:] == 7).all(), name                    # nothing beyond cap
            assert (buf == 7).all(), name                                    # ... and, as documented, nothing at all
        with pytest.raises(P.native.OrrError):
            sc.shard(3)
        sc.close()
        twin.close()
    assert {"an id on two shards", "empty", "inverted window", "no terms"} <= {c[0] for c in cases}
    both = rows.of_ids([500])
    assert list(both) == [500, 2000]                                         # the id on two shards brings both rows


_SMALL_ORACLE_CASES = ("wide", "an id on two shards", "window inside shard 1", "window across both borders", "any of three terms")


@pytest.mark.parametrize("with_vectors", [True, False])
@pytest.mark.parametrize("B", [1, 4])
def test_small_cluster_in_scope_equals_one_index_the_masked_call_and_the_oracle(B, with_vectors):
    cl, one, rows, qs, cases = _small()
    q = qs.copy()
    q[3] = 0.0                                                               # a zero query vector
    q = np.ascontiguousarray(q[4 - B:]) if with_vectors else None            # (B = 1: the zero vector alone)
    texts = TEXTS[4 - B:]
    terms = _terms(texts)
    n = CUTS[-1]
    wide = next(a for name, k, a in cases if name == "wide")
    live = [len(rows.of_ids(wide)[(rows.of_ids(wide) >= CUTS[g]) & (rows.of_ids(wide) < CUTS[g + 1])]) for g in range(3)]
    assert live[0] < 300 < live[0] + live[1]                                 # the 300-row limit ends inside the second shard
    compared = against_masked = against_oracle = 0
    for name, kind, arg in cases:
        sc, twin = _make(cl, kind, arg), _make(one, kind, arg)
        keep = _positions(rows, kind, arg)
        ids = sc.row_ids()
        distinct = 500 not in ids                                            # (not the scopes holding the id that sits on two shards)
        corpus = rows.corpus(keep) if name in _SMALL_ORACLE_CASES else None
        for topk in (1, 10, 100, -1):
            for limit in (1, 300, n):
                what = (name, B, with_vectors, topk, limit)
                got = cl.search_in_scope(q, terms, NOW, topk, sc, candidate_limit=limit)
                assert _equal(got, one.search_in_scope(q, terms, NOW, topk, twin, candidate_limit=limit)), what
                compared += 1
                if distinct:
                    assert _equal(got, cl.search_masked(q, terms, NOW, topk, ids, candidate_limit=limit)), what
                    against_masked += 1
                rws, scores, counts = got
                assert (counts == min(max(1, topk), len(keep), max(1, limit))).all(), what
                if corpus is not None and topk in (10, -1):
                    for b, text in enumerate(texts):
                        orow, osc, _ = corpus.search([] if q is None else q[b], text, NOW, max(1, topk), candidate_limit=limit)
                        k = int(counts[b])
                        assert list(rws[b, :k]) == [int(rows.m.ids[keep[r]]) for r in orow], what + (b,)
                        assert _same(scores[b, :k], np.asarray(osc)), what + (b,)
                        assert (rws[b, k:] == -1).all()
                        against_oracle += 1
        sc.close()
        twin.close()
    assert compared == 12 * len(cases) and against_masked >= 12 * 8 and against_oracle == 6 * B * len(_SMALL_ORACLE_CASES)


# ---- 2. combine and add_ids ---------------------------------------------------------------------------------------------------

def _tiny_cluster(n_per=300, shards=2, dim=64, seal=True):
    P, syn = pkg(), hbase._syn()
    n = n_per * shards
    emb, created, rowbytes = hbase._rows(n, dim)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    off = np.arange(n_per + 1, dtype=np.int64) * syn.ROW_BYTES
    cl = P.RecallCluster([0] * shards, dim)
    for g in range(shards):
        r0, r1 = g * n_per, (g + 1) * n_per
        cl.shard(g).append(emb[r0:r1], created[r0:r1], rowbytes[r0:r1].reshape(-1), off, row_ids=ids[r0:r1])
    if seal:
        cl.seal()
    return cl, ids


def test_combine_and_add_ids_against_numpy_set_operations():
    P = pkg()
    cl, one, rows, qs, cases = _small()
    by_name = {name: (kind, arg) for name, kind, arg in cases}
    ids_of = lambda keep: rows.m.ids[np.sort(keep)]                          # the global candidate order is the position order
    pairs = [("wide", "window across both borders"), ("any of three terms", "open towards the old"), ("one shard only", "wide"),
             ("window inside shard 1", "empty"), ("both ends open", "any of three terms")]
    ops = {"and_": np.intersect1d, "or_": np.union1d, "andnot": np.setdiff1d}
    for left, right in pairs:
        for op, fold in ops.items():
            a, b = _make(cl, *by_name[left]), _make(cl, *by_name[right])
            pa, pb = _positions(rows, *by_name[left]), _positions(rows, *by_name[right])
            assert getattr(a, op)(b) is a
            want = fold(pa, pb)
            assert a.rows == len(want) and np.array_equal(a.row_ids(), ids_of(want)), (left, op, right)
            assert np.array_equal(b.row_ids(), ids_of(pb)), (left, op, right)     # src is unchanged
            ia, ib = ids_of(pa), ids_of(pb)
            if len(np.unique(ia)) == len(ia) and len(np.unique(ib)) == len(ib):     # distinct ids: the same on row_ids() alone
                assert np.array_equal(np.sort(a.row_ids()), fold(ia, ib)), (left, op, right)
            a.close()
            b.close()
    # "contains none of": all rows ANDNOT the ANY scope; src == dst
    terms = by_name["any of three terms"][1]
    none_of, any_of = cl.scope_ticks(I64_MIN, I64_MAX), cl.scope_terms(*terms)
    none_of.andnot(any_of)
    want = np.setdiff1d(np.nonzero(rows.live)[0], rows.of_terms(*terms))
    assert np.array_equal(none_of.row_ids(), ids_of(want)) and len(want) > 0
    got = cl.search_in_scope(qs, _terms(TEXTS), NOW, 10, none_of, candidate_limit=CUTS[-1])
    twin = one.scope(ids_of(want))                                           # (ids 500 / 2000: both rows are in or out together? no: by rows)
    if len(np.unique(ids_of(want))) == len(want) and 500 not in ids_of(want):
        assert _equal(got, one.search_in_scope(qs, _terms(TEXTS), NOW, 10, twin, candidate_limit=CUTS[-1]))
    twin.close()
    any_of.and_(any_of)
    assert any_of.rows == len(rows.of_terms(*terms))
    any_of.andnot(any_of)
    assert any_of.rows == 0 and len(any_of.row_ids()) == 0
    # add_ids: the number of rows newly added, over all shards
    grow = cl.scope(rows.m.ids[[10, 1500]])
    assert grow.rows == 2
    more = rows.m.ids[[10, 20, 1500, 1600, 3800, 5999]]
    fresh = len(np.setdiff1d(rows.of_ids(more), rows.of_ids(rows.m.ids[[10, 1500]])))
    assert grow.add_ids(np.concatenate([more, [-4, 2 ** 41]])) == fresh and grow.add_ids(more) == 0
    assert np.array_equal(grow.row_ids(), ids_of(rows.of_ids(more)))
    assert grow.add_ids([500]) == 2 and grow.shard(0).rows + grow.shard(1).rows + grow.shard(2).rows == grow.rows   # the id on two shards
    dead = rows.m.ids[np.nonzero(~rows.live)[0][:5]]
    assert grow.add_ids(dead) == 0                                            # a deleted row is never in a scope
    # two clusters
    other, other_ids = _tiny_cluster()
    foreign = other.scope(other_ids[:50])
    for op in ("and_", "or_", "andnot"):
        _raises(P.native.ORR_EINVAL, lambda: getattr(grow, op)(foreign))
        assert b"different clusters" in P.native.hip.orr_last_error()
        _raises(P.native.ORR_EINVAL, lambda: getattr(foreign, op)(grow))
    _raises(P.native.ORR_EINVAL, lambda: cl.search_in_scope(qs, _terms(TEXTS), NOW, 10, foreign))
    assert b"another cluster" in P.native.hip.orr_last_error()
    _raises(P.native.ORR_EINVAL, lambda: cl.shard(1).search_shard_in_scope(qs, _terms(TEXTS), NOW, 8, 300, grow.shard(0)))
    assert b"another shard" in P.native.hip.orr_last_error()
    assert foreign.rows == 50
    for s in (none_of, any_of, grow, foreign):
        s.close()
    other.close()


# ---- 3. the screen, and what no longer runs: two shards of 200,000 x 128 -------------------------------------------------------

HALF, N, DIM = base.HALF, base.N, base.DIM
_B = {}


def _word_rows(rowbytes, words):
    """rows (positions) whose content holds one of the 6-letter words as a token"""
    import torch
    syn = hbase._syn()
    rb = torch.from_numpy(np.ascontiguousarray(rowbytes)).cuda()
    rb = torch.cat([rb, torch.full((rb.shape[0], 1), 32, dtype=torch.uint8, device="cuda")], dim=1)
    tok = rb.reshape(rb.shape[0], syn.TOKENS_PER_ROW, syn.WORD_LEN + 1)[:, :, :syn.WORD_LEN]
    hit = torch.zeros(rb.shape[0], dtype=torch.bool, device="cuda")
    for w in words:
        hit |= (tok == torch.tensor(list(w), dtype=torch.uint8, device="cuda")).all(dim=2).any(dim=1)
    return np.nonzero(hit.cpu().numpy())[0]


def _big():
    """The large cluster and its twin with three scopes each: (cluster scope, twin scope, the positions it holds)."""
    if _B:
        return _B["v"]
    syn = hbase._syn()
    cl, one, model, texts, fam, plants, tie_vec, mass_vec = base._big()
    rng = np.random.default_rng(4242)
    pick = np.sort(rng.choice(N, 100_000, replace=False))
    t0, t1 = int(model.created[399_000]), int(model.created[100_000])   # (shard 1's part ends behind row 196,608: it can screen)
    window = np.nonzero((model.created >= t0) & (model.created < t1))[0]
    words = [syn.vocab_word(t) for t in (17, 1203, 2999, 4001)]
    held = _word_rows(model.rowbytes, words)
    scopes = {
        "100,000 ids over both shards": (cl.scope(model.ids[pick]), one.scope(model.ids[pick]), pick),
        "a time window over the border": (cl.scope_ticks(t0, t1), one.scope_ticks(t0, t1), window),
        "any of four terms": (cl.scope_terms(words, "any"), one.scope_terms(words, "any"), held),
    }
    _B["v"] = (cl, one, model, texts, plants["random 10 %"][0], scopes)
    return _B["v"]


def test_the_large_scopes_hold_the_rows_the_model_says():
    cl, one, model, texts, q_all, scopes = _big()
    for name, (sc, twin, keep) in scopes.items():
        assert sc.rows == len(keep) == twin.rows, (name, sc.rows, len(keep))
        assert sc.shard(0).rows == int((keep < HALF).sum()) and sc.shard(1).rows == int((keep >= HALF).sum()), name
        assert sc.shard(0).rows > 0 and sc.shard(1).rows > 0, name
        got = sc.row_ids()
        assert np.array_equal(got, model.ids[keep]) and np.array_equal(got, twin.row_ids()), name
    assert 20_000 < scopes["any of four terms"][0].rows < 80_000


def _reset(cl):
    cl.search_stats(reset=True)
    for g in range(cl.n_shards):
        cl.shard(g).reset_search_stats()


@pytest.mark.parametrize("B", [1, 8, 40])
def test_two_stage_cluster_in_scope_equals_one_index_and_the_oracle(B):
    syn = hbase._syn()
    cl, one, model, texts_all, q_all, scopes = _big()
    texts = list(texts_all[:B])
    terms = _terms(texts)
    q = np.ascontiguousarray(q_all[:B])
    for name, (sc, twin, keep) in scopes.items():
        live0 = sc.shard(0).rows
        for limit in (300, 150_000, sc.rows, live0 + 1000):
            for topk in (1, 10, 64):
                what = (name, B, topk, limit)
                _reset(cl)
                got = cl.search_in_scope(q, terms, syn.NOW_TICKS, topk, sc, candidate_limit=limit)
                st = [cl.shard(g).search_stats() for g in range(2)]
                assert _equal(got, one.search_in_scope(q, terms, syn.NOW_TICKS, topk, twin, candidate_limit=limit)), what
                assert (got[2] == min(topk, len(keep), limit)).all(), what
                if topk == 64:                                                # k' = 86 is beyond a selection list: the list path from
                    for g in (0, 1):                                          # the first rung on (cscope::first_rung), as on one index
                        assert st[g]["pass_mode"] == 4 or st[g]["passes"] == 0, what + (g, st[g])
                elif limit == sc.rows:                                        # both shards screen their whole scope
                    for g in (0, 1):
                        assert st[g]["pass_mode"] == 5 and st[g]["survivor_samples"] > 0 and st[g]["exact_pass_queries"] == 0, what + (g, st[g])
                elif limit == live0 + 1000:                                   # shard 1 is clipped to 1,000 rows: the list path
                    assert st[0]["pass_mode"] == 5 and st[0]["survivor_samples"] > 0, what + (st[0],)
                    assert st[1]["pass_mode"] == 4 and st[1]["survivor_samples"] == 0, what + (st[1],)
                elif limit == 300:                                            # used up inside shard 0: shard 1 runs no pass
                    assert st[1]["passes"] == 0 and st[1]["searches"] >= 1, what + (st[1],)
    # a stated subset against the oracle: the id scope at B = 8, topk 10, limits rows and 300; the term scope at limit rows
    if B == 8:
        for name, limits in (("100,000 ids over both shards", (100_000, 300)), ("any of four terms", (N,))):
            sc, twin, keep = scopes[name]
            width = model.rowbytes.shape[1]
            corpus = orc.OracleCorpus(np.ascontiguousarray(model.emb[keep]), model.created[keep],
                                      (np.ascontiguousarray(model.rowbytes[keep]).reshape(-1), np.arange(len(keep) + 1, dtype=np.int64) * width))
            for limit in limits:
                rows, scores, counts = cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, sc, candidate_limit=limit)
                for b in (0, 3, 7):
                    orow, osc, _ = corpus.search(q[b], texts[b], syn.NOW_TICKS, 10, candidate_limit=limit, threads=16)
                    k = int(counts[b])
                    assert list(rows[b, :k]) == [int(model.ids[keep[r]]) for r in orow], (name, limit, b)
                    assert _same(scores[b, :k], np.asarray(osc)), (name, limit, b)


def _launches(cl, fn):
    """the launch counts of every shard's kernels across fn()"""
    for g in range(cl.n_shards):
        cl.shard(g).set_profiling(True)
    fn()
    out = []
    for g in range(cl.n_shards):
        out.append({k: v["launches"] for k, v in cl.shard(g).kernel_stats().items()})
        cl.shard(g).set_profiling(False)
    return out


RESOLVE = ("scope_lookup", "scope_counts", "scope_handle_lookup")


def test_no_count_step_and_no_resolve_on_the_handle_path():
    syn = hbase._syn()
    cl, one, model, texts_all, q_all, scopes = _big()
    q, terms = np.ascontiguousarray(q_all[:8]), _terms(texts_all[:8])
    sc, twin, keep = scopes["100,000 ids over both shards"]
    ids = model.ids[keep]
    live0 = sc.shard(0).rows
    search = lambda limit: cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, sc, candidate_limit=limit)
    # the id-list call shows all three on every shard, twice over (the count step, then the pass): the check is not vacuous
    st = _launches(cl, lambda: cl.search_masked(q, terms, syn.NOW_TICKS, 10, ids, candidate_limit=N))
    for g in (0, 1):
        assert st[g].get("scope_lookup", 0) >= 2 and st[g].get("scope_counts", 0) >= 2 and st[g].get("mask_clip", 0) >= 1, (g, sorted(st[g]))
    # the limit reaches every row: no lookup, no count, no clip, and the masked screen did run
    for limit in (N, sc.rows):
        st = _launches(cl, lambda: search(limit))
        for g in (0, 1):
            assert not any(k in st[g] for k in RESOLVE + ("mask_clip",)), (limit, g, sorted(st[g]))
            assert "mask_survivors" in st[g], (limit, g, sorted(st[g]))
    # the limit ends inside shard 1: exactly one clip there, none on shard 0 (whose every row takes part)
    st = _launches(cl, lambda: search(live0 + 1000))
    assert st[1].get("mask_clip", 0) == 1 and "mask_clip" not in st[0], (sorted(st[0]), sorted(st[1]))
    assert not any(k in st[g] for k in RESOLVE for g in (0, 1))
    # ... inside shard 0: one clip there; shard 1 lets no row take part and launches nothing of the kind
    st = _launches(cl, lambda: search(live0 - 1000))
    assert st[0].get("mask_clip", 0) == 1 and "mask_clip" not in st[1], (sorted(st[0]), sorted(st[1]))
    assert not any(k in st[g] for k in RESOLVE for g in (0, 1))
    # the time window and the term scope likewise
    for name in ("a time window over the border", "any of four terms"):
        other = scopes[name][0]
        st = _launches(cl, lambda: cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, other, candidate_limit=N))
        for g in (0, 1):
            assert not any(k in st[g] for k in RESOLVE + ("mask_clip",)) and "mask_survivors" in st[g], (name, g, sorted(st[g]))


# ---- 4. the ladder --------------------------------------------------------------------------------------------------------------

def test_the_ladder_a_tie_at_the_cut_and_an_overflow_on_one_shard():
    syn = hbase._syn()
    cl, one, model, texts_all, fam, plants, tie_vec, mass_vec = base._big()
    name = "older half of each shard"
    B = 8
    q = np.ascontiguousarray(plants[name][0][:B]).copy()
    q[2] = tie_vec                                                            # equal to the 70 rows of one timestamp in shard 0: a tie at the cut
    q[5] = mass_vec                                                           # parallel to 20,000 rows of shard 1 only: its survivors overflow there
    terms = _terms(texts_all[:B])
    ids = model.ids[fam[name]]
    assert set(model.ids[base.TIE]) <= set(ids) and set(model.ids[base.MASS]) <= set(ids)
    sc, twin = cl.scope(ids), one.scope(ids)
    window = (int(model.created[N - 1]), int(model.created[HALF // 2]) + 1)  # a window that holds the tie and the mass too
    sc_w, twin_w = cl.scope_ticks(*window), one.scope_ticks(*window)
    for s, t in ((sc, twin), (sc_w, twin_w)):
        _reset(cl)
        got = cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, s, candidate_limit=N)
        st = cl.search_stats()
        assert _equal(got, one.search_in_scope(q, terms, syn.NOW_TICKS, 10, t, candidate_limit=N))
        rows = got[0]
        assert set(rows[2]) <= set(model.ids[base.TIE]) and list(rows[2]) == sorted(rows[2])      # the ties in candidate order
        assert set(rows[5]) <= set(model.ids[base.MASS])
        assert st["requeried"] > 0 and st["passes"] >= 2, st                                      # k' had to grow
    assert _equal(cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, sc, candidate_limit=N),
                  cl.search_masked(q, terms, syn.NOW_TICKS, 10, ids, candidate_limit=N))
    for s in (sc, twin, sc_w, twin_w):
        s.close()


# ---- 5. the shard form, driven by hand ----------------------------------------------------------------------------------------

def _merged(P, shards, parts, q, terms, now, topk, limit, dim, shard_pass, by_ids=False, kp=32, kp_max=1 << 16):
    """The loop a multi-shard caller of the shard form runs: the lives from the handles, prefix sums, search, merge, escalate."""
    live = np.array([p.rows for p in parts], np.int64)
    before = np.concatenate([[0], np.cumsum(live)[:-1]])
    took = np.minimum(live, np.maximum(0, max(1, limit) - before))
    while True:
        if by_ids:
            recs = np.stack([s.search_shard_masked(q, terms, now, kp, limit, p.row_ids(), scope_before=int(before[g]), topk=topk, shard_pass=shard_pass)
                             for g, (s, p) in enumerate(zip(shards, parts))])
        else:
            recs = np.stack([s.search_shard_in_scope(q, terms, now, kp, limit, p, scope_before=int(before[g]), topk=topk, shard_pass=shard_pass)
                             for g, (s, p) in enumerate(zip(shards, parts))])
        rows, scores, counts, unc = P.merge_candidates(recs, dim, q, terms, now, topk)
        if unc == 0 or kp >= kp_max:
            break
        kp *= 4
    assert unc == 0
    return (rows, scores, counts), recs, kp, took


def test_shard_form_on_three_small_shards():
    P = pkg()
    cl, one, rows, qs, cases = _small()
    shards = [cl.shard(g) for g in range(3)]
    terms = _terms(TEXTS)
    for name, kind, arg in cases:
        if name not in ("wide", "one shard only", "empty", "window across both borders", "any of three terms"):
            continue
        sc = _make(cl, kind, arg)
        parts = [sc.shard(g) for g in range(3)]
        for topk, limit in ((10, 300), (10, 6000), (5, 1), (100, 6000)):
            what = (name, topk, limit)
            kp0 = 32 if topk < 64 else 128
            got, recs, kp, took = _merged(P, shards, parts, qs, terms, NOW, topk, limit, 64, 0, kp=kp0)
            trailers = recs[:, :, kp]
            assert ((trailers["flags"] & base.TRAILER) != 0).all()
            assert np.array_equal(trailers["order_key"], np.repeat(took[:, None], len(TEXTS), axis=1)), what
            valid = recs[:, :, :kp]["row_id"] >= 0
            assert np.array_equal(valid.sum(axis=2), trailers["matches"]), what
            assert _equal(got, cl.search_in_scope(qs, terms, NOW, topk, sc, candidate_limit=limit)), what
            again, recs1, kp1, _ = _merged(P, shards, parts, qs, terms, NOW, topk, limit, 64, 1, kp=kp0)
            assert _equal(got, again), what                                   # pass = 1: the same merged result
            by_ids, recs_ids, kp2, _ = _merged(P, shards, parts, qs, terms, NOW, topk, limit, 64, 0, by_ids=True, kp=kp0)
            assert kp2 == kp and recs_ids.tobytes() == recs.tobytes(), what    # record for record what the id-list shard call writes
        sc.close()


def test_shard_form_on_the_two_stage_shards():
    P, syn = pkg(), hbase._syn()
    cl, one, model, texts_all, q_all, scopes = _big()
    B = 8
    terms = _terms(texts_all[:B])
    q = np.ascontiguousarray(q_all[:B])
    shards = [cl.shard(0), cl.shard(1)]
    sc, twin, keep = scopes["100,000 ids over both shards"]
    parts = [sc.shard(0), sc.shard(1)]
    live0 = parts[0].rows
    for limit, screens in ((N, (True, True)), (live0 + 1000, (True, False))):
        got, recs, kp, took = _merged(P, shards, parts, q, terms, syn.NOW_TICKS, 10, limit, DIM, 0)
        trailers = recs[:, :, kp]
        assert np.array_equal(trailers["order_key"], np.repeat(took[:, None], B, axis=1)), limit
        if limit != N:
            assert list(took) == [live0, 1000]
        for g, screened in enumerate(screens):
            assert (((trailers[g]["flags"] & TWO_STAGE) != 0) == screened).all(), (limit, g)      # exactly where the screen ran
        assert _equal(got, cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, sc, candidate_limit=limit)), limit
        again, recs1, kp1, _ = _merged(P, shards, parts, q, terms, syn.NOW_TICKS, 10, limit, DIM, 1)
        assert ((recs1[:, :, kp1]["flags"] & TWO_STAGE) == 0).all()
        assert _equal(got, again), limit
        by_ids, recs_ids, kp2, _ = _merged(P, shards, parts, q, terms, syn.NOW_TICKS, 10, limit, DIM, 0, by_ids=True)
        assert kp2 == kp and recs_ids.tobytes() == recs.tobytes(), limit        # record for record the id-list shard call's


# ---- 6. maintenance: three shards of 23,000 x 64 -------------------------------------------------------------------------------

NM, CUT_M, DIM_M = 69_000, 23_000, 64


def test_scopes_follow_delete_compact_and_insert():
    P, syn = pkg(), hbase._syn()
    emb, created, rowbytes = hbase._rows(NM, DIM_M)
    ids = np.arange(NM, dtype=np.int64) * 3 + 11
    model = hbase.Model(emb, created, rowbytes, ids)
    off = np.arange(CUT_M + 1, dtype=np.int64) * syn.ROW_BYTES
    cl = P.RecallCluster([0, 0, 0], DIM_M, capacity_rows_per_shard=CUT_M + 1000)
    for g in range(3):
        r0, r1 = g * CUT_M, (g + 1) * CUT_M
        cl.shard(g).append(emb[r0:r1], created[r0:r1], rowbytes[r0:r1].reshape(-1), off, row_ids=ids[r0:r1])
    cl.seal()
    one = hbase._build(emb, created, rowbytes, ids, NM + 1000)
    q = syn.query_vectors(0, 8, DIM_M, NM).numpy()
    terms = _terms(syn.query_texts(0, 8, NM))
    rng = np.random.default_rng(77)
    shard_of = {int(i): g for g in range(3) for i in ids[g * CUT_M:(g + 1) * CUT_M]}

    def delete(gone):
        for g in range(3):
            mine = np.array([i for i in gone if shard_of[int(i)] == g], np.int64)
            assert cl.shard(g).delete_rows(mine) == len(mine)
        assert one.delete_rows(gone) == len(gone)
        model.delete(gone)

    words = [syn.vocab_word(t) for t in (77, 2040)]
    t0, t1 = int(created[50_000]), int(created[10_000])                      # a window over all three shards

    def word_ids():
        return set(model.ids[np.setdiff1d(_word_rows(model.rowbytes, words), np.nonzero(model.dead)[0])].tolist())

    def make():
        pick = model.ids[np.sort(rng.choice(len(model.ids), 20_000, replace=False))]
        sets = {"ids": set(model.ids[model.rows_of_ids(pick)].tolist()), "ticks": set(model.ids_in_window(t0, t1).tolist()), "terms": word_ids()}
        mine = {"ids": cl.scope(pick), "ticks": cl.scope_ticks(t0, t1), "terms": cl.scope_terms(words, "any")}
        twins = {"ids": one.scope(pick), "ticks": one.scope_ticks(t0, t1), "terms": one.scope_terms(words, "any")}
        return mine, twins, sets

    def check(mine, twins, sets, step):
        for name, sc in mine.items():
            want = model.ordered(sets[name])
            assert sc.rows == len(want) == twins[name].rows, (step, name, sc.rows, len(want))
            got = sc.row_ids()
            assert np.array_equal(got, want) and np.array_equal(got, twins[name].row_ids()), (step, name)
            assert _equal(cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, sc, candidate_limit=len(want) - 100),
                          one.search_in_scope(q, terms, syn.NOW_TICKS, 10, twins[name], candidate_limit=len(want) - 100)), (step, name)

    delete(rng.choice(model.ids, 500, replace=False))
    mine, twins, sets = make()                                                # scopes made behind the deletes
    assert len(sets["terms"]) > 2000
    check(mine, twins, sets, "made behind deletes")
    in_all = np.fromiter(sets["ids"] & sets["ticks"], np.int64)[:200]
    delete(np.unique(np.concatenate([in_all, rng.choice(model.ids[~model.dead], 2_800, replace=False)]))[:3000])
    check(mine, twins, sets, "after deletes through the shards")
    removed = int(model.dead.sum())
    assert cl.compact() == removed and one.compact() == removed
    model.compact()
    assert cl.rows == len(model.ids) == one.rows
    check(mine, twins, sets, "after compact")
    # 131 rows into shard 1 that carry a term of the term scope and fall inside the tick window
    n1 = cl.shard(0).rows
    lo, hi = n1 + 200, n1 + cl.shard(1).rows - 200
    new_emb, _, new_bytes = hbase._rows(131, DIM_M, row0=5_000_000)
    new_created = (model.created[rng.choice(np.arange(lo, hi), 131, replace=False)] - 3).astype(np.int64)
    assert ((new_created >= t0) & (new_created < t1)).all()
    new_bytes[:, :syn.WORD_LEN] = np.frombuffer(words[0], np.uint8)
    new_ids = 10_000_000 + np.arange(131, dtype=np.int64)
    new_off = np.arange(132, dtype=np.uint64) * new_bytes.shape[1]
    assert cl.insert_rows(1, new_emb, new_created, new_bytes.reshape(-1), new_off, row_ids=new_ids) == 131
    assert one.insert_rows(new_emb, new_created, new_bytes.reshape(-1), new_off, row_ids=new_ids) == 131
    model.insert(new_emb, new_created, new_bytes, new_ids)
    check(mine, twins, sets, "after insert")                                 # the old scopes: the rows they held, no new one
    for name, sc in mine.items():
        assert not np.isin(new_ids, sc.row_ids()).any(), name
    fresh, fresh_twins, fresh_sets = make()                                   # made afterwards: they hold the new rows
    for name in ("ticks", "terms"):
        assert np.isin(new_ids, fresh[name].row_ids()).all(), name
    check(fresh, fresh_twins, fresh_sets, "made after insert")
    assert mine["ids"].add_ids(new_ids) == 131 and twins["ids"].add_ids(new_ids) == 131
    sets["ids"] |= set(new_ids.tolist())
    check({"ids": mine["ids"]}, twins, sets, "add_ids names the new rows")
    for s in list(mine.values()) + list(twins.values()) + list(fresh.values()) + list(fresh_twins.values()):
        s.close()
    cl.close()
    one.close()


# ---- 7. lifetime and threads --------------------------------------------------------------------------------------------------

def test_an_unsealed_cluster_and_device_pointers_are_refused():
    import torch
    P = pkg()
    cl, ids = _tiny_cluster(seal=False)
    for call in (lambda: cl.scope(ids[:10]), lambda: cl.scope_ticks(I64_MIN, I64_MAX), lambda: cl.scope_terms([b"abc"], "any")):
        _raises(P.native.ORR_ESTATE, call)
        assert b"not sealed" in P.native.hip.orr_last_error()
    cl.seal()
    sc = cl.scope(ids[:10])
    assert sc.rows == 10
    dids = torch.from_numpy(ids[:10].copy()).cuda()
    h = P.native.C.c_void_p(7)
    assert P.native.hip.orr_cluster_scope_create(cl._h, 10, dids.data_ptr(), P.native.C.byref(h)) == P.native.ORR_EINVAL and h.value == 7
    assert b"host memory" in P.native.hip.orr_last_error()
    assert P.native.hip.orr_cluster_scope_add_ids(sc._h, 10, dids.data_ptr(), None) == P.native.ORR_EINVAL
    q = np.zeros((1, 64), np.float32)
    dq = torch.from_numpy(q).cuda()
    import omni_recall_rag_amd.index as index
    pool, toff, qoff = index.pack_terms([[b"abc"]])
    rows, scores, counts = np.full((1, 10), 7, np.int64), np.zeros((1, 10)), np.zeros(1, np.int32)
    r = P.native.hip.orr_cluster_search_batch_in_scope(cl._h, 1, 64, dq.data_ptr(), pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, NOW, 10, 300,
                                                       sc._h, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data)
    assert r == P.native.ORR_EINVAL and b"host memory" in P.native.hip.orr_last_error() and (rows == 7).all()
    sc.close()
    cl.close()


def test_orphans_after_the_cluster_is_closed():
    P = pkg()
    cl, ids = _tiny_cluster()
    a, b = cl.scope(ids[:100]), cl.scope_ticks(I64_MIN, I64_MAX)
    part = a.shard(1)
    assert a.rows == 100 and b.rows == len(ids)
    q, terms = np.zeros((1, 64), np.float32), [[b"abc"]]
    cl_handle = cl._h
    cl.close()                                                                # the cluster goes first: its scopes are orphaned
    assert a.rows == -1 and b.rows == -1 and part.rows == -1
    for call in (lambda: a.add_ids(ids[:3]), lambda: a.row_ids(), lambda: a.and_(b), lambda: b.or_(a)):
        _raises(P.native.ORR_ESTATE, call)
    other, other_ids = _tiny_cluster()
    cl._h = other._h                                                          # (a live cluster to ask: the scope is orphaned, not foreign)
    try:
        _raises(P.native.ORR_ESTATE, lambda: cl.search_in_scope(q, terms, NOW, 10, a))
    finally:
        cl._h = None
    assert cl_handle is not None
    a.close()
    b.close()
    other.close()


@pytest.mark.parametrize("scope_first", [True, False])
def test_the_two_closes_race_in_both_orders(scope_first):
    for _ in range(3):
        cl, ids = _tiny_cluster()
        scopes = [cl.scope(ids[::2]), cl.scope_ticks(I64_MIN, I64_MAX), cl.scope_terms([b"abc"], "any")]
        go = threading.Barrier(2)

        def close_scopes():
            go.wait()
            for s in scopes:
                s.close()

        def close_cluster():
            go.wait()
            cl.close()

        order = [close_scopes, close_cluster] if scope_first else [close_cluster, close_scopes]
        threads = [threading.Thread(target=f) for f in order]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=60)
        assert not any(t.is_alive() for t in threads)
        assert all(s._h is None for s in scopes) and cl._h is None


def test_four_threads_search_two_scopes_while_a_third_is_edited():
    cl, one, rows, qs, cases = _small()
    by_name = {name: (kind, arg) for name, kind, arg in cases}
    terms = _terms(TEXTS)
    n = CUTS[-1]
    s1, s2 = _make(cl, *by_name["wide"]), _make(cl, *by_name["window across both borders"])
    window = _make(cl, *by_name["window inside shard 1"])
    want = [cl.search_in_scope(qs, terms, NOW, 10, s, candidate_limit=n) for s in (s1, s2)]
    live_ids = rows.m.ids[np.nonzero(rows.live & (np.arange(n) != 500) & (np.arange(n) != 2000))[0]]
    edited = cl.scope(live_ids[:10])
    bad, added, errors = [], [], []

    def search(i):
        try:
            for _ in range(6):
                if not _equal(cl.search_in_scope(qs, terms, NOW, 10, (s1, s2)[i % 2], candidate_limit=n), want[i % 2]):
                    bad.append(i)
        except Exception as e:                                                # noqa: BLE001
            errors.append(repr(e))

    def edit():
        try:
            for i in range(12):
                added.append(edited.add_ids(live_ids[10 + 50 * i: 10 + 50 * (i + 1)]))
                edited.or_(window)
                edited.andnot(window)
        except Exception as e:                                                # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=search, args=(i,)) for i in range(4)] + [threading.Thread(target=edit)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not errors and not bad, (errors, bad)
    in_window = set(window.row_ids().tolist())
    assert all(0 <= a <= 50 for a in added) and len(added) == 12
    assert np.array_equal(edited.row_ids(), np.array([i for i in live_ids[:610] if i not in in_window], np.int64))
    for s in (s1, s2, window, edited):
        s.close()
