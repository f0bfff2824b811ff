"""Search inside a scope over the shards of a cluster: orr_cluster_search_batch_scoped, orr_cluster_search_batch_masked and the
shard call the masked one drives, orr_search_shard_masked.  The contract: what orr_search_batch_scoped / orr_search_batch_masked
return on ONE index that holds all the cluster's rows in the global candidate order -- so every result is compared with the
oracle on the sub-corpus of live scoped rows (the method of test_gpu_masked_search.py) AND with search_scoped / search_masked
of one RecallIndex built from the same rows.  Rows, order and fp64 scores bit for bit, NaN = NaN.

Shards are several "devices" on ordinal 0, as in test_gpu_cluster.py.  Shapes: 6,000 x 64 in three shards for the semantics
(limits that end inside a shard, shards without a scoped row, deleted rows, an id on two shards); 2 x 200,000 x 128 for the
masked screen -- 196,608 rows is the smallest shard on which it runs, dim 128 takes the int8 shadow.  The large cluster and its
single-index twin are built once per module.  They carry, from the start, the rows the ladder test needs: 70 identical rows of
one timestamp in shard 0 (a tie at the cut) and 20,000 identical embeddings in shard 1 (survivors overflow there only); both lie
in the "older half" scope and are parallel to no query of the other tests."""
import importlib
import threading

import numpy as np
import pytest

from helpers import DAY, NOW, orc, pkg, random_corpus

pytestmark = pytest.mark.gpu

TRAILER, DOT_EXACT, OVERFLOW, TWO_STAGE = 1, 2, 4, 8


def _syn():
    return importlib.import_module("omni_recall_rag_amd.synthetic")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _same_results(x, y):
    return np.array_equal(x[0], y[0]) and _same(x[1], y[1]) and np.array_equal(x[2], y[2])


# ---- 1. small, three shards ---------------------------------------------------------------------------------------------

TEXTS = ["alpha", "the kubernetes helm", "GAMMA delta zzz", "what is the"]
CUTS = [0, 1000, 3700, 6000]


class SmallModel:
    def __init__(self, c, ids):
        self.emb, self.created, self.contents, self.ids = list(c["emb"]), np.asarray(c["created"], np.int64), list(c["contents"]), np.asarray(ids, np.int64)
        self.deleted = set()

    def sub(self, scope_ids):
        want = np.isin(self.ids, np.asarray(list(scope_ids), np.int64))
        if self.deleted:
            want[np.fromiter(self.deleted, np.int64)] = False
        keep = np.nonzero(want)[0]
        if len(keep) == 0:
            return keep, None
        return keep, orc.OracleCorpus([self.emb[r] for r in keep], self.created[keep], [self.contents[r] for r in keep])


def _append_runs(P, target, c, lo, hi, ids):
    """Rows [lo, hi) in order, in runs with / without an embedding, with explicit ids."""
    lower = [P.text.lower_invariant(s) for s in c["contents"]]
    r = lo
    while r < hi:
        has = c["emb"][r] is not None
        e = r
        while e < hi and (c["emb"][e] is not None) == has:
            e += 1
        emb = np.stack(c["emb"][r:e]).astype(np.float32) if has else None
        target.append(emb, c["created"][r:e], lower[r:e], row_ids=ids[r:e])
        r = e


_SMALL = {}


def _small():
    """(cluster of three shards, the single index over the same rows, the model, the scopes, the three bare shards' cuts)."""
    if _SMALL:
        return _SMALL["v"]
    P = pkg()
    rng = np.random.default_rng(171)
    n, dim = CUTS[-1], 64
    c = random_corpus(rng, n, dim, sorted_created=True)
    c["created"] = np.sort(NOW - rng.choice(400 * DAY, n, replace=False))[::-1].astype(np.int64)   # distinct: the split is unambiguous
    ids = np.arange(n, dtype=np.int64)
    ids[2000] = 500                                                          # one id on two shards (rows 500 and 2000)
    cl = P.RecallCluster([0, 0, 0], dim)
    for g in range(3):
        _append_runs(P, cl.shard(g), c, CUTS[g], CUTS[g + 1], ids)
    cl.seal()
    one = P.RecallIndex(dim=dim)
    _append_runs(P, one, c, 0, n, ids)
    one.seal()
    model = SmallModel(c, ids)
    dead = sorted(int(r) for r in rng.choice(np.setdiff1d(np.arange(n), [500, 2000]), 200, replace=False))
    for g in range(3):
        cl.shard(g).delete_rows(ids[[r for r in dead if CUTS[g] <= r < CUTS[g + 1]]])
    one.delete_rows(ids[dead])
    model.deleted |= set(dead)
    wide = rng.choice(np.setdiff1d(np.arange(n), [2000]), 1200, replace=False).astype(np.int64)
    scopes = {
        "wide": wide,                                                         # its 300-row limit ends inside the second shard
        "one shard only": rng.choice(np.arange(CUTS[1], CUTS[2]), 400, replace=False).astype(np.int64),
        "empty": np.zeros(0, np.int64),
        "unknown and negative ids": np.concatenate([wide[:500], [n + 5, -2, 2 ** 40]]),
        "an id on two shards": np.concatenate([[500], wide[600:700]]),
    }
    _SMALL["v"] = (cl, one, model, scopes, rng.standard_normal((len(TEXTS), dim)).astype(np.float32))
    return _SMALL["v"]


_SMALL_ORACLE = {}


def _small_expect(model, name, scope, b, qvec, text, topk, limit):
    key = (name, b, qvec is not None, topk, limit)
    if key not in _SMALL_ORACLE:
        keep, corpus = model.sub(scope)
        if corpus is None:
            _SMALL_ORACLE[key] = ([], np.zeros(0))
        else:
            orow, osc, _ = corpus.search([] if qvec is None else qvec, text, NOW, max(1, topk), candidate_limit=limit)
            _SMALL_ORACLE[key] = ([int(model.ids[keep[r]]) for r in orow], np.asarray(osc))
    return _SMALL_ORACLE[key]


GRID = [(10, 300), (10, 6000), (40, 300), (5, 1), (100, 6000), (-1, 6000)]


def test_the_small_fixture_is_what_the_cases_need():
    cl, one, model, scopes, qs = _small()
    live = np.stack([cl.shard(g).scope_count(scopes["wide"]) for g in range(3)])[:, 0]
    assert live[0] < 300 < live[0] + live[1]                                  # the global limit falls inside the second shard
    live = np.stack([cl.shard(g).scope_count(scopes["one shard only"]) for g in range(3)])[:, 0]
    assert live[0] == 0 and live[2] == 0 and live[1] > 0
    live = np.stack([cl.shard(g).scope_count(np.array([500])) for g in range(3)])[:, 0]
    assert list(live) == [1, 1, 0]                                            # the id on two shards brings both rows


@pytest.mark.parametrize("topk,limit", GRID)
@pytest.mark.parametrize("with_vectors", [True, False])
def test_small_cluster_masked_equals_the_oracle_and_one_index(topk, limit, with_vectors):
    P = pkg()
    cl, one, model, scopes, qs = _small()
    q = qs.copy()
    q[3] = 0.0                                                                # a zero query vector
    terms = [P.text.query_terms(t) for t in TEXTS]
    for name, scope in scopes.items():
        got = cl.search_masked(q if with_vectors else None, terms, NOW, topk, scope, candidate_limit=limit)
        want = one.search_masked(q if with_vectors else None, terms, NOW, topk, scope, candidate_limit=limit)
        assert _same_results(got, want), (name, topk, limit)
        rows, scores, counts = got
        for b, text in enumerate(TEXTS):
            orows, oscores = _small_expect(model, name, scope, b, q[b] if with_vectors else None, text, topk, limit)
            k = int(counts[b])
            assert list(rows[b, :k]) == orows, (name, b, topk, limit, list(rows[b, :k])[:8], orows[:8])
            assert _same(scores[b, :k], oscores), (name, b, topk, limit)
            assert (rows[b, k:] == -1).all()


@pytest.mark.parametrize("topk,limit", GRID)
@pytest.mark.parametrize("with_vectors", [True, False])
def test_small_cluster_scoped_equals_the_oracle_and_one_index(topk, limit, with_vectors):
    P = pkg()
    cl, one, model, scopes, qs = _small()
    q = qs.copy()
    q[3] = 0.0
    terms = [P.text.query_terms(t) for t in TEXTS]
    names = list(scopes)
    # a scope per query, twice so that every scope meets the zero vector's neighbours; then each scope shared by the batch
    for shift in (0, 2):
        mine = [names[(b + shift) % len(names)] for b in range(len(TEXTS))]
        lists = [scopes[m] for m in mine]
        got = cl.search_scoped(q if with_vectors else None, terms, NOW, topk, lists, candidate_limit=limit)
        want = one.search_scoped(q if with_vectors else None, terms, NOW, topk, lists, candidate_limit=limit)
        assert _same_results(got, want), (mine, topk, limit)
        rows, scores, counts = got
        for b, text in enumerate(TEXTS):
            orows, oscores = _small_expect(model, mine[b], scopes[mine[b]], b, q[b] if with_vectors else None, text, topk, limit)
            k = int(counts[b])
            assert list(rows[b, :k]) == orows, (mine[b], b, topk, limit)
            assert _same(scores[b, :k], oscores), (mine[b], b, topk, limit)
    for name in ("wide", "an id on two shards", "empty"):
        got = cl.search_scoped(q if with_vectors else None, terms, NOW, topk, scopes[name], candidate_limit=limit)
        rows, scores, counts = got
        for b, text in enumerate(TEXTS):
            orows, oscores = _small_expect(model, name, scopes[name], b, q[b] if with_vectors else None, text, topk, limit)
            k = int(counts[b])
            assert list(rows[b, :k]) == orows and _same(scores[b, :k], oscores), (name, b, topk, limit)


def _raw_masked(P, cl, qs, terms, q_ptr, n_ids, ids_ptr, expect=None):
    """orr_cluster_search_batch_masked through the raw binding with an argument the library must refuse with ORR_EINVAL;
    returns the untouched-or-not output arrays."""
    pool, toff, qoff = importlib.import_module("omni_recall_rag_amd.index").pack_terms(terms)
    B = len(terms)
    rows, scores, counts = np.full((B, 10), 7, np.int64), np.zeros((B, 10)), np.zeros(B, np.int32)
    r = P.native.hip.orr_cluster_search_batch_masked(cl._h, B, qs.shape[1], q_ptr, pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, NOW, 10, 300,
                                                     n_ids, ids_ptr, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data)
    assert r == P.native.ORR_EINVAL, r
    if expect:
        assert expect in P.native.hip.orr_last_error(), P.native.hip.orr_last_error()
    return rows, scores, counts


def test_small_cluster_counts_in_its_own_stats_and_checks_its_arguments():
    P = pkg()
    cl, one, model, scopes, qs = _small()
    terms = [P.text.query_terms(t) for t in TEXTS]
    cl.search_stats(reset=True)
    cl.search_masked(qs, terms, NOW, 10, scopes["wide"], candidate_limit=6000)
    cl.search_scoped(qs, terms, NOW, 10, scopes["wide"], candidate_limit=6000)
    st = cl.search_stats()
    assert st["searches"] == 2 and st["queries"] == 2 * len(TEXTS) and st["passes"] >= 2, st
    ids = scopes["wide"]
    rows, scores, counts = _raw_masked(P, cl, qs, terms, qs.ctypes.data, -1, ids.ctypes.data)
    assert (rows == 7).all()                                                      # ORR_EINVAL on a real handle, nothing written
    rows, scores, counts = _raw_masked(P, cl, qs, terms, qs.ctypes.data, 5, None)
    assert (rows == 7).all()
    recs = cl.shard(0).search_shard_masked(qs, terms, NOW, 8, 300, ids)
    for bad in (dict(kprime=0), dict(shard_pass=2), dict(scope_before=-1)):
        kw = dict(kprime=8, shard_pass=0, scope_before=0)
        kw.update(bad)
        with pytest.raises(Exception):
            cl.shard(0).search_shard_masked(qs, terms, NOW, kw["kprime"], 300, ids, scope_before=kw["scope_before"], shard_pass=kw["shard_pass"], out=recs)
    fresh = P.RecallCluster([0, 0], 64)
    try:
        with pytest.raises(Exception):
            fresh.search_masked(qs, terms, NOW, 10, ids)                          # ORR_ESTATE: not sealed
        assert b"not sealed" in P.native.hip.orr_last_error()
    finally:
        fresh.close()


# ---- 2. two-stage, two shards ---------------------------------------------------------------------------------------------

HALF = 200_000
N = 2 * HALF
DIM = 128
POOL_Q = 40
TIE = np.arange(120_000, 120_070)                    # shard 0: 70 identical rows of one timestamp
MASS = np.arange(320_000, 340_000)                   # shard 1: 20,000 identical embeddings


class Model:
    """The corpus as the test knows it (test_gpu_masked_search.py's): rows in candidate order with their ids."""

    def __init__(self, emb, created, rowbytes, ids):
        self.emb, self.created, self.rowbytes, self.ids = emb, np.asarray(created, np.int64).copy(), rowbytes, np.asarray(ids, np.int64).copy()

    def sub(self, scope_ids):
        keep = np.nonzero(np.isin(self.ids, np.asarray(scope_ids, np.int64)))[0]
        if len(keep) == 0:
            return keep, None
        width = self.rowbytes.shape[1]
        off = np.arange(len(keep) + 1, dtype=np.int64) * width
        return keep, orc.OracleCorpus(np.ascontiguousarray(self.emb[keep]), self.created[keep], (np.ascontiguousarray(self.rowbytes[keep]).reshape(-1), off))


_BIG, _SUBS, _ORACLE = {}, {}, {}


def _big():
    """The 2 x 200,000-row cluster ("mask_screen" = 1 on both shards), its single-index twin, the model, queries, scopes."""
    if _BIG:
        return _BIG["v"]
    import torch
    P, syn = pkg(), _syn()
    emb = syn.embeddings(0, N, DIM, "cuda:0").cpu().numpy()
    created = syn.created_ticks(0, N, N).numpy()
    pool, _ = syn.contents(0, N, "cuda:0")
    rowbytes = pool.reshape(N, syn.ROW_BYTES).cpu().numpy().copy()
    ids = np.arange(N, dtype=np.int64) * 3 + 11
    q = syn.query_vectors(0, POOL_Q, DIM, N).numpy()
    rng = np.random.default_rng(909)
    tie_vec = rng.standard_normal(DIM).astype(np.float32)
    mass_vec = rng.standard_normal(DIM).astype(np.float32)
    emb[TIE] = tie_vec
    created[TIE] = created[TIE[0]]
    rowbytes[TIE] = rowbytes[TIE[0]]
    emb[MASS] = mass_vec * np.float32(0.5)
    off = np.arange(N + 1, dtype=np.int64) * syn.ROW_BYTES

    def fill(target, lo, hi):
        for r0 in range(lo, hi, 50_000):
            r1 = min(hi, r0 + 50_000)
            target.append(emb[r0:r1], created[r0:r1], rowbytes[r0:r1].reshape(-1), off[: r1 - r0 + 1], row_ids=ids[r0:r1])

    cl = P.RecallCluster([0, 0], DIM, capacity_rows_per_shard=HALF)
    fill(cl.shard(0), 0, HALF)
    fill(cl.shard(1), HALF, N)
    cl.seal()
    one = P.RecallIndex(dim=DIM, capacity_rows=N)
    fill(one, 0, N)
    one.seal()
    for target in (cl.shard(0), cl.shard(1), one):
        target.set_option("mask_screen", 1)
    torch.cuda.synchronize()
    texts = syn.query_texts(0, POOL_Q, N)
    model = Model(emb, created, rowbytes, ids)
    ten = np.sort(rng.choice(N, N // 10, replace=False))
    fam = {
        "random 10 %": ten,
        "older half of each shard": np.concatenate([np.arange(HALF // 2, HALF), np.arange(HALF + HALF // 2, N)]),
        "inside shard 1 only": np.sort(HALF + rng.choice(HALF, HALF // 10, replace=False)),
    }
    plants = {}
    special = set(MASS.tolist()) | set(TIE.tolist())
    for name, rows in fam.items():
        in_scope = set(rows.tolist())
        inside = int(next(r for r in rows[len(rows) * 2 // 3:] if r >= HALF and int(r) not in special))            # a row of shard 1
        outside = next(r for r in range(HALF // 2 - 1, -1, -1) if r not in in_scope)
        qq = q.copy()
        noise = rng.standard_normal((2, DIM)).astype(np.float32) * np.float32(0.01)
        qq[0] = emb[inside] + noise[0]                                         # a near-duplicate inside the scope, in shard 1: ranks first
        qq[1] = emb[outside] + noise[1]                                        # ... and outside the scope: must not appear
        plants[name] = (qq, inside, outside)
    _BIG["v"] = (cl, one, model, texts, fam, plants, tie_vec, mass_vec)
    return _BIG["v"]


def _sub(model, name, scope):
    if name not in _SUBS:
        _SUBS[name] = model.sub(scope)
    return _SUBS[name]


def _checked(B):
    if B <= 8:
        return list(range(B))
    return sorted(set(range(8)) | {B // 2, B - 9, B - 8, B - 1})


def _oracle(key, model, sub, qvec, text, topk, limit):
    """The oracle's (ids, scores) for one query, once per key; a top-40 answer serves every smaller topk at the same limit."""
    keep, corpus = sub
    if corpus is None:
        return [], np.zeros(0)
    full = key + (limit,)
    if full not in _ORACLE:
        orow, osc, _ = corpus.search(qvec, text, _syn().NOW_TICKS, 40, candidate_limit=limit, threads=16)
        _ORACLE[full] = ([int(model.ids[keep[r]]) for r in orow], np.asarray(osc))
    rows, scores = _ORACLE[full]
    return rows[:max(1, topk)], scores[:max(1, topk)]


def _shard_stats(cl):
    return [cl.shard(g).search_stats() for g in range(cl.n_shards)]


def _reset(cl):
    for g in range(cl.n_shards):
        cl.shard(g).reset_search_stats()


@pytest.mark.parametrize("B", [1, 8, 40])
def test_two_stage_cluster_masked_equals_one_index_and_the_oracle(B):
    P, syn = pkg(), _syn()
    cl, one, model, texts_all, fam, plants, _, _ = _big()
    texts = list(texts_all[:B])
    terms = [P.text.query_terms(t) for t in texts]
    live0 = int(cl.shard(0).scope_count(model.ids[fam["random 10 %"]])[0])
    cases = [(name, name, N) for name in fam] + [("random 10 %, shard 1 clipped to 1,000", "random 10 %", live0 + 1000)]
    for what, name, limit in cases:
        q_all, inside, outside = plants[name]
        q = np.ascontiguousarray(q_all[:B])
        scope = model.ids[fam[name]]
        sub = _sub(model, name, scope)
        took = min(len(sub[0]), limit)
        for topk in (1, 10, 40):
            _reset(cl)
            got = cl.search_masked(q, terms, syn.NOW_TICKS, topk, scope, candidate_limit=limit)
            st = _shard_stats(cl)
            want = one.search_masked(q, terms, syn.NOW_TICKS, topk, scope, candidate_limit=limit)
            assert _same_results(got, want), (what, B, topk)                  # every query against the single index
            rows, scores, counts = got
            assert (counts == min(topk, took)).all(), (what, B, topk, counts[:8])
            for b in _checked(B):
                orows, oscores = _oracle((name, b), model, sub, q[b], texts[b], topk, limit)
                k = int(counts[b])
                assert list(rows[b, :k]) == orows, (what, b, topk, list(rows[b, :k])[:6], orows[:6])
                assert _same(scores[b, :k], oscores), (what, b, topk)
            if limit == N:
                assert rows[0, 0] == model.ids[inside], (what, topk)            # the planted near-duplicate in shard 1 ranks first
                if B > 1:
                    assert model.ids[outside] not in rows[1], (what, topk)      # ... the one outside the scope never appears
            # which path ran where, from the shards' own statistics
            if name == "inside shard 1 only":
                assert st[0]["passes"] == 0 and st[0]["searches"] >= 1, (what, st[0])              # empty records, no pass
                assert st[1]["pass_mode"] == 5 and st[1]["survivor_samples"] > 0, (what, st[1])
            elif limit == N:
                for g in (0, 1):
                    assert st[g]["pass_mode"] == 5 and st[g]["survivor_samples"] > 0 and st[g]["exact_pass_queries"] == 0, (what, g, st[g])
            else:
                assert st[0]["pass_mode"] == 5 and st[0]["survivor_samples"] > 0, (what, st[0])    # shard 0 screens its whole scope
                assert st[1]["pass_mode"] == 4 and st[1]["survivor_samples"] == 0, (what, st[1])   # shard 1: 1,000 rows, the list path


def test_two_stage_cluster_scoped_equals_one_index_and_the_oracle():
    P, syn = pkg(), _syn()
    cl, one, model, texts_all, fam, plants, _, _ = _big()
    B = 8
    texts = list(texts_all[:B])
    terms = [P.text.query_terms(t) for t in texts]
    name = "random 10 %"
    q = np.ascontiguousarray(plants[name][0][:B])
    scope = model.ids[fam[name]]
    sub = _sub(model, name, scope)
    live0 = int(cl.shard(0).scope_count(scope)[0])
    for limit in (N, live0 + 1000):
        got = cl.search_scoped(q, terms, syn.NOW_TICKS, 10, scope, candidate_limit=limit)
        assert _same_results(got, one.search_scoped(q, terms, syn.NOW_TICKS, 10, scope, candidate_limit=limit)), limit
        assert _same_results(got, cl.search_masked(q, terms, syn.NOW_TICKS, 10, scope, candidate_limit=limit)), limit
        for b in range(B):
            orows, oscores = _oracle((name, b), model, sub, q[b], texts[b], 10, limit)
            assert list(got[0][b, :got[2][b]]) == orows and _same(got[1][b, :got[2][b]], oscores), (b, limit)


def test_device_pointers_are_refused_by_the_cluster_calls():
    import torch
    P = pkg()
    cl, one, model, texts_all, fam, plants, _, _ = _big()
    terms = [P.text.query_terms(t) for t in texts_all[:4]]
    q = np.ascontiguousarray(plants["random 10 %"][0][:4])
    ids = np.ascontiguousarray(model.ids[fam["inside shard 1 only"]])
    dq, dids = torch.from_numpy(q).cuda(), torch.from_numpy(ids).cuda()
    rows, _, _ = _raw_masked(P, cl, q, terms, dq.data_ptr(), len(ids), ids.ctypes.data, expect=b"query vectors must be in host memory")
    assert (rows == 7).all()
    rows, _, _ = _raw_masked(P, cl, q, terms, q.ctypes.data, len(ids), dids.data_ptr(), expect=b"scope_ids must be in host memory")
    assert (rows == 7).all()


# ---- 3. the ladder --------------------------------------------------------------------------------------------------------

def test_the_ladder_a_tie_at_the_cut_and_an_overflow_on_one_shard():
    P, syn = pkg(), _syn()
    cl, one, model, texts_all, fam, plants, tie_vec, mass_vec = _big()
    name = "older half of each shard"
    B = 8
    q = np.ascontiguousarray(plants[name][0][:B]).copy()
    q[2] = tie_vec                                                            # equal to the 70 rows of one timestamp in shard 0: a tie at the cut
    q[5] = mass_vec                                                           # parallel to 20,000 rows of shard 1 only: its survivors overflow there
    texts = list(texts_all[:B])
    terms = [P.text.query_terms(t) for t in texts]
    scope = model.ids[fam[name]]
    sub = _sub(model, name, scope)
    assert set(model.ids[TIE]) <= set(scope) and set(model.ids[MASS]) <= set(scope)
    cl.search_stats(reset=True)
    _reset(cl)
    got = cl.search_masked(q, terms, syn.NOW_TICKS, 10, scope, candidate_limit=N)
    st, shards = cl.search_stats(), _shard_stats(cl)
    rows, scores, counts = got
    for b in range(B):
        orows, oscores = _oracle(("ladder", b), model, sub, q[b], texts[b], 10, N)
        assert list(rows[b, :counts[b]]) == orows, (b, list(rows[b])[:6], orows[:6])
        assert _same(scores[b, :counts[b]], oscores), b
    assert set(rows[2]) <= set(model.ids[TIE]) and list(rows[2]) == sorted(rows[2])          # the ties in candidate order
    assert set(rows[5]) <= set(model.ids[MASS])
    assert st["requeried"] > 0 and st["passes"] >= 2, st                                     # k' had to grow
    assert shards[1]["overflowed_queries"] >= 1 or shards[1]["survivor_capacity"] >= 32768, shards[1]   # (grown buffers are kept)
    assert shards[0]["overflowed_queries"] == 0, shards[0]                                   # ... the other shard never overflowed
    assert _same_results(got, one.search_masked(q, terms, syn.NOW_TICKS, 10, scope, candidate_limit=N))
    # the scoped call climbs its own ladder for the tie (three queries: every listed row is re-scored per query)
    cl.search_stats(reset=True)
    few = cl.search_scoped(q[:3], terms[:3], syn.NOW_TICKS, 10, scope, candidate_limit=N)
    assert cl.search_stats()["requeried"] > 0
    assert np.array_equal(few[0], rows[:3]) and _same(few[1], scores[:3]) and np.array_equal(few[2], counts[:3])


# ---- 4. the shard form directly -------------------------------------------------------------------------------------------

def _merged(P, shards, q, terms, now, topk, limit, scope, dim, shard_pass, kp=32, kp_max=1 << 16):
    """The loop every multi-shard caller of the shard form runs: count, prefix sums, search, merge, escalate."""
    live = np.array([int(s.scope_count(scope)[0]) for s in shards], np.int64)
    before = np.concatenate([[0], np.cumsum(live)[:-1]])
    took = np.minimum(live, np.maximum(0, max(1, limit) - before))
    while True:
        recs = np.stack([s.search_shard_masked(q, terms, now, kp, limit, scope, scope_before=int(before[g]), topk=topk, shard_pass=shard_pass)
                         for g, s in enumerate(shards)])
        rows, scores, counts, unc = P.merge_candidates(recs, dim, q, terms, now, topk)
        if unc == 0 or kp >= kp_max:
            break
        kp *= 4
    assert unc == 0
    return (rows, scores, counts), recs, kp, took


def test_shard_form_on_three_small_shards():
    P = pkg()
    cl, one, model, scopes, qs = _small()
    shards = [cl.shard(g) for g in range(3)]
    terms = [P.text.query_terms(t) for t in TEXTS]
    for name, scope in scopes.items():
        for topk, limit in ((10, 300), (10, 6000), (5, 1), (100, 6000)):
            kp0 = 32 if topk < 64 else 128
            got, recs, kp, took = _merged(P, shards, qs, terms, NOW, topk, limit, scope, 64, 0, kp=kp0)
            trailers = recs[:, :, kp]
            assert ((trailers["flags"] & TRAILER) != 0).all()
            assert np.array_equal(trailers["order_key"], np.repeat(took[:, None], len(TEXTS), axis=1)), (name, topk, limit)
            assert ((trailers["flags"] & TWO_STAGE) == 0).all()               # shards this small never screen
            valid = recs[:, :, :kp]["row_id"] >= 0
            assert ((recs[:, :, :kp]["flags"] & DOT_EXACT) != 0)[valid].all()
            assert np.array_equal(valid.sum(axis=2), trailers["matches"])
            assert _same_results(got, cl.search_masked(qs, terms, NOW, topk, scope, candidate_limit=limit)), (name, topk, limit)
            again, _, _, _ = _merged(P, shards, qs, terms, NOW, topk, limit, scope, 64, 1, kp=kp0)
            assert _same_results(got, again), (name, topk, limit)             # pass = 1: the same merged result


def test_shard_form_on_the_two_stage_shards():
    P, syn = pkg(), _syn()
    cl, one, model, texts_all, fam, plants, _, _ = _big()
    B = 8
    texts = list(texts_all[:B])
    terms = [P.text.query_terms(t) for t in texts]
    shards = [cl.shard(0), cl.shard(1)]
    name = "random 10 %"
    q = np.ascontiguousarray(plants[name][0][:B])
    scope = model.ids[fam[name]]
    live0 = int(shards[0].scope_count(scope)[0])
    for limit, screens in ((N, (True, True)), (live0 + 1000, (True, False))):
        got, recs, kp, took = _merged(P, shards, q, terms, syn.NOW_TICKS, 10, limit, scope, DIM, 0)
        trailers = recs[:, :, kp]
        assert np.array_equal(trailers["order_key"], np.repeat(took[:, None], B, axis=1)), limit
        if limit != N:
            assert list(took) == [live0, 1000]
        valid = recs[:, :, :kp]["row_id"] >= 0
        assert np.array_equal(valid.sum(axis=2), trailers["matches"])
        for g, screened in enumerate(screens):
            assert (((trailers[g]["flags"] & TWO_STAGE) != 0) == screened).all(), (limit, g)    # exactly where the screen ran
            if screened:
                assert np.isfinite(trailers[g]["norm_b"]).all()                                # the floor L
            else:
                assert ((recs[g, :, :kp]["flags"] & DOT_EXACT) != 0)[valid[g]].all()
        assert _same_results(got, cl.search_masked(q, terms, syn.NOW_TICKS, 10, scope, candidate_limit=limit)), limit
        again, recs1, kp1, _ = _merged(P, shards, q, terms, syn.NOW_TICKS, 10, limit, scope, DIM, 1)
        assert ((recs1[:, :, kp1]["flags"] & TWO_STAGE) == 0).all()
        assert ((recs1[:, :, :kp1]["flags"] & DOT_EXACT) != 0)[recs1[:, :, :kp1]["row_id"] >= 0].all()
        assert _same_results(got, again), limit


# ---- 5. concurrency -------------------------------------------------------------------------------------------------------

def test_four_threads_search_the_cluster_side_by_side():
    P, syn = pkg(), _syn()
    cl, one, model, texts_all, fam, plants, _, _ = _big()
    B = 8
    terms = [P.text.query_terms(t) for t in texts_all[:B]]
    rng = np.random.default_rng(31)
    jobs = []
    for t, name in enumerate(("random 10 %", "older half of each shard", "inside shard 1 only", "random 10 %")):
        q = np.ascontiguousarray(plants[name][0][:B])
        if t == 3:                                                            # the scoped call, a small scope of its own
            jobs.append((cl.search_scoped, q, model.ids[np.sort(rng.choice(N, 3000, replace=False))]))
        else:
            jobs.append((cl.search_masked, q, model.ids[fam[name]]))
    serial = [fn(q, terms, syn.NOW_TICKS, 10, scope, candidate_limit=N) for fn, q, scope in jobs]
    out, errors = [None] * len(jobs), []

    def run(i):
        try:
            fn, q, scope = jobs[i]
            out[i] = fn(q, terms, syn.NOW_TICKS, 10, scope, candidate_limit=N)
        except Exception as e:                                                # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(len(jobs)):
        assert _same_results(out[i], serial[i]), i
