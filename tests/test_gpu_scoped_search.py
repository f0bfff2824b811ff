"""Scoped search (orr_search_batch_scoped, orr_search_shard_scoped, orr_index_scope_count): a query ranks only the rows
whose ids its scope lists.  The contract: the result is what orr_search_batch returns on a shard sealed from scratch from
only the live rows of the scope, in their present candidate order -- so the oracle runs on that sub-corpus (as `_compacted`
does in test_gpu_deletes.py) and its row numbers are mapped back.  Rows, order and fp64 scores must match bit for bit.
Reference behaviour: IIngestionStore.GetChunksByDocumentIdAsync (IIngestionStore.cs:11) feeding RecallSearchService.cs:26-37."""
import threading

import numpy as np
import pytest

from helpers import DAY, NOW, build_index, orc, pkg, random_corpus

pytestmark = pytest.mark.gpu

TEXTS = ["alpha", "the kubernetes helm", "GAMMA delta zzz", "what is the", "azure cosmos vector search"]


class Model:
    """The corpus as the test knows it: rows in append order with their ids; deleted rows are remembered."""

    def __init__(self, emb, created, contents, ids=None):
        self.emb, self.created, self.contents = list(emb), np.asarray(created, np.int64).copy(), list(contents)
        self.ids = np.arange(len(self.contents), dtype=np.int64) if ids is None else np.asarray(ids, np.int64).copy()
        self.deleted = set()

    def sub(self, scope_ids):
        """(rows of the scope that are live, oracle over exactly those) -- None without a row."""
        want = np.isin(self.ids, np.asarray(list(scope_ids), np.int64))
        if self.deleted:
            want[np.fromiter(self.deleted, np.int64)] = False
        keep = np.nonzero(want)[0]
        if len(keep) == 0:
            return keep, None
        return keep, orc.OracleCorpus([self.emb[r] for r in keep], self.created[keep], [self.contents[r] for r in keep])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _expect(model, keep, corpus, qvec, text, topk, limit, threads=1):
    if corpus is None:
        return [], np.zeros(0)
    orow, osc, _ = corpus.search([] if qvec is None else qvec, text, NOW, topk, candidate_limit=limit, threads=threads)
    return [int(model.ids[keep[r]]) for r in orow], np.asarray(osc)


def _check_batch(idx, model, subs, qvecs, texts, topk, limit, scope_ids, q_arg=None, what=None, threads=1):
    """One scoped call of len(texts) queries; subs: one (keep, corpus) for all queries, or one per query."""
    P = pkg()
    terms = [P.text.query_terms(t) for t in texts]
    q = None if qvecs is None else (q_arg if q_arg is not None else np.stack(qvecs).astype(np.float32))
    rows, scores, counts = idx.search_scoped(q, terms, NOW, topk, scope_ids, candidate_limit=limit)
    for b, text in enumerate(texts):
        keep, corpus = subs if isinstance(subs, tuple) else subs[b]
        want_rows, want_scores = _expect(model, keep, corpus, None if qvecs is None else qvecs[b], text, topk, limit, threads)
        k = int(counts[b])
        assert list(rows[b, :k]) == want_rows, (what, b, text, topk, limit, list(rows[b, :k])[:8], want_rows[:8])
        assert _same(scores[b, :k], want_scores), (what, b, text, topk, limit)
    return rows, scores, counts


def _grid(s, n):
    """(topk, limit): the grid of test_gpu_deletes.py over a corpus of s rows, topk beyond a selection list (every pair a
    record), and limits of 0 (floored to 1 as the unscoped call floors it), 1, s - 1, s and 300."""
    return [(10, n), (1, 300), (40, n), (s + 5, n), (64, 300), (3, 2), (10, s - 1),
            (65, n), (200, n), (10, 0), (10, 1), (25, s - 1), (10, s), (10, 300)]


@pytest.mark.parametrize("seed,n,dim", [(21, 400, 3), (22, 3000, 64), (23, 6000, 128), (24, 5000, 256)])
def test_scoped_search_equals_the_oracle_on_the_sub_corpus(seed, n, dim):
    rng = np.random.default_rng(seed)
    c = random_corpus(rng, n, dim)
    model = Model(c["emb"], c["created"], c["contents"])
    idx = build_index(c, chunk=977)
    newest = np.argsort(-c["created"], kind="stable")[:40]
    tenth = rng.choice(n, n // 10, replace=False)
    scopes = {
        "empty": np.zeros(0, np.int64),
        "one row": np.array([int(rng.integers(0, n))]),
        "40 newest": newest,
        "1 %": rng.choice(n, max(2, n // 100), replace=False),
        "10 %": tenth,
        "50 %": rng.choice(n, n // 2, replace=False),
        "every row": np.arange(n),
        "repeats, unknown and negative ids": np.concatenate([tenth, tenth[:50], [n + 17, -5, -1, 2 ** 40], tenth[::-1][:9]]),
        "only unknown ids": np.array([n, n + 1, -3]),
    }
    vecs = [rng.standard_normal(dim).astype(np.float32), next(e for e in c["emb"] if e is not None).copy()]
    with_vec = [(v, t) for v in vecs for t in TEXTS]
    assert list(idx.scope_count(scopes["every row"])) == [n]
    for name, ids in scopes.items():
        ids = np.asarray(ids, np.int64)
        sub = model.sub(ids)
        s = len(sub[0])
        assert list(idx.scope_count(ids)) == [s], name
        for topk, limit in _grid(s, n):
            _check_batch(idx, model, sub, [v for v, _ in with_vec], [t for _, t in with_vec], topk, limit, ids, what=name)
            _check_batch(idx, model, sub, None, TEXTS, topk, limit, ids, what=name + ", no vector")
    st = idx.search_stats()
    assert st["pass_mode"] == 4 and st["exact_pass_queries"] == 0 and st["buffer_growths"] == 0
    # a query vector of another dimension scores cosine 0, as in the unscoped call
    other = rng.standard_normal(dim + 1).astype(np.float32)
    _check_batch(idx, model, model.sub(scopes["10 %"]), [other] * 2, TEXTS[:2], 10, n, scopes["10 %"], what="other dimension")
    idx.close()


@pytest.mark.parametrize("B", [1, 5, 40, 300])
def test_batches_with_a_scope_per_query_and_with_a_shared_scope(B):
    import torch
    rng = np.random.default_rng(30 + B)
    n, dim = 6000, 128
    c = random_corpus(rng, n, dim)
    model = Model(c["emb"], c["created"], c["contents"])
    idx = build_index(c, chunk=1500)
    sizes = [0, 1, 30, 600, 3000]
    scopes = [rng.choice(n, sizes[int(rng.integers(0, len(sizes)))] if B > 1 else 600, replace=False).astype(np.int64) for _ in range(B)]
    if B >= 5:
        scopes[1] = np.zeros(0, np.int64)                                   # some of them empty, whatever the draw
        scopes[B - 1] = np.array([n + 3, -9], np.int64)                     # ... or without a known id
    qvecs = [rng.standard_normal(dim).astype(np.float32) for _ in range(B)]
    texts = [TEXTS[b % len(TEXTS)] for b in range(B)]
    subs = [model.sub(s) for s in scopes]
    live = idx.scope_count(scopes, B)
    assert list(live) == [len(k) for k, _ in subs]
    for topk, limit in ((10, n), (10, 300), (70, n), (5, 7)):
        host = _check_batch(idx, model, subs, qvecs, texts, topk, limit, scopes, what="per-query scopes")
        # the same with the query vectors and the id list in device memory
        q_dev = torch.from_numpy(np.stack(qvecs)).to("cuda:0")
        ids_dev = torch.from_numpy(np.concatenate(scopes)).to("cuda:0")
        off = np.zeros(B + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in scopes])
        terms = [pkg().text.query_terms(t) for t in texts]
        dev = idx.search_scoped(q_dev, terms, NOW, topk, ids_dev, candidate_limit=limit, scope_off=off)
        assert np.array_equal(dev[0], host[0]) and _same(dev[1], host[1]) and np.array_equal(dev[2], host[2])
    # one scope shared by the whole batch (scope_off NULL), host and device pointers
    shared = rng.choice(n, 900, replace=False).astype(np.int64)
    sub = model.sub(shared)
    for topk, limit in ((10, n), (3, 300), (100, n)):
        host = _check_batch(idx, model, sub, qvecs, texts, topk, limit, shared, what="shared scope")
        dev = idx.search_scoped(torch.from_numpy(np.stack(qvecs)).to("cuda:0"), [pkg().text.query_terms(t) for t in texts], NOW, topk,
                                torch.from_numpy(shared).to("cuda:0"), candidate_limit=limit)
        assert np.array_equal(dev[0], host[0]) and _same(dev[1], host[1]) and np.array_equal(dev[2], host[2])
    idx.close()


def test_argument_errors_on_a_sealed_index_leave_it_searchable():
    import ctypes as C
    P = pkg()
    rng = np.random.default_rng(40)
    n, dim = 500, 64
    c = random_corpus(rng, n, dim)
    idx = build_index(c)
    model = Model(c["emb"], c["created"], c["contents"])
    h, E = P.native.hip, P.native.ORR_EINVAL
    B, k = 2, 4
    q = rng.standard_normal((B, dim)).astype(np.float32)
    pool, toff, qoff = P.pack_terms([P.text.query_terms("alpha"), []])
    ids = np.arange(5, dtype=np.int64)
    rows, scores, counts = np.full((B, k), 7, np.int64), np.zeros((B, k)), np.zeros(B, np.int32)
    recs, live = np.zeros((B, k + 1, 56), np.uint8), np.zeros(B, np.int64)
    bad = {"decrease": np.array([0, 4, 3], np.uint64), "end early": np.array([0, 2, 4], np.uint64),
           "end late": np.array([0, 2, 6], np.uint64), "start late": np.array([1, 2, 5], np.uint64)}

    def batch(n_ids, p_ids, p_off):
        return h.orr_search_batch_scoped(idx._h, B, dim, q.ctypes.data, pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, NOW, k, 300,
                                         n_ids, p_ids, p_off, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data)

    def shard(n_ids, p_ids, p_off):
        return h.orr_search_shard_scoped(idx._h, B, dim, q.ctypes.data, pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, NOW, k, 300, 0,
                                         n_ids, p_ids, p_off, None, recs.ctypes.data)

    def count(n_ids, p_ids, p_off):
        return h.orr_index_scope_count(idx._h, B, n_ids, p_ids, p_off, live.ctypes.data)

    for name, call in (("orr_search_batch_scoped", batch), ("orr_search_shard_scoped", shard), ("orr_index_scope_count", count)):
        assert call(-1, ids.ctypes.data, None) == E and name.encode() in h.orr_last_error()
        assert call(5, None, None) == E and name.encode() in h.orr_last_error()
        for what, off in bad.items():
            assert call(5, ids.ctypes.data, off.ctypes.data) == E, (name, what)
            assert name.encode() in h.orr_last_error() and b"scope_off" in h.orr_last_error()
    assert (rows == 7).all()                                                 # nothing was written
    assert h.orr_search_shard_scoped(idx._h, B, dim, q.ctypes.data, pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, NOW, 0, 300, 0,
                                     5, ids.ctypes.data, None, None, recs.ctypes.data) == E          # k' < 1
    # the handle answers afterwards
    _check_batch(idx, model, model.sub(ids), list(q), ["alpha", ""], 10, n, ids)
    idx.close()


def test_an_id_carried_by_several_rows_brings_every_live_one():
    P = pkg()
    rng = np.random.default_rng(41)
    n, dim = 2000, 64
    c = random_corpus(rng, n, dim)
    ids = (np.arange(n, dtype=np.int64) // 2) * 5 - 100                       # every id twice, some negative
    model = Model(c["emb"], c["created"], c["contents"], ids)
    idx = P.RecallIndex(dim=dim)
    present = [r for r in range(n) if c["emb"][r] is not None]
    absent = [r for r in range(n) if c["emb"][r] is None]
    idx.append(np.stack([c["emb"][r] for r in present]), c["created"][present], [P.text.lower_invariant(c["contents"][r]) for r in present], row_ids=ids[present])
    idx.append(None, c["created"][absent], [P.text.lower_invariant(c["contents"][r]) for r in absent], row_ids=ids[absent])
    idx.seal()
    order = present + absent                                                 # append order: what the oracle must see
    model = Model([c["emb"][r] for r in order], c["created"][order], [c["contents"][r] for r in order], ids[order])
    one = np.array([ids[10]])
    assert list(idx.scope_count(one)) == [2]
    q = rng.standard_normal(dim).astype(np.float32)
    rows, _, counts = _check_batch(idx, model, model.sub(one), [q], ["alpha"], 10, n, one)
    assert counts[0] == 2 and list(rows[0, :2]) == [ids[10], ids[10]]
    some = np.unique(ids[rng.choice(n, 150, replace=False)])
    assert list(idx.scope_count(some)) == [2 * len(some)]
    for topk, limit in ((10, n), (10, 31), (80, n)):
        _check_batch(idx, model, model.sub(some), [q] * len(TEXTS), TEXTS, topk, limit, some)
    # one of the two rows of an id is deleted through its position in the batch of deletes: both go (delete is by id)
    assert idx.delete_rows([int(some[0])]) == 2
    model.deleted |= set(int(r) for r in np.nonzero(model.ids == some[0])[0])
    assert list(idx.scope_count(some)) == [2 * len(some) - 2]
    _check_batch(idx, model, model.sub(some), [q] * len(TEXTS), TEXTS, 10, n, some)
    idx.close()


def test_maintenance_in_place_keeps_scoped_searches_exact(tmp_path):
    P = pkg()
    rng = np.random.default_rng(42)
    n, dim = 5000, 256
    c = random_corpus(rng, n, dim)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    idx = P.RecallIndex(dim=dim)
    lower = [P.text.lower_invariant(s) for s in c["contents"]]
    r = 0
    while r < n:                                                               # runs of rows with / without an embedding
        has, e = c["emb"][r] is not None, r
        while e < n and (c["emb"][e] is not None) == has:
            e += 1
        idx.append(np.stack(c["emb"][r:e]) if has else None, c["created"][r:e], lower[r:e], row_ids=ids[r:e])
        r = e
    idx.seal()
    model = Model(c["emb"], c["created"], c["contents"], ids)
    # the file's bytes do not depend on scoped searches: the id table is not saved
    idx.save(str(tmp_path / "a.orr"))
    scope = ids[rng.choice(n, 700, replace=False)]
    qv = [rng.standard_normal(dim).astype(np.float32), c["emb"][next(r for r in range(n) if c["emb"][r] is not None)].copy()]
    vecs, texts = [v for v in qv for _ in TEXTS], TEXTS * 2

    def check(handle, what):
        sub = model.sub(scope)
        assert list(handle.scope_count(scope)) == [len(sub[0])], what
        for topk, limit in ((10, n), (10, 300), (10, len(sub[0]) - 1), (70, n), (1, 1)):
            _check_batch(handle, model, sub, vecs, texts, topk, limit, scope, what=what)
        return sub

    check(idx, "fresh")
    idx.save(str(tmp_path / "b.orr"))
    assert open(str(tmp_path / "a.orr"), "rb").read() == open(str(tmp_path / "b.orr"), "rb").read()
    # deleted rows inside the scope neither rank nor count towards candidate_limit
    top = idx.search_scoped(np.stack(qv), [P.text.query_terms("alpha")] * 2, NOW, 5, scope, candidate_limit=n)[0]
    victims = set(int(x) for x in top.ravel() if x >= 0) | set(int(x) for x in scope[:60]) | set(int(x) for x in ids[rng.choice(n, 200, replace=False)])
    assert idx.delete_rows(sorted(victims)) == len(victims)
    model.deleted |= set(int(r) for r in np.nonzero(np.isin(ids, list(victims)))[0])
    sub = check(idx, "after deletes")
    assert not (set(int(model.ids[r]) for r in sub[0]) & victims)
    # reindex in place: the new vectors are used
    upd = scope[100:160]
    new_vecs = rng.standard_normal((len(upd), dim)).astype(np.float32)
    written = idx.update_rows(upd, new_vecs)
    pos_of = {int(i): r for r, i in enumerate(model.ids)}
    live_upd = [(j, pos_of[int(i)]) for j, i in enumerate(upd) if pos_of[int(i)] not in model.deleted]
    assert written == len(live_upd)
    for j, r in live_upd:
        model.emb[r] = new_vecs[j]
    vecs[0] = new_vecs[live_upd[0][0]].copy()                                # a query that is one of the new vectors
    check(idx, "after update_rows")
    # compaction moves positions: the id table is rebuilt
    assert idx.compact() == len(model.deleted)
    live = [r for r in range(len(model.ids)) if r not in model.deleted]
    model = Model([model.emb[r] for r in live], model.created[live], [model.contents[r] for r in live], model.ids[live])
    check(idx, "after compact")
    # rows inserted into the sealed shard, some of them into the scope
    m = 300
    add = random_corpus(rng, m, dim)
    add_ids = np.arange(m, dtype=np.int64) + 10 ** 6
    add_emb = np.stack([e if e is not None else np.zeros(dim, np.float32) for e in add["emb"]])
    assert idx.insert_rows(add_emb, add["created"], [P.text.lower_invariant(s) for s in add["contents"]], row_ids=add_ids) == m
    model = Model(model.emb + [e for e in add_emb], np.concatenate([model.created, add["created"]]), model.contents + add["contents"],
                  np.concatenate([model.ids, add_ids]))
    scope = np.concatenate([scope, add_ids[::3]])
    check(idx, "after insert_rows")
    # a view answers scoped searches; the shard file round trip
    view = idx.view()
    check(view, "view")
    view.close()
    idx.save(str(tmp_path / "c.orr"))
    idx.close()
    again = P.RecallIndex.load(str(tmp_path / "c.orr"))
    check(again, "loaded")
    again.save(str(tmp_path / "d.orr"))
    assert open(str(tmp_path / "c.orr"), "rb").read() == open(str(tmp_path / "d.orr"), "rb").read()
    again.close()


def _large(rng, n, dim):
    P = pkg()
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    created = np.sort(NOW - rng.integers(0, 300 * DAY, n))[::-1].astype(np.int64)
    words = np.array(["alpha", "beta", "gamma", "delta", "kubernetes", "helm", "azure", "cosmos"])
    contents = [" ".join(w) for w in words[rng.integers(0, len(words), (n, 5))]]
    idx = P.RecallIndex(dim=dim)
    for r0 in range(0, n, 50_000):
        idx.append(emb[r0:r0 + 50_000], created[r0:r0 + 50_000], [s.encode() for s in contents[r0:r0 + 50_000]])
    idx.seal()
    return idx, Model(list(emb), created, contents), emb


@pytest.mark.parametrize("n,dim", [(200_000, 128), (20_000, 3072)])
def test_scopes_on_a_two_stage_sized_shard(n, dim):
    P = pkg()
    rng = np.random.default_rng(50 + dim)
    idx, model, emb = _large(rng, n, dim)
    # a fresh large shard: a scoped search builds no shadow and runs no pass over all rows
    first = rng.choice(n, 2000, replace=False).astype(np.int64)
    q0 = rng.standard_normal((3, dim)).astype(np.float32)
    idx.set_profiling(1)
    _check_batch(idx, model, model.sub(first), list(q0), TEXTS[:3], 10, n, first, threads=8)
    names = idx.kernel_stats().keys()
    idx.set_profiling(0)
    assert not [k for k in names if k.startswith(("screen", "gemm", "gemv")) or k == "dot_exact"], sorted(names)
    # (the kernel names above are the evidence that nothing read a shadow or ran over all rows: every screen and every pass over
    # all rows has one of those names, and pass_mode never held 1 .. 3.  The shadow's build itself is not a timed launch; it is
    # only reached from the plan of an unscoped pass, from "two_stage" = 1 set explicitly and from the making of a lane)
    assert idx.search_stats()["pass_mode"] == 4
    idx.set_option("two_stage", 1)                                          # the int8 shadow, built now
    n_scopes = 6
    for B in (40, 300):
        planted = rng.integers(0, n, B)
        qs = (emb[planted] + 0.2 * rng.standard_normal((B, dim))).astype(np.float32)
        texts = [TEXTS[b % len(TEXTS)] for b in range(B)]
        terms = [P.text.query_terms(t) for t in texts]
        before = idx.search(qs, terms, NOW, 10, candidate_limit=n)
        assert (before[0][:, 0] == planted).all()
        assert idx.search_stats()["pass_mode"] != 4
        # scopes of about 2,000 rows in runs of 25 consecutive positions; query b uses scope b % n_scopes
        base = []
        for j in range(n_scopes):
            starts = rng.choice(n // 25, 80, replace=False) * 25
            base.append(np.unique((starts[:, None] + np.arange(25)[None, :]).ravel()))
        inside = [np.unique(np.concatenate([base[j], planted[j::n_scopes]])).astype(np.int64) for j in range(n_scopes)]
        outside = [np.setdiff1d(base[j], planted).astype(np.int64) for j in range(n_scopes)]
        for kind, family in (("with the planted best", inside), ("without it", outside)):
            subs_j = [model.sub(s) for s in family]
            scopes = [family[b % n_scopes] for b in range(B)]
            subs = [subs_j[b % n_scopes] for b in range(B)]
            idx.reset_search_stats()
            idx.set_profiling(1)
            rows, _, counts = _check_batch(idx, model, subs, list(qs), texts, 10, n, scopes, what=kind, threads=8)
            names = idx.kernel_stats().keys()
            idx.set_profiling(0)
            assert not [k for k in names if k.startswith(("screen", "gemm", "gemv")) or k == "dot_exact"], sorted(names)
            st = idx.search_stats()
            assert st["pass_mode"] == 4 and st["exact_pass_queries"] == 0 and st["buffer_growths"] == 0, st
            assert (counts == 10).all()
            hit = rows[:, 0] == planted
            assert hit.all() if kind == "with the planted best" else not hit.any()
            _check_batch(idx, model, subs, list(qs), texts, 60, 300, scopes, what=kind + ", limit 300", threads=8)
        after = idx.search(qs, terms, NOW, 10, candidate_limit=n)             # the unscoped path is untouched
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
    idx.close()


def test_six_threads_mix_scoped_and_unscoped_searches_on_one_handle():
    P = pkg()
    rng = np.random.default_rng(61)
    n, dim = 6000, 128
    c = random_corpus(rng, n, dim)
    idx = build_index(c, chunk=2000)
    jobs = []
    for t in range(6):
        B = [1, 7, 40][t % 3]
        qs = rng.standard_normal((B, dim)).astype(np.float32)
        terms = [P.text.query_terms(TEXTS[(t + b) % len(TEXTS)]) for b in range(B)]
        scopes = [rng.choice(n, int(rng.integers(1, 900)), replace=False).astype(np.int64) for _ in range(B)]
        jobs.append((qs, terms, scopes))

    def run(handle, job, scoped):
        qs, terms, scopes = job
        if scoped:
            return handle.search_scoped(qs, terms, NOW, 10, scopes, candidate_limit=300)
        return handle.search(qs, terms, NOW, 10, candidate_limit=300)

    serial = [(run(idx, job, True), run(idx, job, False)) for job in jobs]
    results, errors = [None] * 6, []

    def worker(t):
        try:
            out = []
            for rep in range(8):
                out.append((run(idx, jobs[t], True), run(idx, jobs[t], False)) if (t + rep) % 2 else (None, run(idx, jobs[t], False)))
                out.append((run(idx, jobs[t], True), None))
            results[t] = out
        except Exception as e:                                               # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(6):
        for sc, un in results[t]:
            for got, want in ((sc, serial[t][0]), (un, serial[t][1])):
                if got is not None:
                    assert np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2]), t
    view = idx.view()                                                        # a caller's view answers scoped searches
    got = run(view, jobs[2], True)
    assert np.array_equal(got[0], serial[2][0][0]) and _same(got[1], serial[2][0][1])
    view.close()
    idx.close()


def test_three_shards_scope_count_shard_records_and_the_unchanged_merge():
    P = pkg()
    rng = np.random.default_rng(71)
    n, dim = 6000, 64
    c = random_corpus(rng, n, dim, sorted_created=True)
    c["created"] = np.sort(NOW - rng.choice(400 * DAY, n, replace=False))[::-1].astype(np.int64)   # distinct: the split is unambiguous
    model = Model(c["emb"], c["created"], c["contents"])
    cuts = [0, 1000, 3700, n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sub = {"emb": c["emb"][lo:hi], "created": c["created"][lo:hi], "contents": c["contents"][lo:hi], "dim": dim}
        parts.append(build_index(sub, row_base=lo))
    dead = sorted(int(r) for r in rng.choice(n, 200, replace=False))
    for p, (lo, hi) in zip(parts, zip(cuts[:-1], cuts[1:])):
        p.delete_rows([r for r in dead if lo <= r < hi])
    model.deleted |= set(dead)
    B = 4
    qs = rng.standard_normal((B, dim)).astype(np.float32)
    texts = TEXTS[:B]
    terms = [P.text.query_terms(t) for t in texts]
    wide = rng.choice(n, 1200, replace=False).astype(np.int64)               # 300 of its live rows end inside the second shard
    scopes = [wide, rng.choice(np.arange(cuts[1], cuts[2]), 400, replace=False).astype(np.int64),      # one shard only
              np.zeros(0, np.int64), np.concatenate([wide[:500], [n + 5, -2]])]
    subs = [model.sub(s) for s in scopes]
    live = np.stack([p.scope_count(scopes, B) for p in parts])
    assert list(live.sum(axis=0)) == [len(k) for k, _ in subs]
    assert live[0, 0] < 300 < live[0, 0] + live[1, 0]                        # the global limit falls inside the second shard
    assert live[0, 1] == 0 and live[2, 1] == 0 and live[1, 1] > 0
    before = np.concatenate([np.zeros((1, B), np.int64), np.cumsum(live, axis=0)[:-1]])
    for topk, limit in ((10, 300), (10, n), (40, 300), (5, 1), (100, n)):
        kp = 32 if topk < 64 else 128
        while True:                                                           # the escalation every multi-shard caller runs
            recs = np.stack([p.search_shard_scoped(qs, terms, NOW, kp, limit, scopes, scope_before=before[g], topk=topk)
                             for g, p in enumerate(parts)])
            rows, scores, counts, unc = P.merge_candidates(recs, dim, qs, terms, NOW, topk)
            if unc == 0 or kp >= n:
                break
            kp *= 4
        assert unc == 0
        trailers = recs[:, :, kp]
        assert (trailers["flags"] == 1).all()                                 # trailer, no two-stage floor
        took = np.minimum(live, np.maximum(0, max(1, limit) - before))
        assert np.array_equal(trailers["order_key"], took)
        valid = recs[:, :, :kp]["row_id"] >= 0
        assert ((recs[:, :, :kp]["flags"] & 2) != 0)[valid].all()             # ORR_CAND_DOT_EXACT
        for b in range(B):
            want_rows, want_scores = _expect(model, subs[b][0], subs[b][1], qs[b], texts[b], topk, limit)
            assert list(rows[b, :counts[b]]) == want_rows, (b, topk, limit)
            assert _same(scores[b, :counts[b]], want_scores), (b, topk, limit)
    for p in parts:
        p.close()


_TIE_CORPORA = {}


def _tie_corpus(dim):
    """600 rows of which 200 (positions 150 .. 349) are one row repeated: embedding, created and content.  Returns the corpus
    with its model, the two scopes of the ladder test and their oracles, computed once per dimension."""
    if dim not in _TIE_CORPORA:
        rng = np.random.default_rng(80 + dim)
        n = 600
        c = random_corpus(rng, n, dim)
        same = np.arange(150, 350)
        vec = rng.standard_normal(dim).astype(np.float32)
        for r in same:
            c["emb"][r] = vec.copy()
            c["created"][r] = NOW - 30 * DAY
            c["contents"][r] = "alpha kubernetes helm chart"
        # 100 ordinary rows with pairwise distinct `created` (and none of the 200): no two of them tie without a vector either
        ordinary = np.setdiff1d(np.arange(n), same)
        ordinary = ordinary[c["created"][ordinary] != NOW - 30 * DAY]
        _, first = np.unique(c["created"][ordinary], return_index=True)
        plain = np.sort(ordinary[first])[:100].astype(np.int64)
        assert len(plain) == 100
        model = Model(c["emb"], c["created"], c["contents"])
        scopes = [same.astype(np.int64), plain]
        _TIE_CORPORA[dim] = (c, model, scopes, [model.sub(s) for s in scopes], rng.standard_normal((2, dim)).astype(np.float32))
    return _TIE_CORPORA[dim]


@pytest.mark.parametrize("with_vectors", [True, False])
@pytest.mark.parametrize("dim", [3, 64, 256])                                # generic re-score, four-launch tail, one-launch tail
def test_a_scope_of_identical_rows_climbs_the_ladder_to_all_records(dim, with_vectors):
    c, model, scopes, subs, q = _tie_corpus(dim)
    idx = build_index(c)
    idx.reset_search_stats()
    _check_batch(idx, model, subs, list(q) if with_vectors else None, ["the kubernetes helm", "alpha"], 10, len(c["created"]), scopes,
                 what="ties")                                                # (the ties in candidate order: the oracle's order)
    st = idx.search_stats()
    # Two queries of at most 200 scoped rows are one part of one slice.  Both start at k' = 32 (Selection).  Query 1's 100 rows
    # score differently, so it is certified at once.  Query 0's 200 rows score alike: its 10th score equals the cut-off, it is
    # not certified, and its next rung 4 x 32 = 128 > 64 is AllRecords, which certifies by construction: two passes, the second
    # with one query; no rung of the unscoped ladder (no grown buffer, no exact pass over all rows).
    assert st["pass_mode"] == 4 and st["passes"] == 2 and st["requeried"] == 1, st
    assert st["exact_pass_queries"] == 0 and st["buffer_growths"] == 0, st
    idx.close()
