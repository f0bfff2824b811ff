"""Masked search (orr_search_batch_masked): ONE scope shared by every query of the batch, applied as a mask inside the
two-stage screen.  The contract is the scoped call's for a shared list: the result is what orr_search_batch returns on a
shard sealed from scratch from only the live rows of the scope, in their present candidate order -- so the oracle runs on
that sub-corpus (the method of test_gpu_scoped_search.py) and its row numbers are mapped back.  Rows, order and fp64 scores
must match bit for bit.

Shapes: 200,000 rows is the smallest shard on which the two-stage screen runs at all (196,608 rows); dim 128 takes the
int8 shadow (stream for 1..4 queries, eight-wave GEMM above), dim 192 the bf16 shadow, dim 512 the four-wave (B = 100) and
the 16 x 16 x 64 (B = 300) forms of the int8 GEMM.  The oracle is a CPU pass over the sub-corpus per query, so every query's
count is checked but rows and scores are compared for a stated subset of the batch: all of it up to 8 queries, 12 of 40,
17 of 100, and 52 of 300 (every sixth query, the second and the last: each tile of 32 queries has at least five); the oracle's answers
are computed once per (shard, scope, query) and shared by the batch sizes."""
import importlib
import threading

import numpy as np
import pytest

from helpers import orc, pkg

pytestmark = pytest.mark.gpu

N = 200_000
POOL_Q = 300


class Model:
    """The corpus as the test knows it: rows in candidate order with their ids; deleted rows are remembered."""

    def __init__(self, emb, created, rowbytes, ids):
        self.emb, self.created, self.rowbytes, self.ids = emb, np.asarray(created, np.int64).copy(), rowbytes, np.asarray(ids, np.int64).copy()
        self.deleted = set()

    def live_rows(self, scope_ids):
        want = np.isin(self.ids, np.asarray(scope_ids, np.int64))
        if self.deleted:
            want[np.fromiter(self.deleted, np.int64)] = False
        return np.nonzero(want)[0]

    def sub(self, scope_ids):
        """(rows of the scope that are live, oracle over exactly those) -- None without a row."""
        keep = self.live_rows(scope_ids)
        if len(keep) == 0:
            return keep, None
        width = self.rowbytes.shape[1]
        off = np.arange(len(keep) + 1, dtype=np.int64) * width
        return keep, orc.OracleCorpus(np.ascontiguousarray(self.emb[keep]), self.created[keep], (np.ascontiguousarray(self.rowbytes[keep]).reshape(-1), off))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _syn():
    return importlib.import_module("omni_recall_rag_amd.synthetic")


def _make(dim, n=N, edit=None):
    """A synthetic shard of n rows (candidate order = row order), its model, the query pool."""
    import torch
    P, syn = pkg(), _syn()
    emb = syn.embeddings(0, n, dim, "cuda:0").cpu().numpy()
    created = syn.created_ticks(0, n, n).numpy()
    pool, _ = syn.contents(0, n, "cuda:0")
    rowbytes = pool.reshape(n, syn.ROW_BYTES).cpu().numpy()
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    if edit:
        edit(emb, created)
    idx = P.RecallIndex(dim=dim, capacity_rows=n)
    off = np.arange(n + 1, dtype=np.int64) * syn.ROW_BYTES
    step = 50_000
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        idx.append(emb[r0:r1], created[r0:r1], rowbytes[r0:r1].reshape(-1), off[: r1 - r0 + 1], row_ids=ids[r0:r1])
    idx.seal()
    torch.cuda.synchronize()
    q = syn.query_vectors(0, POOL_Q, dim, n).numpy()
    texts = syn.query_texts(0, POOL_Q, n)
    return idx, Model(emb, created, rowbytes, ids), q, texts


_SHARDS, _ORACLE = {}, {}


def _shard(dim):
    """One shard per dimension for the whole module, with its scope families (row positions) and planted queries."""
    if dim in _SHARDS:
        return _SHARDS[dim]
    idx, model, q, texts = _make(dim)
    rng = np.random.default_rng(500 + dim)
    starts = rng.choice(N // 25, N // 500, replace=False) * 25
    fam = {
        "random 10 %": np.sort(rng.choice(N, N // 10, replace=False)),
        "older half": np.arange(N // 2, N),                                   # no row of the newest prefix: a prefix floor would be wrong
        "runs of 25": np.sort((starts[:, None] + np.arange(25)[None, :]).reshape(-1)),
    }
    plants = {}
    for name, rows in fam.items():
        inside = int(rows[len(rows) // 3])
        in_scope = set(rows.tolist())
        outside = next(r for r in range(N // 2 - 1, -1, -1) if r not in in_scope)
        qq = q.copy()
        noise = rng.standard_normal((2, dim)).astype(np.float32) * np.float32(0.01)
        qq[0] = model.emb[inside] + noise[0]                                   # a near-duplicate inside the scope: ranks first
        qq[1] = model.emb[outside] + noise[1]                                  # ... and outside: must not appear
        plants[name] = (qq, inside, outside)
    _SHARDS[dim] = (idx, model, texts, fam, plants)
    return _SHARDS[dim]


def _checked(B):
    if B <= 8:
        return list(range(B))
    if B <= 40:
        return sorted(set(range(8)) | {B // 2, B - 9, B - 8, B - 1})
    if B <= 100:
        return sorted(set(range(0, B, 7)) | {1, B - 1})
    return sorted(set(range(0, B, 6)) | {1, B - 1})


def _oracle(key, model, sub, qvec, text, topk, limit):
    """The oracle's (ids, scores) for one query, once per key; a top-40 answer serves every smaller topk at the same limit."""
    syn = _syn()
    keep, corpus = sub
    if corpus is None:
        return [], np.zeros(0)
    k_run = 40 if topk <= 40 else topk
    full = key + (k_run, limit)
    if full not in _ORACLE:
        orow, osc, _ = corpus.search(qvec, text, syn.NOW_TICKS, k_run, candidate_limit=limit, threads=16)
        _ORACLE[full] = ([int(model.ids[keep[r]]) for r in orow], np.asarray(osc))
    rows, scores = _ORACLE[full]
    k = max(1, topk)
    return rows[:k], scores[:k]


def _search(idx, q, texts, topk, limit, scope_ids, how="masked"):
    P, syn = pkg(), _syn()
    terms = [P.text.query_terms(t) for t in texts]
    fn = {"masked": idx.search_masked, "scoped": idx.search_scoped}[how]
    return fn(np.ascontiguousarray(q, dtype=np.float32), terms, syn.NOW_TICKS, topk, scope_ids, candidate_limit=limit)


def _check(key, idx, model, sub, q, texts, topk, limit, scope_ids, checked, what):
    rows, scores, counts = _search(idx, q, texts, topk, limit, scope_ids)
    took = min(len(sub[0]), max(1, limit))
    assert (counts == min(max(1, topk), took)).all(), (what, topk, limit, counts[:8], took)
    for b in checked:
        want_rows, want_scores = _oracle(key + (b,), model, sub, q[b], texts[b], topk, limit)
        k = int(counts[b])
        assert list(rows[b, :k]) == want_rows, (what, b, topk, limit, list(rows[b, :k])[:6], want_rows[:6])
        assert _same(scores[b, :k], want_scores), (what, b, topk, limit)
    return rows, scores, counts


SCREENS = ("screen_i8_fused", "screen_gemv_i8", "screen_gemv_bf16", "screen_bf16_fused", "gemm_dot_bf16x1_fused")
NEW_KERNELS = ("mask_clip", "row_consts_masked", "mask_survivors", "mask_sample_rescore")


@pytest.mark.parametrize("dim,B,five_terms,screen", [
    (128, 1, False, "screen_gemv_i8"), (128, 3, False, "screen_gemv_i8"), (128, 8, False, "screen_i8_fused"), (128, 40, False, "screen_i8_fused"),
    (192, 2, False, "screen_gemv_bf16"), (192, 40, False, "screen_bf16_fused"),
    (512, 100, False, "screen_i8_fused"), (512, 300, False, "screen_i8_fused"), (512, 300, True, "screen_i8_fused")])
def test_masked_search_equals_the_oracle_on_the_sub_corpus(dim, B, five_terms, screen):
    idx, model, texts_all, fam, plants = _shard(dim)
    syn = _syn()
    texts = list(texts_all[:B])
    if five_terms:
        texts[5] = texts[5] + " " + texts[6].split()[1] + " " + texts[7].split()[1]     # five terms: four-bit count words
    tag = "5t" if five_terms else ""
    # an unscoped search before ... and after: the masked passes leave it alone
    before = idx.search(plants["older half"][0][:B], [pkg().text.query_terms(t) for t in texts], syn.NOW_TICKS, 10, candidate_limit=N)
    for name, rows_of in fam.items():
        q_all, inside, outside = plants[name]
        q = q_all[:B]
        scope = model.ids[rows_of]
        sub = model.sub(scope)
        s = len(sub[0])
        key = (dim, name, tag)
        idx.set_option("mask_screen", 1)
        idx.reset_search_stats()
        idx.set_profiling(True)
        rows, scores, counts = _check(key, idx, model, sub, q, texts, 10, N, scope, _checked(B), name)
        stats = idx.kernel_stats()
        idx.set_profiling(False)
        st = idx.search_stats()
        assert st["pass_mode"] == 5 and st["exact_pass_queries"] == 0, (name, st)
        assert screen in stats and all(k in stats for k in NEW_KERNELS), (name, sorted(stats))
        assert "fuse_select" not in stats and "screen_i8_prefix" not in stats and "screen_gemv_prefix" not in stats and "gemm_dot_bf16x3" not in stats
        assert rows[0, 0] == model.ids[inside]                                   # the planted near-duplicate inside the scope ranks first
        if B > 1:
            assert model.ids[outside] not in rows[1]                             # ... the one outside never appears
        few = _checked(B)[:2] if B > 8 else _checked(B)
        _check(key, idx, model, sub, q, texts, 40, N, scope, _checked(B), name)
        _check(key, idx, model, sub, q, texts, 10, s - 1, scope, few, name)
        _check(key, idx, model, sub, q, texts, 10, s // 2 + 7, scope, few, name)  # a limit that falls mid-scope
        # through the list path: a scope clipped below the screen's size, and topk beyond a selection list
        idx.reset_search_stats()
        _check(key, idx, model, sub, q, texts, 60, 300, scope, few, name)
        if name == "runs of 25" and B <= 40:       # (every pair a record: kept to the smallest scope and the small batches)
            _check(key, idx, model, sub, q, texts, 70, N, scope, few[:1], name)
        assert idx.search_stats()["pass_mode"] == 4
        # mask_screen = 2: the list path, identical outputs
        idx.set_option("mask_screen", 2)
        idx.reset_search_stats()
        r2, s2, c2 = _search(idx, q, texts, 10, N, scope)
        assert idx.search_stats()["pass_mode"] == 4
        assert np.array_equal(r2, rows) and _same(s2, scores) and np.array_equal(c2, counts), name
        idx.set_option("mask_screen", 0)
    after = idx.search(plants["older half"][0][:B], [pkg().text.query_terms(t) for t in texts], syn.NOW_TICKS, 10, candidate_limit=N)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def _adversarial_shard():
    """200,000 x 128 with: 20,000 rows identical to query 0 outside the scope, 20,000 identical rows of one timestamp inside
    it (parallel to query 2), a row with an infinite component on either side."""
    if "adv" in _SHARDS:
        return _SHARDS["adv"]
    dim = 128
    syn = _syn()
    q = syn.query_vectors(0, 40, dim, N).numpy()
    out_same = np.arange(10_000, 30_000)                # 20,000 rows identical to query 0, outside the scope
    in_same = np.arange(120_000, 140_000)               # 20,000 identical rows inside the scope (the older half)

    def edit(emb, created):
        emb[out_same] = q[0]
        emb[in_same] = q[2] * np.float32(0.5)
        created[in_same] = created[in_same[0]]          # one timestamp: equal scores, far more of them than a selection list holds
        emb[5, 3] = np.inf
        emb[150_000, 3] = np.inf
    idx, model, _, texts = _make(dim, edit=edit)
    _SHARDS["adv"] = (idx, model, q, texts)
    return _SHARDS["adv"]


@pytest.mark.parametrize("B", [8, 40])
def test_adversarial_queries_and_rows(B):
    idx, model, q_all, texts_all = _adversarial_shard()
    q, texts = q_all[:B].copy(), list(texts_all[:B])
    q[3] = np.nan
    q[4] = 0.0
    q[5, 7] = np.inf
    scope = model.ids[np.arange(N // 2, N)]
    sub = model.sub(scope)
    idx.set_option("mask_screen", 1)
    idx.reset_search_stats()
    rows, scores, counts = _check(("adv", B), idx, model, sub, q, texts, 10, N, scope, list(range(8)), "adversarial")
    st = idx.search_stats()
    # the 20,000 identical rows inside the scope tie at query 2's cut: its buffer overflows, grows, and the tie goes to the list path
    # (the index keeps the grown buffers: the second batch size of this test finds them in place)
    assert st["requeried"] >= 1 and st["exact_pass_queries"] == 0, st
    assert (st["overflowed_queries"] >= 1 and st["buffer_growths"] >= 1) or st["survivor_capacity"] >= 32768, st
    assert st["pass_mode"] == 4
    out_ids = set(int(x) for x in model.ids[:N // 2])
    assert not (set(int(x) for x in rows.ravel()) & out_ids)                     # nothing from outside the scope, identical to query 0 or not
    # the same with the list path in parts of 5,000 rows and a candidate_limit that ends inside the third part
    idx.set_option("mask_part_rows", 5000)
    idx.reset_search_stats()
    _check(("adv", B), idx, model, sub, q, texts, 10, 12_345, scope, list(range(8)), "parts, limit in the third")
    st3 = idx.search_stats()
    assert st3["pass_mode"] == 4 and st3["passes"] >= 3, st3
    idx.reset_search_stats()
    r5, s5, c5 = _search(idx, q, texts, 10, N, scope)
    assert np.array_equal(r5, rows) and _same(s5, scores) and np.array_equal(c5, counts)
    assert idx.search_stats()["passes"] >= 1 + 20                                # the ladder's end ran over 20 parts
    idx.set_option("mask_part_rows", 4194240)
    idx.set_option("mask_screen", 0)


def test_maintenance_keeps_masked_searches_exact():
    P, syn = pkg(), _syn()
    dim = 128
    idx, model, q_all, texts_all = _make(dim)
    B = 8
    q, texts = q_all[:B], list(texts_all[:B])
    rng = np.random.default_rng(77)
    scope_rows = np.sort(rng.choice(N, N // 8, replace=False))
    scope = model.ids[scope_rows].copy()
    idx.set_option("mask_screen", 1)
    step = [0]

    def check(what):
        step[0] += 1
        sub = model.sub(scope)
        idx.reset_search_stats()
        out = _check(("maint", step[0]), idx, model, sub, q, texts, 10, N, scope, [0, 1, 5], what)
        assert idx.search_stats()["pass_mode"] == 5, what
        return out

    rows0, _, _ = check("fresh")
    # delete: the winners and a slice of the scope
    victims = sorted(set(int(x) for x in rows0[:, :3].ravel()) | set(int(x) for x in scope[:500]))
    assert idx.delete_rows(victims) == len(victims)
    model.deleted |= set(int(r) for r in np.nonzero(np.isin(model.ids, victims))[0])
    check("after delete_rows")
    # update: new vectors for rows of the scope, one of them query 1 itself
    targets = scope[1000:1040]
    new = rng.standard_normal((len(targets), dim)).astype(np.float32)
    new[0] = q[1]
    assert idx.update_rows(targets, new) == len(targets)
    model.emb[np.searchsorted(model.ids, targets)] = new
    r1, _, _ = check("after update_rows")
    assert r1[1, 0] == targets[0]
    # insert: rows of older and newer timestamps, half of them in the scope (the id table is rebuilt)
    m = 64
    ins_emb = rng.standard_normal((m, dim)).astype(np.float32)
    ins_emb[3] = q[5]
    ins_created = np.sort(np.unique(rng.choice(model.created, m, replace=False)) + 1)[::-1].copy()     # between the shard's timestamps, old and new
    m = len(ins_created)
    ins_emb = ins_emb[:m]
    ins_ids = np.arange(m, dtype=np.int64) + 10_000_000
    ins_bytes = model.rowbytes[rng.choice(N, m, replace=False)].copy()
    off = np.arange(m + 1, dtype=np.int64) * ins_bytes.shape[1]
    assert idx.insert_rows(ins_emb, ins_created, ins_bytes.reshape(-1), off, row_ids=ins_ids) == m
    # the model in the new candidate order: created descending, stable, inserted rows behind equal timestamps
    all_created = np.concatenate([model.created, ins_created])
    order = np.argsort(-all_created, kind="stable")
    deleted_ids = model.ids[np.fromiter(model.deleted, np.int64)]
    model = Model(np.concatenate([model.emb, ins_emb])[order], all_created[order], np.concatenate([model.rowbytes, ins_bytes])[order],
                  np.concatenate([model.ids, ins_ids])[order])
    model.deleted = set(int(r) for r in np.nonzero(np.isin(model.ids, deleted_ids))[0])
    scope = np.concatenate([scope, ins_ids[: m // 2]])
    r2, _, _ = check("after insert_rows")
    assert r2[5, 0] == ins_ids[3]
    # compact: positions move again
    idx.compact()
    live = np.array(sorted(set(range(len(model.ids))) - model.deleted))
    model = Model(model.emb[live], model.created[live], model.rowbytes[live], model.ids[live])
    check("after compact")
    idx.close()


def test_unknown_ids_empty_scopes_argument_errors_and_views():
    P, syn = pkg(), _syn()
    idx, model, texts_all, fam, plants = _shard(128)
    q_all, _, _ = plants["random 10 %"]
    B = 3
    q, texts = q_all[:B], list(texts_all[:B])
    scope = model.ids[fam["random 10 %"]]
    sub = model.sub(scope)
    key = (128, "random 10 %", "")
    idx.set_option("mask_screen", 1)
    # unknown ids are skipped, repeats count once
    noisy = np.concatenate([scope, [5, -7, 2 ** 40], scope[:100]])
    _check(key, idx, model, sub, q, texts, 10, N, noisy, [0, 1, 2], "unknown ids")
    # an empty scope, a scope of unknown ids only
    for ids in (np.zeros(0, np.int64), np.array([4, 5, -1], np.int64)):
        rows, scores, counts = _search(idx, q, texts, 10, N, ids)
        assert (counts == 0).all() and (rows == -1).all()
    # a view answers as its owner
    v = idx.view()
    v.set_option("mask_screen", 1)
    rv = _search(v, q, texts, 10, N, scope)
    ro = _search(idx, q, texts, 10, N, scope)
    assert np.array_equal(rv[0], ro[0]) and _same(rv[1], ro[1]) and np.array_equal(rv[2], ro[2])
    v.close()
    # argument errors leave the index searchable
    h, E = P.native.hip, P.native.ORR_EINVAL
    pool, toff, qoff = P.pack_terms([P.text.query_terms(t) for t in texts])
    k = 4
    rows, scores, counts = np.full((B, k), 7, np.int64), np.zeros((B, k)), np.zeros(B, np.int32)
    ids = np.ascontiguousarray(scope[:5])
    qq = np.ascontiguousarray(q, dtype=np.float32)

    def call(handle, n_ids, p_ids, p_rows):
        return h.orr_search_batch_masked(handle, B, 128, qq.ctypes.data, pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, syn.NOW_TICKS, k, 300,
                                         n_ids, p_ids, p_rows, scores.ctypes.data, counts.ctypes.data)

    assert call(idx._h, -1, ids.ctypes.data, rows.ctypes.data) == E and b"orr_search_batch_masked" in h.orr_last_error()
    assert call(idx._h, 5, None, rows.ctypes.data) == E
    assert call(None, 5, ids.ctypes.data, rows.ctypes.data) == E
    assert call(idx._h, 5, ids.ctypes.data, None) == E
    assert (rows == 7).all()
    with pytest.raises(Exception):
        idx.set_option("mask_screen", 3)
    with pytest.raises(Exception):
        idx.set_option("mask_part_rows", 0)
    _check(key, idx, model, sub, q, texts, 10, N, scope, [0, 1, 2], "after the errors")
    # a deleted-only scope: counts of 0 (last: the deletes stay)
    gone = model.ids[[N - 1, N - 2, N - 3]]
    assert idx.delete_rows(gone) == 3
    model.deleted |= {N - 1, N - 2, N - 3}
    _ORACLE.clear()                                                              # the shard changed: no cached answer applies
    rows, scores, counts = _search(idx, q, texts, 10, N, gone)
    assert (counts == 0).all()
    idx.set_option("mask_screen", 0)


def test_six_threads_mix_masked_scoped_and_unscoped_searches():
    P, syn = pkg(), _syn()
    idx, model, texts_all, fam, plants = _shard(128)
    q_all, _, _ = plants["runs of 25"]
    terms_all = [P.text.query_terms(t) for t in texts_all]
    big = model.ids[fam["runs of 25"]]
    small = model.ids[fam["random 10 %"][:400]]
    idx.set_option("mask_screen", 1)
    idx.set_option("max_lanes", 6)

    def job(i):
        b0, B = 5 * i, (1, 3, 8, 40, 2, 8)[i]
        q, terms = np.ascontiguousarray(q_all[b0:b0 + B]), terms_all[b0:b0 + B]
        if i % 3 == 0:
            return idx.search_masked(q, terms, syn.NOW_TICKS, 10, big, candidate_limit=N)
        if i % 3 == 1:
            return idx.search_scoped(q, terms, syn.NOW_TICKS, 10, small, candidate_limit=N)
        return idx.search(q, terms, syn.NOW_TICKS, 10, candidate_limit=N)

    single = [job(i) for i in range(6)]
    got, errors = [None] * 6, []

    def run(i):
        try:
            for _ in range(3):
                got[i] = job(i)
        except Exception as e:                                                   # pragma: no cover
            errors.append((i, e))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(6):
        assert np.array_equal(got[i][0], single[i][0]) and _same(got[i][1], single[i][1]) and np.array_equal(got[i][2], single[i][2]), i
    idx.set_option("mask_screen", 0)
