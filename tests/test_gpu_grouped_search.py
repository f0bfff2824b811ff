"""Grouped masked search (orr_search_batch_masked_groups): G scopes, each shared by the queries that name it, screened together
in ONE two-stage pass.  The contract is the masked call's per query: query b's result is what orr_search_batch_masked returns
for it with its group's ids as the scope -- what orr_search_batch returns on a shard sealed from only the live rows of that
group.  So EVERY query is compared against search_masked run on its group's sub-batch (code the grouped call does not change),
and a stated subset against the oracle on the group's sub-corpus as well (the method of test_gpu_masked_search.py): all
queries up to 8, then that file's subsets (12 of 40, 17 of 100, 52 of 300).  Rows, order and fp64 scores match bit for bit.

The shard has 200,000 rows: the two-stage screen needs 196,608, nothing smaller reaches the new code.  Groups:
  A the older half (100,000 rows, sample 1,024 at topk 10)      B a random 10 % that overlaps A (20,000; 448)
  C 400 runs of 25 (10,000; 320)                                 D 200 random rows (a list group: no more rows than its sample)
  E empty                                                        F non-empty, named by no query
Queries go to A / B / C / D / E by b % 5, so every tile of 32 queries mixes groups.  mask_screen = 1 unless a test says otherwise.
Launches: the issue compares the screening kernel's launches with ONE search_masked call "at the same B".  The grouped pass
screens the queries of the screen groups only (b % 5 <= 2: the list group's and the empty group's queries take no part), so
the comparison call over group A runs with exactly those queries -- the batch the grouped pass really has -- not with all B.
The shapes are the masked test's: dim 128 with 3 queries (int8 stream), 8 and 40 (eight-wave GEMM), dim 192 with 40 (bf16
shadow), dim 512 with 100 (four-wave) and 300 (16 x 16 x 64)."""
import importlib
import threading

import numpy as np
import pytest

from helpers import orc, pkg

pytestmark = pytest.mark.gpu

N = 200_000
POOL_Q = 300
NAMES = "ABCDEF"
SHARED_ROW = 199_500          # a row A and B both hold, behind A's clip at candidate_limit = 99,000
A_ONLY_ROW = 160_003          # a row only A holds
NO_GROUP_ROW = 5              # a row no group holds


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


def _same3(x, y):
    return np.array_equal(x[0], y[0]) and _same(x[1], y[1]) and np.array_equal(x[2], y[2])


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


def _group_rows(seed, b_without=None):
    """The six groups as row positions.  B holds SHARED_ROW and not A_ONLY_ROW; only A holds A_ONLY_ROW; nobody holds
    NO_GROUP_ROW; b_without: rows B must not hold."""
    rng = np.random.default_rng(seed)
    starts = rng.choice(N // 25, 400, replace=False) * 25
    drop = {A_ONLY_ROW, NO_GROUP_ROW}
    b = set(rng.choice(N, N // 10, replace=False).tolist()) - drop
    if b_without is not None:
        b -= set(np.asarray(b_without).tolist())
    b.add(SHARED_ROW)
    rows = [
        np.arange(N // 2, N),
        np.array(sorted(b)),
        np.sort((starts[:, None] + np.arange(25)[None, :]).reshape(-1)),
        np.sort(rng.choice(N, 200, replace=False)),
        np.zeros(0, np.int64),
        np.sort(rng.choice(N, 5_000, replace=False)),
    ]
    return [r if i == 0 else np.array([x for x in r.tolist() if x not in drop], np.int64) for i, r in enumerate(rows)]


_SHARDS, _ORACLE = {}, {}


def _shard(dim):
    """One shard per dimension for the whole module, with its groups (row positions, id lists) and the groups' oracles."""
    if dim not in _SHARDS:
        idx, model, q, texts = _make(dim)
        rows = _group_rows(900 + dim)
        scopes = [model.ids[r] for r in rows]
        _SHARDS[dim] = (idx, model, q, texts, rows, scopes, [model.sub(s) for s in scopes])
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


def _terms(texts):
    P = pkg()
    return [P.text.query_terms(t) for t in texts]


def _grouped(idx, q, texts, topk, limit, scopes, qg):
    return idx.search_masked_groups(np.ascontiguousarray(q, dtype=np.float32), _terms(texts), _syn().NOW_TICKS, topk, scopes, qg, candidate_limit=limit)


def _masked(idx, q, texts, topk, limit, scope):
    return idx.search_masked(np.ascontiguousarray(q, dtype=np.float32), _terms(texts), _syn().NOW_TICKS, topk, scope, candidate_limit=limit)


def _assign(B):
    return np.arange(B, dtype=np.int32) % 5


LAST = {}                     # search_stats right behind the grouped call of the last _check (the masked calls it compares with count too)


def _check(key, idx, model, subs, q, texts, topk, limit, scopes, qg, checked, what):
    """The grouped call against search_masked per group (every query) and against the oracle (the checked ones)."""
    rows, scores, counts = _grouped(idx, q, texts, topk, limit, scopes, qg)
    LAST.clear()
    LAST.update(idx.search_stats())
    qg = np.asarray(qg)
    for g in sorted(set(qg.tolist())):
        mine = np.nonzero(qg == g)[0]
        took = min(len(subs[g][0]), max(1, limit))
        assert (counts[mine] == min(max(1, topk), took)).all(), (what, NAMES[g], topk, limit, counts[mine][:8], took)
        mr, ms, mc = _masked(idx, q[mine], [texts[b] for b in mine], topk, limit, scopes[g])
        assert np.array_equal(rows[mine], mr) and _same(scores[mine], ms) and np.array_equal(counts[mine], mc), (what, NAMES[g], topk, limit)
    for b in checked:
        g = int(qg[b])
        want_rows, want_scores = _oracle(key + (NAMES[g], b), model, subs[g], q[b], texts[b], topk, limit)
        k = int(counts[b])
        assert list(rows[b, :k]) == want_rows, (what, b, NAMES[g], topk, limit, list(rows[b, :k])[:6], want_rows[:6])
        assert _same(scores[b, :k], want_scores), (what, b, NAMES[g], topk, limit)
    return rows, scores, counts


def _kernel_stats(idx):
    """Launches per timed name (RecallIndex.kernel_stats holds every name, however many a call uses)."""
    return {name: st["launches"] for name, st in idx.kernel_stats().items()}


def _in_groups_only(model, rows, counts, qg, group_rows):
    """Nothing from outside a query's own group appears anywhere."""
    for b in range(len(qg)):
        allowed = set(int(x) for x in model.ids[group_rows[int(qg[b])]])
        got = set(int(x) for x in rows[b, :int(counts[b])])
        if not got <= allowed:
            return False
    return True


SCREENS = ("screen_i8_fused", "screen_gemv_i8", "screen_gemv_bf16", "screen_bf16_fused", "gemm_dot_bf16x1_fused")


@pytest.mark.parametrize("dim,B,screen", [(128, 3, "screen_gemv_i8"), (128, 8, "screen_i8_fused"), (128, 40, "screen_i8_fused"),
                                          (192, 40, "screen_bf16_fused"), (512, 100, "screen_i8_fused"), (512, 300, "screen_i8_fused")])
def test_grouped_search_equals_the_masked_call_and_the_oracle_per_group(dim, B, screen):
    idx, model, q_all, texts_all, group_rows, scopes, subs = _shard(dim)
    syn = _syn()
    q, texts, qg = q_all[:B], list(texts_all[:B]), _assign(B)
    # an unscoped search before ... and after: the grouped passes leave it alone
    before = idx.search(q, _terms(texts), syn.NOW_TICKS, 10, candidate_limit=N)
    idx.set_option("mask_screen", 1)
    # ONE masked call over group A with the queries the grouped pass screens: what one stream over the shard launches
    screened = np.nonzero(qg <= 2)[0]
    idx.set_profiling(True)
    _masked(idx, q[screened], [texts[b] for b in screened], 10, N, scopes[0])
    one_call = _kernel_stats(idx)
    idx.reset_search_stats()
    idx.set_profiling(True)
    rows, scores, counts = _grouped(idx, q, texts, 10, N, scopes, qg)
    stats = _kernel_stats(idx)
    idx.set_profiling(False)
    st = idx.search_stats()
    assert st["pass_mode"] == 6 and st["exact_pass_queries"] == 0, st
    assert "row_consts_grouped" in stats and "mask_survivors_grouped" in stats, sorted(stats)
    assert screen in stats and screen in one_call, (sorted(stats), sorted(one_call))
    assert stats[screen] == one_call[screen], (stats[screen], one_call[screen])      # one stream for all groups, not one per group
    assert not any(s in stats for s in SCREENS if s != screen), sorted(stats)
    assert (counts[qg == 4] == 0).all() and (rows[qg == 4] == -1).all()               # the empty group
    key = (dim, "base")
    for topk in (10, 40):
        got = _check(key, idx, model, subs, q, texts, topk, N, scopes, qg, _checked(B), "parity")
        if topk == 10:
            assert _same3(got, (rows, scores, counts))
    assert _in_groups_only(model, rows, counts, qg, group_rows)
    after = idx.search(q, _terms(texts), syn.NOW_TICKS, 10, candidate_limit=N)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    idx.set_option("mask_screen", 0)


def test_a_row_of_another_group_never_leaks_into_a_query():
    """The failure this design can have: the screen buffers a row of group A for a query of group B, and only the filter of
    the query's OWN group removes it."""
    idx, model, q_all, texts_all, group_rows, scopes, subs = _shard(128)
    B = 8
    q, texts, qg = q_all[:B].copy(), list(texts_all[:B]), _assign(B)
    assert A_ONLY_ROW in set(group_rows[0].tolist()) and not any(A_ONLY_ROW in set(r.tolist()) for r in group_rows[1:])
    rng = np.random.default_rng(5)
    x = model.emb[A_ONLY_ROW] + rng.standard_normal(128).astype(np.float32) * np.float32(0.01)
    q[1] = x                  # in group B: must never return the row
    q[0] = x                  # its copy in group A: ranks the row first
    texts[0] = texts[1]
    idx.set_option("mask_screen", 1)
    idx.reset_search_stats()
    rows, scores, counts = _check((128, "leak"), idx, model, subs, q, texts, 10, N, scopes, qg, list(range(B)), "leak")
    assert LAST["pass_mode"] == 6
    assert rows[0, 0] == model.ids[A_ONLY_ROW]
    assert model.ids[A_ONLY_ROW] not in rows[1]
    assert _in_groups_only(model, rows, counts, qg, group_rows)
    idx.set_option("mask_screen", 0)


def test_every_group_is_clipped_at_its_own_candidate_limit():
    idx, model, q_all, texts_all, group_rows, scopes, subs = _shard(128)
    B = 8
    q, texts, qg = q_all[:B].copy(), list(texts_all[:B]), _assign(B)
    rng = np.random.default_rng(6)
    y = model.emb[SHARED_ROW] + rng.standard_normal(128).astype(np.float32) * np.float32(0.01)
    q[5] = y                  # group A
    q[6] = y                  # group B
    texts[6] = texts[5]
    idx.set_option("mask_screen", 1)
    # 15,000: A and B are clipped mid-scope (A at row 115,000), C is not -- and C's runs reach the end of the shard, so the pass
    # still runs over (nearly) every row and is eligible: three clips that differ inside one grouped pass
    assert group_rows[1][15_000 - 1] < 196_608 <= group_rows[2][-1]
    idx.reset_search_stats()
    _check((128, "clip"), idx, model, subs, q, texts, 10, 15_000, scopes, qg, list(range(B)), "limit 15,000")
    assert LAST["pass_mode"] == 6
    # 9,000: C is clipped too, and now every clip lies below 196,608 rows: the grouped pass is not eligible and each group runs
    # as a masked call of its own, same contract
    assert max(int(group_rows[g][9_000 - 1]) for g in (0, 1, 2)) + 1 < 196_608
    idx.reset_search_stats()
    _check((128, "clip"), idx, model, subs, q, texts, 10, 9_000, scopes, qg, list(range(B)), "limit 9,000")
    assert LAST["pass_mode"] in (4, 5)
    # 99,000: only A is clipped, one row in front of row 199,000; B and C reach further and the grouped pass runs
    a_rows = group_rows[0]
    assert a_rows[99_000 - 1] == 199_000 - 1 and SHARED_ROW >= 199_000 and SHARED_ROW in set(group_rows[1].tolist())
    idx.reset_search_stats()
    rows, scores, counts = _check((128, "clip"), idx, model, subs, q, texts, 10, 99_000, scopes, qg, list(range(B)), "limit 99,000")
    assert LAST["pass_mode"] == 6
    pos = (rows - 11) // 3
    for b in np.nonzero(qg == 0)[0]:
        assert (pos[b, :counts[b]] < 199_000).all(), b                          # no row of A beyond A's clip, though the pass ran over them
    assert model.ids[SHARED_ROW] not in rows[5]                                  # A's query may not return the row behind A's clip
    assert rows[6, 0] == model.ids[SHARED_ROW]                                   # B's query holds it in front of B's own clip
    idx.set_option("mask_screen", 0)


def _adversarial_shard():
    """200,000 x 128 with 20,000 rows identical to query 0 inside A that B does not hold, a row with an infinite component
    inside group A and one outside every group."""
    if "adv" in _SHARDS:
        return _SHARDS["adv"]
    dim = 128
    syn = _syn()
    q = syn.query_vectors(0, 40, dim, N).numpy()
    same = np.arange(120_000, 140_000)

    def edit(emb, created):
        emb[same] = q[0]
        emb[NO_GROUP_ROW, 3] = np.inf
        emb[150_000, 3] = np.inf
    idx, model, _, texts = _make(dim, edit=edit)
    rows = _group_rows(77, b_without=same)
    scopes = [model.ids[r] for r in rows]
    _SHARDS["adv"] = (idx, model, q, texts, rows, scopes, [model.sub(s) for s in scopes])
    return _SHARDS["adv"]


@pytest.mark.parametrize("B", [8, 40])
def test_adversarial_queries_and_rows(B):
    idx, model, q_all, texts_all, group_rows, scopes, subs = _adversarial_shard()
    q, texts, qg = q_all[:B].copy(), list(texts_all[:B]), _assign(B)
    qg[0] = 1                 # query 0 searches B, which holds none of the 20,000 rows identical to it
    q[5] = np.nan             # group A
    q[6] = 0.0                # group B
    q[7, 7] = np.inf          # group C
    assert 150_000 in set(group_rows[0].tolist()) and not any(NO_GROUP_ROW in set(r.tolist()) for r in group_rows)
    idx.set_option("mask_screen", 1)
    idx.reset_search_stats()
    capacity = idx.search_stats()["survivor_capacity"]
    rows, scores, counts = _check(("adv", B), idx, model, subs, q, texts, 10, N, scopes, qg, list(range(8)), "adversarial")
    st = dict(LAST)
    # query 0's buffer overflows from rows of another group, grows for this call, and the answer is exact (checked above)
    assert st["overflowed_queries"] >= 1 and st["buffer_growths"] >= 1 and st["requeried"] >= 1 and st["exact_pass_queries"] == 0, st
    # ... and the grown size is the call's own: the index keeps the capacity it had (_check's masked calls see no overflow:
    # B's rows hold none of the identical ones)
    assert st["survivor_capacity"] == capacity and idx.search_stats()["survivor_capacity"] == capacity, (st, capacity)
    assert _in_groups_only(model, rows, counts, qg, group_rows)
    idx.set_option("mask_screen", 0)


def test_one_group_is_the_masked_call_and_mask_screen_2_never_screens_grouped():
    idx, model, q_all, texts_all, group_rows, scopes, subs = _shard(128)
    B = 8
    q, texts, qg = q_all[:B], list(texts_all[:B]), _assign(B)
    idx.set_option("mask_screen", 1)
    # G = 1
    idx.reset_search_stats()
    one = _grouped(idx, q, texts, 10, N, [scopes[1]], np.zeros(B, np.int32))
    assert idx.search_stats()["pass_mode"] == 5
    assert _same3(one, _masked(idx, q, texts, 10, N, scopes[1]))
    # one USED group among several: the others are empty or named by nobody
    idx.reset_search_stats()
    lone = _grouped(idx, q, texts, 10, N, [scopes[4], scopes[1], scopes[5]], np.ones(B, np.int32))
    assert idx.search_stats()["pass_mode"] == 5 and _same3(lone, one)
    # a flat array with offsets, on the device, equals the sequence of arrays
    import torch
    flat = np.concatenate(scopes)
    off = np.cumsum([0] + [len(s) for s in scopes]).astype(np.uint64)
    seq = _grouped(idx, q, texts, 10, N, scopes, qg)
    dev = idx.search_masked_groups(np.ascontiguousarray(q, dtype=np.float32), _terms(texts), _syn().NOW_TICKS, 10, torch.from_numpy(flat).to("cuda:0"), qg,
                                   candidate_limit=N, group_off=off)
    assert _same3(seq, dev)
    # mask_screen = 2
    idx.set_option("mask_screen", 2)
    idx.reset_search_stats()
    idx.set_profiling(True)
    never = _grouped(idx, q, texts, 10, N, scopes, qg)
    stats = _kernel_stats(idx)
    idx.set_profiling(False)
    assert idx.search_stats()["pass_mode"] == 4 and "row_consts_grouped" not in stats and "mask_survivors_grouped" not in stats
    assert _same3(never, seq)
    idx.set_option("mask_screen", 0)


def test_maintenance_keeps_grouped_searches_exact():
    dim = 128
    idx, model, q_all, texts_all = _make(dim)
    B = 8
    q, texts, qg = q_all[:B].copy(), list(texts_all[:B]), _assign(B)
    rng = np.random.default_rng(78)
    scopes = [model.ids[r].copy() for r in _group_rows(31)]
    idx.set_option("mask_screen", 1)
    step = [0]

    def check(what):
        step[0] += 1
        subs = [model.sub(s) for s in scopes]
        idx.reset_search_stats()
        out = _check(("maint", step[0]), idx, model, subs, q, texts, 10, N, scopes, qg, [0, 1, 2, 6], what)
        assert LAST["pass_mode"] == 6, what
        return out

    rows0, _, _ = check("fresh")
    # delete: the winners
    victims = sorted(set(int(x) for x in rows0[:, :3].ravel()) - {-1})
    assert idx.delete_rows(victims) == len(victims)
    model.deleted |= set(int(r) for r in np.nonzero(np.isin(model.ids, victims))[0])
    check("after delete_rows")
    # update: new vectors for rows of B, one of them query 1 itself
    targets = scopes[1][1000:1040]
    new = rng.standard_normal((len(targets), dim)).astype(np.float32)
    new[0] = q[1]
    assert idx.update_rows(targets, new) == len(targets)
    model.emb[np.searchsorted(model.ids, targets)] = new
    r1, _, _ = check("after update_rows")
    assert r1[1, 0] == targets[0]
    # insert: rows of older and newer timestamps, half of them added to B (the id table is rebuilt)
    m = 64
    ins_emb = rng.standard_normal((m, dim)).astype(np.float32)
    ins_emb[3] = q[6]
    ins_created = np.sort(np.unique(rng.choice(model.created, m, replace=False)) + 1)[::-1].copy()
    m = len(ins_created)
    ins_emb = ins_emb[:m]
    ins_ids = np.arange(m, dtype=np.int64) + 10_000_000
    ins_bytes = model.rowbytes[rng.choice(N, m, replace=False)].copy()
    off = np.arange(m + 1, dtype=np.int64) * ins_bytes.shape[1]
    assert idx.insert_rows(ins_emb, ins_created, ins_bytes.reshape(-1), off, row_ids=ins_ids) == m
    all_created = np.concatenate([model.created, ins_created])
    order = np.argsort(-all_created, kind="stable")
    deleted_ids = model.ids[np.fromiter(model.deleted, np.int64)]
    model = Model(np.concatenate([model.emb, ins_emb])[order], all_created[order], np.concatenate([model.rowbytes, ins_bytes])[order],
                  np.concatenate([model.ids, ins_ids])[order])
    model.deleted = set(int(r) for r in np.nonzero(np.isin(model.ids, deleted_ids))[0])
    scopes[1] = np.concatenate([scopes[1], ins_ids[: m // 2]])
    r2, _, _ = check("after insert_rows")
    assert r2[6, 0] == ins_ids[3]                                                # query 6 searches B, which got the row
    # compact: positions move again
    idx.compact()
    live = np.array(sorted(set(range(len(model.ids))) - model.deleted))
    model = Model(model.emb[live], model.created[live], model.rowbytes[live], model.ids[live])
    check("after compact")
    idx.close()


def test_views_and_argument_errors():
    P, syn = pkg(), _syn()
    idx, model, q_all, texts_all, group_rows, scopes, subs = _shard(128)
    B = 8
    q, texts, qg = q_all[:B], list(texts_all[:B]), _assign(B)
    idx.set_option("mask_screen", 1)
    ro = _grouped(idx, q, texts, 10, N, scopes, qg)
    v = idx.view()
    v.set_option("mask_screen", 1)
    assert _same3(_grouped(v, q, texts, 10, N, scopes, qg), ro)
    v.close()
    # unknown ids are skipped, repeats count once, equal and overlapping groups are fine
    noisy = [np.concatenate([scopes[0], [5, -7, 2 ** 40], scopes[0][:100]]), scopes[1], scopes[2], scopes[3], scopes[4], scopes[0]]
    assert _same3(_grouped(idx, q, texts, 10, N, noisy, qg), ro)
    # argument errors: ORR_EINVAL, the function named, the outputs untouched, the index searchable afterwards
    h, E = P.native.hip, P.native.ORR_EINVAL
    pool, toff, qoff = P.pack_terms(_terms(texts))
    k = 4
    rows, scores, counts = np.full((B, k), 7, np.int64), np.full((B, k), 7.0), np.full(B, 7, np.int32)
    ids = np.ascontiguousarray(np.concatenate([scopes[1][:5], scopes[2][:3]]))
    off2 = np.array([0, 5, 8], np.uint64)
    g2 = (np.arange(B) % 2).astype(np.int32)
    qq = np.ascontiguousarray(q, dtype=np.float32)

    def call(handle=idx._h, b=B, n_groups=2, n_ids=8, p_ids=ids.ctypes.data, p_off=off2.ctypes.data, p_qg=g2.ctypes.data, p_rows=rows.ctypes.data,
             p_qoff=qoff.ctypes.data):
        return h.orr_search_batch_masked_groups(handle, b, 128, qq.ctypes.data, pool.ctypes.data, toff.ctypes.data, p_qoff, syn.NOW_TICKS, k, 300,
                                                n_groups, n_ids, p_ids, p_off, p_qg, p_rows, scores.ctypes.data, counts.ctypes.data)

    bad_off = [np.array([1, 5, 8], np.uint64), np.array([0, 6, 5], np.uint64), np.array([0, 5, 7], np.uint64)]
    bad_qg = [np.array([0, 1, 2, 0, 0, 0, 0, 0], np.int32), np.array([0, -1, 0, 0, 0, 0, 0, 0], np.int32)]
    off65 = np.zeros(66, np.uint64)
    off65[1:] = 8
    errors = [dict(n_ids=-1), dict(p_ids=None), dict(handle=None), dict(p_rows=None), dict(b=0), dict(p_qoff=None),      # the masked call's own
              dict(n_groups=0), dict(n_groups=-3), dict(n_groups=65, p_off=off65.ctypes.data),
              dict(p_off=None), dict(p_qg=None)]
    errors += [dict(p_off=o.ctypes.data) for o in bad_off] + [dict(p_qg=g.ctypes.data) for g in bad_qg]
    for kw in errors:
        assert call(**kw) == E, kw
        assert b"orr_search_batch_masked_groups" in h.orr_last_error(), (kw, h.orr_last_error())
        assert (rows == 7).all() and (scores == 7.0).all() and (counts == 7).all(), kw
    assert call() == 0 and (counts[g2 == 0] == k).all() and (counts[g2 == 1] == 3).all()
    assert _same3(_grouped(idx, q, texts, 10, N, scopes, qg), ro)
    idx.set_option("mask_screen", 0)


def test_six_threads_mix_grouped_masked_scoped_and_unscoped_searches():
    P, syn = pkg(), _syn()
    idx, model, q_all, texts_all, group_rows, scopes, subs = _shard(128)
    terms_all = _terms(texts_all)
    small = scopes[3]
    idx.set_option("mask_screen", 1)
    idx.set_option("max_lanes", 6)

    def job(i):
        b0, B = 5 * i, (8, 3, 8, 40, 2, 8)[i]
        q, terms = np.ascontiguousarray(q_all[b0:b0 + B]), terms_all[b0:b0 + B]
        if i % 3 == 0:
            return idx.search_masked_groups(q, terms, syn.NOW_TICKS, 10, scopes, _assign(B), candidate_limit=N)
        if i == 1:
            return idx.search_masked(q, terms, syn.NOW_TICKS, 10, scopes[2], candidate_limit=N)
        if i == 4:
            return idx.search_scoped(q, terms, syn.NOW_TICKS, 10, small, candidate_limit=N)
        return idx.search(q, terms, syn.NOW_TICKS, 10, candidate_limit=N)

    single = [job(i) for i in range(6)]
    got, errors = [None] * 6, []

    def run(i):
        try:
            for _ in range(3):
                got[i] = job(i)
                assert _same3(got[i], single[i]), i
        except Exception as e:                                                   # pragma: no cover
            errors.append((i, e))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    idx.set_option("mask_screen", 0)
