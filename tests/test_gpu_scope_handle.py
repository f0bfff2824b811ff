"""Scope handles (orr_scope): a scope resolved once, searched without a resolve, composed, and carried through maintenance.

The contract of a search inside a handle is the masked call's, stated over ROWS: what orr_search_batch returns on a shard
sealed from scratch from only the scope's live rows in their present candidate order.  So every in-scope search is compared
array for array with search_masked on the ids the test's model says the scope holds, and a stated subset with the oracle on
that sub-corpus (the method of test_gpu_masked_search.py).

Shard A, 200,000 x 128, built once: the smallest shard on which the masked screen runs (int8 shadow).  Shard B, 70,001 x 64,
built fresh per test with capacity reserved: three bitmap chunks with the last one partial and a row count that is no multiple
of 32 -- the shard that is deleted from, compacted and inserted into."""
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
# positions of the planted runs of 5 rows with equal ticks (each the head of a synthetic document of 8 rows)
RUNS_A = (40_000, 40_008, 100_000, 160_000)


def _syn():
    pkg()                                               # (registers the package under its importable name)
    return importlib.import_module("omni_recall_rag_amd.synthetic")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


class Model:
    """The shard as the test knows it: rows in candidate order with their ids; deletes, compaction and insertion restated."""

    def __init__(self, emb, created, rowbytes, ids):
        self.emb, self.created, self.rowbytes = emb.copy(), np.asarray(created, np.int64).copy(), rowbytes.copy()
        self.ids = np.asarray(ids, np.int64).copy()
        self.dead = np.zeros(len(self.ids), bool)

    def rows_of_ids(self, ids):
        """live rows (positions) that carry one of the ids"""
        return np.nonzero(np.isin(self.ids, np.asarray(ids, np.int64)) & ~self.dead)[0]

    def ids_in_window(self, t0, t1):
        if t0 >= t1:
            return np.zeros(0, np.int64)
        upper = np.ones(len(self.ids), bool) if t1 == I64_MAX else self.created < t1
        return self.ids[(self.created >= t0) & upper & ~self.dead]

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

    def insert(self, emb, created, rowbytes, ids):
        """a STABLE descending order by ticks: at equal ticks the rows that were there stay in front"""
        c = np.concatenate([self.created, np.asarray(created, np.int64)])
        order = np.argsort(np.negative(c), kind="stable")
        self.emb = np.concatenate([self.emb, emb])[order]
        self.rowbytes = np.concatenate([self.rowbytes, rowbytes])[order]
        self.ids = np.concatenate([self.ids, np.asarray(ids, np.int64)])[order]
        self.dead = np.concatenate([self.dead, np.zeros(len(ids), bool)])[order]
        self.created = c[order]


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


def _checked(B):
    return list(range(B)) if B <= 8 else sorted(set(range(8)) | {B // 2, B - 9, B - 8, B - 1})       # all up to 8, 12 of 40


# ---- shard A -----------------------------------------------------------------------------------------------------------------

_A = {}


def _shard_a():
    if _A:
        return _A
    emb, created, rowbytes = _rows(NA, DIM_A)
    for p in RUNS_A:                                    # a run of 5 with equal ticks, the document's other 3 rows one tick older
        assert p % 8 == 0 and created[p] == created[p + 7] and created[p + 8] < created[p] - 1
        created[p + 5:p + 8] = created[p] - 1
    assert (np.diff(created) <= 0).all()
    ids = np.arange(NA, dtype=np.int64) * 3 + 11
    idx = _build(emb, created, rowbytes, ids, NA)
    model = Model(emb, created, rowbytes, ids)
    q, texts = _queries(DIM_A, NA)
    rng = np.random.default_rng(628)
    starts = rng.choice(NA // 25, NA // 500, replace=False) * 25
    fam = {
        "random 10 %": np.sort(rng.choice(NA, NA // 10, replace=False)),
        "older half": np.arange(NA // 2, NA),
        "runs of 25": np.sort((starts[:, None] + np.arange(25)[None, :]).reshape(-1)),
    }
    plants = {}
    for name, rows in fam.items():
        inside = int(rows[len(rows) // 3])
        held = set(rows.tolist())
        outside = next(r for r in range(NA // 2 - 1, -1, -1) if r not in held)
        qq = q.copy()
        noise = rng.standard_normal((2, DIM_A)).astype(np.float32) * np.float32(0.01)
        qq[0] = emb[inside] + noise[0]                  # a near-duplicate inside the scope: ranks first
        qq[1] = emb[outside] + noise[1]                 # ... and outside: must never appear
        plants[name] = (qq, inside, outside)
    _A.update(idx=idx, model=model, texts=texts, fam=fam, plants=plants, q=q, scopes={})
    return _A


def _scope_a(name):
    a = _shard_a()
    if name not in a["scopes"]:
        a["scopes"][name] = a["idx"].scope(a["model"].ids[a["fam"][name]])
    return a["scopes"][name]


@pytest.mark.parametrize("B", [1, 8, 40])
@pytest.mark.parametrize("name", ["random 10 %", "older half", "runs of 25"])
def test_search_in_scope_equals_search_masked_and_the_oracle(name, B):
    a = _shard_a()
    idx, model, texts = a["idx"], a["model"], a["texts"][:B]
    q_all, inside, outside = a["plants"][name]
    q = q_all[:B]
    ids = model.ids[a["fam"][name]]
    sc = _scope_a(name)
    s = len(ids)
    assert sc.rows == s and np.array_equal(sc.row_ids(), ids)
    other_ids = model.ids[a["fam"]["runs of 25" if name != "runs of 25" else "random 10 %"]]
    for screen, mode_at_rows in ((1, 5), (2, 4)):
        idx.set_option("mask_screen", screen)
        for topk in (1, 10, 64, 100):
            for limit in (300, 15_000, s):
                # the in-scope call FIRST, behind a masked call on OTHER ids: whatever the lane's workspaces hold is not this scope
                _masked(idx, q, texts, 10, limit, other_ids)
                idx.reset_search_stats()
                got = _in_scope(idx, q, texts, topk, limit, sc)
                mode = idx.search_stats()["pass_mode"]
                idx.reset_search_stats()
                want = _masked(idx, q, texts, topk, limit, ids)
                mode_masked = idx.search_stats()["pass_mode"]
                assert _equal(got, want), (name, B, screen, topk, limit)
                assert mode == mode_masked and mode in (4, 5), (name, B, screen, topk, limit, mode, mode_masked)
                if screen == 2 or topk > 64 or limit == 300:
                    assert mode == 4, (name, B, screen, topk, limit)
                elif topk == 10 and limit == s:
                    assert mode == mode_at_rows, (name, B, screen, mode)
                if screen == 1 and topk == 10 and limit == s:
                    _against_oracle(model, ids, got, q, texts, topk, limit, _checked(B), name)
                    assert got[0][0, 0] == model.ids[inside]
                    if B > 1:
                        assert model.ids[outside] not in got[0][1]
                if screen == 2 and topk == 64 and limit == 300:
                    _against_oracle(model, ids, got, q, texts, topk, limit, _checked(B)[:2], name)
    idx.set_option("mask_screen", 0)


def test_scope_ticks_windows():
    a = _shard_a()
    idx, model = a["idx"], a["model"]
    c = model.created
    r0, r1, r2, r3 = RUNS_A
    windows = [
        (int(c[r2]), int(c[r0])),                       # both borders ON a run: the lower run is in, the upper run is out
        (int(c[r2]), int(c[r0]) + 1),                   # ... the upper run in
        (int(c[r2]) + 1, int(c[r0])),                   # ... the lower run out
        (int(c[r1]), int(c[r1]) + 1),                   # a window that is exactly one run of ties
        (int(c[r1]), int(c[r0]) + 1),                   # two adjacent runs
        (int(c[r3 + 8]) + 1, int(c[r2 - 1]) - 1),       # borders between runs
        (int(c[r3]) + 1, int(c[r3]) + 2),               # between two runs: empty
        (I64_MIN, int(c[r2])), (int(c[r2]), I64_MAX), (I64_MIN, I64_MAX),
        (I64_MIN, I64_MIN + 1), (I64_MAX - 1, I64_MAX),
        (int(c[r0]), int(c[r0])),                       # empty
        (int(c[r0]), int(c[r2])),                       # inverted
    ]
    total = 0
    for t0, t1 in windows:
        sc = idx.scope_ticks(t0, t1)
        want = model.ids_in_window(t0, t1)
        assert sc.rows == len(want) and np.array_equal(sc.row_ids(), want), (t0, t1, sc.rows, len(want))
        total += len(want)
        sc.close()
    assert total > NA                                   # (the open ends held rows)
    # adjacent windows tile
    lo, mid, hi = idx.scope_ticks(I64_MIN, int(c[r2])), idx.scope_ticks(int(c[r2]), int(c[r0])), idx.scope_ticks(int(c[r0]), I64_MAX)
    assert lo.rows + mid.rows + hi.rows == NA
    for s in (lo, mid, hi):
        s.close()
    # a 60,000-row window, searched, against the oracle on that sub-corpus
    t0, t1 = int(c[129_999]), int(c[69_999])
    sc = idx.scope_ticks(t0, t1)
    want = model.ids_in_window(t0, t1)
    assert 59_990 <= sc.rows <= 60_010 and np.array_equal(sc.row_ids(), want)
    B = 8
    q, texts = a["q"][:B], a["texts"][:B]
    idx.set_option("mask_screen", 1)
    got = _in_scope(idx, q, texts, 10, NA, sc)
    idx.set_option("mask_screen", 0)
    _against_oracle(model, want, got, q, texts, 10, NA, range(B), "window")
    assert _equal(got, _in_scope(idx, q, texts, 10, NA, sc))
    sc.close()


def test_combine():
    P = pkg()
    a = _shard_a()
    idx, model = a["idx"], a["model"]
    c = model.created
    tenant = model.ids[a["fam"]["random 10 %"]]
    t0, t1 = int(c[149_999]), int(c[49_999])
    window = model.ids_in_window(t0, t1)
    sc = idx.scope(tenant)
    w = idx.scope_ticks(t0, t1)
    assert sc.and_(w) is sc
    both = np.intersect1d(tenant, window)
    assert sc.rows == len(both) and np.array_equal(sc.row_ids(), model.ordered(set(both.tolist())))
    assert w.rows == len(window)                        # src is unchanged
    B = 8
    q, texts = a["q"][:B], a["texts"][:B]
    got = _in_scope(idx, q, texts, 10, NA, sc)
    _against_oracle(model, both, got, q, texts, 10, NA, range(B), "tenant AND window")
    x, y = model.ids[a["fam"]["runs of 25"]], model.ids[a["fam"]["older half"]]
    sx, sy = idx.scope(x), idx.scope(y)
    sx.or_(sy)
    assert np.array_equal(sx.row_ids(), model.ordered(set(np.union1d(x, y).tolist())))
    sx.andnot(sy)
    assert np.array_equal(sx.row_ids(), model.ordered(set(np.setdiff1d(x, y).tolist())))
    sx.andnot(sx)                                       # with itself: empty
    assert sx.rows == 0 and len(sx.row_ids()) == 0
    got = _in_scope(idx, q, texts, 10, NA, sx)
    assert (got[2] == 0).all() and (got[0] == -1).all()
    # a scope of another shard: combine and search are ORR_EINVAL
    emb, created, rowbytes = _rows(1000, DIM_A)
    other = _build(emb, created, rowbytes, np.arange(1000, dtype=np.int64), 1000)
    so = other.scope(np.arange(10))
    for call in (lambda: sy.and_(so), lambda: so.or_(sy), lambda: _in_scope(idx, q, texts, 10, NA, so),
                 lambda: idx.search_in_scopes(q, _terms(texts), _syn().NOW_TICKS, 10, [sy, so], np.zeros(B, np.int32))):
        with pytest.raises(P.native.OrrError) as e:
            call()
        assert e.value.code == P.native.ORR_EINVAL
    # row_ids with too little room: ORR_EINVAL after the count is set, nothing written beyond cap
    import ctypes as C
    n, out = C.c_int64(0), np.full(4, 7, np.int64)
    r = P.native.hip.orr_scope_row_ids(so._h, 4, out.ctypes.data, C.cast(C.byref(n), C.c_void_p))
    assert r == P.native.ORR_EINVAL and n.value == 10 and (out == 7).all()
    for s in (sc, w, sx, sy, so):
        s.close()
    other.close()


@pytest.mark.parametrize("B", [8, 40])
def test_search_in_scopes(B):
    a = _shard_a()
    idx, model = a["idx"], a["model"]
    rng = np.random.default_rng(77)
    sizes = (100_000, 20_000, 10_000, 200, 0)
    rows_of = [np.sort(rng.choice(NA, s, replace=False)) for s in sizes]
    # the leak case: a near-duplicate of a row only scope 0 holds, asked inside scope 1
    only0 = int(np.setdiff1d(rows_of[0], rows_of[1])[1000])
    q = a["q"][:B].copy()
    q[1] = model.emb[only0] + rng.standard_normal(DIM_A).astype(np.float32) * np.float32(0.01)
    texts = a["texts"][:B]
    scopes = [idx.scope(model.ids[r]) for r in rows_of] + [idx.scope(model.ids[:5000])]      # the last: named by no query
    assert [s.rows for s in scopes] == list(sizes) + [5000]
    qs = np.arange(B, dtype=np.int32) % 5
    idx.set_option("mask_screen", 1)
    idx.reset_search_stats()
    rows, scores, counts = idx.search_in_scopes(q, _terms(texts), _syn().NOW_TICKS, 10, scopes, qs, candidate_limit=NA)
    assert idx.search_stats()["pass_mode"] == 6
    for g in range(5):
        members = np.nonzero(qs == g)[0]
        own = _in_scope(idx, q[members], [texts[b] for b in members], 10, NA, scopes[g])
        assert _equal((rows[members], scores[members], counts[members]), own), g
        want = _masked(idx, q[members], [texts[b] for b in members], 10, NA, model.ids[rows_of[g]])
        assert _equal(own, want), g
    assert model.ids[only0] not in rows[1]
    assert (counts[qs == 4] == 0).all() and (counts[qs == 3] == 10).all()
    # scopes may repeat; one used scope is the in-scope call
    again = idx.search_in_scopes(q, _terms(texts), _syn().NOW_TICKS, 10, [scopes[1], scopes[1], scopes[4]], np.arange(B, dtype=np.int32) % 2, candidate_limit=NA)
    assert _equal(again, _in_scope(idx, q, texts, 10, NA, scopes[1]))
    # a limit below the scopes' sizes goes through the clip
    lim = idx.search_in_scopes(q, _terms(texts), _syn().NOW_TICKS, 10, scopes, qs, candidate_limit=5000)
    for g in range(5):
        members = np.nonzero(qs == g)[0]
        assert _equal(tuple(x[members] for x in lim), _in_scope(idx, q[members], [texts[b] for b in members], 10, 5000, scopes[g])), g
    idx.set_option("mask_screen", 0)
    for s in scopes:
        s.close()


def test_no_resolve_on_the_handle_path():
    a = _shard_a()
    idx, model = a["idx"], a["model"]
    ids = model.ids[a["fam"]["random 10 %"]]
    sc = _scope_a("random 10 %")
    q, texts = a["q"][:8], a["texts"][:8]
    idx.set_option("mask_screen", 1)

    def launches(fn):
        idx.set_profiling(True)
        fn()
        st = idx.kernel_stats()
        idx.set_profiling(False)
        return {k: v["launches"] for k, v in st.items()}

    st = launches(lambda: _masked(idx, q, texts, 10, NA, ids))
    assert all(st.get(k, 0) >= 1 for k in ("scope_lookup", "scope_counts", "mask_clip")), sorted(st)
    st = launches(lambda: _in_scope(idx, q, texts, 10, NA, sc))
    assert not any(k in st for k in ("scope_lookup", "scope_counts", "mask_clip", "scope_handle_lookup")), sorted(st)
    assert "mask_survivors" in st                       # ... and it did run the masked screen
    st = launches(lambda: _in_scope(idx, q, texts, 10, len(ids), sc))       # candidate_limit == rows: still no clip
    assert "mask_clip" not in st
    st = launches(lambda: _in_scope(idx, q, texts, 10, len(ids) - 1, sc))   # below: one clip, still no lookup and no count
    assert st.get("mask_clip", 0) == 1 and "scope_lookup" not in st and "scope_counts" not in st, sorted(st)
    idx.set_option("mask_screen", 0)


# ---- shard B -----------------------------------------------------------------------------------------------------------------

def _shard_b(capacity=NB + 1000):
    emb, created, rowbytes = _rows(NB, DIM_B)
    ids = np.arange(NB, dtype=np.int64) * 3 + 11
    idx = _build(emb, created, rowbytes, ids, capacity)
    q, texts = _queries(DIM_B, NB)
    return idx, Model(emb, created, rowbytes, ids), q[:8], texts[:8]


def _scopes_b(idx, model, rng):
    """an id scope, a ticks scope and a combined one, each with the set of ids the model says it holds"""
    pick = np.sort(rng.choice(NB, 20_000, replace=False))
    t0, t1 = int(model.created[50_000]), int(model.created[9_999])
    sets = {"ids": set(model.ids[pick].tolist()), "ticks": set(model.ids_in_window(t0, t1).tolist())}
    sets["both"] = sets["ids"] & sets["ticks"]
    scopes = {"ids": idx.scope(model.ids[pick]), "ticks": idx.scope_ticks(t0, t1), "both": idx.scope(model.ids[pick])}
    scopes["both"].and_(scopes["ticks"])
    return scopes, sets, (t0, t1)


def _check_scopes(idx, model, scopes, sets, q, texts, oracle=True):
    for name, sc in scopes.items():
        want = model.ordered(sets[name])
        assert sc.rows == len(want), (name, sc.rows, len(want))
        assert np.array_equal(sc.row_ids(), want), name
        got = _in_scope(idx, q, texts, 10, NB + 1000, sc)
        if oracle:
            _against_oracle(model, want, got, q, texts, 10, NB + 1000, range(len(texts)) if name == "both" else (0, 3), name)
        else:
            assert _equal(got, _masked(idx, q, texts, 10, NB + 1000, want)), name


def test_delete_rows_leave_every_scope():
    idx, model, q, texts = _shard_b()
    rng = np.random.default_rng(31)
    scopes, sets, _ = _scopes_b(idx, model, rng)
    in_both = np.fromiter(sets["both"], np.int64)
    gone = np.concatenate([in_both[:120], rng.choice(model.ids, 380, replace=False)])
    gone = np.unique(gone)
    before = {k: s.rows for k, s in scopes.items()}
    assert idx.delete_rows(gone) == len(gone)
    model.delete(gone)
    for k, s in scopes.items():
        assert s.rows == before[k] - len(sets[k] & set(gone.tolist())), k
    _check_scopes(idx, model, scopes, sets, q, texts, oracle=False)
    assert scopes["ids"].add_ids(gone[:50]) == 0        # a deleted id adds nothing
    assert scopes["ids"].rows == len(model.ordered(sets["ids"]))
    fresh = idx.scope_ticks(I64_MIN, I64_MAX)           # a window that holds deleted rows leaves them out
    assert fresh.rows == NB - len(gone)
    for s in list(scopes.values()) + [fresh]:
        s.close()
    idx.close()


def test_a_window_of_deleted_rows_only_is_empty():
    idx, model, q, texts = _shard_b()
    doc = np.arange(800, 808)                           # one document: eight rows of one timestamp
    assert idx.delete_rows(model.ids[doc]) == 8
    sc = idx.scope_ticks(int(model.created[800]), int(model.created[800]) + 1)
    assert sc.rows == 0 and len(sc.row_ids()) == 0
    assert (_in_scope(idx, q, texts, 10, NB, sc)[2] == 0).all()
    sc.close()
    idx.close()


def test_compact_carries_every_scope():
    idx, model, q, texts = _shard_b()
    rng = np.random.default_rng(32)
    scopes, sets, _ = _scopes_b(idx, model, rng)
    # the first row, the last row, a whole 128-row block, rows at both sides of the 32,768 border; 9,000 in all
    special = np.unique(np.concatenate([[0, NB - 1], np.arange(1280, 1408), np.arange(32_760, 32_776)]))
    others = np.setdiff1d(np.arange(NB), special)
    rows = np.concatenate([special, rng.choice(others, 9_000 - len(special), replace=False)])
    gone = model.ids[rows]
    assert len(gone) == 9_000
    assert idx.delete_rows(gone) == len(gone)
    model.delete(gone)
    assert idx.compact() == len(gone)                   # (not ORR_ESTATE: a scope is no view)
    model.compact()
    assert idx.rows == NB - len(gone) == len(model.ids)
    _check_scopes(idx, model, scopes, sets, q, texts)
    for s in scopes.values():
        s.close()
    idx.close()


def _new_rows_b(model, rng):
    """131 rows: 40 newer than everything, 51 through the middle (some at an old row's ticks), 40 older than everything"""
    emb, _, rowbytes = _rows(131, DIM_B, row0=5_000_000)
    c = model.created
    mid = c[rng.choice(NB, 51, replace=False)].copy()
    mid[::2] -= 3                                       # every other one between two old timestamps, the rest exact ties
    created = np.concatenate([c[0] + 1 + np.arange(40), mid, c[-1] - 1 - np.arange(40)]).astype(np.int64)
    ids = 10_000_000 + np.arange(131, dtype=np.int64)
    return emb, created, rowbytes, ids


def _insert_and_check(idx, model, q, texts, rng):
    scopes, sets, (t0, t1) = _scopes_b(idx, model, rng)
    emb, created, rowbytes, ids = _new_rows_b(model, rng)
    assert ((created >= t0) & (created < t1)).any()     # the ticks scope's window covers some of the new rows
    width = rowbytes.shape[1]
    n0 = idx.rows
    assert idx.insert_rows(emb, created, rowbytes.reshape(-1), np.arange(132, dtype=np.uint64) * width, row_ids=ids) == 131
    model.insert(emb, created, rowbytes, ids)
    assert idx.rows == n0 + 131 == len(model.ids)
    # every scope holds the rows it held, in the new candidate order, and no new row
    for name, sc in scopes.items():
        got = sc.row_ids()
        assert np.array_equal(got, model.ordered(sets[name])), name
        assert not np.isin(ids, got).any(), name
    _check_scopes(idx, model, scopes, sets, q[:2], texts[:2], oracle=False)
    # add_ids names them
    assert scopes["ids"].add_ids(ids) == 131 and scopes["ids"].add_ids(ids) == 0
    sets["ids"] |= set(ids.tolist())
    _check_scopes(idx, model, {"ids": scopes["ids"]}, sets, q, texts)
    qn = np.ascontiguousarray(emb[:1] + np.float32(0.001))          # a near-duplicate of a new row: found inside the scope
    assert _in_scope(idx, qn, texts[:1], 10, NB + 1000, scopes["ids"])[0][0, 0] == ids[0]
    assert ids[0] not in _in_scope(idx, qn, texts[:1], 10, NB + 1000, scopes["ticks"])[0]
    for s in scopes.values():
        s.close()


def _insert_behind_a_mid_word_row(idx, model, rng):
    """Seven rows that all land behind one old row in mid-word: the rows in front of them (`first` of the move, no multiple of
    32) stay where they are, and the scopes' bits there must stay with them."""
    j = 33_333
    while True:
        tick = int(model.created[j]) - 1
        first = int((model.created >= tick).sum())      # (old rows at the same ticks stay in front)
        if first % 32 not in (0, 31) and first < len(model.created) and model.created[first] < tick:
            break
        j += 8
    scopes, sets, _ = _scopes_b(idx, model, rng)
    emb, _, rowbytes = _rows(7, DIM_B, row0=6_000_000)
    created = np.full(7, tick, np.int64)
    ids = 20_000_000 + np.arange(7, dtype=np.int64)
    assert idx.insert_rows(emb, created, rowbytes.reshape(-1), np.arange(8, dtype=np.uint64) * rowbytes.shape[1], row_ids=ids) == 7
    model.insert(emb, created, rowbytes, ids)
    assert np.array_equal(model.ids[first:first + 7], ids)
    for name, sc in scopes.items():
        got = sc.row_ids()
        assert np.array_equal(got, model.ordered(sets[name])) and not np.isin(ids, got).any(), name
        sc.close()


def test_insert_rows_carries_every_scope(tmp_path):
    idx, model, q, texts = _shard_b()
    rng = np.random.default_rng(33)
    assert NB // 32 != (NB + 131) // 32                 # the row count crosses a word border
    _insert_and_check(idx, model, q, texts, rng)
    _insert_behind_a_mid_word_row(idx, model, rng)
    # a second insert without reserved capacity, on the shard loaded from a file
    path = str(tmp_path / "shard.orr")
    idx.save(path)
    idx.close()
    loaded = pkg().RecallIndex.load(path)
    assert loaded.rows == NB + 138
    emb, created, rowbytes, ids = _new_rows_b(model, rng)
    scopes, sets, _ = _scopes_b(loaded, model, rng)
    ids = ids + 1000
    width = rowbytes.shape[1]
    assert loaded.insert_rows(emb, created, rowbytes.reshape(-1), np.arange(132, dtype=np.uint64) * width, row_ids=ids) == 131
    model.insert(emb, created, rowbytes, ids)
    for name, sc in scopes.items():
        got = sc.row_ids()
        assert np.array_equal(got, model.ordered(sets[name])) and not np.isin(ids, got).any(), name
    assert scopes["both"].add_ids(ids) == 131
    sets["both"] |= set(ids.tolist())
    _check_scopes(loaded, model, {"both": scopes["both"]}, sets, q, texts)
    for s in scopes.values():
        s.close()
    loaded.close()


def test_update_rows_touch_no_scope():
    idx, model, q, texts = _shard_b()
    rng = np.random.default_rng(34)
    scopes, sets, _ = _scopes_b(idx, model, rng)
    before = {k: s.row_ids() for k, s in scopes.items()}
    target = int(model.ordered(sets["both"])[len(sets["both"]) // 2])
    row = int(np.nonzero(model.ids == target)[0][0])
    vec = np.ascontiguousarray(q[:1] * np.float32(0.5))
    was = _in_scope(idx, q, texts, 10, NB, scopes["both"])
    assert idx.update_rows([target], vec) == 1
    model.emb[row] = vec[0]
    for k, s in scopes.items():
        assert np.array_equal(s.row_ids(), before[k]), k
    got = _in_scope(idx, q, texts, 10, NB, scopes["both"])
    assert target in got[0][0] and target not in was[0][0]      # the search sees the new vector (cosine 1 with query 0)
    _against_oracle(model, model.ordered(sets["both"]), got, q, texts, 10, NB, range(len(texts)), "updated")
    for s in scopes.values():
        s.close()
    idx.close()


def test_lifetime_views_and_orphans():
    P = pkg()
    idx, model, q, texts = _shard_b()
    ids = model.ids[::7]
    view = idx.view()
    on_owner, on_view = idx.scope(ids), view.scope(ids)
    want = _masked(idx, q, texts, 10, NB, ids)
    for handle, sc in ((idx, on_view), (view, on_owner), (view, on_view), (idx, on_owner)):
        assert _equal(_in_scope(handle, q, texts, 10, NB, sc), want)
    both = idx.search_in_scopes(q, _terms(texts), _syn().NOW_TICKS, 10, [on_owner, on_view], np.arange(len(texts), dtype=np.int32) % 2, candidate_limit=NB)
    assert _equal(both, want)
    on_view.or_(on_owner)
    assert on_view.rows == len(ids)
    on_view.close()
    view.close()
    other = idx.scope(ids[:100])
    idx.close()                                         # the index goes first: the scopes are orphaned
    assert on_owner.rows == -1 and other.rows == -1
    for call in (lambda: on_owner.add_ids(ids[:3]), lambda: on_owner.row_ids(), lambda: on_owner.and_(other)):
        with pytest.raises(P.native.OrrError) as e:
            call()
        assert e.value.code == P.native.ORR_ESTATE
    on_owner.close()
    other.close()


def test_threads_search_one_scope_while_another_grows():
    idx, model, q, texts = _shard_b()
    ids = model.ids[::3]
    sc, growing = idx.scope(ids), idx.scope(model.ids[:10])
    want = _in_scope(idx, q, texts, 10, NB, sc)
    assert _equal(want, _masked(idx, q, texts, 10, NB, ids))
    bad, added = [], []

    def search():
        for _ in range(6):
            if not _equal(_in_scope(idx, q, texts, 10, NB, sc), want):
                bad.append(1)

    def grow():
        for i in range(12):
            added.append(growing.add_ids(model.ids[10 + 50 * i: 10 + 50 * (i + 1)]))

    threads = [threading.Thread(target=search) for _ in range(4)] + [threading.Thread(target=grow)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not bad and added == [50] * 12 and growing.rows == 610
    assert np.array_equal(growing.row_ids(), model.ids[:610])
    sc.close()
    growing.close()
    idx.close()
