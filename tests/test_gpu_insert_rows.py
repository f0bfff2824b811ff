"""Rows into a sealed shard in place (orr_index_insert_rows): afterwards every search, every screening image and a shard
file's round trip must be what a shard sealed from scratch from (the old rows, then the new rows) gives.  Reference behaviour
being matched: InMemoryIngestionStore.UpsertChunksAsync (InMemoryIngestionStore.cs:17-25) takes chunks of any CreatedAtUtc,
and GetRecentChunksAsync (:57-65) orders them with a STABLE OrderByDescending -- at equal ticks the rows that were there stay
in front of the new ones.

Two references throughout: the oracle over the merged corpus (its row index = the row id used here: old rows 0..n-1, new rows
n, n+1, ... in the order given) and a shard built from scratch from the same rows."""
import threading

import numpy as np
import pytest

from helpers import DAY, NOW, assert_same_ranking, build_index, orc, pkg, random_corpus

pytestmark = pytest.mark.gpu

LONG17 = "seventeenbyteslong"[:17]
LONG33 = "a-token-of-thirty-three-bytes-xyz"
LONG200 = "u" * 200
TEXTS = ["alpha", "the kubernetes helm", "GAMMA delta zzz", "what is the", "freshly minted", LONG17 + " " + LONG33, LONG200[:40]]


def _new_rows(rng, c, m, dim):
    """m rows for the shard of corpus c: in front of everything, behind everything, in the middle, at exact tick ties; some
    without an embedding, some non-finite; contents that reuse old tokens and bring new ones (over 16, over 32, 200 bytes)."""
    old = c["created"]
    lo, hi = int(old.min()), int(old.max())
    created = np.empty(m, np.int64)
    for i in range(m):
        kind = i % 5
        if kind == 0:
            created[i] = hi + 1 + int(rng.integers(0, 5 * DAY))              # newest
        elif kind == 1:
            created[i] = lo - 1 - int(rng.integers(0, 5 * DAY))              # oldest
        elif kind == 2:
            created[i] = int(rng.integers(lo, hi))                           # somewhere inside
        else:
            created[i] = int(old[int(rng.integers(0, len(old)))])            # an exact tie with an old row
    created[m - 1] = created[m - 2] = created[3]                             # ... and ties among the new rows
    emb, contents = [], []
    extra = ["freshly", "minted", LONG17, LONG33, LONG200, "alpha", "kubernetes", "Été", "zzz"]
    for i in range(m):
        if dim == 0 or i % 7 == 3:
            emb.append(None)
        else:
            v = (rng.standard_normal(dim) * rng.choice([1.0, 1e-2, 30.0])).astype(np.float32)
            if i % 11 == 5:
                v[int(rng.integers(0, dim))] = [np.nan, np.inf, -np.inf][i % 3]
            emb.append(v)
        k = int(rng.integers(0, 6))
        contents.append(" ".join(rng.choice(extra, size=k)) if k else "")
    return {"emb": emb, "created": created, "contents": contents, "dim": dim}


def _insert(idx, rows, first_id, sel=None):
    """The rows (or those of `sel`) in calls of one kind each: with vectors, then without.  Returns the ids in call order."""
    P = pkg()
    sel = list(range(len(rows["created"]))) if sel is None else list(sel)
    order = [i for i in sel if rows["emb"][i] is not None] + [i for i in sel if rows["emb"][i] is None]
    ids = {i: first_id + j for j, i in enumerate(order)}
    for with_v in (True, False):
        part = [i for i in order if (rows["emb"][i] is not None) == with_v]
        if not part:
            continue
        emb = np.stack([rows["emb"][i] for i in part]).astype(np.float32) if with_v else None
        lower = [P.text.lower_invariant(rows["contents"][i]) for i in part]
        done = idx.insert_rows(emb, rows["created"][part], lower, row_ids=np.array([ids[i] for i in part], np.int64))
        assert done == len(part)
    return order


def _merged(c, rows, order):
    """Old rows, then the inserted rows in call order: row index = row id."""
    return {"emb": list(c["emb"]) + [rows["emb"][i] for i in order],
            "created": np.concatenate([c["created"], rows["created"][order]]).astype(np.int64),
            "contents": list(c["contents"]) + [rows["contents"][i] for i in order], "dim": c["dim"]}


def _check_against_oracle_and_fresh(idx, merged, qvecs, texts=TEXTS, fresh=None):
    P = pkg()
    n = len(merged["created"])
    corpus = orc.OracleCorpus(merged["emb"], merged["created"], merged["contents"])
    own = fresh is None
    if own:
        fresh = build_index(merged, chunk=211)
    assert idx.rows == n == fresh.rows
    for qv in qvecs:
        for text in texts:
            for topk, limit in ((1, n), (10, n), (n + 100, n + 5), (10, 300), (n + 100, 300)):
                rows, scores = assert_same_ranking(idx, corpus, merged, qv, text, topk, limit)
                q = None if qv is None else np.asarray(qv, np.float32).reshape(1, -1)
                frow, fsc, fcnt = fresh.search(q, [P.text.query_terms(text)], NOW, topk, candidate_limit=limit)
                assert list(frow[0, :fcnt[0]]) == list(rows) and np.array_equal(fsc[0, :fcnt[0]], scores, equal_nan=True)
    if own:
        fresh.close()


@pytest.mark.parametrize("seed,n,dim", [(11, 400, 3), (12, 500, 16)])
def test_insert_small_shards_equal_the_oracle_and_a_fresh_shard(seed, n, dim):
    P = pkg()
    rng = np.random.default_rng(seed)
    c = random_corpus(rng, n, dim)
    idx = build_index(c, chunk=97)
    rows = _new_rows(rng, c, 60, dim)
    order = _insert(idx, rows, n)
    merged = _merged(c, rows, order)
    near = merged["emb"][n]                                                   # a query that is an inserted row
    queries = [rng.standard_normal(dim).astype(np.float32), np.asarray(near, np.float32), None]
    _check_against_oracle_and_fresh(idx, merged, queries)
    # the errors leave the shard as it is
    with pytest.raises(P.native.OrrError) as e:
        idx.insert_rows(np.ones((1, dim + 1), np.float32), [NOW], [b"x"], row_ids=[10**6])
    assert e.value.code == P.native.ORR_EDIM
    v = idx.view()
    with pytest.raises(P.native.OrrError) as e:
        v.insert_rows(np.ones((1, dim), np.float32), [NOW], [b"x"], row_ids=[10**6])
    assert e.value.code == P.native.ORR_EINVAL                                # on a view
    with pytest.raises(P.native.OrrError) as e:
        idx.insert_rows(np.ones((1, dim), np.float32), [NOW], [b"x"], row_ids=[10**6])
    assert e.value.code == P.native.ORR_ESTATE                                # while a view is alive
    v.close()
    assert idx.insert_rows(np.zeros((0, dim), np.float32), np.zeros(0, np.int64), [], row_ids=np.zeros(0, np.int64)) == 0
    _check_against_oracle_and_fresh(idx, merged, queries[:1], TEXTS[:2])
    idx.close()


def test_insert_before_the_seal_is_estate():
    P = pkg()
    idx = P.RecallIndex(dim=8)
    idx.append(np.ones((4, 8), np.float32), np.full(4, NOW, np.int64), [b"a"] * 4)
    with pytest.raises(P.native.OrrError) as e:
        idx.insert_rows(np.ones((1, 8), np.float32), [NOW], [b"x"], row_ids=[9])
    assert e.value.code == P.native.ORR_ESTATE
    idx.seal()
    assert idx.insert_rows(np.ones((1, 8), np.float32), [NOW], [b"x"], row_ids=[9]) == 1
    assert idx.rows == 5
    idx.close()


def test_insert_into_an_empty_sealed_shard_and_without_embeddings():
    P = pkg()
    rng = np.random.default_rng(5)
    idx = P.RecallIndex(dim=16)
    idx.seal()
    c0 = {"emb": [], "created": np.zeros(0, np.int64), "contents": [], "dim": 16}
    rows = _new_rows(rng, {"created": np.array([NOW - DAY, NOW], np.int64)}, 30, 16)
    order = _insert(idx, rows, 0)
    _check_against_oracle_and_fresh(idx, _merged(c0, rows, order), [rng.standard_normal(16).astype(np.float32), None], TEXTS[:5])
    idx.close()
    c = random_corpus(rng, 300, 0)                                            # a corpus without embeddings (dim 0)
    idx = build_index(c)
    rows = _new_rows(rng, c, 25, 0)
    order = _insert(idx, rows, 300)
    _check_against_oracle_and_fresh(idx, _merged(c, rows, order), [None], TEXTS[:5])
    idx.close()


def test_deleted_rows_stay_deleted_then_compact_and_insert_again():
    P = pkg()
    rng = np.random.default_rng(21)
    n, dim = 600, 16
    c = random_corpus(rng, n, dim)
    idx = build_index(c, chunk=131)
    dead = sorted(int(r) for r in rng.choice(n, 40, replace=False))
    assert idx.delete_rows(dead) == 40
    rows = _new_rows(rng, c, 50, dim)
    order = _insert(idx, rows, n)
    merged = _merged(c, rows, order)
    assert idx.rows == n + 50 and idx.live_rows == n + 50 - 40
    queries = [rng.standard_normal(dim).astype(np.float32), np.asarray(c["emb"][dead[0]] if c["emb"][dead[0]] is not None else merged["emb"][n], np.float32), None]

    def check(merged, dead):
        total = len(merged["created"])
        keep = np.array([r for r in range(total) if r not in set(dead)], np.int64)
        sub = orc.OracleCorpus([merged["emb"][r] for r in keep], merged["created"][keep], [merged["contents"][r] for r in keep])
        for qv in queries:
            for text in TEXTS[:5]:
                for topk, limit in ((10, total), (total, total), (10, 300), (400, 300)):
                    q = None if qv is None else qv.reshape(1, -1)
                    got, scores, counts = idx.search(q, [P.text.query_terms(text)], NOW, topk, candidate_limit=limit)
                    orow, osc, _ = sub.search([] if qv is None else qv, text, NOW, topk, candidate_limit=limit)
                    k = int(counts[0])
                    assert list(got[0, :k]) == [int(keep[r]) for r in orow], (text, topk, limit)
                    assert np.array_equal(scores[0, :k], osc, equal_nan=True), (text, topk, limit)

    check(merged, dead)
    more_dead = [n + 1, n + 7, next(r for r in range(n) if r not in dead)]    # inserted rows can be deleted by their ids too
    assert idx.delete_rows(more_dead) == 3
    dead2 = dead + more_dead
    check(merged, dead2)
    assert idx.compact() == 43
    assert idx.rows == idx.live_rows == n + 50 - 43
    check(merged, dead2)
    rows2 = _new_rows(rng, c, 35, dim)
    order2 = _insert(idx, rows2, n + 50)                                      # ids go on behind the first insert's
    merged2 = _merged(merged, rows2, order2)
    assert idx.rows == n + 85 - 43
    check(merged2, dead2)
    idx.close()


def test_three_inserts_then_save_and_load(tmp_path):
    P = pkg()
    rng = np.random.default_rng(31)
    n, dim = 1500, 16
    c = random_corpus(rng, n, dim)
    idx = build_index(c, chunk=499)
    merged, at = c, n
    for m in (40, 1, 25):
        rows = _new_rows(rng, c, max(m, 5), dim)
        sel = list(range(m)) if m >= 5 else [2]
        order = _insert(idx, rows, at, sel)
        merged = _merged(merged, rows, order)
        at += len(order)
    assert idx.delete_rows([5, n + 3]) == 2
    path = str(tmp_path / "grown.orr")
    idx.save(path)
    back = P.RecallIndex.load(path)
    assert back.rows == idx.rows == at and back.live_rows == at - 2
    queries = [rng.standard_normal(dim).astype(np.float32), None]
    for qv in queries:
        for text in TEXTS:
            for topk, limit in ((10, at), (at, at), (10, 300)):
                q = None if qv is None else qv.reshape(1, -1)
                a = idx.search(q, [P.text.query_terms(text)], NOW, topk, candidate_limit=limit)
                b = back.search(q, [P.text.query_terms(text)], NOW, topk, candidate_limit=limit)
                for x, y in zip(a, b):
                    assert np.array_equal(x, y, equal_nan=True), (text, topk, limit)
    # the loaded shard holds exactly its rows: an insert into it takes the growth path
    rows = _new_rows(rng, c, 30, dim)
    o1 = _insert(idx, rows, at)
    o2 = _insert(back, rows, at)
    assert o1 == o2 and back.rows == at + 30
    for text in TEXTS[:5]:
        for limit in (at + 30, 300, 40):
            a = idx.search(queries[0].reshape(1, -1), [P.text.query_terms(text)], NOW, 20, candidate_limit=limit)
            b = back.search(queries[0].reshape(1, -1), [P.text.query_terms(text)], NOW, 20, candidate_limit=limit)
            for x, y in zip(a, b):
                assert np.array_equal(x, y, equal_nan=True), (text, limit)
    back.close()
    idx.close()


def test_insert_into_a_loaded_shard_with_tombstones(tmp_path):
    """A shard file holds the timestamps as the device has them: 0 at every deleted row.  Rows inserted into the loaded shard
    must still land where their ticks put them among the LIVE rows -- not at the first deleted position -- which a small
    candidate_limit shows: it counts live rows from the front, so a row that is too far in front displaces one that belongs."""
    P = pkg()
    rng = np.random.default_rng(71)
    n, dim = 1500, 16
    c = random_corpus(rng, n, dim)
    idx = build_index(c, chunk=499)
    by_age = np.argsort(-c["created"], kind="stable")                          # candidate order: position -> row id
    dead = sorted({int(by_age[p]) for p in [0, 1, 2, 7, 8, 30, 31, 32, 33, 120, 290, 299, 300, 700, n - 2, n - 1]} |
                  {int(r) for r in rng.choice(n, 60, replace=False)})
    assert idx.delete_rows(dead) == len(dead)
    path = str(tmp_path / "tombstones.orr")
    idx.save(path)
    back = P.RecallIndex.load(path)
    assert back.rows == n and back.live_rows == n - len(dead)
    rows = _new_rows(rng, c, 60, dim)                                         # newest, oldest, inside, exact ties
    order = _insert(back, rows, n)
    assert _insert(idx, rows, n) == order                                     # the shard that never left the device: the control
    merged = _merged(c, rows, order)
    total = n + 60
    assert back.rows == total and back.live_rows == total - len(dead)
    keep = np.array([r for r in range(total) if r not in set(dead)], np.int64)
    sub = orc.OracleCorpus([merged["emb"][r] for r in keep], merged["created"][keep], [merged["contents"][r] for r in keep])
    queries = [rng.standard_normal(dim).astype(np.float32), np.asarray(merged["emb"][n], np.float32), None]

    def check(shard, label):
        for qv in queries:
            for text in TEXTS[:5]:
                for topk, limit in ((10, 300), (300, 300), (40, 40), (5, 3), (10, total), (total, total)):
                    q = None if qv is None else qv.reshape(1, -1)
                    got, scores, counts = shard.search(q, [P.text.query_terms(text)], NOW, topk, candidate_limit=limit)
                    orow, osc, _ = sub.search([] if qv is None else qv, text, NOW, topk, candidate_limit=limit)
                    k = int(counts[0])
                    assert list(got[0, :k]) == [int(keep[r]) for r in orow], (label, text, topk, limit)
                    assert np.array_equal(scores[0, :k], osc, equal_nan=True), (label, text, topk, limit)

    check(back, "loaded")
    check(idx, "control")
    # the repaired mirror travels on: compact the loaded shard, insert again, save and load once more
    assert back.compact() == len(dead)
    rows2 = _new_rows(rng, c, 20, dim)
    order2 = _insert(back, rows2, total)
    young = next(int(r) for r in by_age if int(r) not in set(dead))           # the newest old row still alive
    assert back.delete_rows([young, total + 1]) == 2
    path2 = str(tmp_path / "tombstones2.orr")
    back.save(path2)
    again = P.RecallIndex.load(path2)
    rows3 = _new_rows(rng, c, 15, dim)
    order3 = _insert(again, rows3, total + 20)
    merged = _merged(_merged(merged, rows2, order2), rows3, order3)
    dead = dead + [young, total + 1]
    total += 35
    keep = np.array([r for r in range(total) if r not in set(dead)], np.int64)
    sub = orc.OracleCorpus([merged["emb"][r] for r in keep], merged["created"][keep], [merged["contents"][r] for r in keep])
    assert again.rows == total - (len(dead) - 2) and again.live_rows == total - len(dead)
    check(again, "loaded twice")
    for h in (again, back, idx):
        h.close()


def test_c_level_argument_checks_on_a_sealed_index():
    """The checks the Python wrapper never lets through: NULL row_ids, NULL created_ticks, NULL content_off, NULL emb with a
    dimension, on a real sealed index -- ORR_EINVAL, *out_inserted zeroed, nothing touched."""
    import ctypes as C
    P = pkg()
    N = P.native
    dim = 8
    idx = P.RecallIndex(dim=dim)
    idx.append(np.ones((4, dim), np.float32), np.full(4, NOW, np.int64), [b"a b"] * 4)
    idx.seal()
    emb = np.ones((2, dim), np.float32)
    ticks = np.full(2, NOW, np.int64)
    pool = np.frombuffer(b"xyxy", np.uint8).copy()
    off = np.array([0, 2, 4], np.uint64)
    ids = np.array([10, 11], np.int64)
    f = N.hip.orr_index_insert_rows
    good = [emb.ctypes.data, ticks.ctypes.data, pool.ctypes.data, off.ctypes.data, ids.ctypes.data]
    for hole, word in ((4, b"row_ids"), (1, b"created_ticks"), (3, b"content_off"), (0, b"emb")):
        args = list(good)
        args[hole] = None
        done = C.c_int64(7)
        assert f(idx._h, 2, dim, *args, C.cast(C.byref(done), C.c_void_p)) == N.ORR_EINVAL, word
        assert done.value == 0, word
        assert word in N.hip.orr_last_error(), word
    done = C.c_int64(7)
    assert f(idx._h, -1, dim, *good, C.cast(C.byref(done), C.c_void_p)) == N.ORR_EINVAL and done.value == 0
    assert f(idx._h, 2, 0, *good, None) == N.ORR_EINVAL                       # dim 0 takes emb = NULL
    assert idx.rows == 4
    rows, _, counts = idx.search(np.ones((1, dim), np.float32), [P.text.query_terms("a")], NOW, 10, candidate_limit=10)
    assert counts[0] == 4 and sorted(rows[0, :4]) == [0, 1, 2, 3]
    done = C.c_int64(7)
    assert f(idx._h, 2, dim, *good, C.cast(C.byref(done), C.c_void_p)) == N.ORR_OK and done.value == 2 and idx.rows == 6
    idx.close()


@pytest.mark.parametrize("reserve", [True, False])
def test_insert_with_capacity_reserved_and_without(reserve):
    """capacity_rows reserved: the embeddings move in place.  Without: appended in ONE call the arrays hold exactly the rows
    (at least 1024), so the insert has to grow them first.  Both give the same shard."""
    P = pkg()
    rng = np.random.default_rng(41)
    n, dim = 2048, 20
    c = random_corpus(rng, n, dim, p_null=0.0, dup_frac=0.0)
    idx = P.RecallIndex(dim=dim, capacity_rows=n + 500 if reserve else 0)
    idx.append(np.stack(c["emb"]), c["created"], [P.text.lower_invariant(s) for s in c["contents"]])
    idx.seal()
    rows = _new_rows(rng, c, 300, dim)
    order = _insert(idx, rows, n)
    merged = _merged(c, rows, order)
    _check_against_oracle_and_fresh(idx, merged, [rng.standard_normal(dim).astype(np.float32)], TEXTS[:3])
    idx.close()


def _big(rng, n, dim):
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    created = (NOW - 1000 * np.arange(n)).astype(np.int64)                  # strictly older: position == row id
    words = np.array(["alpha", "beta", "gamma", "delta", "kubernetes", "helm", "azure", "cosmos"])
    contents = [" ".join(w) for w in words[rng.integers(0, len(words), (n, 4))]]
    return emb, created, contents


def _shard(P, emb, created, contents, ids=None, capacity=0):
    n = emb.shape[0]
    idx = P.RecallIndex(dim=emb.shape[1], capacity_rows=capacity)
    for r0 in range(0, n, 65_536):
        idx.append(emb[r0:r0 + 65_536], created[r0:r0 + 65_536], [s.encode() for s in contents[r0:r0 + 65_536]],
                   row_ids=None if ids is None else ids[r0:r0 + 65_536])
    idx.seal()
    return idx


@pytest.mark.parametrize("dim", [512, 192])
def test_insert_into_a_two_stage_shard_equals_a_fresh_shard(dim):
    """dim 512: the int8 shadow; dim 192: the bf16 shadow.  The shadow is built BEFORE the insert, so the insert has to rebuild
    it from the moved rows: the row images of the screening pass must be those of a fresh shard, and the next search runs the
    two-stage pass on it."""
    P = pkg()
    rng = np.random.default_rng(160 + dim)
    n, m = 196_608 + 77, 1000
    emb, created, contents = _big(rng, n, dim)
    idx = _shard(P, emb, created, contents, capacity=n + m if dim == 512 else 0)
    idx.set_option("two_stage", 1)                                           # int8 shadow at 512, bf16 at 192
    qs = rng.standard_normal((200, dim)).astype(np.float32)
    texts = [TEXTS[b % 4] for b in range(200)]
    terms = [P.text.query_terms(t) for t in texts]
    want_mode = 1 if dim % 128 == 0 else 2
    idx.search(qs[:8], terms[:8], NOW, 10, candidate_limit=n)
    assert idx.search_stats()["pass_mode"] == want_mode
    # about 1,000 rows spread over the shard: between two old rows, at exact ties, in front of and behind everything; the
    # first sixteen are near-copies of queries (scaled by 1e-3 and 1e3: a stale int8 scale there loses the row), so that they
    # must rank first
    at = rng.choice(n - 1, m, replace=False)
    new_created = (created[at] - 500).astype(np.int64)
    new_created[100:140] = created[at[100:140]]                               # ties
    new_created[140:150] = NOW + 1 + np.arange(10)
    new_created[150:160] = created[-1] - 1 - np.arange(10)
    new_emb = rng.standard_normal((m, dim)).astype(np.float32)
    for j in range(16):
        new_emb[j] = (qs[j] + np.float32(1e-3) * rng.standard_normal(dim).astype(np.float32)) * np.float32(1e-3 if j % 2 else 1e3)
    new_emb[20, 5] = np.nan
    new_emb[21, 0] = np.inf
    new_emb[22] = 0.0
    new_contents = ["alpha freshly " + LONG33 if j % 3 == 0 else "kubernetes helm gamma" for j in range(m)]
    ids = np.arange(n, n + m, dtype=np.int64)
    assert idx.insert_rows(new_emb, new_created, [s.encode() for s in new_contents], row_ids=ids) == m
    assert idx.rows == n + m

    all_emb = np.concatenate([emb, new_emb])
    all_created = np.concatenate([created, new_created])
    all_contents = contents + new_contents
    fresh = _shard(P, all_emb, all_created, all_contents, ids=np.arange(n + m, dtype=np.int64))
    fresh.set_option("two_stage", 1)
    if dim % 128 == 0:
        d1, iq1, ie1 = idx.screen_i8_dots(qs[:8], 0, images=True)
        d2, iq2, ie2 = fresh.screen_i8_dots(qs[:8], 0, images=True)
        assert np.array_equal(ie1, ie2), "int8 row images differ at rows %s" % np.nonzero((ie1 != ie2).any(1))[0][:10]
        assert np.array_equal(d1, d2)
        c1, c2 = idx.screen_i8_consts(), fresh.screen_i8_consts()             # the bound's row constants, bit for bit
        for name in ("scale", "rel_err", "rel_hat", "rowf"):
            differ = np.nonzero((c1[name].view(np.uint32) != c2[name].view(np.uint32)).reshape(n + m, -1).any(1))[0]
            assert differ.size == 0, f"{name} differs from a fresh shard's at rows {differ[:10]}"
    else:
        assert np.array_equal(idx.screen_dots(qs[:8]), fresh.screen_dots(qs[:8]), equal_nan=True)
    for B in (1, 8, 200):
        a = idx.search(qs[:B], terms[:B], NOW, 10, candidate_limit=n + m)
        assert idx.search_stats()["pass_mode"] == want_mode, B
        b = fresh.search(qs[:B], terms[:B], NOW, 10, candidate_limit=n + m)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), B
    corpus = orc.OracleCorpus(list(all_emb), all_created, all_contents)
    for b in (0, 1, 7, 15, 40):
        orow, osc, _ = corpus.search(qs[b], texts[b], NOW, 10, candidate_limit=n + m, threads=8)
        if b < 16:
            assert int(orow[0]) == n + b, b                                   # the near-copy ranks first
        assert list(a[0][b, :a[2][b]]) == list(orow), b
        assert np.array_equal(a[1][b, :a[2][b]], osc), b
    a300 = idx.search(qs[:4], terms[:4], NOW, 10, candidate_limit=300)
    for b in range(4):
        orow, osc, _ = corpus.search(qs[b], texts[b], NOW, 10, candidate_limit=300, threads=8)
        assert list(a300[0][b, :a300[2][b]]) == list(orow) and np.array_equal(a300[1][b, :a300[2][b]], osc), b
    idx.close()
    fresh.close()


def test_four_threads_search_one_handle_after_an_insert():
    P = pkg()
    rng = np.random.default_rng(51)
    n, dim = 6000, 32
    c = random_corpus(rng, n, dim)
    idx = build_index(c, chunk=1999)
    qs = rng.standard_normal((12, dim)).astype(np.float32)
    texts = [TEXTS[b % 5] for b in range(12)]
    terms = [P.text.query_terms(t) for t in texts]
    errors, got = [], {}

    def run(key, b0):
        try:
            for _ in range(3):
                got[key] = idx.search(qs[b0:b0 + 3], terms[b0:b0 + 3], NOW, 10, candidate_limit=n + 200)
        except Exception as ex:            # pragma: no cover - reported below
            errors.append(ex)

    def four():
        ts = [threading.Thread(target=run, args=(i, 3 * i)) for i in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors and len(got) == 4

    four()                                                                    # the lanes exist before the insert
    rows = _new_rows(rng, c, 200, dim)
    order = _insert(idx, rows, n)
    merged = _merged(c, rows, order)
    got.clear()
    four()                                                                    # ... and are remade on demand behind it
    corpus = orc.OracleCorpus(merged["emb"], merged["created"], merged["contents"])
    for i in range(4):
        rws, scores, counts = got[i]
        for j in range(3):
            orow, osc, _ = corpus.search(qs[3 * i + j], texts[3 * i + j], NOW, 10, candidate_limit=n + 200)
            assert list(rws[j, :counts[j]]) == list(orow), (i, j)
            assert np.array_equal(scores[j, :counts[j]], osc, equal_nan=True), (i, j)
    idx.close()


def test_insert_through_a_cluster():
    P = pkg()
    rng = np.random.default_rng(61)
    n, dim = 3000, 16
    c = random_corpus(rng, n, dim, p_null=0.0)
    order = np.argsort(-c["created"], kind="stable")
    c = {"emb": [c["emb"][i] for i in order], "created": c["created"][order], "contents": [c["contents"][i] for i in order], "dim": dim}
    lower = [P.text.lower_invariant(s) for s in c["contents"]]
    half = n // 2
    while c["created"][half] == c["created"][half - 1]:                       # the shards split between two distinct ticks
        half += 1
    cl = P.RecallCluster([0, 0], dim)
    bounds = [0, half, n]
    for g in range(2):
        cl.shard(g).append(np.stack(c["emb"][bounds[g]:bounds[g + 1]]), c["created"][bounds[g]:bounds[g + 1]],
                           lower[bounds[g]:bounds[g + 1]], row_ids=np.arange(bounds[g], bounds[g + 1], dtype=np.int64))
    cl.seal()
    cut_hi, cut_lo = int(c["created"][half - 1]), int(c["created"][half])     # shard 0 ends at cut_hi, shard 1 starts at cut_lo < cut_hi
    m = 40
    new0 = {"emb": [rng.standard_normal(dim).astype(np.float32) for _ in range(m)],
            "created": np.concatenate([rng.integers(cut_hi, int(c["created"][0]) + DAY, m - 2), [cut_hi, cut_hi]]).astype(np.int64),
            "contents": ["freshly alpha" if i % 2 else "minted " + LONG33 for i in range(m)]}
    new1 = {"emb": [rng.standard_normal(dim).astype(np.float32) for _ in range(m)],
            "created": np.concatenate([rng.integers(int(c["created"][-1]) - DAY, cut_lo + 1, m - 2), [cut_lo, cut_lo]]).astype(np.int64),
            "contents": ["kubernetes minted" if i % 2 else "" for i in range(m)]}
    qs = rng.standard_normal((6, dim)).astype(np.float32)
    qs[1] = new0["emb"][3]
    qs[2] = new1["emb"][4]
    texts = [TEXTS[b % 5] for b in range(6)]
    terms = [P.text.query_terms(t) for t in texts]
    before = cl.search(qs, terms, NOW, 10, candidate_limit=n)

    def put(g, rows, first_id, sel=None):
        sel = list(range(len(rows["created"]))) if sel is None else sel
        return cl.insert_rows(g, np.stack([rows["emb"][i] for i in sel]), rows["created"][sel],
                              [P.text.lower_invariant(rows["contents"][i]) for i in sel],
                              row_ids=np.arange(first_id, first_id + len(sel), dtype=np.int64))

    # an insert that breaks the order of the shards is refused and nothing changes
    bad0 = {"emb": new0["emb"][:2], "created": np.array([cut_hi + 5, cut_lo - 1], np.int64), "contents": ["a", "b"]}
    bad1 = {"emb": new1["emb"][:2], "created": np.array([cut_lo - 5, cut_hi + 1], np.int64), "contents": ["a", "b"]}
    for g, bad in ((0, bad0), (1, bad1)):
        with pytest.raises(P.native.OrrError) as e:
            put(g, bad, 10**6)
        assert e.value.code == P.native.ORR_EINVAL
    assert cl.rows == n
    again = cl.search(qs, terms, NOW, 10, candidate_limit=n)
    for x, y in zip(before, again):
        assert np.array_equal(x, y, equal_nan=True)

    assert put(1, new1, n + m) == m                                           # the shard behind first, then the one in front of it
    assert put(0, new0, n) == m
    assert cl.rows == n + 2 * m
    merged = {"emb": c["emb"] + new0["emb"] + new1["emb"], "created": np.concatenate([c["created"], new0["created"], new1["created"]]),
              "contents": c["contents"] + new0["contents"] + new1["contents"]}
    corpus = orc.OracleCorpus(merged["emb"], merged["created"], merged["contents"])
    one = build_index(dict(merged, dim=dim), chunk=1013)                      # one index over all the rows
    for topk, limit in ((10, n + 2 * m), (1, 300), (300, n + 2 * m), (10, half + m + 3)):
        rows, scores, counts = cl.search(qs, terms, NOW, topk, candidate_limit=limit)
        orows, oscores, ocounts = one.search(qs, terms, NOW, topk, candidate_limit=limit)
        for b in range(6):
            orow, osc, _ = corpus.search(qs[b], texts[b], NOW, topk, candidate_limit=limit)
            assert list(rows[b, :counts[b]]) == list(orow) == list(orows[b, :ocounts[b]]), (topk, limit, b)
            assert np.array_equal(scores[b, :counts[b]], osc, equal_nan=True), (topk, limit, b)
    one.close()
    cl.close()
