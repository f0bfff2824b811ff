"""Row keys and the per-key search (orr_keys_*, orr_scope_create_keys, orr_search_batch_per_key).

The model is a Python restatement of the header's definition: the ranking R is the oracle's OracleCorpus.search over the live
rows (of the scope, where one is given) in candidate order; R is walked once from the top keeping at most max_per_key rows of
a key (_walk_all); out_rounds is restated by the round rule over the same R (_walk_rounds: each round the first `pool` rows of R
without closed keys and seen rows), which must keep exactly what the one walk keeps.  Every check of a call is exact equality of
rows, score BITS, keys, counts and rounds (_check).  On K1 the oracle ranks every candidate; on K2 it is asked for the first
DEPTH rows and the test asserts that the walk ended inside them or that the candidates ran out.  The K2 queries the oracle does
not rank are compared array for array with an emulation through calls that exist without the feature (_emulate: search /
search_in_scope at topk = pool over exclusion scopes made of ids, the candidate set frozen the same way).

Shards (synthetic rows; built once per module, only read except where a test builds its own):
    K1   4,099 x 70      the exact paths, the list path of small scopes, a row count that is no multiple of 32, 64 or 128
    K2 200,000 x 128     the int8 two-stage pass and the grouped screen
    K3  70,001 x 64      maintenance (built fresh, capacity reserved)
Keys: consecutive candidate rows in runs of 1 .. 40 per key; about 5 % of the rows ORR_KEY_NONE; runs with the keys 0, -1,
INT64_MAX and INT64_MIN + 1; one key spread over non-adjacent rows.  Planted at the old end of the shard (recency ~ 0, so the
cosine decides): five documents of 70 copies each of the vector v at five separate distances (target A: query 0 with
max_per_key 1, topk 10, pool 16 needs exactly six rounds), and four documents of 12 copies of a vector w (target B: larger than
take 10, smaller than the pool of 16).  Queries 0 and 1 are v and w (cosine-only), 2 .. 5 cosine-only near a row, 6 holds a NaN
coordinate, the rest are hybrid (terms and recency)."""
import threading

import numpy as np
import pytest

import test_gpu_scope_near as nbase
import test_gpu_scope_terms as tbase
from helpers import pkg

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NONE = I64_MIN
SHAPES = {"K1": (4_099, 70), "K2": (200_000, 128), "K3": (70_001, 64)}
NQ = 24
DEPTH = 1_000                                           # rows the oracle ranks on K2 (the planted case needs about 360)
LEVELS = (0.05, 0.15, 0.25, 0.35, 0.45)                 # |copy - v| / |v| per document of target A: cosines 0.9988 .. 0.912
SPREAD_KEY = 777_777
_syn, _same, _stats, _terms = tbase._syn, tbase._same, tbase._stats, tbase._terms
KERNELS = ("keys_exclude", "keys_clear_seen", "keys_member", "keys_gather", "keys_scatter", "keys_remap")


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def _walk_all(keys, take, cap):
    kept, count = [], {}
    for r, k in enumerate(keys):
        if len(kept) == take:
            break
        k = int(k)
        if k != NONE:
            if count.get(k, 0) >= cap:
                continue
            count[k] = count.get(k, 0) + 1
        kept.append(r)
    return kept


def _walk_rounds(keys, take, cap, pool):
    """(kept ranks, rounds) by the round rule over a ranking's keys"""
    kept, count, closed, seen, rounds = [], {}, set(), set(), 0
    finished = False
    while not finished:
        rounds += 1
        rnd = []
        for r, k in enumerate(keys):
            if len(rnd) == pool:
                break
            if r in seen or (int(k) != NONE and int(k) in closed):
                continue
            rnd.append(r)
        for r in rnd:
            k = int(keys[r])
            if k != NONE:
                if k in closed:
                    continue
                count[k] = count.get(k, 0) + 1
                if count[k] >= cap:
                    closed.add(k)
            kept.append(r)
            if len(kept) >= take:
                finished = True
                break
        seen.update(rnd)
        if len(rnd) < pool:
            finished = True
        assert rounds <= take
    return kept, rounds


# ---- shards ------------------------------------------------------------------------------------------------------------------

def _assign_keys(n, rng):
    keys = np.empty(n, np.int64)
    special = {3: 0, 9: -1, 15: I64_MAX, 21: I64_MIN + 1}   # run number -> key
    r, nxt, i = 0, 1_000, 0
    while r < n:
        run = int(rng.integers(1, 41))
        if i in special:
            k = special[i]
        elif rng.random() < 0.05:
            k = NONE
        else:
            k, nxt = nxt, nxt + 1
        keys[r:r + run] = k
        r += run
        i += 1
    spread = [5, 100, 1_000, 2_500, n - 600]
    keys[spread] = SPREAD_KEY
    return keys


def _copies(rng, v, level, m):
    """m vectors at relative distance `level` from v, each in a direction orthogonal to v: one cosine for the whole document"""
    v64 = v.astype(np.float64)
    g = rng.standard_normal((m, v.shape[0]))
    g -= np.outer(g @ v64, v64) / (v64 @ v64)
    g *= (level * np.linalg.norm(v64) / np.linalg.norm(g, axis=1))[:, None]
    return (v64[None, :] + g).astype(np.float32)


def _build_shard(name, capacity=None):
    n, dim = SHAPES[name]
    rng = np.random.default_rng(91 + n + dim)
    emb, created, rowbytes = tbase._rows(n, dim)
    keys = _assign_keys(n, rng)
    v = rng.standard_normal(dim).astype(np.float32)
    w = rng.standard_normal(dim).astype(np.float32)
    a0 = n - 400                                        # target A: five documents of 70 adjacent rows
    for d, level in enumerate(LEVELS):
        emb[a0 + 70 * d:a0 + 70 * d + 70] = _copies(rng, v, level, 70)
        keys[a0 + 70 * d:a0 + 70 * d + 70] = 9_000_000 + d
    b0 = n - 460                                        # target B: four documents of 12
    for d, level in enumerate(LEVELS[:4]):
        emb[b0 + 12 * d:b0 + 12 * d + 12] = _copies(rng, w, level, 12)
        keys[b0 + 12 * d:b0 + 12 * d + 12] = 9_100_000 + d
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    idx = tbase._build(emb, created, rowbytes, ids, capacity or n)
    model = nbase.Model(emb, created, rowbytes, ids)
    model.keys = keys.copy()
    syn = _syn()
    q = np.ascontiguousarray(emb[rng.choice(n - 500, NQ, replace=False)] + np.float32(0.35) * rng.standard_normal((NQ, dim)).astype(np.float32))
    texts = list(syn.query_texts(0, NQ, n))
    q[0], q[1] = v, w
    for i in range(6):
        texts[i] = ""                                   # cosine-only
    q[6, dim // 3] = np.nan
    kh = idx.keys(ids, keys)
    return dict(name=name, idx=idx, model=model, kh=kh, q=np.ascontiguousarray(q, np.float32), texts=texts, n=n, dim=dim, ids=ids, cache={})


_SHARDS = {}


def _shard(name):
    if name not in _SHARDS:
        _SHARDS[name] = _build_shard(name)
        if name == "K2":
            s = _SHARDS[name]
            s["idx"].set_option("two_stage", 1)
            tbase._search(s["idx"], s["q"][7:15], s["texts"][7:15], 10, s["n"])     # the int8 shadow and the token bitmaps exist
    return _SHARDS[name]


def _key_of_ids(model):
    return dict(zip(model.ids.tolist(), model.keys.tolist()))


def _ranking(s, qi, limit, scope_ids=None, qvec=None, text=None, tag=None):
    """query qi's ranking: (row ids, scores, keys, complete) -- every candidate on K1, the first DEPTH on the larger shards"""
    sk = None if scope_ids is None else np.asarray(scope_ids, np.int64).tobytes()
    key = ("rank", qi if tag is None else tag, limit, sk)
    if key not in s["cache"]:
        model = s["model"]
        ck = ("corpus", sk)
        if ck not in s["cache"]:
            s["cache"][ck] = model.sub(model.ids if scope_ids is None else scope_ids)
        keep, corpus = s["cache"][ck]
        if corpus is None:
            s["cache"][key] = (np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64), True)
        else:
            took = min(len(keep), max(1, limit))
            depth = took if s["name"] == "K1" else min(took, DEPTH)
            qv = s["q"][qi] if qvec is None else qvec
            tx = s["texts"][qi] if text is None else text
            orow, osc, _ = corpus.search(qv, tx, _syn().NOW_TICKS, depth, candidate_limit=limit, threads=16)
            pos = keep[np.asarray(orow, np.int64)]
            s["cache"][key] = (model.ids[pos], np.asarray(osc), model.keys[pos], len(pos) == took)
    return s["cache"][key]


def _want(s, qi, topk, cap, pool, limit, scope_ids=None, **kw):
    ids, sc, keys, complete = _ranking(s, qi, limit, scope_ids, **kw)
    take = max(1, topk)
    kept = _walk_all(keys, take, cap)
    assert len(kept) == take or complete, ("raise DEPTH", s["name"], qi, topk, cap, len(kept))      # the walk ended inside the ranking
    by_rounds, rounds = _walk_rounds(keys, take, cap, pool)
    assert by_rounds == kept, (qi, topk, cap, pool)
    return ids[kept], sc[kept], keys[kept], rounds


def _per_key(idx, kh, q, texts, topk, cap, pool, limit, within=None):
    return idx.search_per_key(np.ascontiguousarray(q, np.float32), _terms(texts), _syn().NOW_TICKS, topk, kh, max_per_key=cap, pool=pool,
                              within=within, candidate_limit=limit)


def _check(got, s, qis, topk, cap, pool, limit, scope_ids=None, checked=None, what=None, **kw):
    rows, scores, keys, counts, rounds = got
    k = max(1, topk)
    assert rows.shape == scores.shape == keys.shape == (len(qis), k) and counts.shape == rounds.shape == (len(qis),)
    memo = {}
    for b, qi in enumerate(qis):
        if checked is not None and b not in checked:
            continue
        if qi not in memo:
            memo[qi] = _want(s, qi, topk, cap, pool, limit, scope_ids, **kw)
        w_ids, w_sc, w_keys, w_rounds = memo[qi]
        c = int(counts[b])
        assert c == len(w_ids), (what, b, qi, c, len(w_ids))
        assert np.array_equal(rows[b, :c], w_ids), (what, b, qi, rows[b, :c], w_ids)
        assert _same_bits(scores[b, :c], w_sc), (what, b, qi, scores[b, :c], w_sc)
        assert np.array_equal(keys[b, :c], w_keys), (what, b, qi, keys[b, :c], w_keys)
        assert int(rounds[b]) == w_rounds, (what, b, qi, int(rounds[b]), w_rounds)
        assert (rows[b, c:] == -1).all() and (scores[b, c:] == 0.0).all() and (keys[b, c:] == NONE).all(), (what, b)
    return memo


def _emulate(s, qv, text, topk, cap, pool, limit, within_ids=None):
    """one query through calls that exist without the feature: round 1 is search / search_in_scope at topk = pool; every later
    round searches a scope made of the frozen candidate set's ids without the ids of the closed keys' rows and the seen ids"""
    idx, model = s["idx"], s["model"]
    take = max(1, topk)
    live = ~model.dead if within_ids is None else (np.isin(model.ids, within_ids) & ~model.dead)
    c_ids = model.ids[live][:max(1, limit)]             # the frozen candidate set, in candidate order
    key_of = s["cache"].setdefault("key_of", _key_of_ids(model))
    q1, t1 = qv[None, :], _terms([text])
    now = _syn().NOW_TICKS
    if within_ids is None:
        r = idx.search(q1, t1, now, pool, candidate_limit=limit)
    else:
        sc = idx.scope(within_ids)
        r = idx.search_in_scope(q1, t1, now, pool, sc, candidate_limit=limit)
        sc.close()
    kept, count, closed, seen, rounds = [], {}, set(), [], 0
    while True:
        rounds += 1
        n = int(r[2][0])
        done = False
        for j in range(n):
            rid = int(r[0][0, j])
            k = key_of[rid]
            if k != NONE:
                if k in closed:
                    continue
                count[k] = count.get(k, 0) + 1
                if count[k] >= cap:
                    closed.add(k)
            kept.append((rid, r[1][0, j], k))
            if len(kept) >= take:
                done = True
                break
        seen += [int(x) for x in r[0][0, :n]]
        if done or n < pool:
            break
        gone = np.concatenate([model.ids[np.isin(model.keys, np.fromiter(closed, np.int64, len(closed)))], np.asarray(seen, np.int64)])
        sc, ex = idx.scope(c_ids), idx.scope(gone)
        sc.andnot(ex)
        r = idx.search_in_scope(q1, t1, now, pool, sc, candidate_limit=len(model.ids))
        sc.close()
        ex.close()
    return kept, rounds


def _check_emulated(got, s, qis, topk, cap, pool, limit, within_ids, bs, what):
    rows, scores, keys, counts, rounds = got
    memo = {}
    for b in bs:
        qi = qis[b]
        if qi not in memo:
            memo[qi] = _emulate(s, s["q"][qi], s["texts"][qi], topk, cap, pool, limit, within_ids)
        kept, rnds = memo[qi]
        c = int(counts[b])
        assert c == len(kept) and int(rounds[b]) == rnds, (what, b, qi, c, len(kept), int(rounds[b]), rnds)
        assert list(rows[b, :c]) == [x[0] for x in kept] and list(keys[b, :c]) == [x[2] for x in kept], (what, b, qi)
        assert _same_bits(scores[b, :c], np.array([x[1] for x in kept], np.float64)), (what, b, qi)


def _batch(s, B):
    qis = [b % NQ for b in range(B)]
    return qis, s["q"][qis], [s["texts"][i] for i in qis]


def _scope_cases(s):
    """name -> (make the scope, its ids): a ticks window, a term scope, a scope smaller than any take"""
    model, idx, n = s["model"], s["idx"], s["n"]
    lo, hi = int(np.sort(model.created)[n // 4]), int(np.sort(model.created)[3 * n // 4])
    tick_ids = model.ids[(model.created >= lo) & (model.created < hi) & ~model.dead]
    word = _syn().vocab_word(17)
    return {"ticks": (lambda: idx.scope_ticks(lo, hi), tick_ids),
            "terms": (lambda: idx.scope_terms([word], "all"), model.term_ids([word], "all")),
            "tiny": (lambda: idx.scope(model.ids[[3, 4, 5, n - 300, n - 299, n - 1]]), model.ids[[3, 4, 5, n - 300, n - 299, n - 1]])}


# ---- the restatement and the planted structure -------------------------------------------------------------------------------

def test_the_two_walks_agree_and_the_planted_documents_rank_in_blocks():
    rng = np.random.default_rng(2)
    for _ in range(300):
        n, pool = int(rng.integers(0, 300)), int(rng.integers(1, 57))
        take, cap = int(rng.integers(1, pool + 1)), int(rng.integers(1, 4))
        keys = np.repeat(rng.integers(0, 40, n), rng.integers(1, 30, n))[:n]
        keys = np.where(rng.random(len(keys)) < 0.05, NONE, keys)
        kept, rounds = _walk_rounds(keys, take, cap, pool)
        assert kept == _walk_all(keys, take, cap) and 1 <= rounds <= take
    for name in ("K1", "K2"):
        s = _shard(name)
        n = s["n"]
        ids, sc, keys, _ = _ranking(s, 0, n)
        assert list(keys[:350]) == [9_000_000 + d for d in range(5) for _ in range(70)], name     # five blocks of 70, nearest first
        assert not any(9_000_000 <= int(k) < 9_000_005 for k in keys[350:])
        ids, sc, keys, _ = _ranking(s, 1, n)
        assert list(keys[:48]) == [9_100_000 + d for d in range(4) for _ in range(12)], name
        mk = s["model"].keys
        # (5 % of the runs: K1 holds about 200 runs, so the share of ROWS has a standard deviation near 0.018 -- three of them)
        assert 0.0 < (mk == NONE).mean() < 0.105 and all((mk == k).any() for k in (0, -1, I64_MAX, I64_MIN + 1))
        assert (mk == SPREAD_KEY).sum() == 5


# ---- the keys themselves -----------------------------------------------------------------------------------------------------

def test_keys_set_get_and_rows_with_host_and_device_ids():
    import torch
    s = _shard("K1")
    idx, model, n = s["idx"], s["model"], s["n"]
    kh = idx.keys(np.zeros(0, np.int64), np.zeros(0, np.int64))                    # n == 0 is legal: every row ORR_KEY_NONE
    try:
        assert kh.rows == 0 and (kh.get(model.ids[:50]) == NONE).all()
        unknown = np.array([1, 2, -5, 10 ** 12], np.int64)                          # ids are 3 r + 11: these name no row
        ids = np.concatenate([model.ids[[0, 31, 32, 63, 64, n - 1]], unknown])
        vals = np.array([0, -1, I64_MAX, I64_MIN + 1, 42, 43, 5, 6, 7, 8], np.int64)
        (done, st) = _stats(idx, lambda: kh.set(ids, vals))
        assert done == 6 and st["keys_scatter"]["launches"] == 1
        (got, st) = _stats(idx, lambda: kh.get(np.concatenate([ids, model.ids[[1, 2]]])))
        assert st["keys_gather"]["launches"] == 1
        assert list(got) == [0, -1, I64_MAX, I64_MIN + 1, 42, 43, NONE, NONE, NONE, NONE, NONE, NONE]
        assert kh.rows == 6
        # device-resident ids and keys; an explicit ORR_KEY_NONE takes a key away again
        d_ids = torch.from_numpy(model.ids[[64, 100, 101]]).to("cuda:0")
        d_vals = torch.tensor([NONE, 9, 9], dtype=torch.int64, device="cuda:0")
        assert kh.set(d_ids, d_vals) == 3
        assert list(kh.get(model.ids[[64, 100, 101]])) == [NONE, 9, 9] and kh.rows == 7
        # tensors of another dtype or layout are converted, not read as raw int64
        two = torch.from_numpy(np.stack([model.ids[[200, 201, 202]], np.array([77, 78, 79])], axis=1)).to("cuda:0")      # [3, 2]: strided columns
        assert kh.set(two[:, 0], two[:, 1].to(torch.int32)) == 3
        assert list(kh.get(model.ids[[200, 201, 202]])) == [77, 78, 79]
        with pytest.raises(ValueError):
            kh.set(two[:, 0], two[:, 1].cpu())
        # the whole column at once equals the model's
        assert kh.set(model.ids, model.keys) == n
        assert np.array_equal(kh.get(model.ids), model.keys) and kh.rows == int((model.keys != NONE).sum())
        assert kh.get(np.zeros(0, np.int64)).shape == (0,) and kh.set(np.zeros(0, np.int64), np.zeros(0, np.int64)) == 0
    finally:
        kh.close()


@pytest.mark.parametrize("name", ["K1", "K2"])
def test_scope_keys_is_the_rows_of_the_listed_keys(name):
    """keys_member against numpy: tables of 0, 1 and 5,000 keys (the LDS form up to 2,048, global memory beyond), duplicates,
    ORR_KEY_NONE listed, the extreme values, the last partial wave"""
    s = _shard(name)
    idx, model, kh, n = s["idx"], s["model"], s["kh"], s["n"]
    present = np.unique(model.keys[model.keys != NONE])
    rng = np.random.default_rng(6)
    many = np.concatenate([rng.choice(present, min(len(present), 4_000), replace=False), np.arange(5_000_000, 5_001_000)])[:5_000]
    if name == "K1":
        many = np.concatenate([present[:100], np.arange(5_000_000, 5_004_900)])
    assert len(np.unique(many)) == 5_000
    last_key = int(model.keys[n - 1])
    cases = {"none": [], "one": [last_key], "one absent": [123_456_789], "dups": [last_key, last_key, SPREAD_KEY, SPREAD_KEY],
             "no key": [NONE], "extremes": [0, -1, I64_MAX, I64_MIN + 1, NONE], "2048": present[:2_048].tolist(), "2049": present[:2_049].tolist(),
             "5000": many.tolist()}
    for what, listed in cases.items():
        if name == "K1" and what in ("2048", "2049"):
            continue                                    # (K1 holds fewer distinct keys)
        sc, st = _stats(idx, lambda: idx.scope_keys(kh, np.asarray(listed, np.int64)))
        try:
            want = model.ids[np.isin(model.keys, np.asarray(listed, np.int64)) & ~model.dead]
            assert sc.rows == len(want), (what, sc.rows, len(want))
            assert np.array_equal(sc.row_ids(), want), what
            assert st.get("keys_member", {"launches": 0})["launches"] == (1 if listed else 0), what
        finally:
            sc.close()
    # an ordinary scope from then on: a search inside it is the search inside the same rows listed by id
    sc = idx.scope_keys(kh, [9_000_001, 9_100_002, SPREAD_KEY])
    try:
        want = model.ids[np.isin(model.keys, [9_000_001, 9_100_002, SPREAD_KEY])]
        qis, q, texts = _batch(s, 4)
        a = tbase._in_scope(idx, q, texts, 10, n, sc)
        b = tbase._masked(idx, q, texts, 10, n, want)
        assert tbase._equal(a, b) and sc.rows == 70 + 12 + 5
    finally:
        sc.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------

LIMITS = (300, 15_000, None)                            # None: every row


def _cases():
    out, i = [], 0
    for topk in (1, 10, 56):
        for cap in (1, 2, 56):
            for pool in sorted({max(1, topk), 16, 56}):
                if pool < max(1, topk):
                    continue
                out.append((topk, cap, pool, LIMITS[i % 3]))
                i += 1
    return out


@pytest.mark.parametrize("within", [None, "ticks", "terms", "tiny"])
@pytest.mark.parametrize("B", [1, 8, 70, 130])
def test_rows_score_bits_keys_counts_and_rounds_on_k1(B, within):
    s = _shard("K1")
    idx, kh, n = s["idx"], s["kh"], s["n"]
    qis, q, texts = _batch(s, B)
    make, scope_ids = _scope_cases(s)[within] if within else (None, None)
    sc = make() if make else None
    multi = 0
    try:
        for topk, cap, pool, limit in _cases():
            limit = n if limit is None else limit
            got = _per_key(idx, kh, q, texts, topk, cap, pool, limit, within=sc)
            _check(got, s, qis, topk, cap, pool, limit, scope_ids=scope_ids, what=(B, within, topk, cap, pool, limit))
            multi += int((got[4] > 1).sum())
            if cap >= max(1, topk):                     # the plain search's first take rows, bit for bit
                plain = tbase._in_scope(idx, q, texts, topk, limit, sc) if sc else tbase._search(idx, q, texts, topk, limit)
                assert np.array_equal(got[0], plain[0]) and _same_bits(got[1], plain[1]) and np.array_equal(got[3], plain[2])
                assert (got[4] == 1).all()
            if within == "tiny":
                assert (got[3] <= 6).all() and (got[4] == 1).all()
    finally:
        if sc:
            sc.close()
    if within != "tiny":
        assert multi > 0, (B, within)                   # the rounds beyond the first did run


def test_the_planted_query_needs_exactly_six_rounds():
    for name in ("K1", "K2"):
        s = _shard(name)
        idx, kh, n = s["idx"], s["kh"], s["n"]
        got = _per_key(idx, kh, s["q"][:2], s["texts"][:2], 10, 1, 16, n)
        _check(got, s, [0, 1], 10, 1, 16, n, what=("planted", name))
        assert int(got[4][0]) == 6 and int(got[3][0]) == 10, (name, got[4], got[3])
        assert list(got[2][0, :5]) == [9_000_000 + d for d in range(5)]
        # documents of 12 in a pool of 16: a round sees a whole document and the head of the next, closes both; then the rest
        assert list(got[2][1, :4]) == [9_100_000 + d for d in range(4)] and int(got[4][1]) == 3
        got = _per_key(idx, kh, s["q"][:2], s["texts"][:2], 10, 2, 16, n)
        _check(got, s, [0, 1], 10, 2, 16, n, what=("planted, two per key", name))
        assert list(got[2][0]) == [9_000_000 + d for d in range(5) for _ in range(2)]


K2_CASES = [(8, None, 10, 1, 16, None), (70, "ticks", 10, 2, 24, 15_000), (130, None, 56, 1, 56, 300), (130, None, 10, 1, 16, None),
            (1, "terms", 10, 1, 16, None), (8, "terms", 1, 1, 1, None)]


@pytest.mark.parametrize("B,within,topk,cap,pool,limit", K2_CASES)
def test_on_k2_against_the_oracle_and_the_emulation(B, within, topk, cap, pool, limit):
    s = _shard("K2")
    idx, kh, n = s["idx"], s["kh"], s["n"]
    limit = n if limit is None else limit
    qis, q, texts = _batch(s, B)
    make, scope_ids = _scope_cases(s)[within] if within else (None, None)
    sc = make() if make else None
    try:
        idx.search_stats(reset=True)
        got, st = _stats(idx, lambda: _per_key(idx, kh, q, texts, topk, cap, pool, limit, within=sc))
        stats = idx.search_stats()
    finally:
        if sc:
            sc.close()
    checked = sorted(set(range(min(B, 6))) | ({B - 1, 64 + 6} if B > 70 else set()))      # at least six, one of them in the second slice
    _check(got, s, qis, topk, cap, pool, limit, scope_ids=scope_ids, checked=checked, what=(B, within, topk, cap, pool, limit))
    _check_emulated(got, s, qis, topk, cap, pool, limit, scope_ids, [b for b in range(min(B, NQ)) if b not in checked], (B, within))
    for b in range(NQ, B):                              # a repeated query gets its first answer again
        assert np.array_equal(got[0][b], got[0][b % NQ]) and _same_bits(got[1][b], got[1][b % NQ]) and got[4][b] == got[4][b % NQ]
    # launch counts: per round beyond the first and per slice of 64 unfinished queries exactly one keys_exclude
    rounds = got[4]
    want_ex = sum(-(-int((rounds >= r).sum()) // 64) for r in range(2, int(rounds.max()) + 1))
    assert st.get("keys_exclude", {"launches": 0})["launches"] == want_ex, (st.get("keys_exclude"), want_ex)
    assert st.get("keys_clear_seen", {"launches": 0})["launches"] == want_ex
    assert st["keys_gather"]["launches"] == int(rounds.max())
    assert stats["searches"] == 1 + want_ex and stats["queries"] == B + sum(int((rounds >= r).sum()) for r in range(2, int(rounds.max()) + 1))


def test_a_batch_that_finishes_in_round_one_launches_the_plain_search_and_one_gather():
    s = _shard("K2")
    idx, kh, n = s["idx"], s["kh"], s["n"]
    qis, q, texts = _batch(s, 70)
    for topk, cap, pool in ((10, 10, 24), (10, 56, 56), (1, 1, 16)):
        tbase._search(idx, q, texts, pool, n)           # (what the lane adapts to a batch -- buffer sizes, the sample -- has settled)
        plain, st_plain = _stats(idx, lambda: tbase._search(idx, q, texts, pool, n))
        got, st = _stats(idx, lambda: _per_key(idx, kh, q, texts, topk, cap, pool, n))
        assert (got[4] == 1).all()
        k = max(1, topk)
        assert np.array_equal(got[0], plain[0][:, :k]) and _same_bits(got[1], plain[1][:, :k])     # max_per_key >= take: the plain search's arrays
        assert np.array_equal(got[3], np.minimum(plain[2], k))
        mine = {name: v["launches"] for name, v in st.items() if not name.startswith("keys_")}
        theirs = {name: v["launches"] for name, v in st_plain.items()}
        assert mine == theirs, (mine, theirs)
        assert st["keys_gather"]["launches"] == 1 and not any(name in st for name in KERNELS if name != "keys_gather")


def test_sixty_four_different_closed_sets_in_one_slice():
    """keys_exclude through the search: 64 queries near 64 different documents close 64 different key sets in round 1; one more
    slot closes none.  Round 2's bitmaps are what the restatement excludes: every query's answer is the model's."""
    s = _shard("K1")
    idx, kh, model, n = s["idx"], s["kh"], s["model"], s["n"]
    rng = np.random.default_rng(12)
    rows = rng.choice(n - 500, 64, replace=False)
    q = np.ascontiguousarray(model.emb[rows] + np.float32(0.05) * rng.standard_normal((64, s["dim"])).astype(np.float32))
    texts = [""] * 64
    got, st = _stats(idx, lambda: _per_key(idx, kh, q, texts, 24, 1, 24, n))
    for b in range(64):
        _check(tuple(x[b:b + 1] for x in got), s, [b], 24, 1, 24, n, qvec=q[b], text="", tag=("slice", b), what=("slice", b))
    assert (got[4] > 1).sum() >= 16 and st["keys_exclude"]["launches"] >= 1
    assert len({tuple(sorted(set(got[2][b].tolist()))) for b in range(64) if got[4][b] > 1}) >= 16      # different closed sets
    # a key closed by all 64 slots: the same query 64 times, then the last partial wave of K1 (rows 4,096 .. 4,098 hold one key)
    got = _per_key(idx, kh, np.repeat(s["q"][:1], 64, axis=0), [""] * 64, 10, 1, 16, n)
    _check(got, s, [0] * 64, 10, 1, 16, n, what="all slots close the same keys")
    tail = model.ids[n - 3:]
    model_tail_keys = model.keys[n - 3:].copy()
    try:
        assert kh.set(tail, np.array([31_337] * 3, np.int64)) == 3
        model.keys[n - 3:] = 31_337
        s["cache"].clear()
        qt = np.ascontiguousarray(model.emb[[n - 1, n - 2]])
        got = _per_key(idx, kh, qt, ["", ""], 10, 1, 10, n)
        for b in range(2):
            _check(tuple(x[b:b + 1] for x in got), s, [b], 10, 1, 10, n, qvec=qt[b], text="", tag=("tail", b), what=("tail", b))
            assert list(got[2][b]).count(31_337) == 1
    finally:
        kh.set(tail, model_tail_keys)
        model.keys[n - 3:] = model_tail_keys
        s["cache"].clear()


def _closed_in_round_one(keys, take, cap, pool):
    """(the keys a query's first round closes, whether the query goes on to a second round) by the round rule"""
    kept, count, closed = 0, {}, set()
    rnd = [int(k) for k in keys[:pool]]
    for k in rnd:
        if k != NONE:
            if k in closed:
                continue
            count[k] = count.get(k, 0) + 1
            if count[k] >= cap:
                closed.add(k)
        kept += 1
        if kept >= take:
            return closed, False
    return closed, len(rnd) == pool


def test_a_union_table_beyond_the_lds_cut_over_goes_through_global_memory():
    """keys_exclude's global-memory form: 64 queries near 64 rows far apart on K2, topk = pool = 56, max_per_key 1, every row a key
    of its own except that each query's ranks 54 and 55 share one -- round 1 keeps 55 rows and closes 55 keys per slot, so the
    slice's union table holds about 64 x 55 = 3,520 entries, beyond per_key::kLdsTable = 2,048.  Every slot against the restatement."""
    s = _shard("K2")
    idx, model, n = s["idx"], s["model"], s["n"]
    rng = np.random.default_rng(21)
    rows = np.arange(64) * 3_000 + 1_500
    q = np.ascontiguousarray(model.emb[rows] + np.float32(0.05) * rng.standard_normal((64, s["dim"])).astype(np.float32))
    texts = [""] * 64
    old_keys = model.keys.copy()
    kh2 = None
    try:
        keys2 = np.arange(n, dtype=np.int64) + 1_000_000
        for b in range(64):
            ids = _ranking(s, None, n, qvec=q[b], text="", tag=("global", b))[0]
            p = (ids[:56] - 11) // 3                    # (ids are 3 r + 11)
            assert np.array_equal(model.ids[p], ids[:56])
            keys2[p[55]] = keys2[p[54]]
        model.keys = keys2
        s["cache"].clear()
        kh2 = idx.keys(model.ids, keys2)
        got, st = _stats(idx, lambda: _per_key(idx, kh2, q, texts, 56, 1, 56, n))
        union, second = set(), 0
        for b in range(64):
            memo = _check(tuple(x[b:b + 1] for x in got), s, [b], 56, 1, 56, n, qvec=q[b], text="", tag=("global", b), what=("global", b))
            closed, goes_on = _closed_in_round_one(_ranking(s, None, n, qvec=q[b], text="", tag=("global", b))[2], 56, 1, 56)
            if goes_on:
                union |= closed
                second += 1
        assert second == 64 and len(union) > 2_048, (second, len(union))       # ONE slice whose table lies beyond the LDS form
        assert (got[4] == 2).all() and (got[3] == 56).all()
        assert st["keys_exclude"]["launches"] == 1 and st["keys_clear_seen"]["launches"] == 1
        assert st["scope_counts"]["launches"] >= 1 and st["mask_clip_slots"]["launches"] == 1     # the 64 scopes' counts: one launch each
    finally:
        if kh2 is not None:
            kh2.close()
        model.keys = old_keys
        s["cache"].clear()


def test_query_kinds_a_foreign_dimension_dim_zero_and_an_empty_batch():
    P = pkg()
    s = _shard("K1")
    idx, kh, n = s["idx"], s["kh"], s["n"]
    rng = np.random.default_rng(3)
    qf = rng.standard_normal((3, 64)).astype(np.float32)                   # a foreign dim: every cosine is 0, keyword and recency only
    texts = [s["texts"][20], s["texts"][21], ""]
    got = _per_key(idx, kh, qf, texts, 10, 1, 16, n)
    for b in range(3):
        _check(tuple(x[b:b + 1] for x in got), s, [b], 10, 1, 16, n, qvec=qf[b], text=texts[b], tag=("foreign", b), what=("foreign", b))
    got = idx.search_per_key(None, _terms(texts), _syn().NOW_TICKS, 10, kh, max_per_key=2, pool=24, candidate_limit=n)      # dim 0
    for b in range(3):
        _check(tuple(x[b:b + 1] for x in got), s, [b], 10, 2, 24, n, qvec=np.zeros(0, np.float32), text=texts[b], tag=("dim0", b), what=("dim0", b))
    assert (got[4] > 1).any()                           # recency alone ranks whole documents on top: more than one round
    h = P.native.hip
    qoff = np.zeros(1, np.uint32)
    out = np.full(4, 7, np.int64)
    o = out.ctypes.data
    assert h.orr_search_batch_per_key(idx._h, 0, 70, None, None, None, qoff.ctypes.data, 0, 4, 300, None, kh._h, 1, 24, o, o, o, o, o) == 0
    assert (out == 7).all()
    # keys and a scope of another shard; out_rounds may be NULL
    other = _shard("K2")
    with pytest.raises(P.OrrError) as e:
        _per_key(idx, other["kh"], s["q"][:1], s["texts"][:1], 10, 1, 16, n)
    assert e.value.code == P.native.ORR_EINVAL and "another shard" in str(e.value)
    with pytest.raises(P.OrrError) as e:
        idx.scope_keys(other["kh"], [1])
    assert e.value.code == P.native.ORR_EINVAL
    B, k = 2, 10
    q = np.ascontiguousarray(s["q"][:B])
    tpool, toff, qoff = P.pack_terms(_terms(s["texts"][:B]))
    rows, scores, keys, counts = np.zeros((B, k), np.int64), np.zeros((B, k)), np.zeros((B, k), np.int64), np.zeros(B, np.int32)
    assert h.orr_search_batch_per_key(idx._h, B, 70, q.ctypes.data, tpool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, _syn().NOW_TICKS, k, n,
                                      None, kh._h, 1, 16, rows.ctypes.data, scores.ctypes.data, keys.ctypes.data, counts.ctypes.data, None) == 0
    _check((rows, scores, keys, counts, _per_key(idx, kh, q, s["texts"][:B], k, 1, 16, n)[4]), s, [0, 1], k, 1, 16, n, what="no out_rounds")


# ---- maintenance, views, threads, orphans ------------------------------------------------------------------------------------

@pytest.mark.parametrize("reserve", [True, False])
def test_maintenance_carries_the_keys(reserve):
    n, dim = SHAPES["K3"]
    s = _build_shard("K3", capacity=n + (1_000 if reserve else 0))
    idx, model, kh = s["idx"], s["model"], s["kh"]
    qis, q, texts = _batch(s, 8)
    sk = idx.scope_keys(kh, [9_000_002, SPREAD_KEY])     # a scope made from keys follows its rows like any other
    in_sk = lambda: model.ids[np.isin(model.keys, [9_000_002, SPREAD_KEY]) & ~model.dead]

    def check(what, **kw):
        s["cache"].clear()
        live = ~model.dead
        assert np.array_equal(kh.get(model.ids[live]), model.keys[live]), what
        assert kh.rows == int((model.keys[live] != NONE).sum()), what
        assert np.array_equal(sk.row_ids(), in_sk()), what
        for topk, cap, pool in ((10, 1, 16), (10, 2, 24)):
            got = _per_key(idx, kh, q, texts, topk, cap, pool, len(model.ids))
            _check(got, s, qis, topk, cap, pool, len(model.ids), checked=[0, 1, 2, 7], what=(what, topk, cap))
        return got

    try:
        got = check("fresh")
        assert int(got[4][0]) >= 3
        # delete: the first document of target A and 9,000 other rows; a deleted id reads ORR_KEY_NONE
        rng = np.random.default_rng(4)
        gone = np.concatenate([model.ids[n - 400:n - 330], model.ids[rng.choice(n - 500, 9_000, replace=False)]])
        assert idx.delete_rows(gone) == len(gone)
        model.delete(gone)
        assert (kh.get(gone[:100]) == NONE).all()
        check("deleted")
        assert 9_000_000 not in _per_key(idx, kh, q[:1], texts[:1], 10, 1, 16, len(model.ids))[2][0]
        # update: the rows move nowhere, the keys stay
        far = model.ids[[n - 5]]
        new = model.emb[n - 100][None, :].copy()
        assert idx.update_rows(far, new) == 1
        model.update(far, new)
        check("updated")
        _, st = _stats(idx, idx.compact)
        assert st["keys_remap"]["launches"] == 1        # ONE launch for every registered column
        keep = ~model.dead
        model.keys = model.keys[keep]
        model.compact()
        check("compacted")
        # insert 131 rows: they read ORR_KEY_NONE until the host sets them, then they are found
        m = 131
        _, c2, b2 = tbase._rows(m, dim, row0=n, n_total=n + m)
        c2 = c2 + (np.arange(m) % 7) * 40 * _syn().TICKS_PER_DAY                # spread through the shard, not only at its old end
        e2 = np.random.default_rng(5).standard_normal((m, dim)).astype(np.float32)
        e2[:20] = _copies(np.random.default_rng(6), s["q"][0], 0.01, 20)         # nearer to v than every planted document
        ids2 = np.arange(m, dtype=np.int64) + 10_000_000
        _, st = _stats(idx, lambda: idx.insert_rows(e2, c2, b2.reshape(-1), np.arange(m + 1, dtype=np.int64) * b2.shape[1], row_ids=ids2))
        assert st["keys_remap"]["launches"] == 1
        old_ids, old_keys = model.ids.copy(), model.keys.copy()
        model.insert(e2, c2, b2, ids2)
        key_of = dict(zip(old_ids.tolist(), old_keys.tolist()))
        model.keys = np.array([key_of.get(int(i), NONE) for i in model.ids], np.int64)
        assert (kh.get(ids2) == NONE).all()
        got = check("inserted")
        assert (got[2][0, :10] == NONE).all()            # twenty rows without a key fill query 0's take: no cap applies to them
        assert kh.set(ids2, np.full(m, 8_000_000, np.int64)) == m
        model.keys[np.isin(model.ids, ids2)] = 8_000_000
        got = check("inserted and set")
        assert list(got[2][0]).count(8_000_000) == 2 and got[2][0, 0] == 8_000_000
        one = idx.scope_keys(kh, [8_000_000])
        assert one.rows == m
        one.close()
    finally:
        sk.close()
        kh.close()
        idx.close()


def test_views_two_threads_and_orphans_in_both_destroy_orders():
    P = pkg()
    s = _shard("K1")
    idx, kh, n = s["idx"], s["kh"], s["n"]
    qis, q, texts = _batch(s, 16)
    view = idx.view()
    try:
        got = _per_key(view, kh, q, texts, 10, 1, 16, n)
        _check(got, s, qis, 10, 1, 16, n, what="view")
    finally:
        view.close()
    results, errors = [None] * 2, []

    def work(i):
        try:
            for _ in range(3):
                results[i] = _per_key(idx, kh, q, texts, 10, 1 + i, 16 + 8 * i, n)
        except Exception as e:                          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, got in enumerate(results):
        _check(got, s, qis, 10, 1 + i, 16 + 8 * i, n, what=("threads", i))
    # orphans: the index first, then the keys; and the keys first
    emb, created, rowbytes = tbase._rows(500, 16)
    ids = np.arange(500, dtype=np.int64)
    for index_first in (True, False):
        small = tbase._build(emb, created, rowbytes, ids, 500)
        k2 = small.keys(ids, ids // 7)
        assert k2.rows == 500
        if index_first:
            small.close()
            assert k2.rows == -1
            with pytest.raises(P.OrrError) as e:
                k2.set(ids[:3], ids[:3])
            assert e.value.code == P.native.ORR_ESTATE
            with pytest.raises(P.OrrError) as e:
                k2.get(ids[:3])
            assert e.value.code == P.native.ORR_ESTATE
            k2.close()
        else:
            k2.close()
            assert tbase._search(small, emb[:2], ["", ""], 5, 500)[2].tolist() == [5, 5]
            small.close()
