"""The diverse search (orr_search_batch_diverse) and its diagnostic (orr_index_pair_dots).

The model is a Python restatement: the pool is the oracle's Corpus.search(..., topk = pool) over the live rows (of the scope,
where one is given); c_ij is the reference's cosine of the two stored rows, restated in numpy (_pair_dots: float32 products
accumulated strictly in index order in float64; then the guards and dot / (sqrt(ni) * sqrt(nj)) in Python floats), which
test_the_restatement_is_the_oracles holds against oracle.cosine and cosine_of(oracle.dot, ...); the two greedy rules are plain
Python.  Every check of a call is exact equality of rows, score BITS, counts and pool ranks (_check).

Shards (Gaussian rows, synthetic contents and ticks; built once per module, only read except where a test builds its own):
    D1   4,099 x 70      the kernel's scalar staging (dim % 4 != 0), a last slab of 70 columns
    D2   4,099 x 128
    D3  20,000 x 1024    four slabs
    D4 200,000 x 128     the two-stage int8 pass (130 queries)
Planted families, the near-duplicate structure a sliding-window chunker produces: for four anchors, three noisy copies each at
cosines near 0.9999, 0.97 and 0.9 and two exact duplicates; and one family of 60 near-copies (cosine near 0.9999) of a fifth
anchor, larger than any pool.  Queries 0 .. 4 of the pool of 40 are aimed at the anchors (cosine-only), 5 .. 7 are cosine-only
queries near a row, query 8 holds a NaN coordinate, the rest are hybrid (terms and recency)."""
import math
import threading

import numpy as np
import pytest

import test_gpu_scope_near as nbase
import test_gpu_scope_terms as tbase
from helpers import orc, pkg

pytestmark = pytest.mark.gpu

INF = float("inf")
SHAPES = {"D1": (4_099, 70), "D2": (4_099, 128), "D3": (20_000, 1024), "D4": (200_000, 128)}
NQ = 40                                                 # the pool of queries (tbase.POOL_Q); a batch cycles through it
LEVELS = (0.01414, 0.2506, 0.4843)                      # noise / |anchor|: cosines near 0.9999, 0.97, 0.9
MAX_COSINES = (0.95, 0.5, -1.0, INF, -INF)
LAMBDAS = (0.0, 0.3, 0.7, 1.0)
_syn, _same, _stats, _terms = tbase._syn, tbase._same, tbase._stats, tbase._terms


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def _pair_dots(E):
    """[m, m] float64: sum_k (double)fl32(E[i][k] * E[j][k]) in index order"""
    E = np.ascontiguousarray(E, np.float32)
    if E.shape[1] == 0:
        return np.zeros((len(E), len(E)))
    with np.errstate(all="ignore"):
        prod = E[:, None, :] * E[None, :, :]
        return np.add.accumulate(prod.astype(np.float64), axis=2)[:, :, -1]


def _cosine_of(dot, na, nb):
    """scope_near::cosine_of in Python floats"""
    dot, na, nb = float(dot), float(na), float(nb)
    if na <= 0.0 or nb <= 0.0:
        return 0.0
    den = math.sqrt(na) * math.sqrt(nb) if na == na and nb == nb else float("nan")
    if den == 0.0:
        return math.copysign(INF, dot) if dot == dot and dot != 0.0 else float("nan")
    return dot / den


def _pair_cos(E):
    d = _pair_dots(E)
    m = len(E)
    return [[_cosine_of(d[i, j], d[i, i], d[j, j]) for j in range(m)] for i in range(m)]


def _cmp(a, b):
    """double.CompareTo: NaN below everything, equal to itself"""
    if a < b:
        return -1
    if a > b:
        return 1
    if a == b:
        return 0
    if a != a:
        return 0 if b != b else -1
    return 1


def _collapse(n, take, t, cos):
    kept = []
    for r in range(n):
        if len(kept) == take:
            break
        if not any(cos[r][k] >= t for k in kept):
            kept.append(r)
    return kept


def _mmr(n, take, lam, score, cos):
    if n == 0:
        return []
    kept = [0]
    w = 1.0 - lam
    fold = [-INF] * n                                   # each member's greatest cosine to a kept one, folded in pick order
    while len(kept) < take and len(kept) < n:
        best, best_v = -1, 0.0
        for r in range(n):
            if r in kept:
                continue
            c = cos[r][kept[-1]]
            if c > fold[r]:                             # (a NaN is skipped)
                fold[r] = c
            m = 0.0 if fold[r] == -INF else fold[r]
            pen = 0.0 if w == 0.0 else w * m
            v = (lam * score[r]) - pen
            if best < 0 or _cmp(v, best_v) > 0:         # a tie stays with the lower rank
                best, best_v = r, v
        kept.append(best)
    return kept


def _greedy(n, take, mode, param, score, cos):
    return _collapse(n, take, param, cos) if mode == "collapse" else _mmr(n, take, param, score, cos)


# ---- shards ------------------------------------------------------------------------------------------------------------------

def _noisy(rng, anchor, level):
    g = rng.standard_normal(anchor.shape[0]).astype(np.float32)
    scale = np.float32(level * float(np.linalg.norm(anchor.astype(np.float64))) / math.sqrt(anchor.shape[0]))
    return (anchor + scale * g).astype(np.float32)


def _plant(emb, rng):
    """{family: [positions]}; the anchors themselves are members.  Returns the families and the five anchors' positions."""
    n = len(emb)
    free = rng.choice(np.arange(1, n - 1), 5 + 4 * 11 + 60, replace=False).tolist()
    anchors = [free.pop() for _ in range(5)]
    fam = {}
    for a in anchors[:4]:
        rows = [a]
        for level in LEVELS:
            for _ in range(3):
                r = free.pop()
                emb[r] = _noisy(rng, emb[a], level)
                rows.append(r)
        for _ in range(2):
            r = free.pop()
            emb[r] = emb[a]
            rows.append(r)
        fam[a] = rows
    big = [anchors[4]]
    for _ in range(60):
        r = free.pop()
        emb[r] = _noisy(rng, emb[anchors[4]], LEVELS[0])
        big.append(r)
    fam[anchors[4]] = big
    return fam, anchors


def _build_shard(name, capacity=None):
    n, dim = SHAPES[name]
    rng = np.random.default_rng(77 + n + dim)
    emb = rng.standard_normal((n, dim), dtype=np.float32)
    _, created, rowbytes = tbase._rows(n, 64)
    fam, anchors = _plant(emb, rng)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    idx = tbase._build(emb, created, rowbytes, ids, capacity or n)
    model = nbase.Model(emb, created, rowbytes, ids)
    syn = _syn()
    q = np.ascontiguousarray(emb[rng.choice(n, NQ, replace=False)] + np.float32(0.35) * rng.standard_normal((NQ, dim), dtype=np.float32))
    texts = list(syn.query_texts(0, NQ, n))
    for i, a in enumerate(anchors):
        q[i] = _noisy(rng, emb[a], 0.05)
    for i in range(8):
        texts[i] = ""                                   # cosine-only
    q[8, dim // 3] = np.nan
    return dict(name=name, idx=idx, model=model, q=np.ascontiguousarray(q, np.float32), texts=texts, fam=fam, anchors=anchors, n=n, dim=dim,
                ids=ids, cache={})


_SHARDS = {}


def _shard(name):
    if name not in _SHARDS:
        _SHARDS[name] = _build_shard(name)
    return _SHARDS[name]


def _corpus(s, scope_ids=None):
    """(positions of the live rows that take part, the oracle over exactly those); cached (a test that changes the model clears
    s["cache"])"""
    key = ("corpus", None if scope_ids is None else np.asarray(scope_ids, np.int64).tobytes())
    if key not in s["cache"]:
        s["cache"][key] = s["model"].sub(s["model"].ids if scope_ids is None else scope_ids)
    return s["cache"][key]


def _pool(s, qi, limit, scope_ids=None, qvec=None, text=None, tag=None):
    """query qi's undiversified best 56: (positions, scores, cosine matrix), cached per (query, limit, scope)"""
    key = ("pool", qi if tag is None else tag, limit, None if scope_ids is None else np.asarray(scope_ids, np.int64).tobytes())
    if key not in s["cache"]:
        keep, corpus = _corpus(s, scope_ids)
        if corpus is None:
            s["cache"][key] = (np.zeros(0, np.int64), np.zeros(0), [])
        else:
            qv = s["q"][qi] if qvec is None else qvec
            tx = s["texts"][qi] if text is None else text
            orow, osc, _ = corpus.search(qv, tx, _syn().NOW_TICKS, 56, candidate_limit=limit, threads=16)
            pos = keep[orow]
            s["cache"][key] = (pos, np.asarray(osc), _pair_cos(s["model"].emb[pos]))
    return s["cache"][key]


def _want(s, qi, topk, pool, mode, param, limit, scope_ids=None, **kw):
    key = ("want", qi if kw.get("tag") is None else kw["tag"], topk, pool, mode, param, limit, None if scope_ids is None else np.asarray(scope_ids, np.int64).tobytes())
    if key not in s["cache"]:
        pos, sc, cos = _pool(s, qi, limit, scope_ids, **kw)
        n = min(len(pos), pool)
        picks = _greedy(n, max(1, topk), mode, param, sc, cos)
        s["cache"][key] = (s["model"].ids[pos[picks]], sc[picks], picks)
    return s["cache"][key]


def _diverse(idx, q, texts, topk, pool, mode, param, limit, within=None):
    return idx.search_diverse(np.ascontiguousarray(q, np.float32), _terms(texts), _syn().NOW_TICKS, topk, pool, mode=mode, param=param,
                              within=within, candidate_limit=limit)


def _check(got, s, qis, topk, pool, mode, param, limit, scope_ids=None, what=None, **kw):
    rows, scores, counts, ranks = got
    k = max(1, topk)
    assert rows.shape == scores.shape == ranks.shape == (len(qis), k) and counts.shape == (len(qis),)
    memo = {}
    for b, qi in enumerate(qis):
        if qi not in memo:
            memo[qi] = _want(s, qi, topk, pool, mode, param, limit, scope_ids, **kw)
        w_ids, w_sc, w_picks = memo[qi]
        c = int(counts[b])
        assert c == len(w_ids), (what, b, qi, c, len(w_ids))
        assert np.array_equal(rows[b, :c], w_ids), (what, b, qi, rows[b, :c], w_ids)
        assert _same_bits(scores[b, :c], w_sc), (what, b, qi, scores[b, :c], w_sc)
        assert list(ranks[b, :c]) == list(w_picks), (what, b, qi, ranks[b, :c], w_picks)
        assert (rows[b, c:] == -1).all() and (scores[b, c:] == 0.0).all() and (ranks[b, c:] == -1).all(), (what, b)


def _same_bits(a, b):
    """bit for bit, any NaN equal to any NaN (the payload of a NaN is not the reference's to define)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def _launches(st):
    return st["pair_dots"]["launches"] if "pair_dots" in st else 0


def _batch(s, B):
    qis = [b % NQ for b in range(B)]
    return qis, s["q"][qis], [s["texts"][i] for i in qis]


# ---- the restatement is the oracle's -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["D1", "D2", "D3"])
def test_the_restatement_is_the_oracles(name):
    s = _shard(name)
    emb = s["model"].emb
    rng = np.random.default_rng(5)
    rows = sorted(set(sum(s["fam"].values(), [])[:40]) | set(rng.choice(s["n"], 16, replace=False).tolist()) | {0, s["n"] - 1})
    E = emb[rows]
    d, c = _pair_dots(E), _pair_cos(E)
    for i in range(len(rows)):
        for j in range(len(rows)):
            assert d[i, j] == orc.dot(E[i], E[j]), (name, rows[i], rows[j])
            want = orc.cosine(E[i], E[j])
            assert c[i][j] == want, (name, rows[i], rows[j], c[i][j], want)
            assert _cosine_of(orc.dot(E[i], E[j]), orc.dot(E[i], E[i]), orc.dot(E[j], E[j])) == want
    # the planted structure is there: cosines near the three levels and exact copies
    a = s["anchors"][0]
    ca = _pair_cos(emb[s["fam"][a]])[0]
    assert all(0.9998 < x < 1.0 for x in ca[1:4]) and all(0.95 < x < 0.985 for x in ca[4:7]) and all(0.85 < x < 0.94 for x in ca[7:10]), ca
    assert ca[10] == ca[11] == ca[0] and abs(ca[0] - 1.0) < 1e-15
    assert len(s["fam"][s["anchors"][4]]) == 61
    assert _cosine_of(1.0, 0.0, 1.0) == 0.0 and _cosine_of(1.0, 1.0, -1.0) == 0.0


# ---- pair_dots ---------------------------------------------------------------------------------------------------------------

def _check_pairs(s, lists, emb_of=None):
    emb = s["model"].emb
    got, st = _stats(s["idx"], lambda: s["idx"].pair_dots(lists))
    stride = max(len(l) for l in lists)
    assert got.shape == (len(lists), stride, stride)
    memo = {}
    for l, rows in enumerate(lists):
        m = len(rows)
        for i in range(m):
            for j in range(i, m):
                key = (min(rows[i], rows[j]), max(rows[i], rows[j]))
                if key not in memo:
                    memo[key] = orc.dot(emb[key[0]], emb[key[1]])
                want = np.float64(memo[key])
                assert _same_bits(got[l, i, j], want) and _same_bits(got[l, j, i], want), (l, i, j, got[l, i, j], want)
        assert np.isnan(got[l, m:, :]).all() and np.isnan(got[l, :, m:]).all()          # beyond a list's length nothing is written
    assert _launches(st) == -(-len(lists) // 1024)
    return got


@pytest.mark.parametrize("name", ["D1", "D2", "D3"])
def test_pair_dots_are_the_oracles_dots(name):
    s = _shard(name)
    n = s["n"]
    rng = np.random.default_rng(11)
    pick = lambda m: rng.choice(n, m, replace=False).tolist()
    fam = s["fam"][s["anchors"][0]]
    one = [[0, n - 1] + pick(53) + fam[:1]]                                             # 56 rows, the first and the last position
    assert len(one[0]) == 56
    got = _check_pairs(s, one)
    norms = nbase._exact_dots(s["model"].emb, s["model"].emb)
    assert np.array_equal(np.diagonal(got[0]).view(np.int64), norms[one[0]].view(np.int64))      # the diagonal: the shard's exact norms
    _check_pairs(s, [[5], pick(2), pick(55)])
    _check_pairs(s, [[n - 1]])
    _check_pairs(s, [[7, 7, 9, 7]])                                                     # a duplicated position
    lists = [pick(1 + l % 8) for l in range(257)]
    lists[3], lists[200], lists[256] = pick(56), pick(55), [0, n - 1, 0]
    lists[100] = []
    _check_pairs(s, lists)


def test_pair_dots_on_rows_no_order_of_which_is_provably_exact():
    """a small shard of its own: products spanning 36 decades, both zeros, subnormal products, infinities and NaNs, a row
    without an embedding; dim 70 and 260 (one slab and a second slab of four columns)"""
    P = pkg()
    for dim in (70, 260):
        rng = np.random.default_rng(dim)
        n = 64
        emb = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-18, 18, (n, dim))).astype(np.float32)
        emb[1] = 0.0
        emb[2] = -0.0
        emb[3] = np.float32(1e-23) * rng.standard_normal(dim).astype(np.float32)        # subnormal products with itself
        emb[4, 5], emb[5, 5], emb[6, 7] = np.inf, -np.inf, np.nan
        emb[7, dim - 1] = np.nan                                                        # in the last slab's tail
        emb[8, dim - 1], emb[9, dim - 1] = np.float32(3e38), np.float32(3e38)           # the product overflows binary32
        _, created, rowbytes = tbase._rows(n, 64)
        ids = np.arange(n, dtype=np.int64) + 100
        idx = tbase._build(emb, created, rowbytes, ids, n)
        assert idx.update_rows(ids[10:11], None) == 1                                   # a row without an embedding
        emb[10] = 0.0
        s = dict(idx=idx, model=nbase.Model(emb, created, rowbytes, ids), n=n)
        got = _check_pairs(s, [list(range(56)), list(range(8, 64)), [10, 1, 2, 10]])
        assert np.isnan(got[0, 6, 6]) and got[0, 4, 4] == INF and got[2, 0, 0] == 0.0 and got[0, 1, 2] == 0.0
        idx.close()


def test_pair_dots_argument_errors_come_from_the_host_before_any_launch():
    P = pkg()
    s = _shard("D2")
    idx, n = s["idx"], s["n"]

    def refused(lists, what):
        idx.set_profiling(True)
        try:
            with pytest.raises(P.native.OrrError) as e:
                idx.pair_dots(lists)
            assert what in str(e.value), str(e.value)
            assert "pair_dots" not in idx.kernel_stats()
        finally:
            idx.set_profiling(False)

    refused([[0, n]], "is outside 0 ..")
    refused([[1, 2], [-1]], "is outside 0 ..")
    refused([list(range(57))], "stride must be in 1 .. 56")
    h = P.native.hip
    off = np.array([0, 5], np.uint32)
    pos = np.arange(5, dtype=np.int64)
    out = np.full((1, 4, 4), 7.0)
    idx.set_profiling(True)
    try:
        assert h.orr_index_pair_dots(idx._h, 1, off.ctypes.data, pos.ctypes.data, 4, out.ctypes.data) == P.native.ORR_EINVAL
        assert b"holds 5 positions, stride is 4" in h.orr_last_error()
        assert "pair_dots" not in idx.kernel_stats() and (out == 7.0).all()
    finally:
        idx.set_profiling(False)


# ---- end to end --------------------------------------------------------------------------------------------------------------

def _all_cases(s, B, limit, what):
    idx = s["idx"]
    qis, q, texts = _batch(s, B)
    n_diff = 0
    for topk in (1, 4, 10):
        plain = idx.search(q, _terms(texts), _syn().NOW_TICKS, topk, candidate_limit=limit)
        for pool in sorted({max(1, topk), 24, 56}):
            for mode, params in (("collapse", MAX_COSINES), ("mmr", LAMBDAS)):
                for param in params:
                    got, st = _stats(idx, lambda: _diverse(idx, q, texts, topk, pool, mode, param, limit))
                    _check(got, s, qis, topk, pool, mode, param, limit, what=(what, topk, pool, mode, param))
                    reads = pool >= 2 and not (mode == "collapse" and param == INF) and not (mode == "mmr" and param == 1.0)
                    assert _launches(st) == (1 if reads else 0), (what, topk, pool, mode, param, st.get("pair_dots"))
                    if not reads:                       # the plain search bit for bit
                        assert np.array_equal(got[0], plain[0]) and _same_bits(got[1], plain[1]), (what, topk, pool, mode, param)
                        assert np.array_equal(got[2], plain[2])
                        c = got[2]
                        assert all(list(got[3][b, :c[b]]) == list(range(c[b])) for b in range(B))
                    elif topk > 1 and pool > topk and param in (0.95, 0.5, 0.3):
                        n_diff += int((got[0][:5] != plain[0][:5]).any())        # the planted queries
    if limit >= s["n"]:                                  # the planted families take part
        assert n_diff > 0, what                          # the feature did something


@pytest.mark.parametrize("name,B,limit", [("D1", 5, 300), ("D1", 64, 4_099), ("D2", 1, 300), ("D2", 130, 4_099), ("D2", 256, 300),
                                          ("D3", 5, 20_000), ("D3", 64, 300)])
def test_rows_score_bits_counts_and_pool_ranks(name, B, limit):
    _all_cases(_shard(name), B, limit, (name, B, limit))


def test_the_planted_queries_lose_their_near_duplicates():
    s = _shard("D2")
    idx, n = s["idx"], s["n"]
    qis, q, texts = _batch(s, 5)
    plain = idx.search(q, _terms(texts), _syn().NOW_TICKS, 4, candidate_limit=n)
    got = _diverse(idx, q, texts, 4, 56, "collapse", 0.95, n)
    _check(got, s, qis, 4, 56, "collapse", 0.95, n)
    for b in range(4):                                  # 12 members of one family: the plain top-4 are near-copies, the collapse keeps one
        fam = set(s["model"].ids[s["fam"][s["anchors"][b]]].tolist())
        assert set(plain[0][b].tolist()) <= fam and not np.array_equal(got[0][b], plain[0][b])
        assert got[0][b, 0] == plain[0][b, 0] and got[2][b] == 4
        c = _pair_cos(s["model"].emb[s["model"].rows_of_ids(got[0][b])])
        assert all(c[i][j] < 0.95 for i in range(4) for j in range(4) if i != j), c
        cp = _pair_cos(s["model"].emb[s["model"].rows_of_ids(plain[0][b])])
        assert any(cp[i][j] >= 0.95 for i in range(4) for j in range(4) if i != j), cp
    # the family of 61: larger than the pool, every member within 0.9999 of every other -- the collapse runs out of pool
    got = _diverse(idx, q[4:5], texts[4:5], 10, 56, "collapse", 0.99, n)
    _check(got, s, [4], 10, 56, "collapse", 0.99, n)
    assert got[2][0] == 1 and got[3][0, 0] == 0
    mm = _diverse(idx, q, texts, 4, 24, "mmr", 0.3, n)
    _check(mm, s, qis, 4, 24, "mmr", 0.3, n)
    assert (mm[2] == 4).all() and any(not np.array_equal(mm[0][b], plain[0][b]) for b in range(4))


def test_the_border():
    """max_cosine at a planted pair's own cosine and one ulp to either side: dropped, dropped, kept"""
    s = _shard("D3")
    idx, n = s["idx"], s["n"]
    pos, sc, cos = _pool(s, 0, n)
    c01 = cos[1][0]
    assert 0.8 < c01 < 1.001 and orc.cosine(s["model"].emb[pos[1]], s["model"].emb[pos[0]]) == c01
    for t, dropped in ((np.nextafter(c01, -INF), True), (c01, True), (np.nextafter(c01, INF), False)):
        got = _diverse(idx, s["q"][:1], s["texts"][:1], 2, 2, "collapse", float(t), n)
        _check(got, s, [0], 2, 2, "collapse", float(t), n, what=("border", t))
        assert got[2][0] == (1 if dropped else 2), (t, c01, got)


def test_a_foreign_query_dimension_and_an_empty_batch():
    s = _shard("D2")
    idx, n = s["idx"], s["n"]
    rng = np.random.default_rng(3)
    qf = rng.standard_normal((3, 64)).astype(np.float32)                   # every query cosine is 0: keyword and recency only
    texts = [s["texts"][20], s["texts"][21], ""]
    for mode, param in (("collapse", 0.5), ("mmr", 0.3)):
        got = _diverse(idx, qf, texts, 4, 24, mode, param, 300)
        for b in range(3):
            _check(tuple(x[b:b + 1] for x in got), s, [b], 4, 24, mode, param, 300, qvec=qf[b], text=texts[b], tag=("foreign", b))
    P = pkg()
    h = P.native.hip
    qoff = np.zeros(1, np.uint32)
    out = np.full(4, 7, np.int64)
    assert h.orr_search_batch_diverse(idx._h, 0, 128, None, None, None, qoff.ctypes.data, 0, 4, 300, None, 24, 0, 0.5, out.ctypes.data, out.ctypes.data,
                                      out.ctypes.data, None) == 0
    assert (out == 7).all()


def test_within_scopes():
    P = pkg()
    s = _shard("D2")
    idx, n, model = s["idx"], s["n"], s["model"]
    qis, q, texts = _batch(s, 12)
    fam_ids = model.ids[sorted(set(sum(s["fam"].values(), [])))]
    rng = np.random.default_rng(8)
    id_list = np.unique(np.concatenate([fam_ids, model.ids[rng.choice(n, 700, replace=False)]]))
    lo, hi = int(np.sort(model.created)[n // 4]), int(np.sort(model.created)[3 * n // 4])
    tick_ids = model.ids[(model.created >= lo) & (model.created < hi)]         # half-open
    word = _syn().vocab_word(17)
    term_ids = model.term_ids([word], "all")
    scopes = (("ids", lambda: idx.scope(id_list), id_list), ("ticks", lambda: idx.scope_ticks(lo, hi), tick_ids),
              ("terms", lambda: idx.scope_terms([word], "all"), term_ids), ("empty", lambda: idx.scope(np.zeros(0, np.int64)), np.zeros(0, np.int64)))
    for what, make, ids in scopes:
        sc = make()
        try:
            assert sc.rows == len(ids), what
            for mode, param, topk, pool in (("collapse", 0.95, 4, 24), ("mmr", 0.3, 10, 56), ("collapse", INF, 4, 4)):
                got = _diverse(idx, q, texts, topk, pool, mode, param, n, within=sc)
                _check(got, s, qis, topk, pool, mode, param, n, scope_ids=ids, what=(what, mode))
                if what == "empty":
                    assert (got[2] == 0).all()
                if param == INF:
                    inside = idx.search_in_scope(q, _terms(texts), _syn().NOW_TICKS, topk, sc, candidate_limit=n)
                    assert np.array_equal(got[0], inside[0]) and _same_bits(got[1], inside[1]) and np.array_equal(got[2], inside[2])
        finally:
            sc.close()


def test_after_maintenance_the_updated_vector_is_the_one_compared():
    s = _build_shard("D2", capacity=SHAPES["D2"][0] + 64)
    idx, model, n = s["idx"], s["model"], s["n"]
    qis, q, texts = _batch(s, 10)

    def check(what):
        s["cache"].clear()                              # the model moved
        for mode, param in (("collapse", 0.95), ("mmr", 0.3)):
            got = _diverse(idx, q, texts, 4, 24, mode, param, len(model.ids))
            _check(got, s, qis, 4, 24, mode, param, len(model.ids), what=(what, mode))
        return got

    check("fresh")
    far = model.ids[[n - 5]]                             # an old row far from every query: in no pool
    in_pool_1 = lambda: int(np.nonzero(model.ids == far[0])[0][0]) in _pool(s, 1, len(model.ids))[0][:24].tolist()
    assert not in_pool_1()
    a = s["anchors"][0]
    fam = s["fam"][a]
    # delete the best-ranked near-copies of family 0
    gone = model.ids[fam[1:3]]
    assert idx.delete_rows(gone) == 2
    model.delete(gone)
    check("deleted")
    # update: a far row becomes an exact copy of anchor 1, and anchor 0's duplicate becomes noise
    new = model.emb[s["anchors"][1]][None, :].copy()
    assert idx.update_rows(far, new) == 1
    model.update(far, new)
    dup = model.ids[[fam[-1]]]
    noise = np.random.default_rng(1).standard_normal((1, s["dim"])).astype(np.float32)
    assert idx.update_rows(dup, noise) == 1
    model.update(dup, noise)
    check("updated")
    assert in_pool_1()                                   # the copy stands in query 1's pool now: the checks above compared its NEW vector
    assert int(far[0]) in _diverse(idx, q, texts, 24, 24, "collapse", INF, len(model.ids))[0][1]
    idx.compact()
    model.compact()
    check("compacted")
    m = 32
    _, c2, b2 = tbase._rows(m, 64, row0=n, n_total=n + m)
    e2 = np.random.default_rng(4).standard_normal((m, s["dim"]), dtype=np.float32)
    e2[0] = model.emb[0]                                                     # an exact copy of a row that is there
    e2[1] = _noisy(np.random.default_rng(2), s["q"][2], 0.02)                # lands in query 2's pool
    ids2 = np.arange(m, dtype=np.int64) + 10_000_000
    idx.insert_rows(e2, c2, b2.reshape(-1), np.arange(m + 1, dtype=np.int64) * b2.shape[1], row_ids=ids2)
    model.insert(e2, c2, b2, ids2)
    check("inserted")


def test_on_a_view_from_four_threads_and_with_device_resident_queries():
    import torch
    s = _shard("D2")
    idx, n = s["idx"], s["n"]
    qis, q, texts = _batch(s, 16)
    view = idx.view()
    try:
        got = _diverse(view, q, texts, 4, 24, "mmr", 0.7, n)
        _check(got, s, qis, 4, 24, "mmr", 0.7, n, what="view")
    finally:
        view.close()
    qd = torch.from_numpy(q).to("cuda:0")
    got = idx.search_diverse(qd, _terms(texts), _syn().NOW_TICKS, 4, 24, mode="collapse", param=0.5, candidate_limit=n)
    _check(got, s, qis, 4, 24, "collapse", 0.5, n, what="device queries")
    results, errors = [None] * 4, []

    def work(i):
        try:
            mode, param = (("collapse", 0.95), ("mmr", 0.3), ("collapse", 0.5), ("mmr", 0.7))[i]
            for _ in range(3):
                results[i] = (_diverse(idx, q, texts, 10, 56, mode, param, n), mode, param)
        except Exception as e:                          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for got, mode, param in results:
        _check(got, s, qis, 10, 56, mode, param, n, what=("threads", mode, param))


def test_the_pool_of_a_two_stage_pass():
    s = _shard("D4")
    idx, n = s["idx"], s["n"]
    idx.set_option("two_stage", 1)
    qis = [b % NQ if b % NQ != 8 else 9 for b in range(130)]     # (without the NaN query: it can only be answered by the exact pass, which would run last)
    q, texts = s["q"][qis], [s["texts"][i] for i in qis]
    idx.search_stats(reset=True)
    got, st = _stats(idx, lambda: _diverse(idx, q, texts, 10, 56, "collapse", 0.95, n))
    stats = idx.search_stats()
    assert stats["pass_mode"] == 1 and stats["searches"] == 1 and stats["queries"] == 130, stats
    assert _launches(st) == 1
    _check(got, s, qis, 10, 56, "collapse", 0.95, n, what="two-stage")
    got = _diverse(idx, q, texts, 10, 24, "mmr", 0.3, n)
    _check(got, s, qis, 10, 24, "mmr", 0.3, n, what="two-stage mmr")
