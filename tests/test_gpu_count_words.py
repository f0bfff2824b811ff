"""The screening epilogue's keyword count words (orr_gemm.hip query_count_planes_kernel -> orr_epilogue.h
fused_epilogue16): a row survives the screen only if its upper bound, which credits count x qz per query, reaches
the floor, so a count read too low drops a row of the top-k without any certificate noticing.

The corpora make the keyword score decide the ranking: random 512-d embeddings (cosine near 0), recency spread over
minutes, rows that hold chosen subsets of the queries' terms.  Every batch is checked three ways: all queries against
the same batch with option "two_stage" 0 (no screen), a sample of queries against the oracle bit for bit, and through
kernel_stats() that the screening GEMM ran with the intended count-word form:
    count_planes algo_bytes = (8 two-bit | 16 four-bit) x ceil(B / 32) x rows
Two-bit words are used when every query of the batch has at most three terms; ORR_COUNT_BITS4=1 forces four bits.
"""
import numpy as np
import pytest

from helpers import NOW, orc, pkg

pytestmark = pytest.mark.gpu

DIM = 512                      # a multiple of 128 with D / 64 > kS4NB: the 16 x 16 x 64 screening form
N_ROWS = 262_144               # 64 segments of 4096 rows (>= 48: the two-stage pass)
FILLER = 99_999                # a token in every row that no query asks for
TOPK = 10
PATTERNS = 8                   # (a): lane group m uses term pattern m % 8
ODD = (1, 3, 5, 7, 11, 13, 101, 77)
POPULAR = (96, 97, 98)         # (b)
LONG_BASE, LONG_LENS = 100, (4, 15, 16, 40, 150)      # (d)
LONG_MATCHES = (0, 1, 14, 15, 16, 20, 24, 150)        # terms s_1 .. s_k of the query in a row (capped at its length)
LONG_CAP = {40: 20}            # the 40-term query's best row holds only 20 of its terms


def _tok(t):
    return "w%05d" % t


def _contents(n, pair_rows, pair_terms):
    """Row r's content: its terms, in increasing id order, plus FILLER; 7 bytes per token."""
    rows = np.concatenate(pair_rows + [np.arange(n, dtype=np.int64)])
    terms = np.concatenate(pair_terms + [np.full(n, FILLER, dtype=np.int64)])
    order = np.lexsort((terms, rows))
    rows, terms = rows[order], terms[order]
    table = np.frombuffer("".join(_tok(t) + " " for t in range(FILLER + 1)).encode(), dtype=np.uint8).reshape(-1, 7)
    pool = table[terms].reshape(-1)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(rows, minlength=n).astype(np.int64) * 7)
    return np.concatenate([pool, np.zeros(1, np.uint8)]), off


def _created(n):
    return (NOW - 864_000_000 - np.arange(n, dtype=np.int64) * 1000).astype(np.int64)     # newest first, 1 ms apart


def _pattern_terms(p, e):
    return [12 * p + 3 * e + j for j in range(3)]


def _digit(r, p, e):
    return ((r * ODD[p]) % 256 >> (2 * e)) & 3


def _mixed_len(m, e):
    """Terms of query 4 m + e in the (a) batches: 3 in the first eight groups, then a mix of 0..3 in every odd group."""
    return 3 if m < PATTERNS or m % 2 == 0 else (3, 2, 1, 0)[(m + e) % 4]


def _long_terms(j):
    return [LONG_BASE + sum(LONG_LENS[:j]) + i for i in range(LONG_LENS[j])]


class _Corpus:
    def __init__(self, n, emb, created, contents):
        P = pkg()
        self.n = n
        self.idx = P.RecallIndex(dim=emb.shape[1])
        step = 1 << 20
        pool, off = contents
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            self.idx.append(emb[r0:r1], created[r0:r1], pool[off[r0]:off[r1] + 1], (off[r0:r1 + 1] - off[r0]).astype(np.uint64))
        self.idx.seal()
        self.oracle = orc.OracleCorpus(emb, created, contents)

    def close(self):
        self.idx.close()


def _make_corpus():
    rng = np.random.default_rng(512)
    n = N_ROWS
    emb = rng.standard_normal((n, DIM), dtype=np.float32)
    r = np.arange(n, dtype=np.int64)
    pr, pt = [], []
    for p in range(PATTERNS):                              # (a) row r: the first d_e terms of query e of pattern p
        for e in range(4):
            d = _digit(r, p, e)
            for j in range(3):
                sel = r[d > j]
                pr.append(sel)
                pt.append(np.full(sel.shape, _pattern_terms(p, e)[j], dtype=np.int64))
    two = r[(r % 5 == 0) & (r % 13 != 0)]                  # (b) 2 of the popular query's 3 terms, or all 3
    for j in range(3):
        sel = two[(two // 5) % 3 != j]
        pr.append(sel)
        pt.append(np.full(sel.shape, POPULAR[j], dtype=np.int64))
    for j in range(3):
        pr.append(r[r % 13 == 0])
        pt.append(np.full(pr[-1].shape, POPULAR[j], dtype=np.int64))
    for j, L in enumerate(LONG_LENS):                      # (d) s_1 .. s_k of long query j
        sel = r[r % 53 == 7 + j]
        k = np.minimum(np.asarray(LONG_MATCHES)[(sel // 53) % len(LONG_MATCHES)], LONG_CAP.get(L, L))
        terms = np.asarray(_long_terms(j), dtype=np.int64)
        for i in range(int(k.max())):
            pr.append(sel[k > i])
            pt.append(np.full(pr[-1].shape, terms[i], dtype=np.int64))
    c = _Corpus(n, emb, _created(n), _contents(n, pr, pt))
    c.rng = rng
    return c


@pytest.fixture(scope="module")
def corpus():
    c = _make_corpus()
    yield c
    c.close()


def _texts_a(B):
    texts = []
    for b in range(B):
        m, e = divmod(b, 4)
        texts.append(" ".join(_tok(t) for t in _pattern_terms(m % PATTERNS, e)[:_mixed_len(m, e)]))
    return texts


def _search_checked(c, qs, texts, bits, n_ranges, oracle_sample, monkeypatch=None):
    """The screened search of the batch, checked against the unscreened one (every query) and the oracle (the sample);
    asserts that the 16 x 16 x 64 screen ran with `bits`-bit count words in `n_ranges` row ranges."""
    P = pkg()
    idx, n, B = c.idx, c.n, len(texts)
    terms = [P.text.query_terms(t) for t in texts]
    idx.set_option("two_stage", 0)
    plain = idx.search(qs, terms, NOW, TOPK, candidate_limit=n)
    idx.set_option("two_stage", 1)
    if monkeypatch is not None:
        monkeypatch.setenv("ORR_COUNT_BITS4", "1")
    # a first screened search sizes the survivors' buffers and the sampled prefix from what it measures (a query that
    # overflows is repeated alone); it must already be right, and the next one runs as a single pass
    warm = idx.search(qs, terms, NOW, TOPK, candidate_limit=n)
    idx.set_profiling(True)
    idx.reset_search_stats()
    try:
        got = idx.search(qs, terms, NOW, TOPK, candidate_limit=n)
        st = idx.kernel_stats()
        ss = idx.search_stats()
    finally:
        idx.set_profiling(False)
        if monkeypatch is not None:
            monkeypatch.delenv("ORR_COUNT_BITS4")
    # one pass of the whole batch (a repeat for some of its queries would add its own count words and screening launches)
    assert "screen_i8_fused" in st and st["screen_i8_fused"]["launches"] == n_ranges, (st, ss)
    assert "count_planes" in st and st["count_planes"]["launches"] == n_ranges, (st, ss)
    per_row = (8 if bits == 2 else 16) * ((B + 31) // 32)
    assert st["count_planes"]["algo_bytes"] == per_row * n, (bits, st["count_planes"], ss)
    assert all(np.array_equal(x, y) for x, y in zip(warm, got))
    rows, scores, counts = got
    for b in range(B):
        assert counts[b] == plain[2][b] and list(rows[b, :counts[b]]) == list(plain[0][b, :counts[b]]), (b, texts[b])
        assert np.array_equal(scores[b, :counts[b]], plain[1][b, :counts[b]]), (b, texts[b])
    for b in sorted(set(oracle_sample)):
        orow, osc, _ = c.oracle.search(qs[b], texts[b], NOW, TOPK, candidate_limit=n, threads=8)
        assert list(rows[b, :counts[b]]) == list(orow), (b, texts[b], rows[b], orow)
        assert np.array_equal(scores[b, :counts[b]], osc), (b, texts[b])
    return got


def _lanes_sample(B, extra=()):
    return [0, 1, 2, 3, 4 * PATTERNS + 4, 4 * PATTERNS + 5, 4 * PATTERNS + 6, 4 * PATTERNS + 7, B - 1] + list(extra)


def _batch_b(c):
    """(b): the popular 3-term query in the four slots of lane group 3 and at slots 5..8 (across groups 1 and 2)."""
    B = 256
    qs = c.rng.standard_normal((B, DIM), dtype=np.float32)
    texts = _texts_a(B)
    pop = " ".join(_tok(t) for t in POPULAR)
    for b in (12, 13, 14, 15, 5, 6, 7, 8):
        texts[b] = pop
    qs[13:16] = qs[12]                                     # the same query four times over
    return qs, texts, [5, 6, 7, 8, 12, 13, 14, 15]


@pytest.mark.parametrize("B", [129, 256])
def test_two_bit_words_every_byte_value(corpus, B):
    """(a) Query e of every lane group holds 3 terms (0..3 in part of the batch); row r holds the first d_e of them, d_e
    the base-4 digits of (r x odd) mod 256: every byte value of a two-bit count word, in the prefix and past it."""
    qs = corpus.rng.standard_normal((B, DIM), dtype=np.float32)
    texts = _texts_a(B)
    rows, _, counts = _search_checked(corpus, qs, texts, 2, 1, _lanes_sample(B))
    # the keyword score decides: a full-pattern query's best row holds all three of its terms
    for b in range(min(B, 4 * PATTERNS)):
        m, e = divmod(b, 4)
        assert counts[b] == TOPK and _digit(int(rows[b, 0]), m % PATTERNS, e) == 3, b


def test_two_bit_words_repeated_popular_query(corpus):
    """(b) Neighbouring lanes of a group that match the same rows: every field of the byte nonzero."""
    qs, texts, planted = _batch_b(corpus)
    rows, _, counts = _search_checked(corpus, qs, texts, 2, 1, _lanes_sample(len(texts), planted))
    for b in planted:
        assert counts[b] == TOPK and all(int(r) % 13 == 0 for r in rows[b, :TOPK]), (b, rows[b])


@pytest.mark.parametrize("batch", ["a129", "a256", "b"])
def test_four_bit_knob_gives_the_same_results(corpus, batch, monkeypatch):
    """(c) ORR_COUNT_BITS4=1 forces nibble count words on the batches of (a) and (b): results identical to the
    two-bit run and to the oracle."""
    if batch == "b":
        qs, texts, planted = _batch_b(corpus)
    else:
        B = int(batch[1:])
        qs, texts, planted = corpus.rng.standard_normal((B, DIM), dtype=np.float32), _texts_a(B), []
    sample = _lanes_sample(len(texts), planted)
    two = _search_checked(corpus, qs, texts, 2, 1, sample)
    four = _search_checked(corpus, qs, texts, 4, 1, sample, monkeypatch=monkeypatch)
    assert all(np.array_equal(x, y) for x, y in zip(two, four))


def test_four_bit_words_and_saturation(corpus):
    """(d) Queries of 4, 15, 16, 40 and 150 terms over rows holding s_1 .. s_k of them, k in 0, 1, 14, 15, 16, 20+:
    past 15 terms the nibble saturates at 15 (credit 15 x 0.2/15 = 0.2, an upper bound); the 40-term query's best row
    holds 20 of its terms."""
    B = 160
    qs = corpus.rng.standard_normal((B, DIM), dtype=np.float32)
    texts = _texts_a(B)
    slots = (0, 5, 10, 15, B - 1)                          # lanes e = 0, 1, 2, 3 and the last query
    for j, b in enumerate(slots):
        texts[b] = " ".join(_tok(t) for t in _long_terms(j))
    rows, _, counts = _search_checked(corpus, qs, texts, 4, 1, _lanes_sample(B, slots))
    for j, b in enumerate(slots):                          # the rows that hold the query's terms come first
        assert counts[b] == TOPK and int(rows[b, 0]) % 53 == 7 + j, (b, rows[b])


def _boundaries(n, n_ranges):
    """range_row of orr_api.hip: whole rounds of 256 workgroups x 256-row tiles."""
    k = 256 * 256
    return [(n * r // n_ranges + k // 2) // k * k for r in range(1, n_ranges)]


def test_range_split_at_two_million_rows():
    """(e) From 2,000,000 rows the first range's count words are formed in front of the GEMM and the later ranges' on the
    keyword stream while it runs: 4 ranges for B <= 256 (two-bit words here), 8 above (four-bit words).  Winners decided
    by the keyword score alone sit at row 0, at every range boundary +-1, in the last partial round and at n - 1."""
    P = pkg()
    n = 2_100_000                                          # a multiple of neither 65,536 nor 32
    rng = np.random.default_rng(2100)
    emb = rng.standard_normal((n, DIM), dtype=np.float32)
    k = 256 * 256
    plans = {}
    for B, n_ranges in ((256, 4), (300, 8)):
        planted = [0] + [x + d for x in _boundaries(n, n_ranges) for d in (-1, 0, 1)] + [n // k * k, n // k * k + 1001, n - 1]
        plans[B] = (n_ranges, planted)
    # every row: 3 of 64 filler terms; planted row i of batch B: its query's own terms as well
    r = np.arange(n, dtype=np.int64)
    pr, pt = [], []
    fill = rng.integers(0, 64, (n, 3))
    for j in range(3):
        pr.append(r)
        pt.append(1000 + fill[:, j])
    q_terms = {}
    next_term = 2000
    for B, (n_ranges, planted) in plans.items():
        for i, row in enumerate(planted):
            nt = 3 if B == 256 else (1, 2, 3, 4, 5, 7)[i % 6]
            q_terms[(B, i)] = list(range(next_term, next_term + nt))
            next_term += nt
            for t in q_terms[(B, i)]:
                pr.append(np.array([row], dtype=np.int64))
                pt.append(np.array([t], dtype=np.int64))
    for B, (n_ranges, planted) in plans.items():          # the winner's own query has cosine ~0 on it
        qs = rng.standard_normal((B, DIM), dtype=np.float32)
        plans[B] = plans[B] + (qs,)
    for B, (n_ranges, planted, qs) in plans.items():
        stride = 19 if B == 256 else 23
        for i, row in enumerate(planted):
            q = qs[(i * stride) % B].astype(np.float64)
            e = emb[row].astype(np.float64)
            emb[row] = (e - (e @ q) / (q @ q) * q).astype(np.float32)
    c = _Corpus(n, emb, _created(n), _contents(n, pr, pt))
    try:
        for B, (n_ranges, planted, qs) in plans.items():
            stride = 19 if B == 256 else 23
            texts = []
            for b in range(B):
                nt = 1 + (b % 3) if B == 256 else 1 + (b % 5)
                texts.append(" ".join(_tok(1000 + (7 * b + 5 * j) % 64) for j in range(nt)))
            slot_of = {}
            for i in range(len(planted)):
                b = (i * stride) % B
                texts[b] = " ".join(_tok(t) for t in q_terms[(B, i)])
                slot_of[i] = b
            assert len(set(slot_of.values())) == len(planted)
            sample = [0, 1, 2, 3, B - 1] + [slot_of[i] for i in range(0, len(planted), max(1, len(planted) // 11))]
            rows, _, counts = _search_checked(c, qs, texts, 2 if B == 256 else 4, n_ranges, sample[:17])
            for i, row in enumerate(planted):
                assert counts[slot_of[i]] == TOPK and rows[slot_of[i], 0] == row, (B, i, row, rows[slot_of[i]])
    finally:
        c.close()
