"""The keyword chain seen directly (orr_index_keyword_bitmaps): the per-term row bitmaps, the (term, token) hit count, the alias
flags and the short-token form that ran, in every match form -- all-pairs and lookup for tokens of at most 16 bytes, the
lane-per-token kernel and the wave scan for tokens of 17..32 bytes, the wave scan in 1 KiB steps for longer ones, both alias
stages and the posting expansion.  Every check is exact.

Three references per corpus, restated here without library code:
  bitmaps     for every term the rows whose BYTES contain it (bytes.find over the rows laid end to end on corpus E; array
              compares byte for byte on the two large corpora, held against bytes.find in test_the_two_restatements_agree):
              independent of the tokeniser;
  hit count   sum over the terms of the DISTINCT tokens that contain the term, the tokens from a Python split on the library's
              whitespace set (csrc/orr_token_index.cpp: U+0009-000D, 0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F,
              3000): exactly one hit per (token, term) pair;
  alias flag  exactly one token contains the term, and that token has postings x 64 >= rows on a shard of at least 196,608 rows.

Corpus E (edges, 4,101 rows), corpus T (140,080 short tokens: the threshold of the default form selection) and corpus A (196,700
rows: stored token bitmaps) are each built once per module, with dim 0 and no embeddings.  After every run on corpus E an ordinary
search on the same index must equal the oracle: the diagnostic leaves the lane as a search leaves it.

profiles/keyword_chain_checks.txt records which of these tests fail for five faults put into the kernels one at a time."""
import bisect
import re

import numpy as np
import pytest

from helpers import NOW, orc, pkg

pytestmark = pytest.mark.gpu

WS = re.compile(b"(?:[\\x09-\\x0d\\x20]|\\xc2[\\x85\\xa0]|\\xe1\\x9a\\x80|\\xe2\\x80[\\x80-\\x8a\\xa8\\xa9\\xaf]|\\xe2\\x81\\x9f|\\xe3\\x80\\x80)+")


def _words(n_rows):
    return ((n_rows + 31) // 32 + 3) // 4 * 4


def _pack(mask, words):
    """bool [n_rows] -> uint32 [words]: bit r & 31 of word r >> 5"""
    out = np.zeros(words * 4, np.uint8)
    packed = np.packbits(mask, bitorder="little")
    out[: len(packed)] = packed
    return out.view("<u4")


class Blob:
    """items (rows, or distinct tokens) laid end to end with one space between them: no term holds whitespace, so a term found
    at a position lies inside the one item that covers the position"""

    def __init__(self, items):
        self.n = len(items)
        self.blob = b" ".join(items)
        self.starts = [0] * (self.n + 1)
        for i, it in enumerate(items):
            self.starts[i + 1] = self.starts[i] + len(it) + 1

    def holders(self, term):
        """the indices of the items that contain the term, ascending"""
        out, pos = [], self.blob.find(term)
        while pos >= 0:
            i = bisect.bisect_right(self.starts, pos) - 1
            out.append(i)
            pos = self.blob.find(term, self.starts[i + 1])      # on with the next item
        return out


def _tokens_of(rows):
    """the distinct tokens of the rows in order of first appearance (rows in candidate order: the library's vocabulary order) and
    per token the number of rows that hold it"""
    seen = {}
    for row in rows:
        for tok in set(t for t in WS.split(row) if t):
            seen[tok] = seen.get(tok, 0) + 1
    order, known = [], set()
    for row in rows:
        for tok in WS.split(row):
            if tok and tok not in known:
                known.add(tok)
                order.append(tok)
    return order, seen


class Reference:
    """the three references of one corpus; rows: list of bytes in candidate order.  has(term) -> bool [n_rows] is given by the
    corpus (bytes.find, or array compares)."""

    def __init__(self, rows, has=None):
        self.rows, self.n = rows, len(rows)
        self.words = _words(self.n)
        self.vocab, self.postings = _tokens_of(rows)
        self.tok_blob = Blob(self.vocab)
        self.row_blob = Blob(rows) if has is None else None
        self._has = has or self._has_by_find
        self._bm, self._holders = {}, {}

    def _has_by_find(self, term):
        m = np.zeros(self.n, bool)
        m[self.row_blob.holders(term)] = True
        return m

    def bitmap(self, term):
        if term not in self._bm:
            self._bm[term] = _pack(self._has(term), self.words)
        return self._bm[term]

    def holders(self, term):
        """vocabulary numbers of the distinct tokens that contain the term"""
        if term not in self._holders:
            self._holders[term] = self.tok_blob.holders(term)
        return self._holders[term]

    def bitmaps(self, terms):
        return np.stack([self.bitmap(t) for t in terms])

    def hits(self, terms):
        return sum(len(self.holders(t)) for t in terms)

    def alias(self, terms):
        out = np.zeros(len(terms), np.uint8)
        if self.n < 196_608:
            return out
        for i, t in enumerate(terms):
            h = self.holders(t)
            out[i] = 1 if len(h) == 1 and self.postings[self.vocab[h[0]]] * 64 >= self.n else 0
        return out


def _build(rows, one_lane=True):
    """dim 0, no embeddings; created ticks strictly descending, so candidate order is the order given"""
    P = pkg()
    n = len(rows)
    created = (NOW - np.arange(n, dtype=np.int64) * 1000).astype(np.int64)
    idx = P.RecallIndex(dim=0)
    for r0 in range(0, n, 50_000):
        idx.append(None, created[r0:r0 + 50_000], rows[r0:r0 + 50_000])
    idx.seal()
    if one_lane:
        idx.set_option("max_lanes", 1)                  # every call uses the index's own workspaces: the search behind a run meets what the run left
    return idx, created


def _exact(got, ref, terms, what):
    """bitmaps, hit count and alias flags against the references: every difference is named, not only the first kind"""
    want = ref.bitmaps(terms)
    assert got["words"] == ref.words and got["bitmaps"].shape == want.shape, (what, got["words"], ref.words)
    wrong = []
    if not np.array_equal(got["bitmaps"], want):
        bad = np.nonzero((got["bitmaps"] != want).any(axis=1))[0]
        t = int(bad[0])
        w = np.nonzero(got["bitmaps"][t] != want[t])[0]
        wrong.append(("bitmaps differ for %d of %d terms" % (len(bad), len(terms)), "first", terms[t][:48], "words", w[:6].tolist(),
                      [hex(int(x)) for x in got["bitmaps"][t][w[:3]]], [hex(int(x)) for x in want[t][w[:3]]]))
    if got["hits"] != ref.hits(terms):
        wrong.append(("hits", got["hits"], ref.hits(terms)))
    want_alias = ref.alias(terms)
    if not np.array_equal(got["alias"], want_alias):
        bad = np.nonzero(got["alias"] != want_alias)[0]
        wrong.append(("alias flags differ for", [terms[int(t)][:24] for t in bad[:8]], "got", got["alias"][bad[:8]].tolist()))
    assert not wrong, (what, wrong)


# ---- corpus E: edges ---------------------------------------------------------------------------------------------------------

NE = 4101
ALPHA = "abcdefgh"
PLANT_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, NE)
LONG_LENS = (1000, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 2100)
_E = {}


def _plant_rows(k):
    last = NE - 1
    rows = {
        1: [last],                                                          # the last row, alone
        63: range(0, 63),                                                   # row 0, a whole word and a word but its bit 31
        64: range(32, 96),                                                  # two whole words
        65: [31, 63, 64] + list(range(200, 200 + 62 * 61, 61)),            # bit 31 of two words, bit 0 of the next, isolated rows
        255: range(0, 255 * 16, 16),                                        # isolated, one per half word, from row 0
        256: range(1024, 1280),                                             # eight whole words
        257: list(range(2048, 2304)) + [last],
        1023: range(0, 1023),                                               # one posting chunk but one
        1024: range(2976, 4000),                                            # exactly one chunk, whole words
        1025: [0] + list(range(1, 4097, 4)),                                # one posting into the second chunk; isolated bits
        2048: range(0, 4096, 2),                                            # two chunks, every other bit
        2049: range(NE - 2049, NE),                                         # a run up to the last row, one posting into the third chunk
        NE: range(NE),                                                      # every row: five chunks, the partial last word
    }[k]
    rows = sorted(rows)
    assert len(rows) == k == len(set(rows)) and rows[0] >= 0 and rows[-1] < NE, k
    return rows


def _plant_name(i, k):
    """short, 17..32 bytes and longer in turn: every kernel of the vocabulary match finds planted postings"""
    return ("p%04d" % k, "plant-%06d-mid-token" % k, "planted-%06d-in-a-token-of-40-bytes-..." % k)[i % 3].encode()


def _long_token(i, ln):
    fill = ("xyzw", "yzwx", "zwxy", "wxyz", "xzyw", "zywx", "ywxz", "wzyx", "xwzy")[i]
    b = bytearray((fill * (ln // 4 + 1))[:ln].encode())
    for at, tag in ((1020, b"k%02d!&+=-" % i), (2044, b"m%02d!&+=-" % i)):    # across the first and the second 1 KiB step
        if at < ln:
            b[at:at + 8] = tag[: max(0, min(8, ln - at))]
    b[ln - 3:] = b"^%02d" % i
    assert len(b) == ln and not WS.search(bytes(b))
    return bytes(b)


def _corpus_e():
    if _E:
        return _E
    rng = np.random.default_rng(20251)
    letters = list(ALPHA)
    rnd = []
    for ln in range(1, 41):                                                 # every length from 1 to 40 bytes, 15/16/17 and 31/32/33 among them
        for _ in range(70):
            rnd.append("".join(rng.choice(letters, size=ln)).encode())
    for ln in range(41, 49):                                                # (a few longer ones: a 40-byte term at every start offset)
        for _ in range(6):
            rnd.append("".join(rng.choice(letters, size=ln)).encode())
    for a in ALPHA:                                                          # tokens that share the first dword of a family of terms
        for b in ALPHA[:4]:
            rnd.append(("abcd" + a + b).encode())
            rnd.append(("h" + a + "abcd" + b + "gg").encode())
    special = [b"a" * 16, b"a" * 17, b"ab" * 8, b"ab" * 9, b"ab" * 16, b"ab" * 17, "é".encode() * 3, "naïve".encode(), "中🚀".encode(),
               "ß中é🚀ß中é🚀".encode(), "x🚀".encode() * 4, "abcdefghijklm中".encode(), "abcdefghijklmn中".encode(), "üab".encode() * 11]
    rnd = list(dict.fromkeys(rnd + special))
    longs = [_long_token(i, ln) for i, ln in enumerate(LONG_LENS)]
    planted = {k: _plant_name(i, k) for i, k in enumerate(PLANT_COUNTS)}
    rows = [[] for _ in range(NE)]
    for k, name in planted.items():
        for r in _plant_rows(k):
            rows[r].append(name)
    for r in range(NE):
        rows[r] += [rnd[(3 * r + j) % len(rnd)] for j in range(3)]
    assert 3 * NE >= len(rnd)                                               # every random token is in some row
    for i, tok in enumerate(longs):
        for r in (7 * i + 3, 2000 + 11 * i, NE - 1 - (i % 2)):
            rows[r].append(tok)
    rows = [b" ".join(r) for r in rows]
    ref = Reference(rows)
    V = len(ref.vocab)
    assert V == len(rnd) + len(longs) + len(planted) and V % 256 != 0 and 2000 < V < 6000, V
    assert NE % 32 != 0 and all(ref.postings[planted[k]] == k and len(ref.holders(planted[k])) == 1 for k in PLANT_COUNTS)
    assert {len(t) for t in ref.vocab} >= set(range(1, 41)) | set(LONG_LENS)

    # ---- the terms, deterministic ----
    terms = [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz"]            # 26 one-byte terms
    terms += [(a + b).encode() for a in ALPHA for b in ALPHA]               # 64 two-byte terms
    by_len = {}
    for t in rnd:
        by_len.setdefault(len(t), []).append(t)
    for ln in (1, 2, 3, 4, 5, 8, 12, 13, 16, 17, 31, 32, 33, 40):           # substrings at every start offset mod 4
        for start in range(8):
            pool = [t for t in rnd if len(t) >= start + ln]
            for pick in range(2):
                tok = pool[int(rng.integers(0, len(pool)))]
                terms.append(tok[start:start + ln])
                if start + ln < len(tok) and pick:                          # ... and up to the token's last byte
                    terms.append(tok[len(tok) - ln:])
    whole = [by_len[ln][j] for ln in range(1, 41) for j in (0, 1)] + special + list(planted.values())
    terms += whole
    for tok in [by_len[ln][2] for ln in (8, 16, 17, 24, 32, 33, 40)] + [b"a" * 16, b"ab" * 8, planted[64], planted[65]]:
        for at in (0, 5, len(tok) - 1):                                     # near-misses: the first dword, a later dword, the last byte only
            terms.append(tok[:at] + (b"0" if tok[at:at + 1] != b"0" else b"1") + tok[at + 1:])
    terms += [b"q" * 2200, b"xyzw" * 600, planted[NE] + b"x", b"a" * 18, b"ab" * 17 + b"a", by_len[40][3] + b"a", by_len[16][3] + b"a"]   # longer than every token (that could hold them)
    nest = by_len[13][4]
    terms += [nest[:k] for k in range(1, 14)] + [nest[-k:] for k in range(1, 13)]     # prefixes and suffixes of one another
    terms += [("abcd" + a + b).encode() for a in ALPHA for b in ALPHA[:5]] + [("abcd" + a).encode() for a in ALPHA] + [b"abcd"]   # one first dword: a long run of equal keys
    terms += [b"aa", b"aaa", b"a" * 15, b"a" * 16, b"a" * 17, b"abab", b"ba", b"bab", b"ab" * 7, b"ba" * 7 + b"b", b"ab" * 8, b"ab" * 9, b"ab" * 15,
              b"ab" * 16, b"ba" * 16]                                       # several starts inside one token
    terms += ["é".encode(), "中".encode(), "🚀".encode(), "中🚀".encode(), "中".encode()[:2], "🚀".encode()[1:], "ïv".encode(), "ß中é".encode(), "üabü".encode()]
    for i, (ln, tok) in enumerate(zip(LONG_LENS, longs)):                   # in and across the 1 KiB steps of the wave scan, and the last 3 bytes
        for a, b in ((1020, 1028), (1022, 1026), (1021, 1027), (1016, 1032), (1023, 1025), (1000, 1040), (2044, 2052), (2046, 2050), (2045, 2051),
                     (2040, 2056), (ln - 3, ln), (ln - 7, ln), (0, 40), (1, 6)):
            if 0 <= a and b <= ln:
                terms.append(tok[a:b])
        terms.append(tok[ln - 3:] + b"x")                                   # ... which must not match past the token's end
    terms.append(longs[2])                                                  # a whole token of 1024 bytes
    terms = [t for t in dict.fromkeys(terms) if t and not WS.search(t)]
    assert 400 <= len(terms) <= 1200, len(terms)
    assert sum(len(t) == 1 for t in terms) >= 26 and sum(len(t) == 2 for t in terms) >= 50

    # one workgroup of 256 consecutive vocabulary tokens reports more than 512 hits of short tokens: the lookup's LDS stage overflows
    short = np.array([1 <= len(t) <= 16 for t in ref.vocab])
    per_token = np.zeros(V, np.int64)
    for t in terms:
        if len(t) <= 16:
            per_token[ref.holders(t)] += 1
    per_token[~short] = 0
    per_block = np.add.reduceat(per_token, np.arange(0, V, 256))
    assert per_block.max() > 512 and per_token.sum() > 2 * short.sum(), (per_block.max(), per_token.sum(), short.sum())
    assert (per_block[:-1] > 512).sum() >= 2 and V % 256 != 0               # ... and the partial last workgroup exists

    idx, created = _build(rows)
    corpus = orc.OracleCorpus([None] * NE, created, rows)
    queries = ["ab %s k03!&+=- %s" % (planted[257].decode(), rnd[500].decode()), "aaaaaaaaaaaaaaaa hg ^07 中"]
    want = [corpus.search([], text, NOW, 10, candidate_limit=NE) for text in queries]
    assert all(len(w[0]) == 10 for w in want)
    _E.update(idx=idx, ref=ref, terms=terms, queries=queries, want=want, planted=planted, longs=longs, corpus=corpus)
    return _E


def _search_equals_the_oracle(e, what):
    P = pkg()
    idx = e["idx"]
    rows, scores, counts = idx.search(None, [P.text.query_terms(t) for t in e["queries"]], NOW, 10, candidate_limit=NE)
    for b, (orow, osc, _) in enumerate(e["want"]):
        assert list(rows[b, :counts[b]]) == list(orow) and np.array_equal(scores[b, :counts[b]], osc), (what, "the search behind the run", b)


def _subset(terms, n):
    """n terms spread over the whole list: every family is in it"""
    return [terms[i * len(terms) // n] for i in range(n)]


@pytest.mark.parametrize("mid", [-1, 0])
@pytest.mark.parametrize("form", [0, 1])
def test_edges_in_every_match_form(form, mid):
    e = _corpus_e()
    idx, ref, terms = e["idx"], e["ref"], e["terms"]
    idx.set_profiling(True)
    try:
        idx.reset_search_stats()
        got = idx.keyword_bitmaps(terms, form=form, mid=mid)
        st = idx.kernel_stats()
        ss = idx.search_stats()
    finally:
        idx.set_profiling(False)
    what = ("corpus E", "form", form, "mid", mid)
    _exact(got, ref, terms, what)
    assert got["form"] == form and got["runs"] == 1, (what, got["form"], got["runs"])
    assert got["hits"] > 3000 and not got["alias"].any()
    # which kernels ran: the kernel statistics record the launches, the search statistics do not move
    assert st["vocab_match"]["launches"] == 1 and st["vocab_scan"]["launches"] == 1 and st["expand_hits"]["launches"] == 1, sorted(st)
    assert st.get("vocab_match_mid", {}).get("launches", 0) == (1 if mid == -1 else 0), sorted(st)
    assert ss["searches"] == 0 and ss["passes"] == 0 and ss["kw_passes"] == 0 and ss["kw_hits_total"] == 0, ss
    # the planted postings, stated outright (not only through the reference)
    for k, name in e["planted"].items():
        t = terms.index(name)
        m = np.unpackbits(got["bitmaps"][t].view(np.uint8), bitorder="little")[:NE].astype(bool)
        assert np.array_equal(np.nonzero(m)[0], np.array(_plant_rows(k))), (what, k)
    _search_equals_the_oracle(e, what)


@pytest.mark.parametrize("n_terms", [1, 63, 64, 65, 130])
def test_edges_with_few_terms(n_terms):
    """1 .. 64 terms take the one-workgroup alias stage, more the two-kernel one; 63, 65 and 130 leave the last term group of the
    lane-per-token kernels (32 terms) and of the wave scan (64 terms) partial."""
    e = _corpus_e()
    idx, ref = e["idx"], e["ref"]
    terms = _subset(e["terms"], n_terms) if n_terms > 1 else [b"ab"]
    assert len(set(terms)) == n_terms
    for form in (0, 1):
        for mid in (-1, 0):
            what = ("corpus E", n_terms, "terms, form", form, "mid", mid)
            got = idx.keyword_bitmaps(terms, form=form, mid=mid)
            _exact(got, ref, terms, what)
            assert got["form"] == form and got["runs"] == 1, what
            _search_equals_the_oracle(e, what)


def test_edges_hit_list_overflow_in_the_lookup_form():
    e = _corpus_e()
    idx, ref, terms = e["idx"], e["ref"], e["terms"]
    idx.set_option("kw_hits_cap", 16)
    try:
        got = idx.keyword_bitmaps(terms, form=1)
        assert got["runs"] > 1 and got["form"] == 1, got["runs"]          # the list was too short: the chain ran again
        _exact(got, ref, terms, "corpus E, a 16-entry hit list")
        _search_equals_the_oracle(e, "a 16-entry hit list")
        again = idx.keyword_bitmaps(terms, form=1)                         # the list has grown and stays grown
        assert again["runs"] == 1 and again["hits"] == got["hits"] and np.array_equal(again["bitmaps"], got["bitmaps"])
    finally:
        idx.set_option("kw_hits_cap", 16 << 20)
    _search_equals_the_oracle(e, "the list put back")


def test_argument_errors_on_a_real_index():
    P = pkg()
    e = _corpus_e()
    idx = e["idx"]
    for call in (lambda: idx.keyword_bitmaps([b"ab", b"ab"]), lambda: idx.keyword_bitmaps([b"ab", b""]), lambda: idx.keyword_bitmaps([]),
                 lambda: idx.keyword_bitmaps([b"ab"], form=2), lambda: idx.keyword_bitmaps([b"ab"], mid=1),
                 lambda: idx.keyword_bitmaps([b"t%d" % i for i in range(4097)])):
        with pytest.raises(P.native.OrrError) as err:
            call()
        assert err.value.code == P.native.ORR_EINVAL
    raw = P.RecallIndex(dim=0)
    raw.append(None, np.array([NOW], np.int64), [b"ab cd"])
    with pytest.raises(P.native.OrrError) as err:
        raw.keyword_bitmaps([b"ab"])
    assert err.value.code == P.native.ORR_ESTATE                            # not sealed
    raw.close()
    _search_equals_the_oracle(e, "refused calls")


def _batch_equals_the_oracle(idx, corpus, texts, n_rows, what):
    """one hybrid batch: rows and score bits of every query against the oracle's, as _search_equals_the_oracle compares them"""
    P = pkg()
    terms = [P.text.query_terms(t) for t in texts]
    rows, scores, counts = idx.search(None, terms, NOW, 10, candidate_limit=n_rows)
    for b, text in enumerate(texts):
        orow, osc, _ = corpus.search([], text, NOW, 10, candidate_limit=n_rows)
        assert len(orow) == 10, (what, b)
        assert list(rows[b, :counts[b]]) == list(orow) and np.array_equal(scores[b, :counts[b]], osc), (what, b)
    return terms


def test_edges_batch_with_shared_terms_and_a_query_without_terms():
    """What the host half of the chain makes of a batch and nothing else looks at: a term that two queries share (one bitmap,
    two entries of the term map), a query with no terms between queries that have some (two equal query offsets), a term of
    17 .. 32 bytes and a longer one (the eight-dword image, the term pool).  A term repeated inside one query is the plan's
    selftest's: the text layer may fold it."""
    e = _corpus_e()
    planted = e["planted"]
    texts = ["ab %s" % planted[257].decode(), "hg ab ^07", "", "%s 中 %s" % (planted[63].decode(), planted[64].decode()), "aaaaaaaaaaaaaaaa k03!&+=-"]
    terms = _batch_equals_the_oracle(e["idx"], e["corpus"], texts, NE, "corpus E, five queries")
    assert set(terms[0]) & set(terms[1]) == {b"ab"} and terms[2] == [] and all(len(q) == len(set(q)) for q in terms)
    assert any(17 <= len(t) <= 32 for t in terms[3]) and any(len(t) > 32 for t in terms[3])
    _search_equals_the_oracle(e, "behind the batch of five")


# ---- the two large corpora: fixed-width rows, the bitmap reference as array compares ---------------------------------------------

class FixedRows:
    """rows of equal width as a [n, width] byte array: has(term) compares byte for byte (position p of a row matches when byte
    p + j equals term[j] for every j), has_by_find is `term in row` with bytes.find over the rows laid end to end"""

    def __init__(self, rowbytes):
        self.rowbytes, self.blob = rowbytes, None

    def rows(self):
        return [r.tobytes() for r in self.rowbytes]

    def has(self, term):
        x = self.rowbytes
        span = x.shape[1] - len(term) + 1
        if span <= 0:
            return np.zeros(x.shape[0], bool)
        m = x[:, 0:span] == term[0]
        for j in range(1, len(term)):
            m &= x[:, j:j + span] == term[j]
        return m.any(axis=1)

    def has_by_find(self, term, most=None):
        """(most: give up with None beyond that many rows -- a frequent term is quicker by array compares)"""
        if self.blob is None:
            self.blob = self.rowbytes.tobytes()
        blob, (n, width) = self.blob, self.rowbytes.shape
        m = np.zeros(n, bool)
        found, pos = 0, blob.find(term)
        while pos >= 0:
            row = pos // width
            if pos + len(term) <= (row + 1) * width:                        # (a match across two rows is no match)
                m[row] = True
                found += 1
                if most is not None and found > most:
                    return None
                pos = blob.find(term, (row + 1) * width)
            else:
                pos = blob.find(term, pos + 1)
        return m

    def has_either(self, term):
        """the reference of the large corpora: bytes.find for a term in few rows, array compares for a frequent one"""
        m = self.has_by_find(term, most=2048)
        return m if m is not None else self.has(term)


def _fixed(slots):
    """[n, k] tokens of 8 bytes each (an S8 array) -> [n, 9 k - 1] bytes, single spaces between the tokens"""
    n, k = slots.shape
    out = np.full((n, 9 * k - 1), 32, np.uint8)
    raw = slots.view(np.uint8).reshape(n, k, 8)
    for j in range(k):
        out[:, 9 * j:9 * j + 8] = raw[:, j]
    return out


# ---- corpus T: the threshold of the default form selection ---------------------------------------------------------------------

NT_ROWS, T_SLOTS = 17_510, 8
_T = {}


def _corpus_t():
    if _T:
        return _T
    n_tok = NT_ROWS * T_SLOTS
    i = np.arange(n_tok, dtype=np.int64)
    h = (i * 2654435761 + 12345) % (1 << 32)
    digits = [(i // 26 ** d) % 26 for d in range(4)] + [(h >> (5 * d)) % 23 for d in range(4)]     # four letters that number the token, four that vary
    letters = (np.stack(digits, axis=1) + ord("a")).astype(np.uint8)
    tokens = np.ascontiguousarray(letters).view("S8").reshape(NT_ROWS, T_SLOTS)
    fixed = FixedRows(_fixed(tokens))
    ref = Reference(fixed.rows(), has=fixed.has_either)
    V = len(ref.vocab)
    assert V == n_tok >= (1 << 17) + 9000 and all(len(t) == 8 for t in ref.vocab[:100])
    flat = tokens.reshape(-1)
    terms = [bytes([c]) for c in b"aqz"] + [b"ab", b"zz", b"qa", b"ba", b"mn", b"aa", b"vw"]
    for j in range(300):
        tok = bytes(flat[(j * 7919 + 13) % n_tok])
        kind = j % 6
        if kind == 0:
            terms.append(tok)                                               # a whole token
        elif kind == 1:
            terms.append(tok[:5])
        elif kind == 2:
            terms.append(tok[3:8])
        elif kind == 3:
            terms.append(tok[1:4])
        elif kind == 4:
            terms.append(tok[:7] + (b"a" if tok[7:8] != b"a" else b"b"))    # a near-miss in the last byte
        else:
            terms.append(tok[4:8] + b"x")                                   # no token holds it: x is no letter of the varied half
    terms = list(dict.fromkeys(terms))
    at = -(-(1 << 25) // V)                                                 # the fewest terms with terms x V >= 2^25
    assert at == 240 and len(terms) >= at and (at - 1) * V < (1 << 25) <= at * V and at - 1 >= 64
    idx, _ = _build(ref.rows)
    idx.search(None, [[b"ab"]], NOW, 5, candidate_limit=100)
    assert idx.search_stats()["vocab_tokens"] == V                         # the library's vocabulary is the Python split's
    _T.update(idx=idx, ref=ref, terms=terms, at=at, fixed=fixed)
    return _T


@pytest.mark.parametrize("case", ["at the threshold", "one term below", "63 terms"])
def test_default_form_selection_at_the_threshold(case):
    """The only place where the default selection is pinned: the lookup form from 64 distinct terms and terms x vocabulary >= 2^25
    on, the all-pairs form below either."""
    t = _corpus_t()
    idx, ref = t["idx"], t["ref"]
    n_terms, form = {"at the threshold": (t["at"], 1), "one term below": (t["at"] - 1, 0), "63 terms": (63, 0)}[case]
    terms = t["terms"][:n_terms]
    got = idx.keyword_bitmaps(terms)                                        # form -1: as a search would choose
    assert got["form"] == form and got["runs"] == 1, (case, n_terms, len(ref.vocab), got["form"])
    _exact(got, ref, terms, ("corpus T", case))
    assert got["hits"] > 10_000
    other = idx.keyword_bitmaps(terms, form=1 - form)                       # ... and the other form agrees on this vocabulary
    assert other["form"] == 1 - form
    _exact(other, ref, terms, ("corpus T", case, "the form not chosen"))


def test_batch_of_many_distinct_terms_takes_the_lookup_form():
    """The lookup form's tables and Bloom bits as a SEARCH uploads them: two queries that together hold four terms more than the
    default selection's threshold, the same four terms in both (150 terms a query at most, as tests/test_gpu_count_words.py has)."""
    P = pkg()
    t = _corpus_t()
    idx, ref = t["idx"], t["ref"]
    pool = [x for x in t["terms"] if len(x) >= 3]
    shared, own = pool[:4], pool[4:]
    need = t["at"] + 4
    n0 = 150 - 4
    queries = [shared[:2] + own[:n0] + shared[2:], own[n0:need - 4] + shared]
    assert len(queries) == 2 and max(len(q) for q in queries) <= 150 and len(own) >= need - 4
    texts = [b" ".join(q).decode() for q in queries]
    distinct = list(dict.fromkeys(x for text in texts for x in P.text.query_terms(text)))
    assert len(distinct) >= need and all(set(shared) <= set(P.text.query_terms(text)) for text in texts), len(distinct)
    got = idx.keyword_bitmaps(distinct)                                     # form -1: as the search below chooses
    assert got["form"] == 1 and got["runs"] == 1, (len(distinct), got["form"])
    _exact(got, ref, distinct, ("corpus T", len(distinct), "terms of two queries"))
    if "corpus" not in t:
        created = (NOW - np.arange(NT_ROWS, dtype=np.int64) * 1000).astype(np.int64)       # _build's
        t["corpus"] = orc.OracleCorpus([None] * NT_ROWS, created, ref.rows)
    _batch_equals_the_oracle(idx, t["corpus"], texts, NT_ROWS, "corpus T, two queries past the threshold")


# ---- corpus A: stored token bitmaps ----------------------------------------------------------------------------------------------

NA = 196_700
AT, BELOW = -(-NA // 64), -(-NA // 64) - 1
_A = {}


def _corpus_a():
    if _A:
        return _A
    assert NA >= 196_608 and NA % 128 != 0 and AT * 64 >= NA > BELOW * 64
    r = np.arange(NA)
    slots = np.empty((NA, 6), "S8")
    slots[:, 0] = np.array([b"fqa-aaaa", b"fqa-bbbb", b"fqa-cccc", b"fqa-dddd"], "S8")[r % 4]       # frequent tokens
    slots[:, 1] = np.array([b"shardone", b"shardtwo", b"plainxyz"], "S8")[r % 3]                     # two frequent tokens share a fragment
    slots[:, 2] = b"fillerzz"
    at_rows = np.unique(np.concatenate([[0, 31, 32, NA - 1], (np.arange(AT - 4) * 64 + 40)]))      # row 0, bits 31 and 0, the last row
    below_rows = np.arange(BELOW) * 64 + 7
    assert len(at_rows) == AT and len(below_rows) == BELOW and at_rows.max() == NA - 1 and below_rows.max() < NA
    assert not np.intersect1d(at_rows, below_rows).size
    slots[at_rows, 2] = b"atbound!"
    slots[below_rows, 2] = b"belowbd!"
    slots[:, 3] = b"commonqq"
    rare_rows = np.arange(400) * 491 + 5
    slots[rare_rows, 3] = np.array([b"rare%04d" % (j // 2) for j in range(400)], "S8")                # 200 rare tokens, two rows each
    slots[:, 4] = b"padpadpa"
    slots[:, 5] = np.array([b"lastlast", b"lastlas2"], "S8")[(r % 7 == 0).astype(int)]
    fixed = FixedRows(_fixed(slots))
    ref = Reference(fixed.rows(), has=fixed.has_either)
    assert ref.postings[b"atbound!"] == AT and ref.postings[b"belowbd!"] == BELOW and ref.postings[b"rare0007"] == 2
    idx, _ = _build(ref.rows, one_lane=False)
    idx.search(None, [[b"shardone"]], NOW, 5, candidate_limit=300)         # a search with terms first: the token store exists
    few = [b"fqa-aaaa", b"one", b"shard", b"rare0007", b"belowbd!", b"atbound!", b"shardtwo", b"rare", b"fqa-", b"nomatchx", b"lastlas", b"lastlas2",
           b"padpadpa", b"bound!", b"owbd", b"plain", b"q", b"commonqq", b"e", b"pad", b"dp"]
    many = few + [b"rare%04d" % j for j in range(20, 120)] + [b"fqa-bbbb", b"fqa-cccc", b"fqa-dddd", b"two", b"xyz"]
    assert len(few) <= 64 < len(many) and len(set(many)) == len(many)
    want = dict(zip(few, ref.alias(few)))
    # what the issue names: a whole frequent token and a fragment of exactly one frequent token are read from the store, a fragment
    # of two tokens, a whole rare token and the token one posting below the boundary are expanded, the token at the boundary is stored
    assert [want[t] for t in (b"fqa-aaaa", b"one", b"shard", b"rare0007", b"belowbd!", b"atbound!", b"nomatchx")] == [1, 1, 0, 0, 0, 1, 0], want
    # ... and a fragment with two starts in the one frequent token that holds it: reported twice, it would not be read from the store
    assert want[b"pad"] == 1 and ref.vocab[ref.holders(b"pad")[0]].count(b"pad") == 2
    _A.update(idx=idx, view=idx.view(), ref=ref, few=few, many=many, fixed=fixed)
    return _A


@pytest.mark.parametrize("n_terms", ["few", "many"])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("handle", ["idx", "view"])
def test_alias_flags_and_bitmaps_with_stored_token_bitmaps(handle, form, n_terms):
    a = _corpus_a()
    terms = a[n_terms]
    got = a[handle].keyword_bitmaps(terms, form=form)
    what = ("corpus A", handle, "form", form, len(terms), "terms")
    _exact(got, a["ref"], terms, what)
    assert got["form"] == form and got["runs"] == 1 and got["alias"].sum() >= 6, what


def test_the_two_restatements_agree():
    """array compares (the bitmap reference of the two large corpora) against bytes.find, on terms of each kind"""
    a, t = _corpus_a(), _corpus_t()
    for fixed, terms in ((a["fixed"], [b"one", b"shard", b"atbound!", b"rare0007", b"nomatchx", b"zz fqa", b"e"]), (t["fixed"], t["terms"][:24])):
        for term in terms:
            assert np.array_equal(fixed.has(term), fixed.has_by_find(term)), term
