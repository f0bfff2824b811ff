"""Uploads that are NOT strictly newer than everything indexed, through the service mirror with "insert_older" on:
UpsertChunksAsync (InMemoryIngestionStore.cs:17-25) takes any CreatedAtUtc, and instead of rebuilding the whole corpus the
mirror inserts such chunks into the sealed shards in place (orr_index_insert_rows), each into the shard its ticks belong to --
when that provably gives the order a rebuild would.  Every search equals the oracle over the store as it stands."""
import numpy as np
import pytest

from helpers import orc, pkg

pytestmark = pytest.mark.gpu

NOW = 639144000000000000
DAY = 864000000000
WORDS = ["alpha", "beta", "gamma", "delta", "kubernetes", "azure"]
TEXTS = ("alpha kubernetes", "the gamma", "zzz", "inserted later")


class _World:
    """A store and the flat chunk list a rebuild would enumerate (documents in first-upload order)."""

    def __init__(self, seed, dim=16):
        self.S = pkg().service
        self.rng = np.random.default_rng(seed)
        self.dim = dim
        self.store = self.S.InMemoryIngestionStore()
        self.flat = []
        self.qv = self.rng.standard_normal(dim).astype(np.float32)

    def upload(self, doc, created, n_chunks=6, spread=0, words=None, null_every=0):
        S, rng = self.S, self.rng
        self.store.UpsertDocument(S.CosmosDocumentRecord(doc, doc + ".md", created))
        cs = [S.CosmosChunkRecord("%s:%04d" % (doc, i), doc, i, " ".join(rng.choice(words or WORDS, 8)),
                                  None if null_every and i % null_every == 0 else rng.standard_normal(self.dim).astype(np.float32),
                                  created + spread * i) for i in range(n_chunks)]
        self.store.UpsertChunks(cs)
        at = next((i for i, c in enumerate(self.flat) if c.DocumentId == doc), None)
        if at is None:
            self.flat.extend(cs)
        else:                                                                  # a replaced list keeps its place in the enumeration
            rest = [c for c in self.flat if c.DocumentId != doc]
            self.flat[:] = rest[:at] + cs + rest[at:]
        return cs

    def check(self, sut, limit, k=8):
        cor = orc.OracleCorpus([c.Embedding for c in self.flat], [c.CreatedAtTicks for c in self.flat], [c.Content for c in self.flat])
        for text in TEXTS:
            body = sut.Search(text, k)
            rows, _, rounded = cor.search(self.qv, text, NOW, k, candidate_limit=limit)
            assert [(c["chunkId"], c["score"]) for c in body["citations"]] == \
                   [(self.flat[r].Id, rd) for r, rd in zip(rows, rounded)], text

    def service(self, limit):
        return self.S.RecallSearchService(self.store, self.S.StubQueryEmbeddingClient(self.qv), candidate_limit=limit, now_ticks=NOW)

    def close(self):
        self.store.close()


@pytest.mark.parametrize("limit", [300, 10**6])
def test_older_uploads_are_inserted_into_a_single_shard(limit):
    w = _World(101)
    base = NOW - 100 * DAY
    for d in range(60):
        w.upload("old-%02d" % d, base + d * 1000)
    sut = w.service(limit)
    w.check(sut, limit)
    st0 = sut.Stats()
    assert st0 == {"shards": 1, "full_rebuilds": 1, "delta_builds": 0, "tombstoned_rows": 0, "compactions": 0, "delta_merges": 0}

    # the default is off: an older upload rebuilds
    w.upload("late-a", base - 5)
    w.check(sut, limit)
    assert sut.Stats()["full_rebuilds"] == 2 and sut.InsertedRows() == 0

    sut.SetOption("insert_older", 1)
    st1 = sut.Stats()
    w.upload("late-b", base - 77, n_chunks=5, words=WORDS + ["inserted", "later"])        # older than everything
    w.check(sut, limit)
    w.upload("late-c", base + 30 * 1000, n_chunks=7, spread=1000, null_every=3)           # inside, at the ticks of old-30 .. old-36's rows; null vectors
    w.check(sut, limit)
    w.upload("late-d", base + 10 * 1000, n_chunks=4)                                      # an exact tie with old-10, behind it in the enumeration
    w.upload("late-e", base + 10 * 1000, n_chunks=3, words=["inserted", "later", "alpha"])  # two documents in ONE insert, tied with each other
    w.check(sut, limit)
    w.check(sut, limit, k=300)
    assert sut.Stats() == st1, (sut.Stats(), st1)
    assert sut.InsertedRows() == 5 + 7 + 4 + 3

    # rows that were inserted can be dropped in place like any others
    w.store.DeleteDocument("late-c")
    w.flat[:] = [c for c in w.flat if c.DocumentId != "late-c"]
    w.check(sut, limit)
    st = sut.Stats()
    assert st["full_rebuilds"] == st1["full_rebuilds"] and st["tombstoned_rows"] == st1["tombstoned_rows"] + 7, st

    # a tie that does not satisfy the order conditions: old-20's list is replaced by chunks at the ticks of old-21 .. old-24's
    # rows.  old-20 precedes those documents in the enumeration, so a rebuild puts its chunks IN FRONT of theirs, where an
    # insert would put them behind: the mirror falls back to what it does without the option, and stays correct.
    st2 = sut.Stats()
    ins = sut.InsertedRows()
    w.upload("old-20", base + 21 * 1000, n_chunks=4, spread=1000)
    w.check(sut, limit)
    st = sut.Stats()
    assert sut.InsertedRows() == ins
    assert st["full_rebuilds"] == st2["full_rebuilds"] + 1, (st, st2)

    # strictly newer uploads keep making delta shards
    w.upload("new-1", NOW - DAY)
    w.check(sut, limit)
    assert sut.Stats()["delta_builds"] == st["delta_builds"] + 1 and sut.Stats()["shards"] == 2
    sut.close()
    w.close()


@pytest.mark.parametrize("limit", [300, 10**6])
def test_older_uploads_go_into_the_shard_where_they_belong(limit):
    w = _World(202)
    base = NOW - 100 * DAY
    for d in range(40):
        w.upload("old-%02d" % d, base + d * 1000)
    sut = w.service(limit)
    sut.SetOption("insert_older", 1)
    w.check(sut, limit)
    t = base + 10**9
    for step in range(3):                                                      # three delta shards in front of the first
        for j in range(2):
            t += 7777
            w.upload("new-%d-%d" % (step, j), t, spread=10)
        w.check(sut, limit)
    st0 = sut.Stats()
    assert st0["shards"] == 4 and st0["full_rebuilds"] == 1 and st0["delta_builds"] == 3, st0

    # one upload whose chunks belong to three different shards: older than everything, between the first build and the first
    # delta shard, and inside the middle delta shard's range
    w.upload("spread", base - 9, n_chunks=3, spread=1)
    w.check(sut, limit)
    w.upload("between", base + 5 * 10**8, n_chunks=4, words=WORDS + ["inserted", "later"])
    w.check(sut, limit)
    mid = base + 10**9 + 3 * 7777 + 5                                          # inside delta shard 2 (new-1-0 .. new-1-1)
    w.upload("inside", mid, n_chunks=5, spread=3, null_every=2)
    w.check(sut, limit)
    cs = w.upload("wide", base - 100, n_chunks=6, spread=(t - base + 200) // 5)  # one document across every shard, the last chunk newest of all
    assert cs[-1].CreatedAtTicks > t
    w.check(sut, limit)
    w.check(sut, limit, k=300)
    assert sut.Stats() == st0, (sut.Stats(), st0)
    assert sut.InsertedRows() == 3 + 4 + 5 + 6

    # a document whose chunks sit in several shards is replaced: its rows leave every shard in place, the new list is newer
    w.upload("wide", t + 10**6, n_chunks=2)
    w.check(sut, limit)
    st = sut.Stats()
    assert st["full_rebuilds"] == 1 and st["tombstoned_rows"] == st0["tombstoned_rows"] + 6 and st["shards"] == 5, st
    sut.close()
    w.close()
