"""SearchInDocuments (orrh_service_search_documents_json): SearchAsync over the chunks of the listed documents only --
GetChunksByDocumentIdAsync (IIngestionStore.cs:11) feeding RecallSearchService.cs:26-37.  The response must be the JSON that
Search returns on a store that holds only those documents, on one shard and with delta shards in place."""
import numpy as np
import pytest

from helpers import pkg

pytestmark = pytest.mark.gpu

NOW = 639144000000000000
DAY = 864000000000
WORDS = ["alpha", "beta", "gamma", "delta", "kubernetes", "azure"]
TEXTS = ("alpha kubernetes", "the gamma", "zzz", "azure delta beta")


class _World:
    """A store, and every upload remembered so that a store holding only some documents can be made from the same records."""

    def __init__(self, seed, dim=16):
        self.S = pkg().service
        self.rng = np.random.default_rng(seed)
        self.dim = dim
        self.store = self.S.InMemoryIngestionStore()
        self.docs = {}                                                        # document -> (record, chunk records), first-upload order
        self.qv = self.rng.standard_normal(dim).astype(np.float32)

    def upload(self, doc, created, n_chunks=6, spread=0, null_every=0):
        S, rng = self.S, self.rng
        rec = S.CosmosDocumentRecord(doc, doc + ".md", created)
        cs = [S.CosmosChunkRecord("%s:%04d" % (doc, i), doc, i, " ".join(rng.choice(WORDS, 8)),
                                  None if null_every and i % null_every == 0 else rng.standard_normal(self.dim).astype(np.float32),
                                  created + spread * i) for i in range(n_chunks)]
        self.store.UpsertDocument(rec)
        self.store.UpsertChunks(cs)
        self.docs[doc] = (rec, cs)

    def delete(self, doc):
        self.store.DeleteDocument(doc)
        del self.docs[doc]

    def service(self, store, limit):
        return self.S.RecallSearchService(store, self.S.StubQueryEmbeddingClient(self.qv), candidate_limit=limit, now_ticks=NOW)

    def check(self, sut, limit, documents, ks=(8, 3, 100)):
        """sut.SearchInDocuments(documents) against Search on a store that holds only those documents."""
        only = self.S.InMemoryIngestionStore()
        held = 0
        for doc, (rec, cs) in self.docs.items():
            if doc in set(documents):
                only.UpsertDocument(rec)
                only.UpsertChunks(cs)
                held += len(cs)
        ref = self.service(only, limit) if held else None
        cited = 0
        for text in TEXTS:
            for k in ks:
                got = sut.SearchInDocuments(text, k, list(documents))
                want = ref.Search(text, k) if ref else {"query": text, "citations": []}
                assert got == want, (text, k, documents)
                assert all(c["documentId"] in set(documents) for c in got["citations"])
                cited += len(got["citations"])
        if ref:
            ref.close()
        only.close()
        return cited

    def close(self):
        self.store.close()


@pytest.mark.parametrize("limit", [300, 10, 10**6])
def test_search_in_documents_on_one_shard_and_with_delta_shards(limit):
    w = _World(201)
    base = NOW - 100 * DAY
    for d in range(60):
        w.upload("doc-%02d" % d, base + d * 1000 * (d % 7), n_chunks=4 + d % 5, spread=d % 3, null_every=5 if d % 4 == 0 else 0)
    sut = w.service(w.store, limit)
    some = ["doc-%02d" % d for d in (3, 17, 18, 40, 59)]
    many = ["doc-%02d" % d for d in range(0, 60, 2)]
    assert w.check(sut, limit, some) > 0
    assert sut.Stats()["shards"] == 1
    w.check(sut, limit, many)
    w.check(sut, limit, ["doc-07"])
    # unknown ids are skipped; an empty list and a list of unknown documents give no citations
    w.check(sut, limit, some + ["no-such-document", ""])
    assert w.check(sut, limit, []) == 0
    assert w.check(sut, limit, ["no-such-document"]) == 0
    assert sut.SearchInDocuments("alpha", 5, []) == {"query": "alpha", "citations": []}
    # the unscoped search is what it was
    full = sut.Search("alpha kubernetes", 8)
    assert len(full["citations"]) == 8
    # a blank query is an argument error, as in Search
    with pytest.raises(Exception) as e:
        sut.SearchInDocuments("   ", 5, some)
    assert "Query is required" in str(e.value)

    # delta shards: strictly newer uploads, some of them in the scope
    for j in range(3):
        w.upload("new-%d" % j, NOW - (3 - j) * DAY, n_chunks=5)
        sut.Search("alpha", 3)                                                # each upload is indexed as its own delta shard
    assert sut.Stats()["shards"] >= 2
    scope = some + ["new-0", "new-2"]
    assert w.check(sut, limit, scope) > 0
    w.check(sut, limit, ["new-1"])                                            # a scope that lies in one shard only
    w.check(sut, limit, many + ["new-1"])
    # a document of the scope is deleted: its chunks neither rank nor count
    w.delete("doc-17")
    w.delete("new-2")
    w.check(sut, limit, scope)
    w.check(sut, limit, [d for d in scope if d in w.docs])
    # ... and one is uploaded again with another chunk list
    w.upload("doc-18", NOW - DAY // 2, n_chunks=9)
    w.check(sut, limit, scope)
    assert sut.Search("alpha kubernetes", 8)["citations"]
    sut.close()
    w.close()
