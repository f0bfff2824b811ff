"""Reindex through the service mirror, the way the reference does it: DocumentIngestionService.ReindexDocumentAsync
(DocumentIngestionService.cs:210-291) re-embeds every chunk of a document and upserts the list again with the same chunk
ids, contents and CreatedAtUtc (:277).  The mirror overwrites those rows' vectors in place (orr_index_update_rows): no
tombstones, no delta shard, no rebuild.  A list that changes anything else, or whose vectors change dimension, takes the
tombstone path as before.  Every search equals the oracle over the store as it stands."""
import numpy as np
import pytest

from helpers import orc, pkg

pytestmark = pytest.mark.gpu

NOW = 639144000000000000
WORDS = np.array(["alpha", "beta", "gamma", "delta", "kubernetes", "azure", "helm", "cosmos", "vector", "search"])
TEXTS = ("alpha kubernetes", "the gamma", "helm cosmos search", "zzz")


def test_reindex_overwrites_vectors_in_place():
    S = pkg().service
    rng = np.random.default_rng(90)
    dim, n_docs, per_doc = 128, 200, 990                       # 198,000 chunks: the int8 shadow and the two-stage pass
    store = S.InMemoryIngestionStore()
    base = NOW - 200 * 864000000000
    docs = {}
    for d in range(n_docs):
        doc = "doc-%03d" % d
        created = base + d * 1000
        store.UpsertDocument(S.CosmosDocumentRecord(doc, doc + ".md", created))
        emb = rng.standard_normal((per_doc, dim)).astype(np.float32)
        words = WORDS[rng.integers(0, len(WORDS), (per_doc, 5))]
        cs = [S.CosmosChunkRecord("%s:%04d" % (doc, i), doc, i, " ".join(words[i]), emb[i], created + i % 7)
              for i in range(per_doc)]
        store.UpsertChunks(cs)
        docs[doc] = cs
    qv = rng.standard_normal(dim).astype(np.float32)

    def flat():
        return [c for doc in sorted(docs, key=lambda x: int(x[4:])) for c in docs[doc]]

    def check(sut, k=10):
        chunks = flat()
        cor = orc.OracleCorpus([None if c.Embedding is None else np.asarray(c.Embedding, np.float32) for c in chunks],
                               [c.CreatedAtTicks for c in chunks], [c.Content for c in chunks])
        for text in TEXTS:
            body = sut.Search(text, k)
            rows, _, rounded = cor.search(qv, text, NOW, k, candidate_limit=10**6, threads=8)
            assert [(c["chunkId"], c["score"]) for c in body["citations"]] == \
                   [(chunks[r].Id, rd) for r, rd in zip(rows, rounded)], text
        return body

    def reindex(doc, vectors, content_of=None):
        """ReindexDocumentAsync: same ids, chunk indices, contents and timestamps; new vectors."""
        new = []
        for i, c in enumerate(docs[doc]):
            content = content_of(i, c.Content) if content_of else c.Content
            new.append(S.CosmosChunkRecord(c.Id, c.DocumentId, c.ChunkIndex, content, vectors[i], c.CreatedAtTicks))
        store.UpsertChunks(new)
        docs[doc] = new

    sut = S.RecallSearchService(store, S.StubQueryEmbeddingClient(qv), candidate_limit=10**6, now_ticks=NOW)
    check(sut)                                                  # the first build, and a search before the reindex
    st0 = sut.Stats()
    assert st0["full_rebuilds"] == 1 and st0["shards"] == 1 and sut.UpdatedRows() == 0

    # three documents re-embedded; near-copies of the query among the new vectors (scaled 1e-3 and 1e3: a stale int8 scale
    # or rel_err would drop them from the screen), a null vector that stays null, non-finite components
    picked = ["doc-000", "doc-117", "doc-199"]
    for j, doc in enumerate(picked):
        vecs = [rng.standard_normal(dim).astype(np.float32) for _ in range(per_doc)]
        vecs[3 + j] = ((qv + np.float32(1e-3) * rng.standard_normal(dim).astype(np.float32)) * np.float32(1e-3 if j % 2 else 1e3)).astype(np.float32)
        if j == 1:
            vecs[10][5] = np.nan
            vecs[11][0] = np.inf
        reindex(doc, vecs)
    body = check(sut)
    assert {c["chunkId"] for c in body["citations"]} & {"%s:%04d" % (d, 3 + j) for j, d in enumerate(picked)}
    st = sut.Stats()
    assert (st["full_rebuilds"], st["delta_builds"], st["tombstoned_rows"], st["shards"]) == \
           (st0["full_rebuilds"], st0["delta_builds"], st0["tombstoned_rows"], st0["shards"]), st
    assert sut.UpdatedRows() == 3 * per_doc

    # a reindex that also changes one chunk's content: today's path (tombstones, then a delta shard or a rebuild)
    reindex("doc-050", [rng.standard_normal(dim).astype(np.float32) for _ in range(per_doc)],
            content_of=lambda i, s: s + " edited" if i == 7 else s)
    check(sut)
    st = sut.Stats()
    assert sut.UpdatedRows() == 3 * per_doc
    assert st["tombstoned_rows"] > st0["tombstoned_rows"] or st["full_rebuilds"] > st0["full_rebuilds"], st

    # new vectors of another dimension: today's path as well
    st1 = st
    reindex("doc-080", [rng.standard_normal(dim // 2).astype(np.float32) for _ in range(per_doc)])
    check(sut)
    st = sut.Stats()
    assert sut.UpdatedRows() == 3 * per_doc
    assert st["tombstoned_rows"] > st1["tombstoned_rows"] or st["full_rebuilds"] > st1["full_rebuilds"], st
    sut.close()
    store.close()
