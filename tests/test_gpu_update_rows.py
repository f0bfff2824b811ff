"""Reindex in place (orr_index_update_rows): after an update every search, every screening image and the shard file must be
what a shard sealed from scratch with the new vectors gives.  Reference behaviour being matched:
DocumentIngestionService.ReindexDocumentAsync (DocumentIngestionService.cs:210-291) re-embeds a document's chunks and
upserts them again with the same ids, contents and CreatedAtUtc (:277) -- only the vectors change.

The updated rows include position 0, rows 255 / 256 (a tile boundary of the shadows), the last row (in the partial last
256-row tile), rows spread over many tiles, rows that gain or lose their vector, non-finite rows, and rows whose magnitude
changes by 1e-3 and 1e3 that are near-copies of test queries: a stale int8 scale or rel_err there saturates the image or
under-states the screening bound, and the screen drops the row that should rank first."""
import threading

import numpy as np
import pytest

from helpers import NOW, assert_same_ranking, build_index, orc, pkg, random_corpus

pytestmark = pytest.mark.gpu

TEXTS = ["alpha", "the kubernetes helm", "GAMMA delta zzz", "what is the", "azure cosmos vector search"]


def _quantise_rows(emb):
    """The int8 shadow's rows restated: se = max|e| / 127 (fp32), ie = rint(e * (1 / se)) clipped to +-127; rows with a
    non-finite value and zero rows get scale 0 and an all-zero image."""
    emb = np.asarray(emb, dtype=np.float32)
    finite = np.isfinite(emb).all(axis=1)
    mx = np.where(finite, np.abs(np.where(np.isfinite(emb), emb, 0)).max(axis=1), 0).astype(np.float32)
    se = (mx / np.float32(127.0)).astype(np.float32)
    inv = np.where(se > 0, np.float32(1.0) / np.where(se > 0, se, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        q = np.rint((np.where(finite[:, None], emb, 0) * inv[:, None]).astype(np.float32))
    return np.clip(q, -127, 127).astype(np.int8)


def _plan(rng, emb, dim, must, queries, n_spread):
    """{row id: new vector or None}: the rows of `must`, n_spread more spread over the shard, rows that gain or lose a
    vector, non-finite rows, and near-copies of the queries scaled by 1e-3 / 1e3 (one per query)."""
    n = len(emb)
    ids = list(dict.fromkeys(list(must) + [int(r) for r in rng.choice(n, n_spread, replace=False)]))
    plan = {}
    for r in ids:
        plan[r] = (rng.standard_normal(dim) * rng.choice([1.0, 1e-2, 30.0])).astype(np.float32)
    nulls = [r for r in range(n) if emb[r] is None]
    for r in nulls[:5]:
        plan[r] = rng.standard_normal(dim).astype(np.float32)                # a null row gains a vector
    free = [r for r in rng.permutation(n) if int(r) not in plan and emb[int(r)] is not None]
    free = [int(r) for r in free]
    for r in free[:6]:
        plan[r] = None                                                        # ... and rows lose theirs
    x = rng.standard_normal(dim).astype(np.float32)
    x[min(2, dim - 1)] = np.nan
    plan[free[6]] = x
    x = rng.standard_normal(dim).astype(np.float32)
    x[0] = np.inf
    plan[free[7]] = x
    x = rng.standard_normal(dim).astype(np.float32)
    x[dim - 1] = -np.inf
    plan[free[8]] = x
    for j, r in enumerate(free[9:19]):                                        # magnitude x 1e-3 / x 1e3 of the old vector
        plan[r] = (emb[r] * np.float32(1e-3 if j % 2 else 1e3)).astype(np.float32)
    for j, q in enumerate(queries):                                           # near-copies of the queries, rescaled
        r = free[19 + j]
        plan[r] = ((q + np.float32(1e-3) * rng.standard_normal(dim).astype(np.float32)) *
                   np.float32(1e-3 if j % 2 else 1e3)).astype(np.float32)
    return plan


def _apply(idx, plan, dim):
    """Two calls: rows with a vector, rows without one (dim 0).  Returns the rows written."""
    with_v = sorted(r for r, v in plan.items() if v is not None)
    without = sorted(r for r, v in plan.items() if v is None)
    done = 0
    if with_v:
        done += idx.update_rows(np.array(with_v, np.int64), np.stack([plan[r] for r in with_v]).astype(np.float32))
    if without:
        done += idx.update_rows(np.array(without, np.int64), None)
    return done


def _updated(emb, plan):
    out = list(emb)
    for r, v in plan.items():
        out[r] = None if v is None else v.copy()
    return out


def _check_small(idx, c, emb, qvecs, n, textsel=TEXTS):
    corpus = orc.OracleCorpus(emb, c["created"], c["contents"])
    cc = dict(c, emb=emb)
    for qv in qvecs:
        for text in textsel:
            for topk, limit in ((1, n), (10, n), (300, n), (10, 300), (300, 300)):
                assert_same_ranking(idx, corpus, cc, qv, text, topk, limit)


@pytest.mark.parametrize("seed,n,dim", [(41, 2500, 3), (42, 3000, 64), (43, 4000, 128)])
def test_update_small_shards_equal_the_oracle(seed, n, dim, tmp_path):
    P = pkg()
    rng = np.random.default_rng(seed)
    c = random_corpus(rng, n, dim)
    idx = build_index(c, chunk=977)
    queries = [rng.standard_normal(dim).astype(np.float32) for _ in range(3)]
    before = idx.search(np.stack(queries), [P.text.query_terms(t) for t in TEXTS[:3]], NOW, 10, candidate_limit=n)
    plan = _plan(rng, c["emb"], dim, [0, n - 1, 255, 256], queries, 40)
    assert _apply(idx, plan, dim) == len(plan)
    emb = _updated(c["emb"], plan)
    after = idx.search(np.stack(queries), [P.text.query_terms(t) for t in TEXTS[:3]], NOW, 10, candidate_limit=n)
    assert not np.array_equal(before[0], after[0])                             # the near-copies now rank first
    _check_small(idx, c, emb, queries + [None], n)

    # a repeated id: ORR_EINVAL and nothing is written
    r0 = next(r for r in range(n) if r not in plan)
    with pytest.raises(P.native.OrrError) as e:
        idx.update_rows(np.array([r0, 5, r0], np.int64), np.full((3, dim), 7.0, np.float32))
    assert e.value.code == P.native.ORR_EINVAL
    # a wrong dimension: ORR_EDIM
    with pytest.raises(P.native.OrrError) as e:
        idx.update_rows(np.array([r0], np.int64), np.ones((1, dim + 1), np.float32))
    assert e.value.code == P.native.ORR_EDIM
    _check_small(idx, c, emb, queries[:1], n, TEXTS[:2])

    # unknown and deleted ids are skipped; update then delete, delete then update
    dead = [r for r in range(n) if r not in plan][1:4]
    assert idx.delete_rows(dead) == 3
    upd_then_del = next(r for r in range(n - 1, 0, -1) if r not in plan and r not in dead)
    ids = np.array([dead[0], n + 11, -3, dead[1], upd_then_del], np.int64)
    vecs = rng.standard_normal((5, dim)).astype(np.float32)
    assert idx.update_rows(ids, vecs) == 1
    emb[upd_then_del] = vecs[4]
    assert idx.delete_rows([upd_then_del]) == 1
    dead.append(upd_then_del)
    assert idx.update_rows(np.array([dead[2]], np.int64), vecs[:1]) == 0        # deleted: stays deleted
    keep = np.array([r for r in range(n) if r not in dead], np.int64)
    sub = orc.OracleCorpus([emb[r] for r in keep], c["created"][keep], [c["contents"][r] for r in keep])
    for qv in queries + [vecs[4]]:
        for text in TEXTS[:3]:
            for topk, limit in ((10, n), (300, 300)):
                rows, scores, counts = idx.search(qv.reshape(1, -1), [P.text.query_terms(text)], NOW, topk, candidate_limit=limit)
                orow, osc, _ = sub.search(qv, text, NOW, topk, candidate_limit=limit)
                k = int(counts[0])
                assert list(rows[0, :k]) == [int(keep[r]) for r in orow], (text, topk, limit)
                a = scores[0, :k]
                assert ((a == osc) | (np.isnan(a) & np.isnan(osc))).all()

    # persistence: save after the update, load, search
    path = str(tmp_path / "shard.orr")
    idx.save(path)
    back = P.RecallIndex.load(path)
    for qv in queries[:2]:
        rows, scores, counts = back.search(qv.reshape(1, -1), [P.text.query_terms("alpha")], NOW, 10, candidate_limit=n)
        orow, osc, _ = sub.search(qv, "alpha", NOW, 10, candidate_limit=n)
        assert list(rows[0, :counts[0]]) == [int(keep[r]) for r in orow]
        assert np.array_equal(scores[0, :counts[0]], osc, equal_nan=True)
    back.close()
    idx.close()


def test_update_before_seal_and_without_embeddings_is_estate():
    P = pkg()
    idx = P.RecallIndex(dim=8)
    idx.append(np.ones((4, 8), np.float32), np.full(4, NOW, np.int64), [b"a"] * 4)
    with pytest.raises(P.native.OrrError) as e:
        idx.update_rows([0], np.ones((1, 8), np.float32))
    assert e.value.code == P.native.ORR_ESTATE
    idx.seal()
    assert idx.update_rows([0, 99], np.zeros((2, 8), np.float32)) == 1
    idx.close()
    idx = P.RecallIndex(dim=0)
    idx.append(None, np.full(4, NOW, np.int64), [b"a"] * 4)
    idx.seal()
    with pytest.raises(P.native.OrrError) as e:
        idx.update_rows([0], None)
    assert e.value.code == P.native.ORR_ESTATE
    idx.close()


def _big(rng, n, dim):
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    created = (NOW - 1000 * np.arange(n)).astype(np.int64)                  # strictly older: position == row id
    words = np.array(["alpha", "beta", "gamma", "delta", "kubernetes", "helm", "azure", "cosmos"])
    contents = [" ".join(w) for w in words[rng.integers(0, len(words), (n, 4))]]
    return emb, created, contents


def _shard(P, emb, created, contents):
    n = emb.shape[0]
    idx = P.RecallIndex(dim=emb.shape[1])
    for r0 in range(0, n, 65_536):
        idx.append(emb[r0:r0 + 65_536], created[r0:r0 + 65_536], [s.encode() for s in contents[r0:r0 + 65_536]])
    idx.seal()
    return idx


@pytest.mark.parametrize("dim", [512, 192])
def test_update_two_stage_shard_equals_a_fresh_shard(dim, tmp_path):
    """dim 512: the int8 shadow (forms 0, 1 and 2 of the screening GEMM) and the bf16 one; dim 192: the bf16 shadow only.
    Every shadow is built BEFORE the update, so the update itself has to rewrite their rows."""
    P = pkg()
    rng = np.random.default_rng(60 + dim)
    n = 196_608 + 77
    emb, created, contents = _big(rng, n, dim)
    idx = _shard(P, emb, created, contents)
    idx.set_option("two_stage", 1)                                           # int8 shadow at 512, bf16 at 192
    qs = rng.standard_normal((256, dim)).astype(np.float32)
    terms = [P.text.query_terms(TEXTS[b % len(TEXTS)]) for b in range(256)]
    idx.screen_dots(qs[:8])                                                  # the bf16 shadow (built on demand at 512)
    idx.search(qs[:64], terms[:64], NOW, 10, candidate_limit=n)
    emb_list = list(emb)
    tiles = [int(t) * 256 + int(rng.integers(0, 256)) for t in rng.choice(n // 256, 600, replace=False)]
    must = [0, 255, 256, n - 1, n - 2, 256 * 300 + 3] + tiles
    plan = _plan(rng, emb_list, dim, must, list(qs[:8]), 800)
    assert 1300 <= len(plan) <= 1700
    assert _apply(idx, plan, dim) == len(plan)
    new = emb.copy()
    for r, v in plan.items():
        new[r] = 0.0 if v is None else v
    fresh = _shard(P, new, created, contents)
    fresh.set_option("two_stage", 1)
    fresh.screen_dots(qs[:8])
    upd = np.array(sorted(plan), np.int64)

    if dim % 128 == 0:
        qi = qs[:70].copy()
        for form in (0, 1, 2):
            d1, iq1, ie1 = idx.screen_i8_dots(qi, form)
            d2, iq2, ie2 = fresh.screen_i8_dots(qi, form)
            assert np.array_equal(ie1, ie2), f"form {form}: int8 images differ at rows {np.nonzero((ie1 != ie2).any(1))[0][:10]}"
            assert np.array_equal(d1, d2), f"form {form}: accumulators differ"
        assert np.array_equal(ie1[upd], _quantise_rows(new[upd]))
        # the row constants of the bound (the saved file does not hold them): what update_rows_kernel wrote against the shadow build
        c1, c2 = idx.screen_i8_consts(), fresh.screen_i8_consts()
        for name in ("scale", "rel_err", "rel_hat", "rowf"):
            differ = np.nonzero((c1[name].view(np.uint32) != c2[name].view(np.uint32)).reshape(n, -1).any(1))[0]
            assert differ.size == 0, f"{name} differs from a fresh shard's at rows {differ[:10]}"
    s1, s2 = idx.screen_dots(qs[:8]), fresh.screen_dots(qs[:8])
    assert np.array_equal(s1, s2, equal_nan=True)

    p1, p2 = str(tmp_path / "upd.orr"), str(tmp_path / "fresh.orr")
    idx.save(p1)
    fresh.save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()

    want_mode = 1 if dim % 128 == 0 else 2
    for fuse in (0, 1):
        idx.set_option("fuse_epilogue", fuse)
        fresh.set_option("fuse_epilogue", fuse)
        for B in (1, 4, 6, 64, 129, 256):
            a = idx.search(qs[:B], terms[:B], NOW, 10, candidate_limit=n)
            assert idx.search_stats()["pass_mode"] == want_mode, (B, fuse)
            b = fresh.search(qs[:B], terms[:B], NOW, 10, candidate_limit=n)
            for x, y in zip(a, b):
                assert np.array_equal(x, y, equal_nan=True), (B, fuse)
    corpus = orc.OracleCorpus(_updated(emb_list, plan), created, contents)
    for b in range(8):
        text = TEXTS[b % len(TEXTS)]
        orow, osc, _ = corpus.search(qs[b], text, NOW, 10, candidate_limit=n, threads=8)
        assert set(int(r) for r in orow) & set(plan), b                       # updated rows rank in the top 10
        assert list(a[0][b, :a[2][b]]) == list(orow), b
        assert np.array_equal(a[1][b, :a[2][b]], osc), b
    idx.close()
    fresh.close()


def test_update_is_seen_by_lanes_and_views():
    P = pkg()
    rng = np.random.default_rng(70)
    n, dim = 200_000, 128
    emb, created, contents = _big(rng, n, dim)
    idx = _shard(P, emb, created, contents)
    qs = rng.standard_normal((12, dim)).astype(np.float32)
    texts = [TEXTS[b % len(TEXTS)] for b in range(12)]
    terms = [P.text.query_terms(t) for t in texts]
    views = [idx.view(), idx.view()]
    errors = []

    def run(h, b0):
        try:
            for _ in range(3):
                h.search(qs[b0:b0 + 3], terms[b0:b0 + 3], NOW, 10, candidate_limit=n)
        except Exception as ex:            # pragma: no cover - reported below
            errors.append(ex)

    ts = [threading.Thread(target=run, args=(idx, 3 * i)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors
    plan = _plan(rng, list(emb), dim, [0, 255, 256, n - 1], list(qs), 300)
    assert _apply(idx, plan, dim) == len(plan)
    corpus = orc.OracleCorpus(_updated(list(emb), plan), created, contents)
    want = [corpus.search(qs[b], texts[b], NOW, 10, candidate_limit=n, threads=8)[:2] for b in range(12)]
    got = {}

    def run2(h, key, b0, nb):
        try:
            got[key] = (b0, h.search(qs[b0:b0 + nb], terms[b0:b0 + nb], NOW, 10, candidate_limit=n))
        except Exception as ex:            # pragma: no cover
            errors.append(ex)

    jobs = [(idx, "lane%d" % i, 3 * i, 3) for i in range(4)] + [(views[0], "view0", 0, 12), (views[1], "view1", 2, 1)]
    ts = [threading.Thread(target=run2, args=j) for j in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and len(got) == len(jobs)
    for key, (b0, (rows, scores, counts)) in got.items():
        for i in range(rows.shape[0]):
            orow, osc = want[b0 + i]
            assert list(rows[i, :counts[i]]) == list(orow), (key, b0 + i)
            assert np.array_equal(scores[i, :counts[i]], osc), (key, b0 + i)
    for v in views:
        v.close()
    idx.close()


def test_update_through_cluster_shards():
    P = pkg()
    rng = np.random.default_rng(80)
    n, dim = 3000, 64
    c = random_corpus(rng, n, dim)
    order = np.argsort(-c["created"], kind="stable")
    c = {"emb": [c["emb"][i] for i in order], "created": c["created"][order], "contents": [c["contents"][i] for i in order], "dim": dim}
    lower = [P.text.lower_invariant(s) for s in c["contents"]]
    cl = P.RecallCluster([0, 0], dim)
    bounds = [0, n // 2, n]
    for g in range(2):
        r = bounds[g]
        while r < bounds[g + 1]:
            has = c["emb"][r] is not None
            e = r
            while e < bounds[g + 1] and (c["emb"][e] is not None) == has:
                e += 1
            emb = np.stack(c["emb"][r:e]).astype(np.float32) if has else None
            cl.shard(g).append(emb, c["created"][r:e], lower[r:e], row_ids=np.arange(r, e, dtype=np.int64))
            r = e
    cl.seal()
    qs = rng.standard_normal((6, dim)).astype(np.float32)
    plan = _plan(rng, c["emb"], dim, [0, n // 2 - 1, n // 2, n - 1], list(qs), 60)
    for g in range(2):
        part = {r: v for r, v in plan.items() if bounds[g] <= r < bounds[g + 1]}
        other = {r: v for r, v in plan.items() if not bounds[g] <= r < bounds[g + 1]}
        assert _apply(cl.shard(g), part, dim) == len(part)
        assert _apply(cl.shard(g), {r: v for r, v in list(other.items())[:3] if v is not None}, dim) == 0   # ids of the other shard
    corpus = orc.OracleCorpus(_updated(c["emb"], plan), c["created"], c["contents"])
    texts = [TEXTS[b % len(TEXTS)] for b in range(6)]
    terms = [P.text.query_terms(t) for t in texts]
    for topk, limit in ((10, n), (1, 300), (300, n)):
        rows, scores, counts = cl.search(qs, terms, NOW, topk, candidate_limit=limit)
        for b in range(6):
            orow, osc, _ = corpus.search(qs[b], texts[b], NOW, topk, candidate_limit=limit)
            assert list(rows[b, :counts[b]]) == list(orow), (topk, limit, b)
            assert np.array_equal(scores[b, :counts[b]], osc, equal_nan=True), (topk, limit, b)
    cl.close()
