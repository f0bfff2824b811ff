"""The cosine range search (orr_search_range_cosine): for each query EVERY live row whose reference cosine to it is at least the
query's own min_cosine, with that cosine, best first.

Membership and cosines are restated in numpy by tests/test_gpu_scope_near.py's Model.cos: float32 products accumulated strictly
in index order in float64, the reference's guards, dot / (sqrt(na) * sqrt(nb)).  test_the_restatement_is_the_oracles holds it
against oracle.cosine on every pair within 1e-6 of a threshold and on every planted row.  Every check of a call is exact
equality of ids, order, order keys, cosine BITS and totals (_check).

Shards (Gaussian rows, one seed each; built once, only read, except where a test builds its own):
    S1  20,000 x 128    screen and exact form
    S2   4,099 x 128    a partial last 256-row tile AND a partial last 128-row unit; screen and exact form
    S3  20,000 x 1024   screen and exact form; 9 distinct queries (a batch of 64 repeats them with 64 different thresholds, so the
                        restatement of a 1024-wide shard is computed 9 times, not 64)
    S4   4,099 x 70     the exact form only
Planted rows sit at positions 0, 127, 128, 255, 256, in the last full tile, in the partial tile and at the last row: copies of
query 0 (ties, ordered by position), 2 x and 0.5 x the query, a zero row, a row without an embedding, a row holding a NaN, one
holding an infinity, one with 0 < normB < 2^-96 and one whose squares overflow float.  Planted queries: a zero query, a query
holding a NaN and a tiny query (max|q| = 1e-20)."""
import threading

import numpy as np
import pytest

import test_gpu_scope_near as nbase
import test_gpu_scope_terms as tbase
from helpers import orc, pkg

pytestmark = pytest.mark.gpu

INF = float("inf")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
KINDS = ("double", "half", "zero", "none", "nan", "inf", "tiny", "huge")
SHAPES = {"S1": (20_000, 128), "S2": (4_099, 128), "S3": (20_000, 1024), "S4": (4_099, 70)}
BATCHES = (1, 3, 4, 5, 9, 64)
_stats = tbase._stats


def _anchors(n):
    full = (n // 256) * 256 - 256                       # the first row of the last full tile
    partial = [n // 256 * 256] if n % 256 else []       # the first row of the partial tile
    return [0, 127, 128, 255, 256, full + 5] + partial + [n - 1]


def _plant(emb, probe):
    """copies of the probe at the anchors; the eight other kinds beside the first anchors, in the last full tile and (as many as
    fit) in the partial tile.  Returns {position: kind}."""
    n = len(emb)
    planted = {a: "copy" for a in _anchors(n)}
    full = (n // 256) * 256 - 256
    free = [1, 126, 129, 254, 257, 2, 125, 130] + [full + 6 + k for k in range(8)] + [r for r in range(n // 256 * 256 + 1, n - 1)][:8]
    for j, r in enumerate(free):
        assert r not in planted
        planted[r] = KINDS[j % 8]
    for r, kind in planted.items():
        e = probe.copy()
        if kind == "double":
            e *= np.float32(2.0)
        elif kind == "half":
            e *= np.float32(0.5)
        elif kind in ("zero", "none"):
            e[:] = 0.0
        elif kind == "nan":
            e[3] = np.nan
        elif kind == "inf":
            e[len(e) // 2] = np.inf
        elif kind == "tiny":
            e[:] = np.where(e < 0, np.float32(-1e-18), np.float32(1e-18))   # normB = dim x 1e-36: positive, below 2^-96
        elif kind == "huge":
            e[:] = np.where(e < 0, np.float32(-1e30), np.float32(1e30))
        emb[r] = e
    return planted


def _build_shard(name, capacity=None):
    n, dim = SHAPES[name]
    rng = np.random.default_rng(1000 + dim + n)
    emb = rng.standard_normal((n, dim), dtype=np.float32)
    _, created, rowbytes = tbase._rows(n, 64)
    # 9 queries: query 0 is planted as rows; the others are a row plus noise, so that each has near rows of its own
    q = np.ascontiguousarray(emb[rng.choice(n, 9, replace=False)] + np.float32(0.35) * rng.standard_normal((9, dim), dtype=np.float32))
    planted = _plant(emb, q[0])
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    idx = tbase._build(emb, created, rowbytes, ids, capacity or n)
    none = sorted(r for r, k in planted.items() if k == "none")
    assert idx.update_rows(ids[none], None) == len(none)                    # rows without an embedding
    model = nbase.Model(emb, created, rowbytes, ids)
    special = {"zero": np.zeros(dim, np.float32), "nan": q[1].copy(), "tiny": (q[2] * np.float32(1e-20) / np.abs(q[2]).max()).astype(np.float32)}
    special["nan"][dim // 3] = np.nan
    assert 0.99e-20 < np.abs(special["tiny"]).max() < 1.01e-20
    return dict(name=name, idx=idx, model=model, q=q, planted=planted, n=n, dim=dim, ids=ids, special=special, screens=dim % 128 == 0)


_SHARDS = {}


def _shard(name):
    if name not in _SHARDS:
        _SHARDS[name] = _build_shard(name)
    return _SHARDS[name]


def _quantiles(s, p):
    """the 0.9 / 0.99 / 0.999 quantiles of the restated cosines of query p over the rows that were not planted"""
    key = ("quant", p.tobytes())
    if key not in s:
        c = s["model"].cos(p)
        ok = np.isfinite(c)
        ok[list(s["planted"])] = False
        s[key] = tuple(float(np.quantile(c[ok], x)) for x in (0.9, 0.99, 0.999))
    return s[key]


def _batch(s, B, wide=False):
    """B queries with a threshold each.  The planted queries stand inside the batch from 5 queries on (so the walked queries are
    NOT a prefix of the batch).  wide: the thresholds that keep (nearly) every row as well."""
    q = [s["q"][b % 9] for b in range(B)]
    if B >= 5:
        q[1], q[3] = s["special"]["zero"], s["special"]["nan"]
        q[B - 1] = s["special"]["tiny"]
    t = []
    for b in range(B):
        q90, q99, q999 = _quantiles(s, s["q"][b % 9])
        menu = (q99, q999, 1.0, 2.0, INF, q999, 0.5 * (q99 + q999)) + ((-INF, -1.0, 0.0, q90) if wide else ())
        t.append(menu[(b + b // 9) % len(menu)])
    if B >= 5 and wide:
        t[1] = 0.0                                      # the zero query at the threshold its cosines meet
    return np.ascontiguousarray(np.stack(q), np.float32), np.array(t, np.float64)


def _want(model, p, t, within=None, row_base=0):
    """(ids, order keys, cosines) of every hit of query p in order, restated"""
    c = model.cos(p)
    with np.errstate(invalid="ignore"):
        m = (c >= t) & ~model.dead
    if within is not None:
        m &= within
    rows = np.nonzero(m)[0]
    order = np.lexsort((rows, -c[rows]))                # cosine descending, then the position (-0 and +0 tie)
    rows = rows[order]
    return model.ids[rows], rows + row_base, c[rows]


def _check(got, model, q, t, max_hits, within=None, what=None, keys=True):
    ids, okeys, cos, totals = got
    assert len(ids) == len(okeys) == len(cos) == len(totals) == len(t)
    for b in range(len(t)):
        w_ids, w_keys, w_cos = _want(model, q[b], t[b], within)
        k = min(len(w_ids), max_hits)
        assert totals[b] == len(w_ids), (what, b, t[b], int(totals[b]), len(w_ids))
        assert np.array_equal(ids[b], w_ids[:k]), (what, b, t[b], ids[b][:8], w_ids[:8])
        if keys:
            assert np.array_equal(okeys[b], w_keys[:k]), (what, b)
        assert np.array_equal(cos[b].view(np.int64), w_cos[:k].view(np.int64)), (what, b, cos[b][:4], w_cos[:4])


def _form(idx, form):
    idx.set_option("range_form", form)


def _forms(s):
    return (1, 2) if s["screens"] else (2,)


def _both_forms(s, q, t, max_hits, within_of=None, what=None):
    """the call under "range_form" 1 and 2 (where the screen applies), each checked against the restatement, and bit for bit
    against each other"""
    outs = []
    for form in _forms(s):
        _form(s["idx"], form)
        try:
            sc, mask = within_of() if within_of else (None, None)
            got, st = _stats(s["idx"], lambda: s["idx"].range_cosine(q, t, max_hits, within=sc))
            if sc is not None:
                sc.close()
        finally:
            _form(s["idx"], 0)
        _check(got, s["model"], q, t, max_hits, within=mask, what=(what, form))
        walked = "screen_gemv_i8_range" if form == 1 else "range_dot_exact"
        other = "range_dot_exact" if form == 1 else "screen_gemv_i8_range"
        if form == 2:
            assert other not in st, (what, sorted(st))
        outs.append((got, st, walked))
    if len(outs) == 2:
        a, b = outs[0][0], outs[1][0]
        for x, y in zip(a[:3], b[:3]):
            assert all(np.array_equal(u.view(np.int64), v.view(np.int64)) for u, v in zip(x, y)), what
        assert np.array_equal(a[3], b[3]), what
    return outs


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES))
def test_the_restatement_is_the_oracles(name):
    s = _shard(name)
    model, planted = s["model"], s["planted"]
    assert set(planted.values()) == set(KINDS) | {"copy"} and all(a in planted for a in _anchors(s["n"]))
    emb_of = lambda r: None if planted.get(r) == "none" else model.emb[r]
    rng = np.random.default_rng(3)
    checked = 0
    for p in [s["q"][0], s["q"][4]] + list(s["special"].values()):
        c = model.cos(p)
        rows = set(planted) | set(rng.choice(s["n"], 100, replace=False).tolist())
        if p.any() and np.isfinite(p).all() and np.abs(p).max() > 1e-10:
            for t in _quantiles(s, p) + (1.0, 0.0):
                with np.errstate(invalid="ignore"):
                    rows |= set(np.nonzero(np.abs(c - t) <= 1e-6)[0].tolist())
        assert len(rows) < 2_000
        for r in rows:
            want = orc.cosine(p, emb_of(r))
            assert c[r] == want or (np.isnan(c[r]) and np.isnan(want)), (name, r, planted.get(r), c[r], want)
        checked += len(rows)
    assert checked > 500
    c0, one = model.cos(s["q"][0]), orc.cosine(s["q"][0], s["q"][0])
    for r, kind in planted.items():
        if kind == "copy":
            assert c0[r] == one
        elif kind in ("double", "half"):
            assert abs(c0[r] - 1.0) < 1e-15
        elif kind in ("zero", "none", "huge"):
            assert c0[r] == 0.0, (kind, c0[r])
        elif kind == "tiny":
            nb = float(nbase._exact_dots(model.emb[r][None, :], model.emb[r])[0])
            assert 0.0 < nb < 2.0 ** -96 and 0.5 < c0[r] < 1.0, (nb, c0[r])
        else:
            assert np.isnan(c0[r]), (kind, c0[r])


# ---- the call against the restatement, both forms ----------------------------------------------------------------------------

@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_hits_totals_order_and_cosine_bits(name, B):
    s = _shard(name)
    q, t = _batch(s, B)
    outs = _both_forms(s, q, t, 50, what=(name, B))
    got, st, _ = outs[0]
    assert sum(len(x) for x in got[0]) > 0                                  # the planted copies at least
    if s["screens"]:
        walked = B - (3 if B >= 5 else 0)                                   # the zero query walks nothing; the NaN and the tiny one go exact
        assert st["screen_gemv_i8_range"]["launches"] == -(-walked // 4), (st["screen_gemv_i8_range"], walked)
        assert st["range_rescore_exact"]["launches"] >= 1 and st["range_collect"]["launches"] >= 1
        assert ("range_dot_exact" in st) == (B >= 5)
    else:
        assert "screen_gemv_i8_range" not in st and st["range_dot_exact"]["launches"] == -(-(B - (1 if B >= 5 else 0)) // 8)


@pytest.mark.parametrize("name", ["S1", "S2", "S4"])
def test_wide_thresholds_with_the_pair_cap_raised_and_the_limit_at_a_low_cap(name):
    P = pkg()
    s = _shard(name)
    idx = s["idx"]
    q, t = _batch(s, 9, wide=True)
    idx.set_option("range_pair_cap", 1 << 22)
    try:
        for max_hits in (0, 1, 7, s["n"] + 5):
            _both_forms(s, q, t, max_hits, what=(name, "wide", max_hits))
    finally:
        idx.set_option("range_pair_cap", 1 << 20)
    # the same batch under a cap that the wide queries exceed: ORR_ELIMIT, no hits, an upper bound per query
    for form in _forms(s):
        idx.set_option("range_pair_cap", 500)
        _form(idx, form)
        try:
            with pytest.raises(P.OrrError) as e:
                idx.range_cosine(q, t, 7)
        finally:
            idx.set_option("range_pair_cap", 1 << 20)
            _form(idx, 0)
        assert e.value.code == P.native.ORR_ELIMIT == -7 and b"range_pair_cap" in P.native.hip.orr_last_error()
        upper = e.value.totals
        exact = np.array([len(_want(s["model"], q[b], t[b])[0]) for b in range(9)])
        assert (upper >= exact).all(), (form, upper, exact)
        # (the query holding a NaN keeps every pair for the host: a cosine that is not finite is never dropped on the device)
        selective = np.array([b not in (1, 3, 8) and exact[b] <= 100 for b in range(9)])
        assert (upper > 500).any() and selective.any() and (upper[selective] <= 500).all(), (form, upper, exact)
    # the default cap (1,048,576 pairs per query) is far above what a shard of this size can keep
    _check(idx.range_cosine(q, t, 7), s["model"], q, t, 7, what=(name, "default cap"))


@pytest.mark.parametrize("name", ["S1", "S4"])
def test_the_border_is_decided_as_the_oracle_decides_it(name):
    s = _shard(name)
    model, p = s["model"], s["q"][0]
    c = model.cos(p)
    natural = [r for r in np.argsort(-np.nan_to_num(c, nan=-9.0))[:40] if r not in s["planted"]][:3]
    rows = natural + [r for r, k in s["planted"].items() if k in ("copy", "double", "tiny")][:4]
    q, t = [], []
    for r in rows:
        at = orc.cosine(p, model.emb[r])
        assert at == c[r]
        q += [p, p]
        t += [at, float(np.nextafter(at, 9.0))]                             # at the row's own cosine it is in; one double above, out
    q, t = np.ascontiguousarray(np.stack(q)), np.array(t)
    outs = _both_forms(s, q, t, 40, what=(name, "border"))
    ids = outs[0][0][0]
    for j, r in enumerate(rows):
        assert model.ids[r] in ids[2 * j] and model.ids[r] not in ids[2 * j + 1], (name, r)


def test_ties_are_ordered_by_position():
    s = _shard("S1")
    one = orc.cosine(s["q"][0], s["q"][0])
    got = s["idx"].range_cosine(s["q"][:1], [one], 100)
    _check(got, s["model"], s["q"][:1], [one], 100, what="ties")
    copies = sorted(r for r, k in s["planted"].items() if k == "copy")
    tied = [int(k) for k, c in zip(got[1][0], got[2][0]) if c == one and int(k) in copies]
    assert len(copies) == 8 and tied == copies                             # equal cosines: the position decides


# ---- scopes, maintenance, views, threads, device queries ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S2", "S4"])
def test_within_an_id_scope_a_ticks_scope_a_cosine_scope_and_an_empty_scope(name):
    s = _shard(name)
    idx, model, n = s["idx"], s["model"], s["n"]
    q, t = _batch(s, 5, wide=True)
    rng = np.random.default_rng(5)
    some = np.zeros(n, bool)
    some[rng.choice(n, n // 3, replace=False)] = True
    some[list(s["planted"])] = True
    mid = int(model.created[n // 2])
    window = (model.created >= mid) & (model.created < I64_MAX)
    near = model.near_rows(s["q"][:1], 0.05, "all")
    cases = {"ids": (lambda: idx.scope(model.ids[some]), some), "ticks": (lambda: idx.scope_ticks(mid, I64_MAX), window),
             "near": (lambda: idx.scope_near(s["q"][:1], 0.05), near), "empty": (lambda: idx.scope(np.zeros(0, np.int64)), np.zeros(n, bool))}
    for what, (make, mask) in cases.items():
        outs = _both_forms(s, q, t, 30, within_of=lambda: (make(), mask), what=(name, what))
        if what == "empty":
            assert (outs[0][0][3] == 0).all() and "range_dot_exact" not in outs[0][1] and "screen_gemv_i8_range" not in outs[0][1]


def test_errors_that_need_a_handle():
    P = pkg()
    s, other = _shard("S2"), _shard("S4")
    q, t = _batch(s, 3)
    sc = other["idx"].scope(other["ids"][:10])
    with pytest.raises(P.OrrError) as e:
        s["idx"].range_cosine(q, t, 5, within=sc)
    assert e.value.code == P.native.ORR_EINVAL and b"another shard" in P.native.hip.orr_last_error()
    sc.close()
    idx = P.RecallIndex(dim=128, capacity_rows=16)
    with pytest.raises(P.OrrError) as e:
        idx.range_cosine(q, t, 5)
    assert e.value.code == P.native.ORR_ESTATE
    idx.close()
    for name, value in (("range_pair_cap", 0), ("range_pair_cap", (1 << 31) + 1), ("range_buffer", 0), ("range_buffer", 65535 * 64 + 1), ("range_form", 3)):
        with pytest.raises(P.OrrError) as e:
            s["idx"].set_option(name, value)
        assert e.value.code == P.native.ORR_EINVAL
    # B == 0 writes nothing; a foreign dim and dim 0 have cosine 0 with every row
    assert s["idx"].range_cosine(None, [], 5)[3].shape == (0,)
    for qq in (np.ones((2, 64), np.float32), None):
        got = s["idx"].range_cosine(qq, [0.0, 1e-9], 4)
        assert list(got[3]) == [s["n"], 0] and list(got[0][0]) == list(s["ids"][:4]) and (got[2][0] == 0.0).all() and len(got[0][1]) == 0


def test_deletes_compact_insert_and_update():
    name = "S2"
    s = _build_shard(name, capacity=SHAPES[name][0] + 600)
    idx, model, n, dim = s["idx"], s["model"], s["n"], s["dim"]
    q, t = _batch(s, 9, wide=True)                      # (with thresholds <= 0: a deleted row's norm is 0, its cosine 0)
    rng = np.random.default_rng(9)
    counted = lambda: {k: v for k, v in idx.search_stats().items() if k in ("searches", "queries", "passes", "requeried", "exact_pass_queries", "survivors_total")}
    stats0 = counted()
    gone = np.concatenate([model.ids[rng.choice(n, 300, replace=False)], model.ids[[0, 128]]])
    assert idx.delete_rows(gone) == len(np.unique(gone))
    model.delete(gone)
    _both_forms(s, q, t, 25, what="deleted")
    assert idx.compact() == int(model.dead.sum())
    model.compact()
    _both_forms(s, q, t, 25, what="compacted")
    emb2 = np.ascontiguousarray(np.concatenate([s["q"][:1], s["q"][4:5], rng.standard_normal((298, dim), dtype=np.float32)]))
    _, created2, bytes2 = tbase._rows(300, 64, row0=50_000, n_total=n)
    ids2 = np.arange(300, dtype=np.int64) + 10_000_000
    off = np.arange(301, dtype=np.int64) * tbase._syn().ROW_BYTES
    assert idx.insert_rows(emb2, created2, bytes2.reshape(-1), off, row_ids=ids2) == 300
    model.insert(emb2, created2, bytes2, ids2)
    outs = _both_forms(s, q, t, 25, what="inserted")
    assert 10_000_000 in outs[0][0][0][0]                                   # the inserted copy of query 0 is a hit of query 0
    upd = model.ids[[5, 300, 2000]]
    new = np.ascontiguousarray(np.stack([s["q"][0], s["q"][0] * np.float32(0.5), rng.standard_normal(dim, dtype=np.float32)]))
    assert idx.update_rows(upd, new) == 3
    model.update(upd, new)
    _both_forms(s, q, t, 25, what="updated")
    assert counted() == stats0 and stats0["searches"] == 0                  # no search statistic moved
    idx.close()


def test_a_view_four_threads_and_device_resident_queries():
    import torch
    s = _shard("S1")
    idx, model = s["idx"], s["model"]
    q, t = _batch(s, 9)
    first = idx.range_cosine(q, t, 20)                                      # (the shadow exists before the view and the lanes are made)
    _check(first, model, q, t, 20, what="first")
    view = idx.view()
    _check(view.range_cosine(q, t, 20), model, q, t, 20, what="view")
    view.close()
    dq = torch.from_numpy(q).cuda()
    _check(idx.range_cosine(dq, t, 20), model, q, t, 20, what="device queries")
    errors = []

    def work(i):
        try:
            qq, tt = _batch(s, (4, 5, 9, 3)[i])
            for _ in range(3):
                _check(idx.range_cosine(qq, tt, 20), model, qq, tt, 20, what=("thread", i))
        except Exception as e:                          # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


@pytest.mark.parametrize("form", [1, 2])
def test_growth_five_thousand_copies_through_buffers_of_sixteen(form):
    n, dim = 12_000, 128
    rng = np.random.default_rng(21)
    emb = rng.standard_normal((n, dim), dtype=np.float32)
    p = rng.standard_normal(dim, dtype=np.float32)
    rows = np.sort(rng.choice(n, 5_000, replace=False))
    emb[rows] = p
    _, created, rowbytes = tbase._rows(n, 64)
    ids = np.arange(n, dtype=np.int64) + 1
    idx = tbase._build(emb, created, rowbytes, ids, n)
    model = nbase.Model(emb, created, rowbytes, ids)
    q, t = np.ascontiguousarray(np.stack([p, emb[0], p])), np.array([orc.cosine(p, p), 0.9, 2.0])
    idx.set_option("range_buffer", 16)
    idx.set_option("range_form", form)
    got, st = _stats(idx, lambda: idx.range_cosine(q, t, 6_000))
    _check(got, model, q, t, 6_000, what=("growth", form))
    assert got[3][0] == 5_000 and np.array_equal(got[0][0], ids[rows])
    assert st["range_buffer_growths"]["algo_bytes"] >= 1.0, st                 # the buffers grew, and the launches ran again
    walked = "screen_gemv_i8_range" if form == 1 else "range_collect_dense"
    assert st[walked]["launches"] >= 2, st[walked]
    got, st = _stats(idx, lambda: idx.range_cosine(q, t, 6_000))             # the lane kept the grown size
    _check(got, model, q, t, 6_000, what=("grown", form))
    assert "range_buffer_growths" not in st and st[walked]["launches"] == 1
    idx.close()


# ---- the screen screens ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_the_screen_keeps_at_most_three_times_the_hits(name):
    """every threshold at the 0.99 quantile of its query's cosines: a numpy restatement of the bound gives 1.24 x the hits at
    dim 128 and 1.9 x at dim 1024 for these seeds"""
    s = _shard(name)
    rng = np.random.default_rng(77 + s["dim"])
    q = np.ascontiguousarray(np.concatenate([rng.standard_normal((4, s["dim"]), dtype=np.float32), s["q"][4:8]]))
    if name == "S3":
        q = np.ascontiguousarray(s["q"][:8])                                # (restated already)
    t = np.array([_quantiles(s, p)[1] for p in q])
    _form(s["idx"], 1)
    try:
        got, st = _stats(s["idx"], lambda: s["idx"].range_cosine(q, t, 10))
    finally:
        _form(s["idx"], 0)
    _check(got, s["model"], q, t, 10, what=(name, "0.99"))
    hits, survivors = int(got[3].sum()), st["range_screen_pairs"]["algo_bytes"] / 16.0
    print(f"{name}: {hits} hits, {survivors:.0f} survivors of the screen, {survivors / hits:.3f} x; the host decided "
          f"{st['range_host_pairs']['algo_bytes'] / 32.0:.0f} pairs")
    assert hits >= 0.009 * 8 * s["n"]
    assert hits <= survivors <= 3 * hits, (name, hits, survivors)
    assert st["screen_gemv_i8_range"]["launches"] == 2 and "range_dot_exact" not in st


# ---- the cluster form --------------------------------------------------------------------------------------------------------

def test_a_three_shard_cluster_answers_as_one_index_over_the_same_rows():
    P, syn = pkg(), tbase._syn()
    s = _shard("S2")
    model, n, dim = s["model"], s["n"], s["dim"]
    cuts = [0, 1_500, 2_900, n]
    cl = P.RecallCluster([0, 0, 0], dim)
    for g in range(3):
        r0, r1 = cuts[g], cuts[g + 1]
        off = np.arange(r1 - r0 + 1, dtype=np.int64) * syn.ROW_BYTES
        cl.shard(g).append(model.emb[r0:r1], model.created[r0:r1], model.rowbytes[r0:r1].reshape(-1), off, row_ids=model.ids[r0:r1])
    cl.seal()
    none = np.array(sorted(model.ids[r] for r, k in s["planted"].items() if k == "none"), np.int64)
    assert sum(cl.shard(g).update_rows(none, None) for g in range(3)) == len(none)
    q, t = _batch(s, 9, wide=True)
    one = s["idx"].range_cosine(q, t, 40)
    _check(one, model, q, t, 40, what="one index")
    for form in (1, 2):
        for g in range(3):
            cl.shard(g).set_option("range_form", form)
        got = cl.range_cosine(q, t, 40)
        for x, y in zip(got[:3], one[:3]):
            assert all(np.array_equal(u.view(np.int64), v.view(np.int64)) for u, v in zip(x, y)), form
        assert np.array_equal(got[3], one[3])
    # inside a cluster scope, and the limit of one shard is the call's
    some = np.zeros(n, bool)
    some[::3] = True
    some[list(s["planted"])] = True
    csc = cl.scope(model.ids[some])
    _check(cl.range_cosine(q, t, 40, within=csc), model, q, t, 40, within=some, what="cluster scope")
    csc.close()
    cl.shard(1).set_option("range_pair_cap", 200)
    with pytest.raises(P.OrrError) as e:
        cl.range_cosine(q, t, 40)
    assert e.value.code == P.native.ORR_ELIMIT
    exact = np.array([len(_want(model, q[b], t[b])[0]) for b in range(9)])
    assert (e.value.totals >= exact).all() and (e.value.totals > 200).any()
    import torch
    with pytest.raises(P.OrrError) as e:
        P.index._range_cosine(P.native.hip.orr_cluster_search_range_cosine, cl._h, torch.from_numpy(q).cuda(), t, 5, None, True)
    assert e.value.code == P.native.ORR_EINVAL and b"host memory" in P.native.hip.orr_last_error()
    cl.close()
