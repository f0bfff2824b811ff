"""The bulk cosine range search (orr_search_range_cosine_bulk): orr_search_range_cosine's answers for up to 1024 queries, the
walked queries screened by ONE pass of the int8 screening GEMM per launch group (screen_tile16_kernel with the RANGE ending)
where csrc/orr_range_bulk_plan.h sends them there.

Every check of a call is exact equality of ids, order, order keys, cosine BITS and totals against the numpy restatement
Model.cos (tests/test_gpu_scope_near.py), through tests/test_gpu_range_cosine.py's _want / _check; the planted rows and queries
are that file's.  test_the_restatement_is_the_oracles holds the restatement against oracle.cosine for THIS file's shards.

Shards (Gaussian rows, one seed each; built once, only read, except where a test builds its own):
    B1   4,099 x 512   17 row tiles, the last of 3 rows (448 is not a multiple of 128: 512 is the smallest dim the GEMM takes)
    B2  70,001 x 512   274 row tiles: more than one output tile per workgroup on 256 CUs, the last tile 113 rows
    B3   4,099 x 128   the GEMM does not apply: the bulk call answers through the stream
    B4   4,099 x 70    the exact form only
A batch repeats nine distinct queries with different thresholds (the restatement is computed nine times per shard); the zero,
NaN and tiny queries stand inside it, so of B >= 5 queries B - 3 are screened, one walks nothing and two take the exact form."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import test_gpu_range_cosine as rbase
import test_gpu_scope_near as nbase
import test_gpu_scope_terms as tbase
from helpers import orc, pkg

pytestmark = pytest.mark.gpu

INF = float("inf")
I64_MAX = (1 << 63) - 1
SHAPES = {"B1": (4_099, 512), "B2": (70_001, 512), "B3": (4_099, 128), "B4": (4_099, 70)}
GEMM, STREAM, EXACT = "screen_tile16_range", "screen_gemv_i8_range", "range_dot_exact"
_stats, _plant, _want, _check, _batch, _quantiles = tbase._stats, rbase._plant, rbase._want, rbase._check, rbase._batch, rbase._quantiles


def _build_shard(name, capacity=None):
    n, dim = SHAPES[name]
    rng = np.random.default_rng(5000 + dim + n)
    emb = rng.standard_normal((n, dim), dtype=np.float32)
    _, created, rowbytes = tbase._rows(n, 64)
    q = np.ascontiguousarray(emb[rng.choice(n, 9, replace=False)] + np.float32(0.35) * rng.standard_normal((9, dim), dtype=np.float32))
    planted = _plant(emb, q[0])
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    idx = tbase._build(emb, created, rowbytes, ids, capacity or n)
    none = sorted(r for r, k in planted.items() if k == "none")
    assert idx.update_rows(ids[none], None) == len(none)                    # rows without an embedding
    model = nbase.Model(emb, created, rowbytes, ids)
    special = {"zero": np.zeros(dim, np.float32), "nan": q[1].copy(), "tiny": (q[2] * np.float32(1e-20) / np.abs(q[2]).max()).astype(np.float32)}
    special["nan"][dim // 3] = np.nan
    return dict(name=name, idx=idx, model=model, q=q, planted=planted, n=n, dim=dim, ids=ids, special=special,
                screens=dim % 128 == 0, gemm=dim % 128 == 0 and dim // 64 > 6)


_SHARDS = {}


def _shard(name):
    if name not in _SHARDS:
        _SHARDS[name] = _build_shard(name)
    return _SHARDS[name]


class _options:
    """sticky options for the length of a with block, put back to their defaults behind it"""
    DEFAULTS = {"range_gemm": 0, "range_form": 0, "range_pair_cap": 1 << 20}

    def __init__(self, idx, **kw):
        self.idx, self.kw = idx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.idx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.idx.set_option(k, self.DEFAULTS[k])


def _same(a, b, what):
    for x, y in zip(a[:3], b[:3]):
        assert len(x) == len(y) and all(np.array_equal(u.view(np.int64), v.view(np.int64)) for u, v in zip(x, y)), what
    assert np.array_equal(a[3], b[3]), what


def _launches(st):
    return {k: v["launches"] for k, v in st.items() if v["launches"] > 0}


def _screened(B):
    return B - (3 if B >= 5 else 0)                     # the zero query walks nothing; the NaN and the tiny one go exact


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES))
def test_the_restatement_is_the_oracles(name):
    s = _shard(name)
    model, planted = s["model"], s["planted"]
    assert set(planted.values()) == set(rbase.KINDS) | {"copy"} and all(a in planted for a in rbase._anchors(s["n"]))
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


# ---- the call against the restatement: the rule, the GEMM, the stream, the exact form -----------------------------------------

CASES = [("B1", B) for B in (65, 128, 129, 256, 257, 300, 1024)] + [("B2", B) for B in (65, 128, 129, 256, 257, 300)]


@pytest.mark.parametrize("name,B", CASES)
def test_hits_totals_order_and_cosine_bits(name, B):
    s = _shard(name)
    idx = s["idx"]
    q, t = _batch(s, B)
    got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
    _check(got, s["model"], q, t, 50, what=(name, B))
    assert sum(len(x) for x in got[0]) > 0
    # option 0: the GEMM from 65 SCREENED queries up (B = 65 screens 62: the stream), one launch for the group
    if _screened(B) >= 65:
        assert st[GEMM]["launches"] == 1 and STREAM not in st, _launches(st)
    else:
        assert GEMM not in st and st[STREAM]["launches"] == -(-_screened(B) // 4), _launches(st)
    assert st[EXACT]["launches"] == 1 and st["range_rescore_exact"]["launches"] >= 1 and st["range_collect"]["launches"] >= 1
    # the GEMM wherever it applies, never, and the exact form for everything: bit for bit the same
    with _options(idx, range_gemm=1):
        g1, st1 = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
    assert st1[GEMM]["launches"] == 1 and STREAM not in st1, _launches(st1)
    with _options(idx, range_gemm=2):
        g2, st2 = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
    assert GEMM not in st2 and st2[STREAM]["launches"] == -(-_screened(B) // 4), _launches(st2)
    with _options(idx, range_gemm=1, range_form=2):
        g3, st3 = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
    assert GEMM not in st3 and STREAM not in st3 and st3[EXACT]["launches"] == -(-(B - 1) // 8), _launches(st3)
    for other in (g1, g2, g3):
        _same(got, other, (name, B))


@pytest.mark.parametrize("B", [1, 5, 64])
def test_a_partial_query_tile_through_the_gemm(B):
    s = _shard("B1")
    idx = s["idx"]
    q, t = _batch(s, B)
    with _options(idx, range_gemm=1):
        got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
    _check(got, s["model"], q, t, 50, what=("partial tile", B))
    assert st[GEMM]["launches"] == 1 and STREAM not in st, _launches(st)
    # under option 0 the bulk call launches what the old call launches, and answers the same
    bulk, st_bulk = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
    old, st_old = _stats(idx, lambda: idx.range_cosine(q, t, 50))
    assert _launches(st_bulk) == _launches(st_old) and GEMM not in st_bulk, (_launches(st_bulk), _launches(st_old))
    _same(got, bulk, B)
    _same(got, old, B)


@pytest.mark.parametrize("name", ["B3", "B4"])
def test_where_the_gemm_does_not_apply_the_stream_and_the_exact_form_answer(name):
    s = _shard(name)
    idx = s["idx"]
    B = 130
    q, t = _batch(s, B)
    for gemm in (0, 1):
        with _options(idx, range_gemm=gemm):
            got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
        _check(got, s["model"], q, t, 50, what=(name, gemm))
        assert GEMM not in st and "range_i8_tile_queries" not in st, _launches(st)
        if name == "B3":
            assert st[STREAM]["launches"] == -(-_screened(B) // 4) and st[EXACT]["launches"] == 1, _launches(st)
        else:
            assert STREAM not in st and st[EXACT]["launches"] == -(-(B - 1) // 8), _launches(st)
    # the same queries through the old call in slices of 64
    parts = [idx.range_cosine(q[a:a + 64], t[a:a + 64], 50) for a in range(0, B, 64)]
    sliced = tuple([x for p in parts for x in p[k]] for k in range(3)) + (np.concatenate([p[3] for p in parts]),)
    _same(got, sliced, name)


def test_the_old_entry_point_keeps_its_limit_on_a_live_handle():
    P = pkg()
    s = _shard("B1")
    q, t = _batch(s, 65)
    with pytest.raises(P.OrrError) as e:
        s["idx"].range_cosine(q, t, 5)
    assert e.value.code == P.native.ORR_EINVAL and b"0 .. 64" in P.native.hip.orr_last_error()
    with pytest.raises(P.OrrError) as e:
        s["idx"].set_option("range_gemm", 3)
    assert e.value.code == P.native.ORR_EINVAL
    assert s["idx"].range_cosine_bulk(None, [], 5)[3].shape == (0,)         # B == 0 writes nothing


# ---- the walk of the output tiles -------------------------------------------------------------------------------------------

def test_the_answers_do_not_depend_on_which_workgroup_gets_which_tile():
    """B1 with 8 workgroups: every one walks several output tiles and draws tickets (17 row tiles x 2 query tiles); B2's 274 row
    tiles under the default grid are walked in test_hits_totals_order_and_cosine_bits"""
    s = _shard("B1")
    idx = s["idx"]
    q, t = _batch(s, 300)
    ref, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
    assert st[GEMM]["launches"] == 1
    before = os.environ.get("ORR_SCREEN_GRID")
    os.environ["ORR_SCREEN_GRID"] = "8"
    try:
        got, st8 = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 50))
    finally:
        if before is None:
            del os.environ["ORR_SCREEN_GRID"]
        else:
            os.environ["ORR_SCREEN_GRID"] = before
    assert st8[GEMM]["launches"] == 1
    _check(got, s["model"], q, t, 50, what="grid 8")
    _same(ref, got, "grid 8")
    assert st8["range_screen_pairs"]["algo_bytes"] == st["range_screen_pairs"]["algo_bytes"]       # the same survivors


# ---- the border ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["B1", "B2"])
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
        q += [p, p, p]
        t += [at, float(np.nextafter(at, 9.0)), float(np.nextafter(at, -9.0))]     # at the row's cosine: in; one double above: out; one below: in
    q, t = np.ascontiguousarray(np.stack(q)), np.array(t)
    with _options(s["idx"], range_gemm=1):
        got, st = _stats(s["idx"], lambda: s["idx"].range_cosine_bulk(q, t, 40))
    assert st[GEMM]["launches"] == 1 and STREAM not in st
    _check(got, model, q, t, 40, what=(name, "border"))
    for j, r in enumerate(rows):
        assert model.ids[r] in got[0][3 * j] and model.ids[r] not in got[0][3 * j + 1] and model.ids[r] in got[0][3 * j + 2], (name, r)


# ---- scopes, maintenance, views, threads, device queries ---------------------------------------------------------------------

def test_within_an_id_scope_a_ticks_scope_a_cosine_scope_and_an_empty_scope():
    s = _shard("B1")
    idx, model, n = s["idx"], s["model"], s["n"]
    q, t = _batch(s, 70, wide=True)
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
        sc = make()
        got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 30, within=sc))
        with _options(idx, range_gemm=2):
            other = idx.range_cosine_bulk(q, t, 30, within=sc)
        sc.close()
        _check(got, model, q, t, 30, within=mask, what=what)
        _same(got, other, what)
        if what == "empty":
            assert (got[3] == 0).all() and GEMM not in st and STREAM not in st and EXACT not in st
        else:
            assert st[GEMM]["launches"] == 1 and STREAM not in st, (what, _launches(st))


def test_deletes_compact_insert_and_update():
    name = "B1"
    s = _build_shard(name, capacity=SHAPES[name][0] + 600)
    idx, model, n, dim = s["idx"], s["model"], s["n"], s["dim"]
    q, t = _batch(s, 70, wide=True)                     # (with thresholds <= 0: a deleted row's norm is 0, its cosine 0)
    rng = np.random.default_rng(9)

    def both(what):
        got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 25))
        assert st[GEMM]["launches"] == 1, (what, _launches(st))
        _check(got, model, q, t, 25, what=what)
        with _options(idx, range_gemm=2):
            _same(got, idx.range_cosine_bulk(q, t, 25), what)
        return got

    gone = np.concatenate([model.ids[rng.choice(n, 300, replace=False)], model.ids[[0, 128]]])
    assert idx.delete_rows(gone) == len(np.unique(gone))
    model.delete(gone)
    both("deleted")
    assert idx.compact() == int(model.dead.sum())
    model.compact()
    both("compacted")
    emb2 = np.ascontiguousarray(np.concatenate([s["q"][:1], s["q"][4:5], rng.standard_normal((298, dim), dtype=np.float32)]))
    _, created2, bytes2 = tbase._rows(300, 64, row0=50_000, n_total=n)
    ids2 = np.arange(300, dtype=np.int64) + 10_000_000
    off = np.arange(301, dtype=np.int64) * tbase._syn().ROW_BYTES
    assert idx.insert_rows(emb2, created2, bytes2.reshape(-1), off, row_ids=ids2) == 300
    model.insert(emb2, created2, bytes2, ids2)
    got = both("inserted")
    assert 10_000_000 in got[0][0]                                          # the inserted copy of query 0 is a hit of query 0
    upd = model.ids[[5, 300, 2000]]
    new = np.ascontiguousarray(np.stack([s["q"][0], s["q"][0] * np.float32(0.5), rng.standard_normal(dim, dtype=np.float32)]))
    assert idx.update_rows(upd, new) == 3
    model.update(upd, new)
    both("updated")
    idx.close()


def test_a_view_four_threads_and_device_resident_queries():
    import torch
    s = _shard("B1")
    idx, model = s["idx"], s["model"]
    q, t = _batch(s, 130)
    first = idx.range_cosine_bulk(q, t, 20)                                 # (the shadow exists before the view and the lanes are made)
    _check(first, model, q, t, 20, what="first")
    view = idx.view()
    got, st = _stats(view, lambda: view.range_cosine_bulk(q, t, 20))
    assert st[GEMM]["launches"] == 1
    _same(first, got, "view")
    view.close()
    _same(first, idx.range_cosine_bulk(torch.from_numpy(q).cuda(), t, 20), "device queries")
    errors = []

    def work(i):
        try:
            qq, tt = _batch(s, (70, 129, 257, 5)[i])
            want = None
            for _ in range(3):
                got = idx.range_cosine_bulk(qq, tt, 20)
                if want is None:
                    _check(got, model, qq, tt, 20, what=("thread", i))
                    want = got
                else:
                    _same(want, got, ("thread", i))
        except Exception as e:                          # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---- growth and limits --------------------------------------------------------------------------------------------------------

def test_growth_five_thousand_copies_through_buffers_of_sixteen():
    n, dim = 12_000, 512
    rng = np.random.default_rng(21)
    emb = rng.standard_normal((n, dim), dtype=np.float32)
    p = rng.standard_normal(dim, dtype=np.float32)
    rows = np.sort(rng.choice(n, 5_000, replace=False))
    emb[rows] = p
    _, created, rowbytes = tbase._rows(n, 64)
    ids = np.arange(n, dtype=np.int64) + 1
    idx = tbase._build(emb, created, rowbytes, ids, n)
    model = nbase.Model(emb, created, rowbytes, ids)
    B = 66
    q = np.ascontiguousarray(np.stack([(p, emb[0], p)[b % 3] for b in range(B)]))
    t = np.array([(orc.cosine(p, p), 0.9, 2.0)[b % 3] for b in range(B)])
    idx.set_option("range_buffer", 16)
    got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 6_000))
    _check(got, model, q, t, 6_000, what="growth")
    assert got[3][0] == 5_000 and np.array_equal(got[0][0], ids[rows])
    assert st["range_buffer_growths"]["algo_bytes"] >= 1.0, st                 # the buffers grew, and the launch group ran again
    assert st[GEMM]["launches"] == 2 and STREAM not in st, _launches(st)
    got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 6_000))        # the lane kept the grown size
    _check(got, model, q, t, 6_000, what="grown")
    assert "range_buffer_growths" not in st and st[GEMM]["launches"] == 1
    idx.close()


def test_wide_thresholds_with_the_pair_cap_raised_and_the_limit_at_a_low_cap():
    P = pkg()
    s = _shard("B1")
    idx = s["idx"]
    B = 70
    q, t = _batch(s, B, wide=True)
    with _options(idx, range_pair_cap=1 << 22):
        for max_hits in (0, 7, s["n"] + 5):
            got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, max_hits))
            _check(got, s["model"], q, t, max_hits, what=("wide", max_hits))
            assert st[GEMM]["launches"] >= 1 and STREAM not in st
    # the same batch under a cap that the wide queries exceed: ORR_ELIMIT, no hit written, an upper bound per query
    exact = np.array([len(_want(s["model"], q[b], t[b])[0]) for b in range(B)])
    hits = np.full((B, 7), 7, dtype=P.index.RANGE_HIT_DTYPE)
    n_out, totals = np.full(B, 7, np.int32), np.full(B, 7, np.int64)
    for gemm in (0, 2):
        with _options(idx, range_pair_cap=500, range_gemm=gemm):
            r = P.native.hip.orr_search_range_cosine_bulk(idx._h, B, s["dim"], q.ctypes.data, t.ctypes.data, None, 7, hits.ctypes.data,
                                                          n_out.ctypes.data, totals.ctypes.data)
        assert r == P.native.ORR_ELIMIT == -7 and b"range_pair_cap" in P.native.hip.orr_last_error()
        assert (n_out == 0).all() and (hits["row_id"] == 7).all() and (hits["cosine"] == 7).all()
        assert (totals >= exact).all() and (totals > 500).any(), (gemm, totals, exact)
        selective = np.array([b not in (1, 3, B - 1) and exact[b] <= 100 for b in range(B)])
        assert selective.any() and (totals[selective] <= 500).all(), (gemm, totals, exact)
    _check(idx.range_cosine_bulk(q, t, 7), s["model"], q, t, 7, what="default cap")


# ---- the screen screens -------------------------------------------------------------------------------------------------------

def _cos_bound(re, rh, qe):
    return (1.000001 * (re * 1.0000003 + qe * rh + 1.2e-7) + 1e-9) * (1.0 + 2.0 ** -40)


def _simulated_survivors(model, q, t):
    """the one-level int8 quantisation of orr_screen.hip and range::cos_bound in float64 numpy: the pairs the GEMM screen keeps"""
    emb = model.emb.astype(np.float64)
    with np.errstate(all="ignore"):
        se = (np.abs(model.emb).max(axis=1) / np.float32(127.0)).astype(np.float32)
        ok = np.isfinite(se) & (se > 0)
        inv = np.where(ok, np.float32(1.0) / np.where(ok, se, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        ie = np.clip(np.rint(model.emb * inv[:, None]), -127, 127)
        ie[~ok] = 0.0
        hat = se.astype(np.float64)[:, None] * ie
        nb = nbase._exact_dots(model.emb, model.emb)
        re = np.sqrt(((emb - hat) ** 2).sum(axis=1) / nb) * 1.000001
        rh = np.sqrt((hat ** 2).sum(axis=1) / nb) * 1.000001
    usable = ok & np.isfinite(re) & (nb >= 2.0 ** -96)           # the others are never screened out (rel_err = +inf) ...
    empty = nb == 0.0                                            # ... but for a zero row: cosine 0 and a bound of 1.2e-7
    kept = 0
    for p, tt in zip(q, t):
        s1 = np.float32(np.abs(p).max() / np.float32(127.0))
        a = np.clip(np.rint(p / s1), -127, 127)
        na = nbase._exact_dots(p[None, :], p)[0]
        qe1 = np.sqrt(((p.astype(np.float64) - float(s1) * a) ** 2).sum() * 1.000001) / np.sqrt(na)
        with np.errstate(all="ignore"):
            cos_hat = se.astype(np.float64) * float(s1) * (ie @ a) / (np.sqrt(na) * np.sqrt(nb))
            keep = ~(cos_hat + _cos_bound(re, rh, qe1) < tt)
        kept += int(np.where(empty, 0.0 + _cos_bound(0.0, 0.0, qe1) >= tt, keep | ~usable)[~model.dead].sum())
    return kept


@pytest.mark.parametrize("name", ["B1", "B2"])
def test_the_gemm_screen_keeps_at_most_four_times_the_hits(name):
    """every threshold at the 0.99 quantile of its query's cosines.  A condition that keeps a keep-everything screen from passing,
    not a measurement: a numpy simulation of the one-level quantisation and cos_bound on these shapes gives 2.1 - 2.6 x the hits,
    and is run here for the test's own inputs (below 3.5 x: the inputs leave the margin)."""
    s = _shard(name)
    idx = s["idx"]
    q = np.ascontiguousarray(s["q"][:8])
    t = np.array([_quantiles(s, p)[1] for p in q])
    with _options(idx, range_gemm=1):
        got, st = _stats(idx, lambda: idx.range_cosine_bulk(q, t, 10))
    _check(got, s["model"], q, t, 10, what=(name, "0.99"))
    hits, survivors = int(got[3].sum()), st["range_screen_pairs"]["algo_bytes"] / 16.0
    simulated = _simulated_survivors(s["model"], q, t)
    print(f"{name}: {hits} hits, {survivors:.0f} survivors of the GEMM screen, {survivors / hits:.3f} x; simulated {simulated}, "
          f"{simulated / hits:.3f} x; the host decided {st['range_host_pairs']['algo_bytes'] / 32.0:.0f} pairs")
    assert hits >= 0.009 * 8 * s["n"]
    assert simulated < 3.5 * hits, (name, hits, simulated)
    assert hits <= survivors <= 4 * hits, (name, hits, survivors)
    # ... and the kernel keeps what the simulation keeps: a screen that charged less than the bound (the row term dropped, the
    # two-level query error) would keep fewer.  The simulation differs from the kernel by the binary32 round-up of the two
    # relative norms (1e-6 of themselves) and the order of its sums: pairs within 1e-6 of the border, far below 2 % of the count.
    assert abs(survivors - simulated) <= 0.02 * simulated + 8, (name, survivors, simulated)
    assert st[GEMM]["launches"] == 1 and STREAM not in st and EXACT not in st


# ---- the cluster form --------------------------------------------------------------------------------------------------------

def test_a_three_shard_cluster_answers_as_one_index_over_the_same_rows():
    P, syn = pkg(), tbase._syn()
    s = _shard("B2")
    model, n, dim = s["model"], s["n"], s["dim"]
    cuts = [0, 20_000, 45_100, n]
    cl = P.RecallCluster([0, 0, 0], dim)
    for g in range(3):
        r0, r1 = cuts[g], cuts[g + 1]
        off = np.arange(r1 - r0 + 1, dtype=np.int64) * syn.ROW_BYTES
        cl.shard(g).append(model.emb[r0:r1], model.created[r0:r1], model.rowbytes[r0:r1].reshape(-1), off, row_ids=model.ids[r0:r1])
    cl.seal()
    none = np.array(sorted(model.ids[r] for r, k in s["planted"].items() if k == "none"), np.int64)
    assert sum(cl.shard(g).update_rows(none, None) for g in range(3)) == len(none)
    q, t = _batch(s, 130)
    one = s["idx"].range_cosine_bulk(q, t, 40)
    _check(one, model, q, t, 40, what="one index")
    for gemm in (0, 2):
        for g in range(3):
            cl.shard(g).set_option("range_gemm", gemm)
        _same(cl.range_cosine_bulk(q, t, 40), one, ("cluster", gemm))
    for g in range(3):
        cl.shard(g).set_option("range_gemm", 0)
    # inside a cluster scope, and the limit of one shard is the call's
    some = np.zeros(n, bool)
    some[::3] = True
    some[list(s["planted"])] = True
    csc = cl.scope(model.ids[some])
    _check(cl.range_cosine_bulk(q, t, 40, within=csc), model, q, t, 40, within=some, what="cluster scope")
    csc.close()
    cl.shard(1).set_option("range_pair_cap", 100)
    with pytest.raises(P.OrrError) as e:
        cl.range_cosine_bulk(q, t, 40)
    assert e.value.code == P.native.ORR_ELIMIT
    exact = np.array([len(_want(model, q[b], t[b])[0]) for b in range(len(t))])
    assert (e.value.totals >= exact).all() and (e.value.totals > 100).any()
    with pytest.raises(P.OrrError) as e:
        cl.range_cosine(q, t, 40)                                           # the old cluster call keeps its limit too
    assert e.value.code == P.native.ORR_EINVAL
    cl.close()
