"""Cosine scopes (orr_scope_create_near): the scope of the live rows whose reference cosine to all, or any, of up to 8 probes is
at least min_cosine.

Membership is restated here in numpy (Model.cos): products in float32, accumulated strictly in index order in float64
(np.add.accumulate, not np.sum, which adds pairwise), then the reference's guards and dot / (sqrt(na) * sqrt(nb)); `>=` with NaN
never in.  test_the_restatement_is_the_oracles holds the restatement itself against oracle.cosine on every pair within 1e-6 of
a threshold, on every planted row and on a few hundred random rows.  Every check of a scope is exact set equality: row_ids() is
the restated ids in candidate order.  Behind the handle nothing is new, so a search inside a cosine scope is compared array for
array with search_masked on the restated ids, and a stated subset with the oracle on that sub-corpus (the method and the
helpers of tests/test_gpu_scope_terms.py).

Shards: A 200,000 x 128 (the tiled walk; built once, only read), B 70,001 x 64 (rows % 64 != 0, a partial last word; built per
test that changes it), C 4,099 x 70 (the generic form).  Every shard carries planted rows -- exact copies of probe 0 at positions
0, 31, 32, 63, 64, in the last full word, at the first row of the partial last word and at the last row, and beside them 2 x
and 0.5 x the probe, a zero row, a row without an embedding, a row holding a NaN, one holding an infinity and one whose squares
overflow float."""
import threading

import numpy as np
import pytest

import test_gpu_scope_terms as tbase
from helpers import orc, pkg

pytestmark = pytest.mark.gpu

NA, DIM_A = 200_000, 128
NB, DIM_B = 70_001, 64
NC, DIM_C = 4_099, 70
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INF = float("inf")
KINDS = ("double", "half", "zero", "none", "nan", "inf", "huge")
_syn, _same, _equal, _stats = tbase._syn, tbase._same, tbase._equal, tbase._stats
_in_scope, _masked, _search, _terms = tbase._in_scope, tbase._masked, tbase._search, tbase._terms


def _exact_dots(E, p):
    """sum_i (double)fl32(E[r][i] * p[i]) for every row, in index order (RecallSearchService.cs:77-82)"""
    out = np.empty(len(E), np.float64)
    with np.errstate(all="ignore"):
        for a in range(0, len(E), 25_000):
            prod = E[a:a + 25_000] * (p[None, :] if p.ndim == 1 else p[a:a + 25_000])          # float32 products
            out[a:a + 25_000] = np.add.accumulate(prod.astype(np.float64), axis=1)[:, -1] if prod.shape[1] else 0.0
    return out


class Model(tbase.Model):
    """tests/test_gpu_scope_terms.py's model of a shard with the restatement of a cosine scope."""

    def __init__(self, emb, created, rowbytes, ids):
        super().__init__(emb, created, rowbytes, ids)
        self._cos = {}

    def _changed(self):
        super()._changed()
        self._cos = {}

    def cos(self, p):
        """CosineSimilarity(p, row) for every row (a row without an embedding is a zero row here: norm 0, cosine 0)"""
        p = np.ascontiguousarray(p, np.float32).reshape(-1)
        n = len(self.ids)
        if p.shape[0] == 0 or p.shape[0] != self.emb.shape[1]:
            return np.zeros(n)                                              # :71-72
        key = p.tobytes()
        if key not in self._cos:
            if "nb" not in self._cos:
                self._cos["nb"] = _exact_dots(self.emb, self.emb)
            nb, na = self._cos["nb"], _exact_dots(p[None, :], p)[0]
            dot = _exact_dots(self.emb, p)
            with np.errstate(all="ignore"):
                c = dot / (np.sqrt(na) * np.sqrt(nb))
                c[nb <= 0.0] = 0.0                                          # :84-85 (a NaN norm passes the guard, as in C#)
            if na <= 0.0:
                c = np.zeros(n)
            self._cos[key] = c
        return self._cos[key]

    def near_rows(self, probes, t, mode):
        n = len(self.ids)
        if len(probes) == 0:
            return np.zeros(n, bool)
        with np.errstate(invalid="ignore"):
            hits = [self.cos(p) >= t for p in probes]
        m = np.logical_and.reduce(hits) if mode == "all" else np.logical_or.reduce(hits)
        return m & ~self.dead

    def near_ids(self, probes, t, mode):
        return self.ids[self.near_rows(probes, t, mode)]

    def update(self, ids, emb):
        for i, e in zip(ids, emb):
            self.emb[int(np.nonzero(self.ids == i)[0][0])] = e
        self._changed()


def _anchors(n):
    full = (n // 32) * 32 - 32                          # the first row of the last full word
    partial = [n // 32 * 32] if n % 32 else []          # the first row of the partial last word
    return [0, 31, 32, 63, 64, full + 5] + partial + [n - 1]


def _plant(emb, probe):
    """copies of the probe at the anchors; the seven other kinds beside the first anchors, in the last full word and (as many as
    fit) in the partial last word.  Returns {position: kind}."""
    n = len(emb)
    planted = {a: "copy" for a in _anchors(n)}
    free = [1, 30, 33, 62, 65, 2, 29]
    full = (n // 32) * 32 - 32
    free += [full + 6 + k for k in range(7)]
    free += [r for r in range(n // 32 * 32 + 1, n - 1)][:7]
    for j, r in enumerate(free):
        assert r not in planted
        planted[r] = KINDS[j % 7]
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
        elif kind == "huge":
            e[:] = np.where(e < 0, np.float32(-1e30), np.float32(1e30))
        emb[r] = e
    return planted


def _probes(emb, n_rows, dim, seed):
    """8 probes: probe 0 is a row of the corpus, the others lie around it (so ALL of several is not empty, ANY not everything)"""
    rng = np.random.default_rng(seed)
    p0 = emb[n_rows // 3].copy()
    noise = rng.uniform(-1, 1, (7, dim)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([p0[None, :], p0[None, :] + np.float32(0.6) * noise]), np.float32)


def _shard(n, dim, capacity=None, seed=7):
    emb, created, rowbytes = tbase._rows(n, dim)
    probes = _probes(emb, n, dim, seed)
    planted = _plant(emb, probes[0])
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    idx = tbase._build(emb, created, rowbytes, ids, capacity or n)
    none = sorted(r for r, k in planted.items() if k == "none")
    assert idx.update_rows(ids[none], None) == len(none)                     # rows without an embedding
    model = Model(emb, created, rowbytes, ids)
    c0 = model.cos(probes[0])
    ok = np.isfinite(c0)
    ok[list(planted)] = False
    t10, t1000 = float(np.quantile(c0[ok], 0.9)), float(np.quantile(c0[ok], 0.999))   # about a tenth and a thousandth of the rows
    q, texts = tbase._queries(dim, n)
    return dict(idx=idx, model=model, probes=probes, planted=planted, t10=t10, t1000=t1000, q=q, texts=texts, n=n, dim=dim,
                words=((n + 31) // 32 + 3) // 4 * 4)


_A = {}


def _shard_a():
    if not _A:
        _A.update(_shard(NA, DIM_A))
        _A["idx"].set_option("two_stage", 1)
        _search(_A["idx"], _A["q"][:8], _A["texts"][:8], 10, NA)            # the shadows of the screening pass exist
    return _A


_C = {}


def _shard_c():
    if not _C:
        _C.update(_shard(NC, DIM_C))
    return _C


_B = {}


def _shard_b_shared():
    """shard B for the tests that only read it"""
    if not _B:
        _B.update(_shard(NB, DIM_B))
    return _B


def _thresholds(s):
    return (-INF, -1.0, 0.0, s["t10"], s["t1000"], 1.0, 2.0, INF)


def _check(sc, model, probes, t, mode, what=None):
    want = model.near_ids(probes, t, mode)
    assert sc.rows == len(want), (what, t, mode, sc.rows, len(want))
    assert np.array_equal(sc.row_ids(), want), (what, t, mode)
    return want


def _walk_bytes(s):
    return 4.0 * s["n"] * s["dim"] + 8.0 * s["n"] + 4.0 * s["words"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shard", ["A", "B", "C"])
def test_the_restatement_is_the_oracles(shard):
    s = {"A": _shard_a, "B": _shard_b_shared, "C": _shard_c}[shard]()
    model, probes, planted = s["model"], s["probes"], s["planted"]
    rng = np.random.default_rng(3)
    kinds = set(planted.values())
    assert kinds == set(KINDS) | {"copy"} and all(a in planted for a in _anchors(s["n"]))
    emb_of = lambda r: None if planted.get(r) == "none" else model.emb[r]
    checked = 0
    for p in list(probes[:3]) + [np.zeros(s["dim"], np.float32)]:
        c = model.cos(p)
        rows = set(planted) | set(rng.choice(s["n"], 300, replace=False).tolist())
        for t in _thresholds(s):
            if np.isfinite(t):
                with np.errstate(invalid="ignore"):
                    rows |= set(np.nonzero(np.abs(c - t) <= 1e-6)[0].tolist())
        assert len(rows) < 5_000 or not p.any()                              # (the zero probe: cosine 0 with EVERY row, all of them at the threshold 0)
        for r in rows:
            want = orc.cosine(p, emb_of(r))
            assert c[r] == want or (np.isnan(c[r]) and np.isnan(want)), (shard, r, planted.get(r), c[r], want)
        checked += len(rows)
    assert checked > 1200
    # what the planted kinds are worth against probe 0
    c0, one = model.cos(probes[0]), orc.cosine(probes[0], probes[0])
    assert abs(one - 1.0) < 1e-15
    for r, kind in planted.items():
        if kind in ("copy",):
            assert c0[r] == one
        elif kind in ("double", "half"):
            assert abs(c0[r] - 1.0) < 1e-15
        elif kind in ("zero", "none", "huge"):
            assert c0[r] == 0.0, (kind, c0[r])
        else:
            assert np.isnan(c0[r]), (kind, c0[r])
    natural = np.ones(s["n"], bool)
    natural[list(planted)] = False
    with np.errstate(invalid="ignore"):
        assert 0.08 * s["n"] < (c0[natural] >= s["t10"]).sum() < 0.12 * s["n"]
        assert 0.0005 * s["n"] < (c0[natural] >= s["t1000"]).sum() < 0.002 * s["n"]


# ---- membership --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["all", "any"])
@pytest.mark.parametrize("n_probes", [1, 2, 8])
def test_membership_on_the_tiled_walk(n_probes, mode):
    a = _shard_a()
    idx, model, probes = a["idx"], a["model"], a["probes"][:n_probes]
    for t in _thresholds(a):
        sc, st = _stats(idx, lambda: idx.scope_near(probes, t, mode))
        want = _check(sc, model, probes, t, mode, n_probes)
        sc.close()
        assert st["scope_near"]["launches"] == 1 and st["scope_near"]["algo_bytes"] == _walk_bytes(a), st["scope_near"]
        assert st["scope_near_probe_norms"]["launches"] == 1
        if t == -INF:
            nan_rows = sum(k in ("nan", "inf") for k in a["planted"].values())
            assert len(want) == NA - nan_rows                                 # a NaN cosine is never >= anything
        if t in (2.0, INF):
            assert len(want) == 0
        if t == 1.0 and mode == "any":                                        # the copies: their cosine IS oracle.cosine(p, p), 1 to an ulp
            assert np.isin(model.ids[_anchors(NA)], want).all() == (orc.cosine(probes[0], probes[0]) >= 1.0)


def test_membership_special_probes():
    a = _shard_a()
    idx, model, probes = a["idx"], a["model"], a["probes"]
    zero = np.zeros((1, DIM_A), np.float32)
    live = model.ids[~model.dead]
    for mode in ("all", "any"):
        for t in (-INF, 0.0, a["t10"], INF):
            # the same probe twice counts once
            twice = np.stack([probes[1], probes[1]])
            sc = idx.scope_near(twice, t, mode)
            assert np.array_equal(_check(sc, model, twice, t, mode, "twice"), model.near_ids(probes[1:2], t, mode))
            sc.close()
            # a zero probe: norm 0, cosine 0 with every row
            sc = idx.scope_near(zero, t, mode)
            assert np.array_equal(_check(sc, model, zero, t, mode, "zero"), live if t <= 0 else live[:0])
            sc.close()
            with_zero = np.concatenate([probes[:2], zero])
            sc = idx.scope_near(with_zero, t, mode)
            _check(sc, model, with_zero, t, mode, "a zero probe among others")
            sc.close()
            # dim 0 and a foreign dim: cosine 0 everywhere, all rows or none, and NO walk
            for foreign in (np.zeros((3, 0), np.float32), np.ones((2, 64), np.float32), np.ones((1, 256), np.float32)):
                sc, st = _stats(idx, lambda: idx.scope_near(foreign, t, mode))
                assert np.array_equal(sc.row_ids(), live if t <= 0 else live[:0]) and sc.rows == (NA if t <= 0 else 0)
                assert "scope_near" not in st and "scope_near_probe_norms" not in st and st["scope_fill_range"]["launches"] == 1, sorted(st)
                sc.close()
            # no probes: the empty scope in both modes, nothing launched
            for none in (None, np.zeros((0, DIM_A), np.float32), []):
                sc, st = _stats(idx, lambda: idx.scope_near(none, t, mode))
                assert sc.rows == 0 and len(sc.row_ids()) == 0 and "scope_near" not in st and "scope_fill_range" not in st
                sc.close()
    # probes in device memory
    import torch
    dev = torch.from_numpy(probes[:3]).to("cuda:0")
    sc = idx.scope_near(dev, a["t10"], "any")
    _check(sc, model, probes[:3], a["t10"], "any", "device probes")
    sc.close()
    P = pkg()
    with pytest.raises(P.native.OrrError) as e:                               # 9 probes: refused
        idx.scope_near(np.ones((9, DIM_A), np.float32), 0.5, "any")
    assert e.value.code == P.native.ORR_EINVAL
    with pytest.raises(P.native.OrrError) as e:
        idx.scope_near(probes[:1], float("nan"), "any")
    assert e.value.code == P.native.ORR_EINVAL
    with pytest.raises(ValueError):
        idx.scope_near(probes[:1], 0.5, "both")


@pytest.mark.parametrize("shard", ["B", "C"])
def test_membership_with_a_partial_last_word_and_on_the_generic_form(shard):
    s = {"B": _shard_b_shared, "C": _shard_c}[shard]()
    idx, model, planted = s["idx"], s["model"], s["planted"]
    n = s["n"]
    assert n % 64 != 0 and n % 32 != 0 and (s["dim"] % 64 == 0) == (shard == "B")
    for n_probes in (1, 3, 8):
        probes = s["probes"][:n_probes]
        for mode in ("all", "any"):
            for t in _thresholds(s):
                sc, st = _stats(idx, lambda: idx.scope_near(probes, t, mode))
                want = _check(sc, model, probes, t, mode, (shard, n_probes))   # rows() counts every set bit: tail and padding are clear
                sc.close()
                assert st["scope_near"]["launches"] == 1 and st["scope_near"]["algo_bytes"] == _walk_bytes(s)
                if t in (-INF, -1.0, 0.0) and n_probes == 1:
                    out = [r for r, k in planted.items() if k in ("nan", "inf")]
                    assert model.ids[n - 1] in want and not np.isin(model.ids[out], want).any()
                    if t == 0.0:                                              # cosine 0 >= 0: the zero row, the row without an embedding
                        assert np.isin(model.ids[[r for r, k in planted.items() if k in ("zero", "none", "huge")]], want).all()


@pytest.mark.parametrize("shard", ["A", "B", "C"])
def test_the_border(shard):
    """min_cosine = oracle.cosine(probe, probe): every copy is in; the next double above it: every copy is out -- and both scopes
    are the restatement's.  The device does not decide these pairs: they go through the band list to the host."""
    s = {"A": _shard_a, "B": _shard_b_shared, "C": _shard_c}[shard]()
    idx, model, p = s["idx"], s["model"], s["probes"][:1]
    copies = model.ids[[r for r, k in s["planted"].items() if k == "copy"] + [s["n"] // 3]]       # the planted ones and the row the probe came from
    t = orc.cosine(p[0], p[0])
    for mode in ("all", "any"):
        sc, st = _stats(idx, lambda: idx.scope_near(p, t, mode))
        want = _check(sc, model, p, t, mode, "at the border")
        assert np.isin(copies, want).all() and len(want) < 40
        assert st["scope_near_band_pairs"]["algo_bytes"] >= 16.0 * len(copies)
        sc.close()
        up = float(np.nextafter(t, 2.0))
        sc = idx.scope_near(p, up, mode)
        want = _check(sc, model, p, up, mode, "one above the border")
        assert not np.isin(copies, want).any()
        sc.close()
    # two probes, ALL: a copy of probe 0 is at the border of probe 0 and far inside or outside for probe 1
    two = s["probes"][:2]
    for t2 in (t, float(np.nextafter(t, 2.0)), float(np.nextafter(t, -2.0))):
        for mode in ("all", "any"):
            sc = idx.scope_near(two, t2, mode)
            _check(sc, model, two, t2, mode, "two probes at the border")
            sc.close()


def _with_copies(n_copies, cap):
    """a 70,001 x 64 shard on one lane with n_copies copies of the probe at random positions"""
    emb, created, rowbytes = tbase._rows(NB, DIM_B)
    probes = _probes(emb, NB, DIM_B, 7)
    rng = np.random.default_rng(19)
    at = np.sort(rng.choice(NB, n_copies, replace=False))
    emb[at] = probes[0]
    emb[NB - 1] = probes[0]
    ids = np.arange(NB, dtype=np.int64) * 3 + 11
    idx = tbase._build(emb, created, rowbytes, ids, NB)
    idx.set_option("max_lanes", 1)                      # every call uses the index's own band list
    idx.set_option("near_band_cap", cap)
    return idx, Model(emb, created, rowbytes, ids), probes, at


def test_band_list_overflow_grows_the_list_and_walks_again():
    idx, model, probes, at = _with_copies(5_000, 16)
    p = probes[:1]
    t = orc.cosine(p[0], p[0])
    idx.reset_search_stats()
    sc, st = _stats(idx, lambda: idx.scope_near(p, t, "all"))
    want = _check(sc, model, p, t, "all", "5,000 copies")                     # never a scope of a truncated list
    assert len(want) >= 5_000 and np.isin(model.ids[at], want).all()
    assert st["scope_near"]["launches"] == 2, st["scope_near"]                # the second walk
    assert st["scope_near_band_pairs"]["algo_bytes"] >= 16.0 * 5_000
    ss = idx.search_stats()
    assert ss["searches"] == 0 and ss["passes"] == 0 and ss["queries"] == 0   # no search statistic moved
    up = float(np.nextafter(t, 2.0))                                          # the same band, every copy decided OUT by the host
    out, st = _stats(idx, lambda: idx.scope_near(p, up, "all"))
    assert st["scope_near"]["launches"] == 1, st["scope_near"]                # the list has grown and stays grown
    assert st["scope_near_fixup"]["launches"] == 1
    _check(out, model, p, up, "all", "5,000 copies, one above")
    assert not np.isin(model.ids[at], out.row_ids()).any()
    # two probes: a pending row lists only its band pairs; ANY with a far probe that holds settles the row on the device
    for mode in ("all", "any"):
        for tt in (t, up):
            both = idx.scope_near(probes[:2], tt, mode)
            _check(both, model, probes[:2], tt, mode, "two probes, 5,000 copies")
            both.close()
    with pytest.raises(pkg().native.OrrError):
        idx.set_option("near_band_cap", 0)
    sc.close()
    out.close()
    idx.close()


# ---- use ---------------------------------------------------------------------------------------------------------------------

def _against_oracle(model, ids, got, q, texts, topk, limit, checked, what):
    tbase._against_oracle(model, ids, got, q, texts, topk, limit, checked, what)


@pytest.mark.parametrize("B", [1, 8, 40])
def test_search_in_a_cosine_scope_equals_search_masked_and_the_oracle(B):
    a = _shard_a()
    idx, model, probes = a["idx"], a["model"], a["probes"]
    q, texts = a["q"][:B], a["texts"][:B]
    large, small = idx.scope_near(probes[:4], 0.005, "any"), idx.scope_near(probes[:1], a["t1000"], "all")
    ids_large, ids_small = _check(large, model, probes[:4], 0.005, "any"), _check(small, model, probes[:1], a["t1000"], "all")
    assert len(ids_large) > NA // 2 and 50 < len(ids_small) < 1000
    try:
        for screen, sc, ids, what in ((1, large, ids_large, "large ANY"), (2, small, ids_small, "small ALL")):
            idx.set_option("mask_screen", screen)
            for topk in (1, 10, 64):
                for limit in (300, NA):
                    got = _in_scope(idx, q, texts, topk, limit, sc)
                    idx.reset_search_stats()
                    want = _masked(idx, q, texts, topk, limit, ids)
                    mode = idx.search_stats()["pass_mode"]
                    assert _equal(got, want), (what, B, topk, limit)
                    if screen == 1 and topk == 10 and limit == NA:
                        assert mode == 5, (what, B, mode)                  # the masked screen did run
                        _against_oracle(model, ids, got, q, texts, topk, limit, (0, B - 1) if B > 1 else (0,), what)
                    if screen == 2:
                        assert mode == 4, (what, B, topk, limit, mode)
                        if topk == 10:
                            _against_oracle(model, ids, got, q, texts, topk, limit, range(min(B, 8)), what)
    finally:
        idx.set_option("mask_screen", 0)
        large.close()
        small.close()


def test_one_grouped_call_with_a_cosine_a_term_an_id_scope_and_a_window():
    a = _shard_a()
    idx, model, probes = a["idx"], a["model"], a["probes"]
    B = 40
    q, texts = a["q"][:B], a["texts"][:B]
    rng = np.random.default_rng(91)
    listed = model.ids[np.sort(rng.choice(NA, 20_000, replace=False))]
    word = _syn().vocab_word(1500)
    t0, t1 = int(model.created[150_000]), int(model.created[20_000])
    scopes = [idx.scope_near(probes[:4], 0.005, "any"), idx.scope_terms([word, tbase.FRAG], "any"), idx.scope(listed), idx.scope_ticks(t0, t1),
              idx.scope_near(probes[:3], a["t10"], "all")]
    window = model.ids[(model.created >= t0) & (model.created < t1) & ~model.dead]
    ids = [model.near_ids(probes[:4], 0.005, "any"), model.term_ids([word, tbase.FRAG], "any"), listed, window, model.near_ids(probes[:3], a["t10"], "all")]
    assert [s.rows for s in scopes] == [len(i) for i in ids]
    qs = np.arange(B, dtype=np.int32) % 5
    idx.set_option("mask_screen", 1)
    try:
        idx.reset_search_stats()
        rows, scores, counts = idx.search_in_scopes(q, _terms(texts), _syn().NOW_TICKS, 10, scopes, qs, candidate_limit=NA)
        assert idx.search_stats()["pass_mode"] == 6                        # ONE grouped screening pass
        for g in range(5):
            members = np.nonzero(qs == g)[0]
            own = _in_scope(idx, q[members], [texts[b] for b in members], 10, NA, scopes[g])
            assert _equal((rows[members], scores[members], counts[members]), own), g
            assert _equal(own, _masked(idx, q[members], [texts[b] for b in members], 10, NA, ids[g])), g
    finally:
        idx.set_option("mask_screen", 0)
        for s in scopes:
            s.close()


def test_combine_with_cosine_scopes_and_the_search_statistics():
    a = _shard_a()
    idx, model, probes, t = a["idx"], a["model"], a["probes"], a["t10"]
    idx.reset_search_stats()
    # "everything but the rows close to X": all rows ANDNOT the cosine scope
    far = idx.scope_ticks(I64_MIN, I64_MAX)
    close = idx.scope_near(probes[:2], t, "any")
    far.andnot(close)
    held = ~model.near_rows(probes[:2], t, "any") & ~model.dead
    assert 0 < held.sum() < NA and np.array_equal(far.row_ids(), model.ids[held]) and far.rows + close.rows == NA
    # ALL(a, b) == ALL(a) AND ALL(b); ANY(a, b) == ANY(a) OR ANY(b): how a caller folds more than 8 probes
    for x, y in ((probes[:1], probes[1:2]), (probes[:4], probes[4:])):
        xy = np.concatenate([x, y])
        both_all, both_any = idx.scope_near(xy, t, "all"), idx.scope_near(xy, t, "any")
        sx, sy = idx.scope_near(x, t, "all"), idx.scope_near(y, t, "all")
        sx.and_(sy)
        assert np.array_equal(both_all.row_ids(), sx.row_ids()) and np.array_equal(sx.row_ids(), model.near_ids(xy, t, "all"))
        ox, oy = idx.scope_near(x, t, "any"), idx.scope_near(y, t, "any")
        ox.or_(oy)
        assert np.array_equal(both_any.row_ids(), ox.row_ids()) and np.array_equal(ox.row_ids(), model.near_ids(xy, t, "any"))
        for s in (both_all, both_any, sx, sy, ox, oy):
            s.close()
    # a topic filter inside a tenant: a cosine scope AND an id scope
    rng = np.random.default_rng(5)
    tenant_ids = model.ids[np.sort(rng.choice(NA, 60_000, replace=False))]
    tenant = idx.scope(tenant_ids)
    tenant.and_(close)
    assert np.array_equal(tenant.row_ids(), model.ids[model.near_rows(probes[:2], t, "any") & np.isin(model.ids, tenant_ids)])
    for s in (far, close, tenant):
        s.close()
    ss = idx.search_stats()
    assert ss["searches"] == 0 and ss["passes"] == 0 and ss["queries"] == 0 and ss["kw_passes"] == 0      # orr_index_search_stats did not move


# ---- maintenance -------------------------------------------------------------------------------------------------------------

def test_maintenance_carries_a_cosine_scope():
    s = _shard(NB, DIM_B, capacity=NB + 1000)
    idx, model, probes, q, texts = s["idx"], s["model"], s["probes"], s["q"][:8], s["texts"][:8]
    rng = np.random.default_rng(35)
    one = orc.cosine(probes[0], probes[0])
    made = {"tenth": (probes[:1], s["t10"], "all"), "copies": (probes[:1], one, "all"), "any of three": (probes[:3], s["t1000"], "any"),
            "not negative": (probes[:2], 0.0, "all")}
    scopes = {k: idx.scope_near(*v) for k, v in made.items()}
    sets = {k: set(model.near_ids(*v).tolist()) for k, v in made.items()}
    assert len(sets["tenth"]) > 5000 and 8 <= len(sets["copies"]) < 40

    def check(what):
        for k, sc in scopes.items():
            want = model.ordered(sets[k])               # the rows that were in it and are still alive, in present order
            assert sc.rows == len(want) and np.array_equal(sc.row_ids(), want), (what, k)

    check("made")
    # delete members and non-members (copies at both ends among them): the deleted rows leave the scope
    members = np.fromiter(sets["tenth"], np.int64)
    gone = np.unique(np.concatenate([members[:150], model.ids[[0, 64, NB - 1]], rng.choice(model.ids, 400, replace=False)]))
    assert idx.delete_rows(gone) == len(gone)
    model.delete(gone)
    check("deleted")
    # a scope made behind deletes holds no deleted row: the walk still reads them
    for k, v in made.items():
        fresh = idx.scope_near(*v)
        got = _check(fresh, model, *v, ("behind deletes", k))
        assert not np.isin(gone, got).any() and fresh.rows == scopes[k].rows
        fresh.close()
    # compact after 9,000 deletes in all
    more = rng.choice(model.ids[~model.dead], 9_000 - len(gone), replace=False)
    assert idx.delete_rows(more) == len(more)
    model.delete(more)
    check("deleted more")
    assert idx.compact() == 9_000
    model.compact()
    check("compacted")
    for k, v in made.items():
        fresh = idx.scope_near(*v)
        _check(fresh, model, *v, ("after compaction", k))
        fresh.close()
    # insert 131 copies of the probe: NOT in the old scopes; a new scope holds them
    _, _, rowbytes = tbase._rows(131, DIM_B, row0=5_000_000)
    emb = np.repeat(probes[:1], 131, axis=0)
    c = model.created
    mid = c[rng.choice(len(c), 51, replace=False)].copy()
    mid[::2] -= 3
    created = np.concatenate([c[0] + 1 + np.arange(40), mid, c[-1] - 1 - np.arange(40)]).astype(np.int64)
    new_ids = 10_000_000 + np.arange(131, dtype=np.int64)
    width = rowbytes.shape[1]
    assert idx.insert_rows(emb, created, rowbytes.reshape(-1), np.arange(132, dtype=np.uint64) * width, row_ids=new_ids) == 131
    model.insert(emb, created, rowbytes, new_ids)
    check("inserted")
    for k, sc in scopes.items():
        assert not np.isin(new_ids, sc.row_ids()).any(), k
    for k in ("tenth", "copies"):
        new = idx.scope_near(*made[k])
        got = _check(new, model, *made[k], ("made after the insert", k))
        assert np.isin(new_ids, got).all() and len(got) == len(model.ordered(sets[k])) + 131, k
        if k == "tenth":                                # ... and it is searched like any other, against the oracle
            _against_oracle(model, got, _in_scope(idx, q, texts, 10, NB + 1000, new), q, texts, 10, NB + 1000, (0, 5), k)
        new.close()
    # update_rows of scoped rows to vectors far from the probe: the old scope is unchanged, a new one is without them
    before = {k: sc.row_ids() for k, sc in scopes.items()}
    moved = before["tenth"][:: len(before["tenth"]) // 60][:50]
    away = np.ascontiguousarray(np.repeat(-probes[:1], len(moved), axis=0))
    assert idx.update_rows(moved, away) == len(moved)
    model.update(moved, away)
    for k, sc in scopes.items():
        assert np.array_equal(sc.row_ids(), before[k]), k
    new = idx.scope_near(*made["tenth"])
    got = _check(new, model, *made["tenth"], "made after the update")
    assert not np.isin(moved, got).any()
    new.close()
    got = _in_scope(idx, q, texts, 10, NB + 1000, scopes["tenth"])
    assert _equal(got, _masked(idx, q, texts, 10, NB + 1000, before["tenth"]))
    for sc in scopes.values():
        sc.close()
    idx.close()


# ---- handles and threads -----------------------------------------------------------------------------------------------------

def test_views_orphans_and_an_unsealed_index():
    P = pkg()
    s = _shard(NB, DIM_B)
    idx, model, probes, q, texts = s["idx"], s["model"], s["probes"], s["q"][:8], s["texts"][:8]
    args = (probes[:2], s["t10"], "any")
    want_ids = model.near_ids(*args)
    view = idx.view()
    on_owner, on_view = idx.scope_near(*args), view.scope_near(*args)
    assert np.array_equal(on_view.row_ids(), want_ids) and np.array_equal(on_owner.row_ids(), want_ids)
    want = _masked(idx, q, texts, 10, NB, want_ids)
    for handle, sc in ((idx, on_view), (view, on_owner), (view, on_view), (idx, on_owner)):
        assert _equal(_in_scope(handle, q, texts, 10, NB, sc), want)
    on_view.close()
    view.close()
    idx.close()                                         # the index goes first: the scope is orphaned
    assert on_owner.rows == -1
    for call in (lambda: on_owner.row_ids(), lambda: on_owner.and_(on_owner)):
        with pytest.raises(P.native.OrrError) as e:
            call()
        assert e.value.code == P.native.ORR_ESTATE
    on_owner.close()
    # an index that is not sealed: ORR_ESTATE, after every argument error
    emb, created, rowbytes = tbase._rows(64, DIM_B)
    raw = P.RecallIndex(dim=DIM_B, capacity_rows=64)
    raw.append(emb, created, rowbytes.reshape(-1), np.arange(65, dtype=np.int64) * rowbytes.shape[1], row_ids=np.arange(64, dtype=np.int64))
    with pytest.raises(P.native.OrrError) as e:
        raw.scope_near(probes[:1], 0.5, "all")
    assert e.value.code == P.native.ORR_ESTATE
    with pytest.raises(P.native.OrrError) as e:
        raw.scope_near(probes[:1], float("nan"), "all")
    assert e.value.code == P.native.ORR_EINVAL
    raw.close()


def test_four_threads_create_and_search_cosine_scopes_on_one_handle():
    s = _shard_b_shared()
    idx, model, probes, q, texts = s["idx"], s["model"], s["probes"], s["q"][:8], s["texts"][:8]
    one = orc.cosine(probes[0], probes[0])
    jobs = [(probes[:1], s["t10"], "all"), (probes[:8], s["t1000"], "any"), (probes[:1], one, "all"), (probes[2:5], 0.0, "all")]
    want_ids = [model.near_ids(*j) for j in jobs]
    want = [_masked(idx, q, texts, 10, NB, ids) for ids in want_ids]
    bad = []

    def work(i):
        for _ in range(4):
            sc = idx.scope_near(*jobs[i])
            if not np.array_equal(sc.row_ids(), want_ids[i]) or not _equal(_in_scope(idx, q, texts, 10, NB, sc), want[i]):
                bad.append(i)
            sc.close()

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not bad


# ---- cluster -----------------------------------------------------------------------------------------------------------------

def test_cluster_scope_near_is_the_union_of_the_shards_parts():
    """three shards of 20,000 x 64 on one device, built the way tests/test_gpu_cluster_scope_handle.py builds its own"""
    P, syn = pkg(), _syn()
    cut, dim = 20_000, 64
    n = 3 * cut
    emb, created, rowbytes = tbase._rows(n, dim)
    probes = _probes(emb, n, dim, 7)
    for r in (0, cut - 1, cut, 2 * cut + 63, n - 1):    # copies of probe 0 at the shard borders
        emb[r] = probes[0]
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    model = Model(emb, created, rowbytes, ids)
    off = np.arange(cut + 1, dtype=np.int64) * syn.ROW_BYTES
    cl = P.RecallCluster([0, 0, 0], dim)
    for g in range(3):
        r0, r1 = g * cut, (g + 1) * cut
        cl.shard(g).append(emb[r0:r1], created[r0:r1], rowbytes[r0:r1].reshape(-1), off, row_ids=ids[r0:r1])
    cl.seal()
    gone = ids[[5, cut, cut + 77, n - 2]]
    for g in range(3):
        mine = np.array([i for i in gone if g * cut <= (i - 11) // 3 < (g + 1) * cut], np.int64)
        assert cl.shard(g).delete_rows(mine) == len(mine)
    model.delete(gone)
    c0 = model.cos(probes[0])
    t10, one = float(np.quantile(c0, 0.9)), orc.cosine(probes[0], probes[0])
    q = syn.query_vectors(0, 8, dim, n).numpy()
    terms = _terms(syn.query_texts(0, 8, n))
    for pr, t, mode in ((probes[:1], t10, "all"), (probes[:8], t10, "any"), (probes[:1], one, "all"), (probes[:2], -INF, "all"),
                        (np.ones((2, 32), np.float32), 0.0, "any"), (None, 0.0, "any")):
        sc = cl.scope_near(pr, t, mode)
        want = model.near_ids([] if pr is None else pr, t, mode)         # the global candidate order is the position order
        assert sc.rows == len(want) and np.array_equal(sc.row_ids(), want), (t, mode)
        if len(want):
            got = cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, sc, candidate_limit=n)
            assert _equal(got, cl.search_masked(q, terms, syn.NOW_TICKS, 10, want, candidate_limit=n)), (t, mode)
        sc.close()
    import torch
    dev = torch.from_numpy(probes[:1]).to("cuda:0")
    h = P.native.C.c_void_p(7)
    assert P.native.hip.orr_cluster_scope_create_near(cl._h, 1, dim, dev.data_ptr(), 0.5, 0, P.native.C.byref(h)) == P.native.ORR_EINVAL and h.value == 7
    cl.close()
