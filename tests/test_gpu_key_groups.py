"""Key groups on the device (orr_keys_groups, orr_keys_centroids, orr_scope_centroid).

The model is a numpy restatement of the header's rule over the test's OWN host copy of the vectors: the members of a key are
the live rows that carry it (inside the scope, where one is given) in candidate order -- read from the library through calls
that exist without the feature (scope(...).row_ids(): "the ids of the scope's live rows, in candidate order") -- the
participating ones are those with a finite-or-infinite, non-zero vector (normB > 0), their fp64 sum is taken in blocks of 256
consecutive members (_sum_blocked), the centroid is float32(S / n).  Every comparison is on raw bits: uint64 views of the sums,
uint32 views of the centroids, exact counts and keys.

Shards (built once per module, only read except where a test builds its own):
    G1   4,099 x 70     the scalar form of keys_block_sums (dim % 4 != 0, ragged last words); keys in runs, one scattered key,
                        ORR_KEY_NONE, the keys INT64_MIN + 1, -1, 0, INT64_MAX; rows without an embedding, a zero vector, a row
                        with a NaN coordinate, a row with +inf, deleted rows
    G2  20,000 x 128    the vector form; planted keys of 1, 255, 256, 257 and 1,000 members (four blocks: 256, 256, 256, 232);
                        coordinates over some 30 decades with mixed signs; every row participates: the whole shard is 79 blocks"""
import threading

import numpy as np
import pytest

import test_gpu_per_key as kbase
import test_gpu_scope_terms as tbase
from helpers import pkg

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NONE = I64_MIN
BLOCK = 256
N1, D1 = 4_099, 70
N2, D2 = 20_000, 128
PLANTED = {9_000_001: 1, 9_000_255: 255, 9_000_256: 256, 9_000_257: 257, 9_001_000: 1_000}
ABSENT = 4_242_424_242
_syn, _stats = tbase._syn, tbase._stats


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((_bits64(a) == _bits64(b)) | (np.isnan(a) & np.isnan(b))).all())


def _same32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((_bits32(a) == _bits32(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def _sum_blocked(E, block=BLOCK, reverse_fold=False):
    """S of the rows E [n, dim] float32, in this order: P_j from +0.0 over 256 rows, S from +0.0 over the P_j"""
    E = np.asarray(E, np.float32)
    parts = []
    with np.errstate(all="ignore"):
        for b0 in range(0, E.shape[0], block):
            P = np.zeros(E.shape[1], np.float64)
            for row in E[b0:b0 + block].astype(np.float64):
                P = P + row
            parts.append(P)
        S = np.zeros(E.shape[1], np.float64)
        for P in (reversed(parts) if reverse_fold else parts):
            S = S + P
    return S


def _sum_sequential(E):
    return _sum_blocked(E, block=1 << 40)


def _participates(E):
    return ~np.isnan(E).any(axis=1) & (E != 0).any(axis=1)


def _finish(S, n):
    with np.errstate(all="ignore"):
        return (S / np.float64(n)).astype(np.float32) if n else np.zeros(S.shape, np.float32)


class Model:
    """the host copy: one vector and one key per row id, and the library's present candidate order of the live ids"""

    def __init__(self, idx, emb, ids, keys):
        self.idx, self.dim = idx, emb.shape[1]
        self.emb = {int(i): emb[r].copy() for r, i in enumerate(ids)}
        self.key = {int(i): int(k) for i, k in zip(ids, keys)}

    def order(self, within=None):
        if within is not None:
            return within.row_ids()
        sc = self.idx.scope(np.fromiter(self.emb.keys(), np.int64))
        try:
            return sc.row_ids()
        finally:
            sc.close()

    def rows(self, order):
        """(keys, vectors) of the ids of `order`, in that order"""
        order = [int(i) for i in order]
        ks = np.array([self.key[i] for i in order], np.int64).reshape(-1)
        E = np.stack([self.emb[i] for i in order]) if order else np.zeros((0, self.dim), np.float32)
        return ks, E

    def groups(self, order):
        ks, _ = self.rows(order)
        return np.unique(ks[ks != NONE], return_counts=True)

    def centroid(self, rows, key=None):
        """(c, S, n) of the rows (self.rows(order)) with this key (None: all of them)"""
        ks, E = rows
        if key is not None:
            E = E[ks == key]
        E = E[_participates(E)]
        S = _sum_blocked(E)
        return _finish(S, len(E)), S, len(E)


def _check_groups(model, hk, within=None, what=None):
    order = model.order(within)
    wk, wn = model.groups(order)
    gk, gn = hk.groups(within)
    assert np.array_equal(gk, wk) and np.array_equal(gn, wn), (what, gk[:6], wk[:6], gn[:6], wn[:6])
    return wk, wn


def _check_centroids(model, hk, keys, within=None, what=None):
    rows = model.rows(model.order(within))
    cent, sums, used = hk.centroids(keys, within, sums=True)
    assert cent.shape == (len(keys), model.dim) and sums.shape == cent.shape and used.shape == (len(keys),)
    for i, k in enumerate(keys):
        c, S, n = model.centroid(rows, int(k))
        assert int(used[i]) == n, (what, int(k), int(used[i]), n)
        assert _same64(sums[i], S), (what, int(k), n, np.nonzero(_bits64(sums[i]) != _bits64(S))[0][:8])
        assert _same32(cent[i], c), (what, int(k), n)
    only, used2 = hk.centroids(keys, within)
    assert _same32(only, cent) and np.array_equal(used2, used)
    return cent, sums, used


def _check_scope_centroid(model, sc, what=None):
    c, S, n = model.centroid(model.rows(sc.row_ids()))
    gc, gS, gn = sc.centroid(sums=True)
    assert gn == n and _same64(gS, S) and _same32(gc, c), (what, gn, n)
    c2, n2 = sc.centroid()
    assert n2 == n and _same32(c2, gc)
    return gS, gn


# ---- shards ------------------------------------------------------------------------------------------------------------------

_G = {}


def _g1():
    if "g1" in _G:
        return _G["g1"]
    rng = np.random.default_rng(811)
    _, created, rowbytes = tbase._rows(N1, D1)
    emb = (rng.standard_normal((N1, D1)) * rng.choice([1.0, 1e-3, 250.0], (N1, 1))).astype(np.float32)
    emb[77] = 0.0                                       # a zero vector
    emb[1_203, 69] = np.nan                             # a NaN in the ragged last word
    emb[2_950, 3] = np.inf
    ids = np.arange(N1, dtype=np.int64) * 5 + 3
    idx = tbase._build(emb, created, rowbytes, ids, N1)
    keys = kbase._assign_keys(N1, rng)
    by_pos = idx.scope(ids).row_ids()                   # candidate order: keys are laid out in runs of consecutive candidates
    key_of = dict(zip(by_pos.tolist(), keys.tolist()))
    keys = np.array([key_of[int(i)] for i in ids], np.int64)
    # the special rows share keys with ordinary rows
    for r in (77, 1_203, 2_950):
        keys[r] = keys[r - 1] if keys[r - 1] != NONE else 31_337
    none_emb = ids[[10, 11, 500, 4_000, 4_098]]
    assert idx.update_rows(none_emb, None) == len(none_emb)           # rows without an embedding
    for i in none_emb:
        emb[(int(i) - 3) // 5] = 0.0
    hk = idx.keys(ids, keys)
    model = Model(idx, emb, ids, keys)
    gone = np.unique(np.concatenate([ids[[0, 12, 13, 2_949, 4_097]], rng.choice(ids, 200, replace=False)]))
    gone = np.setdiff1d(gone, np.concatenate([ids[[77, 1_203, 2_950]], none_emb]))              # the special rows stay
    assert idx.delete_rows(gone) == len(gone)
    for i in gone:
        del model.emb[int(i)], model.key[int(i)]
    _G["g1"] = (idx, hk, model, ids)
    return _G["g1"]


def _g2_rows():
    rng = np.random.default_rng(812)
    _, created, rowbytes = tbase._rows(N2, D2)
    emb = (rng.standard_normal((N2, D2)) * 10.0 ** rng.uniform(-15, 15, (N2, D2))).astype(np.float32)
    ids = np.arange(N2, dtype=np.int64) * 3 + 1
    return rng, emb, created, rowbytes, ids


def _g2_keys(idx, ids, rng):
    """keys by candidate position: runs of 1 .. 40, then the planted keys scattered over the shard"""
    by_pos = idx.scope(ids).row_ids()
    keys = np.empty(N2, np.int64)
    r, nxt = 0, 1_000
    while r < N2:
        run = int(rng.integers(1, 41))
        keys[r:r + run] = NONE if rng.random() < 0.04 else nxt
        nxt += 1
        r += run
    free = rng.permutation(N2)
    at = 0
    for k, m in PLANTED.items():
        keys[np.sort(free[at:at + m])] = k
        at += m
    key_of = dict(zip(by_pos.tolist(), keys.tolist()))
    return np.array([key_of[int(i)] for i in ids], np.int64)


def _g2():
    if "g2" in _G:
        return _G["g2"]
    rng, emb, created, rowbytes, ids = _g2_rows()
    idx = tbase._build(emb, created, rowbytes, ids, N2)
    keys = _g2_keys(idx, ids, rng)
    hk = idx.keys(ids, keys)
    _G["g2"] = (idx, hk, Model(idx, emb, ids, keys), ids, created)
    return _G["g2"]


# ---- G1 ----------------------------------------------------------------------------------------------------------------------

def test_g1_groups_with_cap_zero_smaller_and_larger():
    idx, hk, model, ids = _g1()
    wk, wn = _check_groups(model, hk)
    total = len(wk)
    assert total > 100 and {I64_MIN + 1, -1, 0, I64_MAX, kbase.SPREAD_KEY} <= set(wk.tolist()) and NONE not in wk
    assert wk[0] == I64_MIN + 1 and wk[-1] == I64_MAX and (np.diff(wk.astype(object)) > 0).all()
    gk, gn = hk.groups(cap=0)
    assert len(gk) == 0 and len(gn) == 0
    gk, gn = hk.groups(cap=17)
    assert np.array_equal(gk, wk[:17]) and np.array_equal(gn, wn[:17])
    gk, gn = hk.groups(cap=total + 1000)
    assert np.array_equal(gk, wk) and np.array_equal(gn, wn)
    # the C call itself: cap == 0 with NULL arrays reports the total only
    import ctypes as C
    P = pkg()
    n, tot = C.c_int64(-7), C.c_int64(-7)
    assert P.native.hip.orr_keys_groups(hk._h, None, 0, None, None, C.cast(C.byref(n), C.c_void_p), C.cast(C.byref(tot), C.c_void_p)) == 0
    assert (n.value, tot.value) == (0, total)
    # the counts are of ALL members: they add up to the live rows with a key
    assert int(wn.sum()) == hk.rows


def test_g1_centroids_of_every_key_an_absent_key_none_and_a_key_twice():
    idx, hk, model, ids = _g1()
    wk, wn = model.groups(model.order())
    keys = np.concatenate([wk, [ABSENT, NONE, wk[5], wk[5], I64_MAX]]).astype(np.int64)
    cent, sums, used = _check_centroids(model, hk, keys, what="g1")
    T = len(wk)
    assert used[T] == 0 and not _bits64(sums[T]).any() and not _bits32(cent[T]).any()          # absent: +0.0 everywhere
    assert used[T + 1] > 0                                                                     # the rows without a key
    assert _same64(sums[T + 2], sums[5]) and _same64(sums[T + 3], sums[5]) and used[T + 2] == used[5]
    assert (used <= np.concatenate([wn, [0, N1, wn[5], wn[5], wn[-1]]])).all() and (used[:T] < wn).any()   # members that take no part
    # the +inf row takes part: its key's sum is +inf in that coordinate; the NaN row and the zero rows do not
    k_inf = model.key[int(ids[2_950])]
    i = int(np.nonzero(wk == k_inf)[0][0])
    assert np.isposinf(sums[i, 3]) and np.isfinite(np.delete(sums[i], 3)).all()
    k_nan = model.key[int(ids[1_203])]
    assert np.isfinite(sums[int(np.nonzero(wk == k_nan)[0][0])]).all()


def test_g1_a_dim_other_than_the_index_is_edim_and_zero_keys_write_nothing():
    import ctypes as C
    P = pkg()
    idx, hk, model, ids = _g1()
    h = P.native.hip
    keys = np.array([0, -1], np.int64)
    cent = np.full((2, D1 + 2), 7, np.float32)
    used = np.full(2, 7, np.int64)
    for dim in (D1 + 2, D1 - 1, 0, -3):
        assert h.orr_keys_centroids(hk._h, None, 2, keys.ctypes.data, dim, cent.ctypes.data, None, used.ctypes.data) == P.native.ORR_EDIM
    assert h.orr_keys_centroids(hk._h, None, 0, None, D1, None, None, None) == 0
    assert (cent == 7).all() and (used == 7).all()
    sc = idx.scope(ids[:100])
    u = C.c_int64(7)
    assert h.orr_scope_centroid(sc._h, D1 + 1, None, None, C.cast(C.byref(u), C.c_void_p)) == P.native.ORR_EDIM and u.value == 7
    _check_scope_centroid(model, sc, "g1 ids")          # the scalar form as one group, deleted rows and rows that take no part inside
    sc.close()


# ---- G2 ----------------------------------------------------------------------------------------------------------------------

def test_g2_the_inputs_tell_the_orders_apart():
    """a condition on the DATA, on the CPU: for the 1,000-member key the blocked sum differs in bits from the plain sequential
    sum, from the sum with the blocks folded in reverse and from the sum in blocks of 255"""
    idx, hk, model, ids, _ = _g2()
    order = model.order()
    for k, m in PLANTED.items():
        rows = [int(i) for i in order if model.key[int(i)] == k]
        assert len(rows) == m
    E = np.stack([model.emb[i] for i in order if model.key[int(i)] == 9_001_000])
    S = _sum_blocked(E)
    assert (_bits64(S) != _bits64(_sum_sequential(E))).any()
    assert (_bits64(S) != _bits64(_sum_blocked(E, reverse_fold=True))).any()
    assert (_bits64(S) != _bits64(_sum_blocked(E, block=255))).any()


def test_g2_groups_and_the_planted_keys_centroids():
    idx, hk, model, ids, _ = _g2()
    wk, wn = _check_groups(model, hk)
    for k, m in PLANTED.items():
        assert wn[int(np.nonzero(wk == k)[0][0])] == m
    keys = np.array(list(PLANTED) + [NONE, 1_000, 1_001, ABSENT], np.int64)
    cent, sums, used = _check_centroids(model, hk, keys, what="g2 planted")
    assert used[:5].tolist() == list(PLANTED.values())


def test_g2_centroids_of_every_key_in_one_call():
    idx, hk, model, ids, _ = _g2()
    wk, wn = model.groups(model.order())
    assert len(wk) > 800
    _check_centroids(model, hk, wk, what="g2 all")


def test_g2_within_a_ticks_scope_a_terms_scope_and_a_scope_that_empties_a_key():
    idx, hk, model, ids, created = _g2()
    lo, hi = np.sort(created)[[N2 // 4, 3 * N2 // 4]]
    probe = np.array(list(PLANTED) + [NONE, 1_000, 1_500], np.int64)
    ticks = idx.scope_ticks(int(lo), int(hi))
    terms = idx.scope_terms([tbase.FRAG], "any")
    k255 = [int(i) for i in ids if model.key[int(i)] == 9_000_255]
    rest = idx.scope(np.setdiff1d(ids, np.array(k255, np.int64)))
    for name, sc in (("ticks", ticks), ("terms", terms), ("rest", rest)):
        assert 0 < sc.rows < N2, name
        wk, wn = _check_groups(model, hk, sc, name)
        cent, sums, used = _check_centroids(model, hk, probe, sc, name)
        _check_scope_centroid(model, sc, name)
        if name == "rest":
            assert 9_000_255 not in wk and used[1] == 0 and not _bits64(sums[1]).any() and not _bits32(cent[1]).any()
    for sc in (ticks, terms, rest):
        sc.close()


def test_g2_the_whole_shard_is_79_blocks_through_the_fold_and_an_empty_scope_is_zero():
    idx, hk, model, ids, created = _g2()
    whole = idx.scope_ticks(int(created.min()), int(created.max()) + 1)
    assert whole.rows == N2
    (S, n), stats = _stats(idx, lambda: _check_scope_centroid(model, whole, "whole"))
    assert n == N2 and -(-N2 // BLOCK) == 79
    assert stats["keys_block_sums"]["launches"] == 2 and stats["keys_block_fold"]["launches"] == 2      # (two calls: with and without sums)
    E = np.stack([model.emb[int(i)] for i in whole.row_ids()])
    assert (_bits64(S) != _bits64(_sum_sequential(E))).any()
    whole.close()
    empty = idx.scope(np.zeros(0, np.int64))
    c, S, n = empty.centroid(sums=True)
    assert n == 0 and not _bits64(S).any() and not _bits32(c).any() and S.shape == (D2,)
    gk, gn = hk.groups(empty)
    assert len(gk) == 0
    cent, used = hk.centroids([1_000, NONE], empty)
    assert not _bits32(cent).any() and not used.any()
    empty.close()


def test_g2_the_slice_option_changes_no_bit_and_the_launch_counts():
    idx, hk, model, ids, _ = _g2()
    wk, wn = model.groups(model.order())
    small = wk[wn <= BLOCK][:23]                        # no listed key above one block
    keys = np.concatenate([small, [9_001_000, 9_000_257]]).astype(np.int64)
    base = hk.centroids(keys, sums=True)
    try:
        for per_slice in (1, 7):
            idx.set_option("key_groups_slice", per_slice)
            got, stats = _stats(idx, lambda: hk.centroids(keys, sums=True))
            assert _same32(got[0], base[0]) and _same64(got[1], base[1]) and np.array_equal(got[2], base[2]), per_slice
            assert stats["keys_block_sums"]["launches"] == -(-len(keys) // per_slice), (per_slice, stats["keys_block_sums"])
            assert stats["keys_block_fold"]["launches"] == (2 if per_slice == 1 else 1)         # only the slices with a long key
            got, stats = _stats(idx, lambda: hk.centroids(small))
            assert stats["keys_block_sums"]["launches"] == -(-len(small) // per_slice) and "keys_block_fold" not in stats
            for name in ("keys_pairs_count", "keys_pairs", "keys_pairs_sort", "keys_runs"):
                assert stats[name]["launches"] == 1, (name, stats[name])
    finally:
        idx.set_option("key_groups_slice", 0)
    got, stats = _stats(idx, lambda: hk.centroids(keys, sums=True))
    assert stats["keys_block_sums"]["launches"] == 1 and stats["keys_block_fold"]["launches"] == 1 and _same64(got[1], base[1])
    with pytest.raises(pkg().native.OrrError):
        idx.set_option("key_groups_slice", 65_537)
    before = idx.search_stats()
    hk.groups()
    hk.centroids(small)
    assert idx.search_stats() == before                 # no search: the search statistics do not move


def test_g2_a_table_beyond_2048_keys_takes_the_global_memory_lookup():
    idx, hk, model, ids, _ = _g2()
    wk, wn = model.groups(model.order())
    filler = np.arange(50_000_000, 50_000_000 + 2_100, dtype=np.int64)                          # absent keys, around the real ones
    keys = np.concatenate([filler[:1_000], wk[:40], [9_001_000, I64_MAX, I64_MIN + 1], filler[1_000:]]).astype(np.int64)
    assert len(np.unique(keys)) > 2_048
    rows = model.rows(model.order())
    cent, sums, used = hk.centroids(keys, sums=True)
    for i in list(range(1_000, 1_043)) + [0, 999, len(keys) - 1]:
        c, S, n = model.centroid(rows, int(keys[i]))
        assert int(used[i]) == n and _same64(sums[i], S) and _same32(cent[i], c), int(keys[i])
    assert not used[:1_000].any() and not _bits64(sums[:1_000]).any()


# ---- maintenance, views, threads, handles ------------------------------------------------------------------------------------

def test_maintenance_on_g2():
    rng, emb, created, rowbytes, ids = _g2_rows()
    idx = tbase._build(emb, created, rowbytes, ids, N2 + 500)
    keys = _g2_keys(idx, ids, rng)
    hk = idx.keys(ids, keys)
    model = Model(idx, emb, ids, keys)
    probe = np.array(list(PLANTED) + [NONE, 1_000, 1_200], np.int64)

    def check(what):
        _check_groups(model, hk, None, what)
        _check_centroids(model, hk, probe, None, what)

    check("made")
    big = np.array([i for i in ids if model.key[int(i)] == 9_001_000], np.int64)
    gone = np.unique(np.concatenate([big[100:140], rng.choice(ids, 700, replace=False)]))
    assert idx.delete_rows(gone) == len(gone)
    for i in gone:
        del model.emb[int(i)], model.key[int(i)]
    check("deleted")
    upd = np.array([i for i in big[300:330] if int(i) in model.emb], np.int64)
    new = (rng.standard_normal((len(upd), D2)) * 10.0 ** rng.uniform(-10, 10, (len(upd), D2))).astype(np.float32)
    assert idx.update_rows(upd, new) == len(upd)
    for r, i in enumerate(upd):
        model.emb[int(i)] = new[r]
    lost = np.array([i for i in big[400:405] if int(i) in model.emb], np.int64)
    assert idx.update_rows(lost, None) == len(lost)      # they lose their embedding: members still, no part in the sum
    for i in lost:
        model.emb[int(i)] = np.zeros(D2, np.float32)
    check("updated")
    assert idx.compact() == len(gone)
    check("compacted")
    m = 300
    e2 = (rng.standard_normal((m, D2)) * 10.0 ** rng.uniform(-15, 15, (m, D2))).astype(np.float32)
    _, _, rb2 = tbase._rows(m, D2, row0=7_000_000)
    c2 = rng.choice(created, m).astype(np.int64) + rng.integers(-2, 3, m)
    new_ids = 90_000_000 + np.arange(m, dtype=np.int64)
    assert idx.insert_rows(e2, c2, rb2.reshape(-1), np.arange(m + 1, dtype=np.uint64) * rb2.shape[1], row_ids=new_ids) == m
    for r, i in enumerate(new_ids):
        model.emb[int(i)], model.key[int(i)] = e2[r], NONE
    check("inserted")                                   # the new rows read ORR_KEY_NONE
    k2 = np.where(np.arange(m) % 3 == 0, 9_001_000, np.where(np.arange(m) % 3 == 1, 9_000_255, 77_000_000 + np.arange(m))).astype(np.int64)
    assert hk.set(new_ids, k2) == m
    for i, k in zip(new_ids, k2):
        model.key[int(i)] = int(k)
    check("keys set")
    hk.close()
    idx.close()


def test_a_view_two_threads_both_destroy_orders_and_an_orphan():
    P = pkg()
    rng = np.random.default_rng(815)
    n, dim = 3_000, 36
    _, created, rowbytes = tbase._rows(n, dim)
    emb = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-6, 6, (n, dim))).astype(np.float32)
    ids = np.arange(n, dtype=np.int64) + 50
    keys = (np.arange(n) % 7).astype(np.int64)         # seven keys of about 429 scattered rows: two blocks each
    idx = tbase._build(emb, created, rowbytes, ids, n)
    hk = idx.keys(ids, keys)
    model = Model(idx, emb, ids, keys)
    want = _check_centroids(model, hk, np.arange(7, dtype=np.int64), what="owner")
    view = idx.view()
    sc_view = view.scope(ids[:1_500])
    _check_centroids(model, hk, np.arange(7, dtype=np.int64), sc_view, "a scope made through a view")
    _check_scope_centroid(model, sc_view, "view")
    errors = []

    def work():
        try:
            for _ in range(4):
                got = hk.centroids(np.arange(7, dtype=np.int64), sums=True)
                assert _same64(got[1], want[1]) and np.array_equal(got[2], want[2])
                gk, gn = hk.groups()
                assert gk.tolist() == list(range(7)) and int(gn.sum()) == n
        except BaseException as e:                      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    # a scope of another shard
    other = tbase._build(emb[:64], created[:64], rowbytes[:64], ids[:64], 64)
    foreign = other.scope(ids[:10])
    with pytest.raises(P.native.OrrError) as e:
        hk.centroids([1], foreign)
    assert e.value.code == P.native.ORR_EINVAL
    with pytest.raises(P.native.OrrError) as e:
        hk.groups(foreign)
    assert e.value.code == P.native.ORR_EINVAL
    foreign.close()
    other.close()
    # the keys go first, then the index; then an index goes first and the handles are orphaned
    sc_view.close()
    view.close()
    hk2 = idx.keys(ids, keys)
    hk2.close()
    sc = idx.scope(ids[:100])
    idx.close()
    for call in (lambda: hk.groups(), lambda: hk.centroids([1]), lambda: sc.centroid()):
        with pytest.raises(P.native.OrrError) as e:
            call()
        assert e.value.code == P.native.ORR_ESTATE
    hk.close()
    sc.close()
