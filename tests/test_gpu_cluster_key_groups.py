"""Key groups over a cluster (orr_cluster_keys_groups, orr_cluster_keys_centroids, orr_cluster_scope_centroid).

The contract: the answers of the single-index call on ONE index holding all the cluster's rows in the global candidate order,
bit for bit.  Every case is held two ways: against the twin -- test_gpu_key_groups's kind of single index over the same rows --
and against that module's numpy restatement (Model, _sum_blocked, _finish) over the cluster's own candidate order, which the
library reports through calls that exist without the feature (RecallClusterScope.row_ids).  Every comparison is on raw bits.

Clusters (three or four shards on ordinal 0, built once per module, only read except where a test builds its own):
    C1   G1's rows (4,099 x 70) cut at (211, 3,804): the scalar form (dim % 4 != 0) with a zero vector, a NaN, a +inf, rows
         without an embedding, deleted rows, the extreme keys; the keys lie in runs of candidates, so runs straddle both borders
    C2   G2's rows (20,000 x 128, values over 30 decades) in four shards, with this file's own key assignment by candidate
         position; the cuts are computed FROM it: the first directly behind the 256th member of the 1,000-member key BIG (a
         border on a block edge: S seeded, no head), the second three of its members later (a free block left open and carried),
         the third behind its 900th member (a head that closes, a free block, a tail that stays open).  Planted beside it:
         A    100 + 5 + 300 members on shards 0, 1, 2: on shard 1 too few to close the open block (a head that stays open)
         B    300 + 50 members on shards 0 and 3 only: the carry passes over two shards
         K255 100 + 155 over the last border, K256 128 + 128 on shards 0 and 2, K257 256 + 1 on shards 0 and 2 (a block edge),
         K1   one member, the first row behind the first border; W600 wholly on shard 2 (three blocks through the fold)"""
import ctypes as C
import threading

import numpy as np
import pytest

import test_gpu_cluster_diverse as cbase
import test_gpu_key_groups as gbase
import test_gpu_per_key as kbase
import test_gpu_scope_terms as tbase
from helpers import pkg

pytestmark = pytest.mark.gpu

NONE, BLOCK, ABSENT = gbase.NONE, gbase.BLOCK, gbase.ABSENT
I64_MIN, I64_MAX = gbase.I64_MIN, gbase.I64_MAX
N1, D1, N2, D2 = gbase.N1, gbase.D1, gbase.N2, gbase.D2
Model, _sum_blocked, _finish, _same64, _same32, _bits64, _bits32 = (gbase.Model, gbase._sum_blocked, gbase._finish, gbase._same64, gbase._same32,
                                                                  gbase._bits64, gbase._bits32)
_check_groups, _check_centroids, _check_scope_centroid = gbase._check_groups, gbase._check_centroids, gbase._check_scope_centroid
_cstats, _raises = cbase._cstats, cbase._raises
CUTS1 = (211, 3_804)
BIG, KA, KB, K255, K256, K257, K1, W600 = 9_001_000, 9_000_405, 9_000_350, 9_000_255, 9_000_256, 9_000_257, 9_000_001, 9_000_600
PLAN = {BIG: (256, 3, 641, 100), KA: (100, 5, 300, 0), KB: (300, 0, 0, 50), K255: (0, 0, 100, 155), K256: (128, 0, 128, 0),
        K257: (256, 0, 1, 0), K1: (0, 1, 0, 0), W600: (0, 0, 600, 0)}
SPANNING = (BIG, KA, KB, K255, K256, K257)


def _n(st, name):
    return int(st.get(name, {}).get("launches", 0))


def _in_candidate_order(emb, created, rowbytes, ids, capacity):
    """(the twin, the rows in the twin's candidate order): cut anywhere, such rows give a cluster whose global order is the twin's"""
    twin = tbase._build(emb, created, rowbytes, ids, capacity)
    sc = twin.scope(ids)
    by_pos = sc.row_ids()
    sc.close()
    assert len(by_pos) == len(ids)
    at = {int(i): r for r, i in enumerate(ids)}
    perm = np.array([at[int(i)] for i in by_pos], np.int64)
    return twin, emb[perm], created[perm], rowbytes[perm], ids[perm]


def _order_of(cl, ids):
    sc = cl.scope(ids)
    try:
        return sc.row_ids()
    finally:
        sc.close()


# ---- the wrong orders --------------------------------------------------------------------------------------------------------

def _sum_restarted(parts):
    """blocks restart at every border: the fold runs over each part's own blocks"""
    S = np.zeros(parts[0].shape[1], np.float64)
    with np.errstate(all="ignore"):
        for E in parts:
            for b0 in range(0, len(E), BLOCK):
                S = S + _sum_blocked(E[b0:b0 + BLOCK])
    return S


def _sum_added(parts):
    """per-shard blocked sums added up"""
    S = np.zeros(parts[0].shape[1], np.float64)
    with np.errstate(all="ignore"):
        for E in parts:
            if len(E):
                S = S + _sum_blocked(E)
    return S


# ---- clusters ----------------------------------------------------------------------------------------------------------------

_C = {}


def _c1():
    """G1's recipe (test_gpu_key_groups._g1), on a twin and on a cluster of three shards"""
    if "c1" in _C:
        return _C["c1"]
    rng = np.random.default_rng(811)
    _, created, rowbytes = tbase._rows(N1, D1)
    emb = (rng.standard_normal((N1, D1)) * rng.choice([1.0, 1e-3, 250.0], (N1, 1))).astype(np.float32)
    ids = np.arange(N1, dtype=np.int64) * 5 + 3
    twin, emb, created, rowbytes, ids = _in_candidate_order(emb, created, rowbytes, ids, N1)      # from here on: row r is candidate r
    emb[77] = 0.0
    emb[1_203, 69] = np.nan
    emb[2_950, 3] = np.inf
    twin.close()
    twin = tbase._build(emb, created, rowbytes, ids, N1)
    cl = cbase._cluster_of(emb, created, rowbytes, ids, CUTS1)
    assert np.array_equal(_order_of(cl, ids), ids) and np.array_equal(_order_of(twin, ids), ids)
    keys = kbase._assign_keys(N1, rng)                  # runs of consecutive candidates, the extreme keys, one scattered key
    for r in (77, 1_203, 2_950):
        keys[r] = keys[r - 1] if keys[r - 1] != NONE else 31_337
    none_emb = ids[[10, 11, 212, 500, 4_000, 4_098]]
    edges = (0,) + CUTS1 + (N1,)
    on = lambda some, g: some[np.isin(some, ids[edges[g]:edges[g + 1]])]      # noqa: E731 -- the ids of `some` that shard g holds
    assert twin.update_rows(none_emb, None) == len(none_emb)
    assert sum(cl.shard(g).update_rows(on(none_emb, g), None) for g in range(3)) == len(none_emb)
    emb[np.isin(ids, none_emb)] = 0.0
    tk, ck = twin.keys(ids, keys), cl.keys(ids, keys)
    gone = np.unique(np.concatenate([ids[[0, 12, 13, 210, 211, 2_949, 3_804, 4_097]], rng.choice(ids, 200, replace=False)]))
    gone = np.setdiff1d(gone, np.concatenate([ids[[77, 1_203, 2_950]], none_emb]))
    assert twin.delete_rows(gone) == len(gone)
    assert sum(cl.shard(g).delete_rows(on(gone, g)) for g in range(3)) == len(gone)
    tm, cm = Model(twin, emb, ids, keys), Model(cl, emb, ids, keys)
    for i in gone:
        del tm.emb[int(i)], tm.key[int(i)], cm.emb[int(i)], cm.key[int(i)]
    _C["c1"] = dict(twin=twin, tk=tk, tm=tm, cl=cl, ck=ck, cm=cm, ids=ids, keys=keys, created=created)
    return _C["c1"]


def _c2_keys(rng):
    """(keys by candidate position, the cuts computed from them)"""
    keys = np.empty(N2, np.int64)
    r, nxt = 0, 1_000
    while r < N2:
        run = int(rng.integers(1, 41))
        keys[r:r + run] = NONE if rng.random() < 0.04 else nxt
        nxt += 1
        r += run
    big = np.arange(1_000) * 20 + rng.integers(0, 8, 1_000)          # ascending, at least 13 apart
    cuts = (int(big[255]) + 1, int(big[258]) + 1, int(big[899]) + 1)
    edges = (0,) + cuts + (N2,)
    taken = np.zeros(N2, bool)
    taken[big] = True
    keys[big] = BIG
    keys[cuts[0]] = K1                                  # the first row behind the first border (never a member of BIG: 13 apart)
    taken[cuts[0]] = True
    for k, per_shard in PLAN.items():
        if k in (BIG, K1):
            continue
        for g, m in enumerate(per_shard):
            free = np.nonzero(~taken[edges[g]:edges[g + 1]])[0] + edges[g]
            pick = np.sort(rng.choice(free, m, replace=False))
            keys[pick] = k
            taken[pick] = True
    return keys, cuts


def _c2_parts(capacity=0):
    rng, emb, created, rowbytes, ids = gbase._g2_rows()
    twin, emb, created, rowbytes, ids = _in_candidate_order(emb, created, rowbytes, ids, capacity or N2)
    keys, cuts = _c2_keys(rng)
    cl = cbase._cluster_of(emb, created, rowbytes, ids, cuts, capacity=capacity)
    assert np.array_equal(_order_of(cl, ids), _order_of(twin, ids))
    tk, ck = twin.keys(ids, keys), cl.keys(ids, keys)
    return dict(twin=twin, tk=tk, tm=Model(twin, emb, ids, keys), cl=cl, ck=ck, cm=Model(cl, emb, ids, keys), ids=ids, keys=keys, created=created,
                cuts=cuts, edges=(0,) + cuts + (N2,), emb=emb, rowbytes=rowbytes, rng=rng)


def _c2():
    if "c2" not in _C:
        _C["c2"] = _c2_parts()
    return _C["c2"]


def _both(c, keys, within=(None, None), what=None):
    """the cluster's centroids against the restatement and, bit for bit, against the twin's"""
    got = _check_centroids(c["cm"], c["ck"], keys, within[0], what)
    want = c["tk"].centroids(keys, within[1], sums=True)
    assert _same32(got[0], want[0]) and _same64(got[1], want[1]) and np.array_equal(got[2], want[2]), what
    return got


def _both_groups(c, within=(None, None), what=None):
    wk, wn = _check_groups(c["cm"], c["ck"], within[0], what)
    tk, tn = c["tk"].groups(within[1])
    assert np.array_equal(wk, tk) and np.array_equal(wn, tn), what
    return wk, wn


def _both_scope(c, sc, tsc, what=None):
    S, n = _check_scope_centroid(c["cm"], sc, what)
    tc, tS, tn = tsc.centroid(sums=True)
    assert n == tn and _same64(S, tS) and _same32(sc.centroid()[0], tc), what
    return S, n


# ---- the placement -------------------------------------------------------------------------------------------------------------

def test_c2_the_cuts_place_every_case_and_the_data_tell_the_orders_apart():
    """conditions on the DATA, on the CPU: every planted key has its members where the module's docstring says, the borders cut
    BIG behind its 256th, 259th and 900th member, and for every spanning key whose cuts are not all on block edges both wrong
    orders differ in bits from the blocked sum over the concatenated members"""
    c = _c2()
    keys, edges, emb = c["keys"], c["edges"], c["emb"]
    assert np.array_equal(c["cm"].order(), c["ids"]) and np.array_equal(c["tm"].order(), c["ids"])
    for k, per_shard in PLAN.items():
        pos = np.nonzero(keys == k)[0]
        got = tuple(int(((pos >= edges[g]) & (pos < edges[g + 1])).sum()) for g in range(4))
        assert got == per_shard, (k, got)
    big = np.nonzero(keys == BIG)[0]
    assert edges[1] == big[255] + 1 and edges[2] == big[258] + 1 and edges[3] == big[899] + 1
    assert gbase._participates(emb).all()               # every row takes part: the members are the participating members
    for k in SPANNING:
        pos = np.nonzero(keys == k)[0]
        parts = [emb[pos[(pos >= edges[g]) & (pos < edges[g + 1])]] for g in range(4)]
        right = _sum_blocked(emb[pos])
        on_edges = all(int((pos < e).sum()) % BLOCK == 0 for e in edges[1:4] if 0 < (pos < e).sum() < len(pos))      # the borders that cut it
        assert on_edges == (k == K257), k
        a, b = (_bits64(_sum_restarted(parts)) != _bits64(right)).any(), (_bits64(_sum_added(parts)) != _bits64(right)).any()
        assert (a and b) if not on_edges else not a, (k, a, b)


# ---- C1 ----------------------------------------------------------------------------------------------------------------------

def test_c1_groups_with_cap_zero_smaller_and_larger():
    c = _c1()
    ck = c["ck"]
    wk, wn = _both_groups(c, what="c1")
    total = len(wk)
    assert total > 100 and {I64_MIN + 1, -1, 0, I64_MAX, kbase.SPREAD_KEY} <= set(wk.tolist()) and NONE not in wk
    gk, gn = ck.groups(cap=0)
    assert len(gk) == 0 and len(gn) == 0
    gk, gn = ck.groups(cap=17)
    assert np.array_equal(gk, wk[:17]) and np.array_equal(gn, wn[:17])
    gk, gn = ck.groups(cap=total + 1000)
    assert np.array_equal(gk, wk) and np.array_equal(gn, wn)
    P = pkg()
    n, tot = C.c_int64(-7), C.c_int64(-7)
    assert P.native.hip.orr_cluster_keys_groups(ck._h, None, 0, None, None, C.cast(C.byref(n), C.c_void_p), C.cast(C.byref(tot), C.c_void_p)) == 0
    assert (n.value, tot.value) == (0, total) and int(wn.sum()) == ck.rows


def test_c1_centroids_of_every_key_an_absent_key_none_and_a_key_twice():
    c = _c1()
    wk, wn = c["cm"].groups(c["cm"].order())
    keys = np.concatenate([wk, [ABSENT, NONE, wk[5], wk[5], I64_MAX]]).astype(np.int64)
    cent, sums, used = _both(c, keys, what="c1")
    T = len(wk)
    assert used[T] == 0 and not _bits64(sums[T]).any() and not _bits32(cent[T]).any()
    assert used[T + 1] > 0 and _same64(sums[T + 2], sums[5]) and _same64(sums[T + 3], sums[5]) and used[T + 2] == used[5]
    assert (used[:T] < wn).any()                        # members that take no part
    k_inf = c["cm"].key[int(c["ids"][2_950])]
    i = int(np.nonzero(wk == k_inf)[0][0])
    assert np.isposinf(sums[i, 3]) and np.isfinite(np.delete(sums[i], 3)).all()
    # keys lie across the borders: the scattered key on shards 0 and 1, runs of candidates wherever a border falls inside one
    order = c["cm"].order()
    live_edges = [0] + [int(np.isin(order, c["ids"][:e]).sum()) for e in CUTS1] + [len(order)]
    ks, _ = c["cm"].rows(order)
    per_shard = [set(ks[live_edges[g]:live_edges[g + 1]].tolist()) - {NONE} for g in range(3)]
    assert kbase.SPREAD_KEY in per_shard[0] & per_shard[1] and len((per_shard[0] & per_shard[1]) | (per_shard[1] & per_shard[2])) >= 2
    whole = c["cl"].scope(c["ids"])
    twhole = c["twin"].scope(c["ids"])
    _both_scope(c, whole, twhole, "c1 whole")           # the scalar form as one group over three shards
    whole.close(); twhole.close()


def test_c1_edim_zero_keys_and_the_scope_forms():
    P = pkg()
    h = P.native.hip
    c = _c1()
    ck, cl, ids = c["ck"], c["cl"], c["ids"]
    keys = np.array([0, -1], np.int64)
    cent = np.full((2, D1 + 2), 7, np.float32)
    used = np.full(2, 7, np.int64)
    for dim in (D1 + 2, D1 - 1, 0, -3):
        assert h.orr_cluster_keys_centroids(ck._h, None, 2, keys.ctypes.data, dim, cent.ctypes.data, None, used.ctypes.data) == P.native.ORR_EDIM
    assert h.orr_cluster_keys_centroids(ck._h, None, 0, None, D1, None, None, None) == 0
    assert (cent == 7).all() and (used == 7).all()
    sc, tsc = cl.scope(ids[150:400]), c["twin"].scope(ids[150:400])      # across the first border
    u = C.c_int64(7)
    assert h.orr_cluster_scope_centroid(sc._h, D1 + 1, None, None, C.cast(C.byref(u), C.c_void_p)) == P.native.ORR_EDIM and u.value == 7
    _both_scope(c, sc, tsc, "c1 ids")
    _both_groups(c, (sc, tsc), "c1 ids")
    _both(c, np.array([0, -1, NONE, kbase.SPREAD_KEY, I64_MAX], np.int64), (sc, tsc), "c1 ids")
    sc.close(); tsc.close()


# ---- C2 ----------------------------------------------------------------------------------------------------------------------

def test_c2_groups_and_the_planted_keys_centroids():
    c = _c2()
    wk, wn = _both_groups(c, what="c2")
    for k, per_shard in PLAN.items():
        assert wn[int(np.nonzero(wk == k)[0][0])] == sum(per_shard)
    keys = np.array(list(PLAN) + [NONE, 1_000, 1_001, ABSENT, BIG], np.int64)
    cent, sums, used = _both(c, keys, what="c2 planted")
    assert used[:len(PLAN)].tolist() == [sum(p) for p in PLAN.values()] and used[-2] == 0 and used[-1] == 1_000
    assert _same64(sums[-1], sums[0])                   # a key listed twice is answered twice


def test_c2_centroids_of_every_key_in_one_call():
    c = _c2()
    wk, wn = c["cm"].groups(c["cm"].order())
    assert len(wk) > 800
    _both(c, wk, what="c2 all")


def test_c2_within_a_ticks_scope_a_terms_scope_a_scope_that_empties_a_key_on_one_shard_and_the_empty_scope():
    c = _c2()
    cl, twin, ids, created, keys, edges = c["cl"], c["twin"], c["ids"], c["created"], c["keys"], c["edges"]
    lo, hi = np.sort(created)[[N2 // 4, 3 * N2 // 4]]
    probe = np.array(list(PLAN) + [NONE, 1_000, 1_500], np.int64)
    pos = np.nonzero(keys == BIG)[0]
    on2 = ids[pos[(pos >= edges[2]) & (pos < edges[3])]]          # BIG's members on shard 2 leave: shards 0, 1 and 3 carry on
    pairs = {"ticks": (cl.scope_ticks(int(lo), int(hi)), twin.scope_ticks(int(lo), int(hi))),
             "terms": (cl.scope_terms([tbase.FRAG], "any"), twin.scope_terms([tbase.FRAG], "any")),
             "rest": (cl.scope(np.setdiff1d(ids, on2)), twin.scope(np.setdiff1d(ids, on2))),
             "empty": (cl.scope(np.zeros(0, np.int64)), twin.scope(np.zeros(0, np.int64)))}
    for name, (sc, tsc) in pairs.items():
        assert sc.rows == tsc.rows and (0 < sc.rows < N2 or name == "empty"), name
        _both_groups(c, (sc, tsc), name)
        cent, sums, used = _both(c, probe, (sc, tsc), name)
        S, n = _both_scope(c, sc, tsc, name)
        if name == "rest":
            assert used[0] == 359
        if name == "empty":
            assert n == 0 and not _bits64(S).any() and not used.any() and not _bits64(sums).any() and not _bits32(cent).any()
    rows = [sc.shard(g).rows for sc in (pairs["ticks"][0],) for g in range(4)]
    assert sum(1 for r in rows if r > 0) >= 2           # the ticks scope lies across a border
    for sc, tsc in pairs.values():
        sc.close(); tsc.close()


def test_c2_the_whole_cluster_is_79_blocks_over_four_shards_and_a_scope_on_one_shard():
    c = _c2()
    cl, twin, ids, created, edges = c["cl"], c["twin"], c["ids"], c["created"], c["edges"]
    whole, twhole = cl.scope_ticks(int(created.min()), int(created.max()) + 1), twin.scope_ticks(int(created.min()), int(created.max()) + 1)
    assert whole.rows == N2 and -(-N2 // BLOCK) == 79
    (S, n), sts = _cstats(cl, lambda: _both_scope(c, whole, twhole, "whole"))
    assert n == N2
    assert (_bits64(S) != _bits64(gbase._sum_sequential(np.stack([c["cm"].emb[int(i)] for i in ids])))).any()
    for g in range(4):                                  # (three calls: with sums, without, and the twin comparison's)
        assert _n(sts[g], "keys_chain_step") == 3 and _n(sts[g], "keys_block_sums") == 3, (g, sts[g].keys())
        assert _n(sts[g], "keys_block_fold") == 0       # the one group spans: its closed blocks go through the chain
    one, tone = cl.scope(ids[edges[2] + 10:edges[2] + 900]), twin.scope(ids[edges[2] + 10:edges[2] + 900])
    (S, n), sts = _cstats(cl, lambda: _both_scope(c, one, tone, "one shard"))
    assert n == 890
    for g in range(4):
        assert _n(sts[g], "keys_chain_step") == 0 and _n(sts[g], "keys_block_sums") == (3 if g == 2 else 0)
        assert _n(sts[g], "keys_block_fold") == (3 if g == 2 else 0)
    for sc in (whole, twhole, one, tone):
        sc.close()


def _chain_launches(c, table, per_slice):
    """per shard: the slices of the sorted table in which a spanning key has members there"""
    keys, edges = c["keys"], c["edges"]
    table = np.unique(np.asarray(table, np.int64))
    want = [0, 0, 0, 0]
    for s0 in range(0, len(table), per_slice):
        hit = set()
        for k in table[s0:s0 + per_slice]:
            pos = np.nonzero(keys == k)[0]
            on = [g for g in range(4) if ((pos >= edges[g]) & (pos < edges[g + 1])).any()]
            if len(on) > 1:
                hit.update(on)
        for g in hit:
            want[g] += 1
    return want


def test_c2_the_slice_option_changes_no_bit_and_the_launch_counts():
    c = _c2()
    cl, ck, twin, tk = c["cl"], c["ck"], c["twin"], c["tk"]
    wk, wn = c["cm"].groups(c["cm"].order())
    keys, edges = c["keys"], c["edges"]
    inside = [int(k) for k in wk[wn <= 40] if len({int(np.searchsorted(edges, p, "right")) for p in np.nonzero(keys == k)[0]}) == 1][:23]
    listed = np.array(inside + [BIG, K257, KB, W600, K1], np.int64)
    base = ck.centroids(listed, sums=True)
    want = tk.centroids(listed, sums=True)
    assert _same32(base[0], want[0]) and _same64(base[1], want[1]) and np.array_equal(base[2], want[2])
    try:
        for per_slice in (1, 7):
            cl.shard(0).set_option("key_groups_slice", per_slice)
            got, sts = _cstats(cl, lambda: ck.centroids(listed, sums=True))
            assert _same32(got[0], base[0]) and _same64(got[1], base[1]) and np.array_equal(got[2], base[2]), per_slice
            chain = _chain_launches(c, listed, per_slice)
            assert [_n(st, "keys_chain_step") for st in sts] == chain and sum(chain) > 0, (per_slice, chain)
            for st in sts:
                for name in ("keys_pairs_count", "keys_pairs", "keys_pairs_sort", "keys_runs"):
                    assert _n(st, name) == 1, (name, per_slice)
    finally:
        cl.shard(0).set_option("key_groups_slice", 0)
    got, sts = _cstats(cl, lambda: ck.centroids(listed, sums=True))
    assert _same64(got[1], base[1])
    assert [_n(st, "keys_chain_step") for st in sts] == [1, 1, 1, 1]
    assert [_n(st, "keys_block_sums") for st in sts] == [1, 1, 1, 0]          # shard 3 holds two head fragments and no block of its own
    assert [_n(st, "keys_block_fold") for st in sts] == [0, 0, 1, 0]          # W600: wholly on shard 2, three blocks
    # keys that lie on one shard each: no chain anywhere; the single-index twin launches none ever
    got, sts = _cstats(cl, lambda: ck.centroids(np.array(inside + [W600], np.int64)))
    assert [_n(st, "keys_chain_step") for st in sts] == [0, 0, 0, 0]
    _, st = gbase._stats(twin, lambda: tk.centroids(listed, sums=True))
    assert "keys_chain_step" not in st and _n(st, "keys_block_sums") == 1
    before = cl.search_stats()
    ck.groups()
    ck.centroids(listed)
    assert cl.search_stats() == before                  # no search: the search statistics do not move


def test_a_cluster_cut_between_documents_launches_exactly_the_single_index_calls_on_every_shard():
    rng = np.random.default_rng(821)
    n, dim = 3_000, 36
    _, created, rowbytes = tbase._rows(n, dim)
    emb = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-6, 6, (n, dim))).astype(np.float32)
    ids = np.arange(n, dtype=np.int64) + 50
    twin, emb, created, rowbytes, ids = _in_candidate_order(emb, created, rowbytes, ids, n)
    keys = (np.arange(n) // 300).astype(np.int64)       # ten documents of 300 consecutive candidates: two blocks each
    cl = cbase._cluster_of(emb, created, rowbytes, ids, (900, 1_200, 2_400))      # every border between two documents
    ck, tk = cl.keys(ids, keys), twin.keys(ids, keys)
    listed = np.arange(10, dtype=np.int64)
    got, sts = _cstats(cl, lambda: ck.centroids(listed, sums=True))
    want, st = gbase._stats(twin, lambda: tk.centroids(listed, sums=True))
    assert _same32(got[0], want[0]) and _same64(got[1], want[1]) and np.array_equal(got[2], want[2])
    for g, sh in enumerate(sts):
        assert "keys_chain_step" not in sh, g
        for name in ("keys_pairs_count", "keys_pairs", "keys_pairs_scan", "keys_pairs_sort", "keys_runs", "keys_block_sums", "keys_block_fold"):
            assert _n(sh, name) == _n(st, name) == 1, (g, name)
    gk, gn = ck.groups()
    assert gk.tolist() == list(range(10)) and (gn == 300).all()
    for h in (ck, tk, cl, twin):
        h.close()


# ---- refusals, maintenance, threads ------------------------------------------------------------------------------------------

def test_refusals_foreign_and_orphaned_handles_and_both_destroy_orders():
    N = pkg().native
    cl, ids = cbase._tiny()
    other, _ = cbase._tiny()
    mine, theirs = cl.keys(ids, ids // 7), other.keys(ids, ids // 7)
    my_scope, their_scope = cl.scope(ids[:100]), other.scope(ids[:100])
    assert mine.centroids([3, 5], my_scope)[1].tolist() == [2, 3] and my_scope.centroid()[1] == 100
    _raises(N.ORR_EINVAL, lambda: mine.centroids([3], their_scope), "scope belongs to another cluster")
    _raises(N.ORR_EINVAL, lambda: mine.groups(their_scope), "scope belongs to another cluster")
    # the cluster first: its keys and scopes are orphaned; then the handles
    other.close()
    _raises(N.ORR_ESTATE, lambda: theirs.groups(), "orphaned")
    _raises(N.ORR_ESTATE, lambda: theirs.centroids([3]), "orphaned")
    _raises(N.ORR_ESTATE, lambda: their_scope.centroid(), "orphaned")
    _raises(N.ORR_ESTATE, lambda: mine.centroids([3], their_scope), "orphaned")          # orphaned comes before "another cluster"
    theirs.close()
    their_scope.close()
    # the handles first: the cluster goes on working
    mine.close()
    my_scope.close()
    again = cl.keys(ids, ids // 7)
    assert len(again.groups()[0]) == len(np.unique(ids // 7))
    cl.close()
    _raises(N.ORR_ESTATE, lambda: again.groups(), "orphaned")
    again.close()


def test_maintenance_on_the_shards_mirrored_on_the_twin():
    c = _c2_parts(capacity=N2 + 500)
    cl, twin, ck, tk, cm, tm, ids, keys, edges, rng = c["cl"], c["twin"], c["ck"], c["tk"], c["cm"], c["tm"], c["ids"], c["keys"], c["edges"], c["rng"]
    probe = np.array(list(PLAN) + [NONE, 1_000, 1_200], np.int64)

    def check(what):
        assert np.array_equal(cm.order(), tm.order()), what
        _both_groups(c, what=what)
        _both(c, probe, what=what)

    try:
        check("made")
        # 1. deletes on shard 2 only: 40 of BIG's members there (every block behind them shifts) and 500 other rows
        pos = np.nonzero(keys == BIG)[0]
        gone = np.unique(np.concatenate([ids[pos[300:340]], ids[rng.choice(np.arange(edges[2], edges[3]), 500, replace=False)]]))
        assert cl.shard(2).delete_rows(gone) == len(gone) == twin.delete_rows(gone)
        for i in gone:
            del cm.emb[int(i)], cm.key[int(i)], tm.emb[int(i)], tm.key[int(i)]
        check("deleted")
        # 2. update on a shard: new vectors for members of BIG on shard 0, and members that lose their embedding
        upd = ids[pos[10:40]]
        new = (rng.standard_normal((len(upd), D2)) * 10.0 ** rng.uniform(-10, 10, (len(upd), D2))).astype(np.float32)
        assert cl.shard(0).update_rows(upd, new) == len(upd) == twin.update_rows(upd, new)
        lost = ids[pos[100:105]]
        assert cl.shard(0).update_rows(lost, None) == len(lost) == twin.update_rows(lost, None)
        for m in (cm, tm):
            for r, i in enumerate(upd):
                m.emb[int(i)] = new[r]
            for i in lost:
                m.emb[int(i)] = np.zeros(D2, np.float32)
        check("updated")
        # 3. compaction
        assert cl.compact() == len(gone) == twin.compact()
        check("compacted")
        # 4. insertion into shard 1, as new as its newest row; the new rows read ORR_KEY_NONE until the host sets them
        m = 300
        live_created = c["created"][~np.isin(ids, gone)]
        at = sum(cl.shard(g).rows for g in range(1))
        e2 = (rng.standard_normal((m, D2)) * 10.0 ** rng.uniform(-15, 15, (m, D2))).astype(np.float32)
        c2 = np.full(m, live_created[at], np.int64)
        b2 = c["rowbytes"][:m]
        off2 = np.arange(m + 1, dtype=np.int64) * b2.shape[1]
        new_ids = 90_000_000 + np.arange(m, dtype=np.int64)
        assert cl.insert_rows(1, e2, c2, b2.reshape(-1), off2, row_ids=new_ids) == m
        twin.insert_rows(e2, c2, b2.reshape(-1), off2, row_ids=new_ids)
        for mdl in (cm, tm):
            for r, i in enumerate(new_ids):
                mdl.emb[int(i)], mdl.key[int(i)] = e2[r], NONE
        check("inserted")
        k2 = np.where(np.arange(m) % 3 == 0, BIG, np.where(np.arange(m) % 3 == 1, K255, 77_000_000 + np.arange(m))).astype(np.int64)
        assert ck.set(new_ids, k2) == m == tk.set(new_ids, k2)
        for mdl in (cm, tm):
            for i, k in zip(new_ids, k2):
                mdl.key[int(i)] = int(k)
        check("keys set")
    finally:
        for h in (ck, tk, cl, twin):
            h.close()


def test_six_threads_on_the_cluster_each_get_the_single_thread_answer():
    c = _c2()
    cl, ck, ids, edges = c["cl"], c["ck"], c["ids"], c["edges"]
    sc = cl.scope(ids[edges[1] - 2_000:edges[3] + 500])
    listed = [np.array(list(PLAN), np.int64), np.array([BIG, KA], np.int64), np.array([KB, W600, NONE], np.int64)]
    calls = [lambda: ck.centroids(listed[0], sums=True), lambda: ck.centroids(listed[1], sc, sums=True), lambda: ck.groups(),
             lambda: sc.centroid(sums=True), lambda: ck.centroids(listed[2], sums=True), lambda: ck.groups(sc)]
    alone = [f() for f in calls]
    results, errors = [None] * 6, []

    def work(i):
        try:
            for _ in range(3):
                results[i] = calls[i]()
        except BaseException as e:                      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a call did not come back: the lanes or the holds deadlocked"
    assert not errors, errors
    for got, want in zip(results, alone):
        for a, b in zip(got, want):
            if np.asarray(a).dtype == np.float64:
                assert _same64(a, b)
            elif np.asarray(a).dtype == np.float32:
                assert _same32(a, b)
            else:
                assert np.array_equal(a, b)
    sc.close()
