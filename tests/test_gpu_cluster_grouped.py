"""Several cluster scopes in one batch: orr_cluster_search_batch_in_scopes and the shard form it drives,
orr_search_shard_in_scopes.  The contract: query b's rows, order and fp64 scores are bit for bit what
orr_cluster_search_batch_in_scope returns for it with scopes[query_scope[b]] -- so every result is compared with search_in_scope
on the cluster with the query's scope, on the large shards also with search_in_scopes of ONE index over all rows with twin
scopes, and a stated subset with the oracle on the sub-corpus.  Every comparison is exact: rows and counts with np.array_equal,
fp64 scores bit for bit, NaN = NaN.

The clusters, their single-index twins and the scopes' cases are tests/test_gpu_cluster_scope.py's and
tests/test_gpu_cluster_scope_handle.py's fixtures, built once per session and only read here; the maintenance, refusal and
thread tests make clusters or scopes of their own, which they change."""
import threading

import numpy as np
import pytest

import test_gpu_cluster_scope as base
import test_gpu_cluster_scope_handle as hnd
import test_gpu_scope_handle as hbase
from helpers import NOW, orc, pkg

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
TEXTS, CUTS = base.TEXTS, base.CUTS
TRAILER, TWO_STAGE = base.TRAILER, base.TWO_STAGE
HALF, N, DIM = base.HALF, base.N, base.DIM
_same, _equal = base._same, base._same_results
_terms, _raises, _make, _positions, _reset, _launches = hnd._terms, hnd._raises, hnd._make, hnd._positions, hnd._reset, hnd._launches


def _row(res, b):
    return res[0][b], res[1][b], res[2][b]


def _check_against_in_scope(cl, q, terms, now, topk, limit, scopes, query_scope, got, what):
    """got (a grouped result) query by query against the in-scope cluster call of the query's scope (one call per named scope
    over the whole batch: a query's result does not depend on its batch)."""
    ref = {}
    for b, g in enumerate(query_scope):
        if g not in ref:
            ref[g] = cl.search_in_scope(q, terms, now, topk, scopes[g], candidate_limit=limit)
        want = _row(ref[g], b)
        have = _row(got, b)
        assert np.array_equal(have[0], want[0]) and _same(have[1], want[1]) and have[2] == want[2], what + (b, g, have[0][:6], want[0][:6])
    return ref


# ---- 1. semantics: three small shards (the list path) ---------------------------------------------------------------------------

# the scopes of a call, in the order that b % n names them: the duplicate (5) and the empty one (3) are named from B = 7 / 4 on
_SMALL_ORDER = ("wide", "window across both borders", "any of three terms", "empty", "an id on two shards", "wide",
                "window inside shard 1", "one shard only", "unknown and negative ids", "window = shard 1 exactly",
                "open towards the old", "all of two terms", "a term matching nothing")
_SMALL_ORACLE = ("wide", "window across both borders", "any of three terms")
_SS = {}


def _small_scopes():
    if _SS:
        return _SS["v"]
    cl, one, rows, qs, cases = hnd._small()
    by_name = {name: (kind, arg) for name, kind, arg in cases}
    made = {}
    scopes, keeps = [], []
    for name in _SMALL_ORDER:
        if name not in made:
            made[name] = _make(cl, *by_name[name])
        scopes.append(made[name])                                            # "wide" twice: the SAME handle listed twice
        keeps.append(_positions(rows, *by_name[name]))
    kinds = [by_name[n][0] for n in _SMALL_ORDER]
    assert kinds.count("ids") == 6 and kinds.count("ticks") == 4 and kinds.count("terms") == 3
    _SS["v"] = (cl, rows, qs, scopes, keeps)
    return _SS["v"]


@pytest.mark.parametrize("with_vectors", [True, False])
@pytest.mark.parametrize("B", [1, 4, 7])
def test_small_cluster_grouped_equals_the_in_scope_call_and_the_oracle(B, with_vectors):
    cl, rows, qs, scopes, keeps = _small_scopes()
    n_sc = len(scopes)
    q = np.stack([qs[b % 4] for b in range(B)])
    if B >= 4:
        q[3] = 0.0                                                           # a zero query vector
    q = np.ascontiguousarray(q) if with_vectors else None
    texts = [TEXTS[b % 4] for b in range(B)]
    terms = _terms(texts)
    qscope = [b % n_sc for b in range(B)]
    n = CUTS[-1]
    assert scopes[0] is scopes[5] and scopes[3].rows == 0                    # listed twice; empty; scopes 7 .. 12 are named by nobody
    against_oracle = 0
    for topk in (1, 10, 100, -1):
        for limit in (1, 300, n):
            what = (B, with_vectors, topk, limit)
            got = cl.search_in_scopes(q, terms, NOW, topk, scopes, qscope, candidate_limit=limit)
            _check_against_in_scope(cl, q, terms, NOW, topk, limit, scopes, qscope, got, what)
            for b, g in enumerate(qscope):
                assert got[2][b] == min(max(1, topk), len(keeps[g]), max(1, limit)), what + (b,)
            if B == 4 and topk in (10, -1) and limit in (300, n):            # the stated subset against the oracle
                for b, g in enumerate(qscope):
                    if _SMALL_ORDER[g] not in _SMALL_ORACLE:
                        continue
                    keep = keeps[g]
                    orow, osc, _ = rows.corpus(keep).search([] if q is None else q[b], texts[b], NOW, max(1, topk), candidate_limit=limit)
                    k = int(got[2][b])
                    assert list(got[0][b, :k]) == [int(rows.m.ids[keep[r]]) for r in orow], what + (b,)
                    assert _same(got[1][b, :k], np.asarray(osc)) and (got[0][b, k:] == -1).all(), what + (b,)
                    against_oracle += 1
    assert against_oracle == (12 if B == 4 else 0)
    # every query in ONE scope, and scopes nobody names around it: the in-scope call itself
    got = cl.search_in_scopes(q, terms, NOW, 10, scopes, [2] * B, candidate_limit=n)
    assert _equal(got, cl.search_in_scope(q, terms, NOW, 10, scopes[2], candidate_limit=n))
    # ... every query in the empty scope
    got = cl.search_in_scopes(q, terms, NOW, 10, scopes, [3] * B, candidate_limit=n)
    assert (got[2] == 0).all() and (got[0] == -1).all()


# ---- 2. the shared screen: two shards of 200,000 x 128 -------------------------------------------------------------------------

_BS = {}
_BIG_NAMES = ("100,000 ids over both shards", "a time window over the border", "any of four terms")


def _big_scopes():
    """(cluster, twin index, model, texts, queries, cluster scopes, twin scopes, positions): the three large scopes of the handle
    test, a 200-row scope (a list group) and an empty one."""
    if _BS:
        return _BS["v"]
    cl, one, model, texts, q_all, big = hnd._big()
    rng = np.random.default_rng(5151)
    few = np.sort(rng.choice(N, 200, replace=False))
    scopes = [big[n][0] for n in _BIG_NAMES] + [cl.scope(model.ids[few]), cl.scope(np.zeros(0, np.int64))]
    twins = [big[n][1] for n in _BIG_NAMES] + [one.scope(model.ids[few]), one.scope(np.zeros(0, np.int64))]
    keeps = [big[n][2] for n in _BIG_NAMES] + [few, np.zeros(0, np.int64)]
    _BS["v"] = (cl, one, model, texts, q_all, scopes, twins, keeps)
    return _BS["v"]


def _limits(scopes):
    ids0, ids_all = scopes[0].shard(0).rows, scopes[0].rows
    win0 = scopes[1].shard(0).rows
    term0, term_all = scopes[2].shard(0).rows, scopes[2].rows
    a = ids0 + 20_000                    # the id scope's limit ends inside shard 1, the window's inside shard 0
    b = term0 + 1_000                    # the term scope's ends inside shard 1, the id scope's and the window's inside shard 0
    assert ids0 < a < ids_all and a < win0 and term0 < b < term_all and b < ids0 and b < win0, (ids0, ids_all, win0, term0, term_all)
    return a, b


@pytest.mark.parametrize("B", [8, 40])
def test_two_stage_cluster_grouped_equals_the_in_scope_call_and_one_index(B):
    syn = hbase._syn()
    cl, one, model, texts_all, q_all, scopes, twins, keeps = _big_scopes()
    terms = _terms(list(texts_all[:B]))
    q = np.ascontiguousarray(q_all[:B])
    qscope = [b % 5 for b in range(B)]
    lim_a, lim_b = _limits(scopes)
    for limit in (N, 300, lim_a, lim_b):
        for topk in (1, 10, 64):
            what = (B, topk, limit)
            _reset(cl)
            got = cl.search_in_scopes(q, terms, syn.NOW_TICKS, topk, scopes, qscope, candidate_limit=limit)
            st = [cl.shard(g).search_stats() for g in range(2)]
            cst = cl.search_stats()
            _check_against_in_scope(cl, q, terms, syn.NOW_TICKS, topk, limit, scopes, qscope, got, what)
            assert _equal(got, one.search_in_scopes(q, terms, syn.NOW_TICKS, topk, twins, qscope, candidate_limit=limit)), what
            for b, g in enumerate(qscope):
                assert got[2][b] == min(topk, len(keeps[g]), limit), what + (b,)
            if topk < 64 and limit in (N, lim_a):                             # k' within a selection list: both shards share a screen
                assert cst["pass_mode"] == 6, what + (cst,)
                for g in (0, 1):
                    assert st[g]["survivor_samples"] > 0 and st[g]["exact_pass_queries"] == 0, what + (g, st[g])
            if topk < 64 and limit == N and cst["requeried"] == 0:            # ... and nothing ran behind it
                assert st[0]["pass_mode"] == 6 and st[1]["pass_mode"] == 6, what + (st,)
    # a stated subset against the oracle: B = 8, topk 10, the id scope's and the term scope's queries
    if B == 8:
        width = model.rowbytes.shape[1]
        for limit in (N, lim_a):
            rows, scores, counts = cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, scopes, qscope, candidate_limit=limit)
            for b in (0, 2, 5):
                keep = keeps[qscope[b]]
                corpus = orc.OracleCorpus(np.ascontiguousarray(model.emb[keep]), model.created[keep],
                                          (np.ascontiguousarray(model.rowbytes[keep]).reshape(-1), np.arange(len(keep) + 1, dtype=np.int64) * width))
                orow, osc, _ = corpus.search(q[b], texts_all[b], syn.NOW_TICKS, 10, candidate_limit=limit, threads=16)
                k = int(counts[b])
                assert list(rows[b, :k]) == [int(model.ids[keep[r]]) for r in orow], (limit, b)
                assert _same(scores[b, :k], np.asarray(osc)), (limit, b)


def _screens(st):
    return sum(v for k, v in st.items() if k.startswith("screen_") and "prefix" not in k)


def test_one_screen_per_slice_and_one_gather_per_front():
    syn = hbase._syn()
    cl, one, model, texts_all, q_all, scopes, twins, keeps = _big_scopes()
    B = 8
    terms, q = _terms(list(texts_all[:B])), np.ascontiguousarray(q_all[:B])
    qscope = [b % 5 for b in range(B)]
    lim_a, lim_b = _limits(scopes)
    # the loop of in-scope calls screens once per large scope on every shard: the check below is not vacuous
    loop = _launches(cl, lambda: [cl.search_in_scope(q, terms, syn.NOW_TICKS, 10, scopes[g], candidate_limit=N) for g in range(3)])
    for g in (0, 1):
        assert _screens(loop[g]) == 3 and "group_gather_clip" not in loop[g], (g, sorted(loop[g]))
    # (lim_b leaves shard 1 a thousand rows of one scope and the 200-row scope: no screen group there, and a clipped list group
    # clips inside its own in-scope pass; the two limits of this test leave screen groups on both shards)
    for limit in (N, lim_a):
        cl.search_stats(reset=True)
        st = _launches(cl, lambda: cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, scopes, qscope, candidate_limit=limit))
        requeried = cl.search_stats()["requeried"]
        for g in (0, 1):
            what = (limit, g, sorted(st[g].items()))
            if requeried == 0:
                assert _screens(st[g]) == 1, what                              # ONE screen for the slice, not one per scope
                assert st[g].get("group_gather_clip", 0) == 1, what            # exactly one launch in front of it
                assert "mask_clip" not in st[g], what                         # (the 200-row scope takes part whole: no clip of its own)
            for k in ("scope_lookup", "scope_counts", "scope_handle_lookup"):
                assert k not in st[g], what
    # the single index's handle path runs through the same front: one gather, no clip launch of its own
    one.set_profiling(True)
    one.search_in_scopes(q, terms, syn.NOW_TICKS, 10, twins, qscope, candidate_limit=lim_a)
    st1 = {k: v["launches"] for k, v in one.kernel_stats().items()}
    one.set_profiling(False)
    assert st1.get("group_gather_clip", 0) == 1 and "mask_clip" not in st1 and "scope_lookup" not in st1, sorted(st1.items())


def test_different_clips_per_group_and_per_shard_in_one_pass():
    """The clip case: one limit ends the id scope inside shard 1 and the window inside shard 0, another ends the term scope inside
    shard 1 -- every group's clip is its own on every shard.  The last row that takes part and the first that does not are
    planted as near-duplicates of two queries: a clip too far out lets a row in, one too far in drops a row."""
    syn = hbase._syn()
    cl, one, model, texts_all, q_all, scopes, twins, keeps = _big_scopes()
    B = 8
    terms = _terms(list(texts_all[:B]))
    qscope = [0, 1, 2, 0, 1, 2, 0, 1]
    lim_a, lim_b = _limits(scopes)
    rng = np.random.default_rng(77)
    for limit in (lim_a, lim_b):
        q = np.ascontiguousarray(q_all[:B]).copy()
        # queries 0 .. 2: the last row inside their scope's limit; 3 .. 5: the first row behind it
        for b in range(6):
            keep = keeps[qscope[b]]
            if limit >= len(keep):
                continue
            r = keep[limit - 1] if b < 3 else keep[limit]
            q[b] = model.emb[r] + rng.standard_normal(DIM).astype(np.float32) * np.float32(0.01)
        got = cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, scopes, qscope, candidate_limit=limit)
        _check_against_in_scope(cl, q, terms, syn.NOW_TICKS, 10, limit, scopes, qscope, got, (limit,))
        assert _equal(got, one.search_in_scopes(q, terms, syn.NOW_TICKS, 10, twins, qscope, candidate_limit=limit)), limit
        for b in range(6):
            keep = keeps[qscope[b]]
            if limit >= len(keep):
                continue
            if b < 3:
                assert got[0][b, 0] == model.ids[keep[limit - 1]], (limit, b)     # the last row that takes part ranks first
            else:
                assert model.ids[keep[limit]] not in got[0][b], (limit, b)        # the first row behind the limit never appears


def test_no_row_leaks_from_another_group_across_shards():
    syn = hbase._syn()
    cl, one, model, texts_all, fam, plants, tie_vec, mass_vec = base._big()
    qq, inside, outside = plants["random 10 %"]                             # qq[0]: a near-duplicate of row `inside`, in shard 1
    assert inside >= HALF
    B = 8
    q = np.ascontiguousarray(qq[:B])
    terms = _terms(list(texts_all[:B]))
    rows_a = fam["random 10 %"]
    rows_b = np.setdiff1d(fam["older half of each shard"], rows_a)          # scope B holds no row of scope A
    assert inside in rows_a and inside not in rows_b
    a, b = cl.scope(model.ids[rows_a]), cl.scope(model.ids[rows_b])
    try:
        # asked inside A the planted row ranks first; asked inside B it must not appear, though A's group screens it in the same pass
        got = cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, [a, b], [0] + [b_ % 2 for b_ in range(1, B)], candidate_limit=N)
        assert got[0][0, 0] == model.ids[inside]
        qscope = [1] + [b_ % 2 for b_ in range(1, B)]
        _reset(cl)
        got = cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, [a, b], qscope, candidate_limit=N)
        assert cl.search_stats()["pass_mode"] == 6
        assert model.ids[inside] not in got[0][0]
        in_b = set(model.ids[rows_b].tolist())
        in_a = set(model.ids[rows_a].tolist())
        for b_, g in enumerate(qscope):
            k = int(got[2][b_])
            assert set(got[0][b_, :k].tolist()) <= (in_b if g == 1 else in_a), b_
        _check_against_in_scope(cl, q, terms, syn.NOW_TICKS, 10, N, [a, b], qscope, got, ("leak",))
    finally:
        a.close()
        b.close()


def test_an_overflow_on_one_shard_only_stays_exact_and_grows_the_calls_own_buffers():
    """(Runs in front of every test that searches for mass_vec inside a scope holding the mass: those grow shard 1's own buffers
    for good, after which nothing overflows here.)"""
    syn = hbase._syn()
    cl, one, model, texts_all, fam, plants, tie_vec, mass_vec = base._big()
    B = 8
    q = np.ascontiguousarray(plants["older half of each shard"][0][:B]).copy()
    q[5] = mass_vec                                                          # parallel to 20,000 rows of shard 1 ...
    terms = _terms(list(texts_all[:B]))
    rows_a = np.setdiff1d(fam["random 10 %"], base.MASS)                     # ... which lie OUTSIDE query 5's scope
    rows_b = fam["older half of each shard"]                                 # ... and inside the other group's
    assert set(base.MASS.tolist()) <= set(rows_b.tolist())
    a, b = cl.scope(model.ids[rows_a]), cl.scope(model.ids[rows_b])
    try:
        qscope = [1, 1, 1, 1, 1, 0, 0, 0]
        _reset(cl)
        before = [cl.shard(g).search_stats() for g in range(2)]
        got = cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, [a, b], qscope, candidate_limit=N)
        after = [cl.shard(g).search_stats() for g in range(2)]
        _check_against_in_scope(cl, q, terms, syn.NOW_TICKS, 10, N, [a, b], qscope, got, ("overflow",))
        assert not set(got[0][5].tolist()) & set(model.ids[base.MASS].tolist())
        assert after[1]["buffer_growths"] > before[1]["buffer_growths"], (before[1], after[1])
        assert after[0]["buffer_growths"] == before[0]["buffer_growths"], (before[0], after[0])
        for g in (0, 1):
            assert after[g]["survivor_capacity"] == before[g]["survivor_capacity"], (g, before[g], after[g])
    finally:
        a.close()
        b.close()


def test_a_tie_at_the_cut_goes_down_its_own_scopes_ladder():
    syn = hbase._syn()
    cl, one, model, texts_all, fam, plants, tie_vec, mass_vec = base._big()
    B = 8
    q = np.ascontiguousarray(plants["older half of each shard"][0][:B]).copy()
    q[2] = tie_vec                                                           # equal to 70 rows of one timestamp in shard 0: a tie at the cut
    terms = _terms(list(texts_all[:B]))
    rows_a, rows_b = fam["random 10 %"], fam["older half of each shard"]
    assert set(base.TIE.tolist()) <= set(rows_b.tolist())
    a, b = cl.scope(model.ids[rows_a]), cl.scope(model.ids[rows_b])
    try:
        qscope = [0, 0, 1, 1, 0, 0, 1, 1]
        _reset(cl)
        got = cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, [a, b], qscope, candidate_limit=N)
        st = cl.search_stats()
        _check_against_in_scope(cl, q, terms, syn.NOW_TICKS, 10, N, [a, b], qscope, got, ("tie",))
        assert set(got[0][2].tolist()) <= set(model.ids[base.TIE].tolist()) and list(got[0][2]) == sorted(got[0][2])
        assert st["pass_mode"] == 6 and st["passes"] >= 2, st
        # only the tied query ran again: its scope's ladder from the first rung (one requeried query per rung), the others were final
        first = st["requeried"]
        _reset(cl)
        cl.search_in_scope(np.ascontiguousarray(q[2:3]), terms[2:3], syn.NOW_TICKS, 10, b, candidate_limit=N)
        alone = cl.search_stats()
        assert alone["requeried"] >= 1                                       # the tie defeats the first rung of the in-scope call too
        assert first == alone["requeried"] + 1, (first, alone)
    finally:
        a.close()
        b.close()


# ---- 3. the shard form, driven by hand --------------------------------------------------------------------------------------------

def _merged_grouped(P, shards, scopes, qscope, q, terms, now, topk, limit, dim, kp, shard_pass=0, kp_max=1 << 16):
    """The loop a multi-shard caller of the grouped shard form runs: lives from the handles, prefix sums per scope, one call per
    shard, merge, and k' x 4 for everything while a query stays uncertified."""
    G = len(shards)
    live = np.array([[sc.shard(g).rows for sc in scopes] for g in range(G)], np.int64)          # [shard][scope]
    before = np.concatenate([np.zeros((1, len(scopes)), np.int64), np.cumsum(live, axis=0)[:-1]])
    took = np.minimum(live, np.maximum(0, max(1, limit) - before))
    while True:
        recs = np.stack([shards[g].search_shard_in_scopes(q, terms, now, kp, limit, [sc.shard(g) for sc in scopes], qscope, before[g],
                                                          topk=topk, shard_pass=shard_pass) for g in range(G)])
        rows, scores, counts, unc = P.merge_candidates(recs, dim, q, terms, now, topk)
        if unc == 0 or kp >= kp_max:
            break
        kp *= 4
    assert unc == 0
    return (rows, scores, counts), recs, kp, took, before


def test_grouped_shard_form_on_three_small_shards():
    P = pkg()
    cl, rows, qs, scopes_all, keeps = _small_scopes()
    shards = [cl.shard(g) for g in range(3)]
    scopes = [scopes_all[i] for i in (0, 1, 2, 3, 4, 0, 7)]                   # a duplicate, the empty one, one on a single shard
    terms = _terms(TEXTS)
    for qscope in ([0, 1, 2, 3], [4, 5, 6, 1], [2, 2, 0, 0]):
        for topk, limit in ((10, 300), (10, 6000), (5, 1), (100, 6000)):
            what = (qscope, topk, limit)
            kp0 = 32 if topk < 64 else 128
            got, recs, kp, took, before = _merged_grouped(P, shards, scopes, qscope, qs, terms, NOW, topk, limit, 64, kp0)
            trailers = recs[:, :, kp]
            assert ((trailers["flags"] & TRAILER) != 0).all()
            assert np.array_equal(trailers["order_key"], took[:, qscope]), what                  # the took of the query's OWN scope
            valid = recs[:, :, :kp]["row_id"] >= 0
            assert np.array_equal(valid.sum(axis=2), trailers["matches"]), what
            assert _equal(got, cl.search_in_scopes(qs, terms, NOW, topk, scopes, qscope, candidate_limit=limit)), what
            again = _merged_grouped(P, shards, scopes, qscope, qs, terms, NOW, topk, limit, 64, kp0, shard_pass=1)[0]
            assert _equal(got, again), what                                                     # pass = 1: the same merged result
    # one used scope: orr_search_shard_in_scope's records, record for record (scopes nobody names, and the empty one, beside it)
    for g in range(3):
        before = [sum(sc.shard(s).rows for s in range(g)) for sc in scopes]
        many = shards[g].search_shard_in_scopes(qs, terms, NOW, 32, 300, [sc.shard(g) for sc in scopes], [1, 1, 1, 1], before, topk=10)
        single = shards[g].search_shard_in_scope(qs, terms, NOW, 32, 300, scopes[1].shard(g), scope_before=before[1], topk=10)
        assert many.tobytes() == single.tobytes(), g
        # ... and with two of the four queries in the empty scope: the other two's records are the single call's for them
        mixed = shards[g].search_shard_in_scopes(qs, terms, NOW, 32, 300, [sc.shard(g) for sc in scopes], [1, 3, 1, 3], before, topk=10)
        sub = shards[g].search_shard_in_scope(np.ascontiguousarray(qs[[0, 2]]), [terms[0], terms[2]], NOW, 32, 300, scopes[1].shard(g),
                                              scope_before=before[1], topk=10)
        assert mixed[[0, 2]].tobytes() == sub.tobytes(), g
        assert (mixed[[1, 3]][:, :32]["row_id"] == -1).all() and (mixed[[1, 3]][:, 32]["order_key"] == 0).all(), g


def test_grouped_shard_form_on_the_two_stage_shards():
    P, syn = pkg(), hbase._syn()
    cl, one, model, texts_all, q_all, scopes, twins, keeps = _big_scopes()
    B = 8
    terms = _terms(list(texts_all[:B]))
    q = np.ascontiguousarray(q_all[:B])
    shards = [cl.shard(0), cl.shard(1)]
    qscope = [b % 5 for b in range(B)]
    lim_a, lim_b = _limits(scopes)
    for limit in (N, lim_a):
        got, recs, kp, took, before = _merged_grouped(P, shards, scopes, qscope, q, terms, syn.NOW_TICKS, 10, limit, DIM, 32)
        trailers = recs[:, :, kp]
        assert np.array_equal(trailers["order_key"], took[:, qscope]), limit
        for g in (0, 1):
            for b, s in enumerate(qscope):
                screened = (trailers[g, b]["flags"] & TWO_STAGE) != 0
                if s < 3 and took[g, s] > 0 and kp == 32:
                    assert screened and trailers[g, b]["norm_b"] == trailers[g, b]["norm_b"], (limit, g, b)     # behind the screen: a floor
                if s >= 3:
                    assert not screened, (limit, g, b)                         # the list group and the empty scope
        assert _equal(got, cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, scopes, qscope, candidate_limit=limit)), limit
        again = _merged_grouped(P, shards, scopes, qscope, q, terms, syn.NOW_TICKS, 10, limit, DIM, 32, shard_pass=1)
        assert ((again[1][:, :, again[2]]["flags"] & TWO_STAGE) == 0).all()
        assert _equal(got, again[0]), limit
    # one used scope on the screening shards: record for record the in-scope shard form's
    for g in (0, 1):
        before = [sum(sc.shard(s).rows for s in range(g)) for sc in scopes]
        many = shards[g].search_shard_in_scopes(q, terms, syn.NOW_TICKS, 32, lim_a, [sc.shard(g) for sc in scopes], [0] * B, before, topk=10)
        single = shards[g].search_shard_in_scope(q, terms, syn.NOW_TICKS, 32, lim_a, scopes[0].shard(g), scope_before=before[0], topk=10)
        assert many.tobytes() == single.tobytes(), g


# ---- 4. maintenance: three shards of 23,000 x 64 ----------------------------------------------------------------------------------

def test_grouped_search_follows_delete_compact_and_insert():
    P, syn = pkg(), hbase._syn()
    NM, CUT_M, DIM_M = hnd.NM, hnd.CUT_M, hnd.DIM_M
    emb, created, rowbytes = hbase._rows(NM, DIM_M)
    ids = np.arange(NM, dtype=np.int64) * 3 + 11
    model = hbase.Model(emb, created, rowbytes, ids)
    off = np.arange(CUT_M + 1, dtype=np.int64) * syn.ROW_BYTES
    cl = P.RecallCluster([0, 0, 0], DIM_M, capacity_rows_per_shard=CUT_M + 1000)
    for g in range(3):
        r0, r1 = g * CUT_M, (g + 1) * CUT_M
        cl.shard(g).append(emb[r0:r1], created[r0:r1], rowbytes[r0:r1].reshape(-1), off, row_ids=ids[r0:r1])
    cl.seal()
    one = hbase._build(emb, created, rowbytes, ids, NM + 1000)
    B = 8
    q = syn.query_vectors(0, B, DIM_M, NM).numpy()
    terms = _terms(syn.query_texts(0, B, NM))
    rng = np.random.default_rng(78)
    shard_of = {int(i): g for g in range(3) for i in ids[g * CUT_M:(g + 1) * CUT_M]}
    words = [syn.vocab_word(t) for t in (77, 2040)]
    t0, t1 = int(created[50_000]), int(created[10_000])                      # a window over all three shards
    pick = model.ids[np.sort(rng.choice(NM, 20_000, replace=False))]
    mine = [cl.scope(pick), cl.scope_ticks(t0, t1), cl.scope_terms(words, "any")]
    twins = [one.scope(pick), one.scope_ticks(t0, t1), one.scope_terms(words, "any")]
    qscope = [b % 3 for b in range(B)]

    def delete(gone):
        for g in range(3):
            part = np.array([i for i in gone if shard_of[int(i)] == g], np.int64)
            assert cl.shard(g).delete_rows(part) == len(part)
        assert one.delete_rows(gone) == len(gone)
        model.delete(gone)

    def check(step):
        for sc, tw in zip(mine, twins):
            assert sc.rows == tw.rows and np.array_equal(sc.row_ids(), tw.row_ids()), step
        for limit in (NM, 5_000):
            got = cl.search_in_scopes(q, terms, syn.NOW_TICKS, 10, mine, qscope, candidate_limit=limit)
            assert _equal(got, one.search_in_scopes(q, terms, syn.NOW_TICKS, 10, twins, qscope, candidate_limit=limit)), (step, limit)
            _check_against_in_scope(cl, q, terms, syn.NOW_TICKS, 10, limit, mine, qscope, got, (step, limit))

    check("as made")
    delete(rng.choice(model.ids, 3_000, replace=False))
    check("after deletes through the shards")
    removed = int(model.dead.sum())
    assert cl.compact() == removed and one.compact() == removed
    model.compact()
    check("after compact")
    n1 = cl.shard(0).rows
    lo, hi = n1 + 200, n1 + cl.shard(1).rows - 200
    new_emb, _, new_bytes = hbase._rows(131, DIM_M, row0=5_000_000)
    new_created = (model.created[rng.choice(np.arange(lo, hi), 131, replace=False)] - 3).astype(np.int64)
    new_ids = 10_000_000 + np.arange(131, dtype=np.int64)
    new_off = np.arange(132, dtype=np.uint64) * new_bytes.shape[1]
    assert cl.insert_rows(1, new_emb, new_created, new_bytes.reshape(-1), new_off, row_ids=new_ids) == 131
    assert one.insert_rows(new_emb, new_created, new_bytes.reshape(-1), new_off, row_ids=new_ids) == 131
    check("after insert")
    assert mine[0].add_ids(new_ids) == 131 and twins[0].add_ids(new_ids) == 131
    check("add_ids names the new rows")
    for s in mine + twins:
        s.close()
    cl.close()
    one.close()


# ---- 5. refusals and threads --------------------------------------------------------------------------------------------------------

def test_an_unsealed_cluster_device_pointers_foreign_and_orphaned_scopes_are_refused():
    import torch
    import omni_recall_rag_amd.index as index
    P = pkg()
    C = P.native.C
    cl, ids = hnd._tiny_cluster()
    a, b = cl.scope(ids[:100]), cl.scope_ticks(I64_MIN, I64_MAX)
    q, terms = np.zeros((2, 64), np.float32), [[b"abc"], [b"abd"]]
    pool, toff, qoff = index.pack_terms(terms)
    rows, scores, counts = np.full((2, 10), 7, np.int64), np.full((2, 10), 7.0), np.full(2, 7, np.int32)
    handles = (C.c_void_p * 2)(a._h, b._h)
    qs = np.array([0, 1], np.int32)

    def raw(cluster, qptr):
        return P.native.hip.orr_cluster_search_batch_in_scopes(cluster, 2, 64, qptr, pool.ctypes.data, toff.ctypes.data, qoff.ctypes.data, NOW, 10, 300,
                                                               2, C.cast(handles, C.c_void_p), qs.ctypes.data, rows.ctypes.data, scores.ctypes.data,
                                                               counts.ctypes.data)
    assert raw(cl._h, q.ctypes.data) == 0 and (counts == 10).all()           # the call as such is fine
    rows[:], scores[:], counts[:] = 7, 7.0, 7
    dq = torch.from_numpy(q).cuda()
    assert raw(cl._h, dq.data_ptr()) == P.native.ORR_EINVAL and b"host memory" in P.native.hip.orr_last_error()
    fresh, _ = hnd._tiny_cluster(seal=False)
    assert raw(fresh._h, q.ctypes.data) == P.native.ORR_ESTATE and b"not sealed" in P.native.hip.orr_last_error()
    fresh.close()
    other, other_ids = hnd._tiny_cluster()
    assert raw(other._h, q.ctypes.data) == P.native.ORR_EINVAL and b"another cluster" in P.native.hip.orr_last_error()
    foreign = other.scope(other_ids[:50])
    _raises(P.native.ORR_EINVAL, lambda: cl.search_in_scopes(q, terms, NOW, 10, [a, foreign], [0, 0]))        # named by nobody, refused all the same
    _raises(P.native.ORR_EINVAL, lambda: cl.shard(1).search_shard_in_scopes(q, terms, NOW, 8, 300, [a.shard(1), b.shard(0)], [0, 0], [0, 0]))
    assert b"another shard" in P.native.hip.orr_last_error()
    assert (rows == 7).all() and (scores == 7.0).all() and (counts == 7).all()                                   # every refusal left the outputs alone
    # an orphaned scope among live ones
    other.close()
    _raises(P.native.ORR_ESTATE, lambda: cl.search_in_scopes(q, terms, NOW, 10, [a, foreign, b], [0, 2]))
    assert b"orphaned" in P.native.hip.orr_last_error()
    assert _equal(cl.search_in_scopes(q, terms, NOW, 10, [a, b], [0, 1]),
                  tuple(np.stack([x[0], y[1]]) for x, y in zip(cl.search_in_scope(q, terms, NOW, 10, a), cl.search_in_scope(q, terms, NOW, 10, b))))
    for s in (a, b, foreign):
        s.close()
    cl.close()


def test_four_threads_search_three_scopes_while_one_of_them_is_edited():
    cl, one, rows, qs, cases = hnd._small()
    by_name = {name: (kind, arg) for name, kind, arg in cases}
    terms = _terms(TEXTS)
    n = CUTS[-1]
    s1, s2 = _make(cl, *by_name["wide"]), _make(cl, *by_name["any of three terms"])
    window = _make(cl, *by_name["window across both borders"])              # rows on ALL three shards
    assert all(window.shard(g).rows > 0 for g in range(3))
    in_window = set(window.row_ids().tolist())
    live_ids = rows.m.ids[np.nonzero(rows.live & (np.arange(n) != 500) & (np.arange(n) != 2000))[0]]
    base_ids = np.array([i for i in live_ids if int(i) not in in_window][:400], np.int64)
    edited = cl.scope(base_ids)                                              # the two states: these rows, or these and the window's
    qscope = [0, 1, 2, 2]
    call = lambda: cl.search_in_scopes(qs, terms, NOW, 10, [s1, s2, edited], qscope, candidate_limit=n)
    before = call()
    edited.or_(window)
    after = call()
    edited.andnot(window)
    assert _equal(call(), before) and not _equal(before, after)
    window_ids = window.row_ids()
    bad, errors = [], []

    def search(i):
        try:
            for _ in range(8):
                got = call()
                for b in range(4):                                          # each query: the result before the edit or after it, whole
                    if all(np.array_equal(_row(got, b)[j], _row(before, b)[j]) for j in (0, 2)) and _same(got[1][b], before[1][b]):
                        continue
                    if not (all(np.array_equal(_row(got, b)[j], _row(after, b)[j]) for j in (0, 2)) and _same(got[1][b], after[1][b])):
                        bad.append((i, b))
                # the two queries of the edited scope saw the SAME state: an edit is on all shards or on none, for the whole call
                if not (_equal(tuple(x[2:] for x in got), tuple(x[2:] for x in before)) or _equal(tuple(x[2:] for x in got), tuple(x[2:] for x in after))):
                    bad.append((i, "mixed"))
        except Exception as e:                                                # noqa: BLE001
            errors.append(repr(e))

    def edit():
        try:
            for i in range(10):
                if i % 2 == 0:
                    edited.or_(window)
                else:
                    edited.add_ids(window_ids)
                edited.andnot(window)
        except Exception as e:                                                # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=search, args=(i,)) for i in range(4)] + [threading.Thread(target=edit)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not errors and not bad, (errors, bad)
    assert _equal(call(), before)
    for s in (s1, s2, window, edited):
        s.close()
