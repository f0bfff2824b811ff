"""The two-stage screen, seen directly: the floor every query is screened against and the survivors its fused epilogue keeps,
against the oracle's exact score of EVERY row.

A fast search is exact only while four links hold: (1) every approximate dot stays inside its stated bound, (2) the per-pair
int8 bound is sound, (3) the floor a query is screened against is a lower bound of its exact k-th best score, (4) the fused
epilogue keeps every pair whose exact score can reach that floor.  tests/test_gpu_screen_bounds.py and
tests/test_gpu_i8_gemm_exact.py pin (1) and (2).  End-to-end parity sees a violation of (3) or (4) only when a row of the true
top k is the one that gets lost; here orr_index_capture_screen hands over the floor (floor_key, L), the survivors' buffers and
the plan's scalars of a search's first pass, and for a dozen queries per batch every row's exact score E(b, r)
(OracleCorpus.score_all) decides what had to be kept and what had to go.  With F = key_score(floor_key + 1):

  invisible    the captured search returns the records of the same search without capture, bit for bit;
  floor valid  (3): L <= the kth best E over the participating rows (in-scope rows / the query's own group); floor_key 0 <=> L = -inf;
  floor tight  full-ranking prefix only: L >= the kth best lower bound of the prefix rows - 2 eps3 - (L - F);
  must keep    (4): a query that did not overflow holds EVERY participating row with E >= L.  No tolerance.
  must drop    a buffered pair with a key satisfies E + 2 bound + (L - F) >= F: a K-slice counted twice shows here;
  entries      pos < n, no position twice, key > floor_key, key_score(key) + (L - F) >= E, key_score(key) - E <= 2 bound + (L - F);
  overflow     cnt > cap: cnt >= min(|must-keep set|, cap + 1).

bound is the float64 restatement of tests/test_gpu_screen_bounds.py fed from screen_i8_consts (_bound_k2i for the int8 stream,
_bound_k2j for the int8 GEMM), or the captured eps1 for the bf16 forms; every expected score is the oracle's.

Where the assertions are narrower than "every buffered pair", and why:
  * An entry whose key is all ones was kept WITHOUT a key: a pair whose bound or accumulator is not finite, or one a thread
    appended straight to the buffer because its parking queue was full ("every buffer entry gets its exact key afterwards
    anyway", csrc/orr_epilogue.h, fused_epilogue).  The second kind passed only the fp32 test of pass 1, whose margin is
    1e-5 (1 + |F|) and, in the 16 x 16 x 64 form, the batch-wide query term QW in place of the pair's own (fused_epilogue16:
    "the bound only grows").  Must-drop with the pair's own bound is therefore not promised for them; they are counted and
    printed, and the strict form is evaluated on them for information.  Must-keep, pos < n and no-duplicates hold for them as
    for every entry.
  * A query without a floor (floor_key 0: a NaN query, fewer than kth rows) has no F: L - F is undefined, so the relations
    between a key and E are not evaluated for it; it must hold every row (it overflows) and the overflow assertion applies.
  * Under a scope mask an OVERFLOWED buffer is compacted in place by mask_survivors while its count stays as the overflow signal
    (its comment in csrc/orr_kernels.hip): which of the cap slots are the compacted ones is not recorded, so the entry
    assertions skip such a query (here: the NaN query) and the overflow assertion alone applies.
  * NaN scores.  The reference scores a pair NaN when the query holds a NaN, or the row a non-finite value; double.CompareTo puts
    NaN below every number.  The screens never drop such a pair ("NaN and overflowed sums are never dropped here",
    csrc/orr_epilogue.h; "never dropped: re-scored exactly later", csrc/orr_screen.hip; an int8 bound that is not finite), so
    must-keep counts every participating row whose exact score is NaN as a row to keep, whatever L.  Floor validity is asserted
    where the exact kth best score is a number.  Where it is not -- the NaN query, whose every score is NaN -- the prefix may
    still hold kth rows the selection arithmetic gives a number (rows of norm 0 or inf: fused_score_fast's guard makes their
    cosine 0 where the reference's is NaN; the planted zero, 1e25 and infinite rows are exactly ten), and L comes out finite on
    the bf16 forms: harmless, every pair of that query is kept (asserted through must-keep), overflows and is repeated exactly.
    What this file did find there: the bf16 stream gave the NaN query's prefix rows keys of all ones, whose kth "score" is NaN,
    and two_stage_floor_of left L = NaN beside floor_key 0; it now treats a kth key without a finite score as no floor (L = -inf).
  * Tightness on the int8 shadow: the prefix keys are LOWER bounds, approx - bound(b, r) (prefix_i8, plan_form), so the floor is
    the kth best of E - 2 bound over the prefix rows, not of E; on the bf16 forms the prefix is the split-bf16 product with
    eps3, and the kth best of E itself stands in that place.
  * At dim 128 the int8 stream's sampled prefix is NOT left as sorted lists (screen_gemv_i8_prefix_makes_lists: dim % 1024 == 0):
    the 1- and 4-query cases run the stream with buffer_to_lists behind the prefix.
"""
import os

import numpy as np
import pytest

from helpers import DAY, NOW, orc, pkg
from test_gpu_screen_bounds import _bound_k2i, _bound_k2j, _ref_norm

pytestmark = pytest.mark.gpu

N_ROWS = 196_608 + 83                                                     # the two-stage pass starts at 196,608; the last 256-row tile is partial
TOPK = 10
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
TEXTS = ["alpha", "the kubernetes helm", "what is the", "gamma delta zzz", "rollout beta", "helm", "kubernetes alpha beta gamma", "delta"]
SCREEN_NAMES = {1: "screen_i8_fused", 2: "screen_gemv_i8", 3: "screen_gemv_bf16", 4: "screen_bf16_fused", 5: "gemm_dot_bf16x1_fused"}
# planted queries, at the front of every batch
Q_LAST, Q_FIRST, Q_CROWD, Q_TIE, Q_ZERO, Q_NAN, Q_HUGE = range(7)
PLANTED = (Q_LAST, Q_FIRST, Q_CROWD, Q_TIE, Q_ZERO, Q_NAN, Q_HUGE)
TIE_ROWS = np.arange(5000, 5040)
ZERO_ROWS, INF_ROW, HUGE_ROWS = np.arange(2000, 2004), 2100, np.arange(3000, 3005)
FLAT_ROWS = np.arange(100_000, 120_000)                                   # dim 128 only: 20,000 identical rows


# ---------------------------------------------------------------------------
# score <-> key, restated from csrc/orr_device.h
# ---------------------------------------------------------------------------

def _key_score(k):
    k = np.atleast_1d(np.asarray(k, dtype=np.uint64))
    top = (k >> np.uint64(63)) != 0
    u = np.where(top, k & np.uint64(0x7FFFFFFFFFFFFFFF), ~k)
    s = u.view(np.float64).copy()
    s[k <= 1] = np.nan
    return s


def _score_key(s):
    s = np.atleast_1d(np.asarray(s, dtype=np.float64)) + 0.0              # -0 -> +0
    u = s.view(np.uint64)
    k = np.where((u >> np.uint64(63)) != 0, ~u, u | np.uint64(1 << 63))
    return np.where(np.isnan(s), np.uint64(1), k)


def test_key_restatement_round_trips():
    """(no GPU work: the numpy restatement of score_key / key_score orders like the scores and inverts itself)"""
    s = np.array([-np.inf, -3.5, -1e-300, 0.0, 1e-300, 0.25, 1.0, 7e300, np.inf])
    k = _score_key(s)
    assert np.all(k[1:] > k[:-1]) and np.array_equal(_key_score(k), s)
    assert _score_key(np.array([-0.0]))[0] == _score_key(np.array([0.0]))[0]
    assert _score_key(np.array([np.nan]))[0] == 1 and np.isnan(_key_score(np.array([0, 1], dtype=np.uint64))).all()


# ---------------------------------------------------------------------------
# One corpus per dimension
# ---------------------------------------------------------------------------

def _ladder(rng, q, dim, n_rungs=40):
    """0.01 noise + c_j q with the cosines stepping from about 0.05 to 0.9."""
    t = np.linspace(0.05, 0.9, n_rungs)
    noise = rng.standard_normal((n_rungs, dim)).astype(np.float32) * np.float32(0.01)
    c = t / np.sqrt(1 - t * t) * (0.01 * np.sqrt(dim)) / float(np.linalg.norm(q))
    return (noise + c[:, None].astype(np.float32) * q[None, :]).astype(np.float32)


class Case:
    def __init__(self, dim, n_queries):
        P = pkg()
        rng = np.random.default_rng(7100 + dim)
        n = N_ROWS
        emb = rng.standard_normal((n, dim)).astype(np.float32)
        qs = rng.standard_normal((n_queries, dim)).astype(np.float32)
        # all the energy in ONE K-tile: the last 64 dimensions, the first 64
        qs[Q_LAST] = 0.0
        qs[Q_LAST, dim - 64:] = rng.standard_normal(64).astype(np.float32)
        qs[Q_FIRST] = 0.0
        qs[Q_FIRST, :64] = rng.standard_normal(64).astype(np.float32)
        self.ladders = {
            "last, tiles beyond a workgroup's first": (Q_LAST, 70_001 + 257 * np.arange(40)),
            "last, inside the sampled prefix": (Q_LAST, 100 + 13 * np.arange(40)),
            "first, the partial last tile": (Q_FIRST, 196_608 + 2 * np.arange(40)),
            "first, a later tile": (Q_FIRST, 150_003 + 300 * np.arange(40)),
        }
        for b, rows in self.ladders.values():
            emb[rows] = _ladder(rng, qs[b], dim)
        # the ten best rows of one query at positions 0..9: one lane's and one wave's rows of the prefix
        t = np.linspace(0.95, 0.5, 10)
        c = t / np.sqrt(1 - t * t) * (0.01 * np.sqrt(dim)) / float(np.linalg.norm(qs[Q_CROWD]))
        emb[:10] = rng.standard_normal((10, dim)).astype(np.float32) * np.float32(0.01) + c[:, None].astype(np.float32) * qs[Q_CROWD][None, :]
        emb[TIE_ROWS] = emb[TIE_ROWS[0]]                                  # 40 identical rows straddling the cut of their own query
        qs[Q_TIE] = emb[TIE_ROWS[0]]
        emb[ZERO_ROWS] = 0.0
        emb[INF_ROW, 5] = np.inf
        emb[HUGE_ROWS] *= np.float32(1e25)
        qs[Q_ZERO] = 0.0
        qs[Q_NAN, 3] = np.nan
        qs[Q_HUGE] = emb[HUGE_ROWS[1]] * np.float32(1e-25)
        if dim == 128:
            emb[FLAT_ROWS] = emb[FLAT_ROWS[0]]
            qs[n_queries - 1] = emb[FLAT_ROWS[0]]                         # the overflow query: never part of an ordinary batch
        created = (NOW - np.arange(n, dtype=np.int64) * (300 * DAY // n)).astype(np.int64)   # strictly newest first: position = row
        words = np.array(["alpha", "beta", "gamma", "delta", "kubernetes", "helm", "rollout"])
        contents = [" ".join(w).encode() for w in words[rng.integers(0, len(words), (n, 4))]]
        self.P, self.dim, self.n, self.emb, self.qs = P, dim, n, emb, qs
        self.texts = [TEXTS[b % len(TEXTS)] if b % 3 else "" for b in range(n_queries)]   # every third query without terms
        self.terms = [P.text.query_terms(t) if t else [] for t in self.texts]
        self.idx = P.RecallIndex(dim=dim)
        for r0 in range(0, n, 50_000):
            r1 = min(n, r0 + 50_000)
            self.idx.append(emb[r0:r1], created[r0:r1], contents[r0:r1], row_ids=np.arange(r0, r1, dtype=np.int64))
        self.idx.seal()
        self.corpus = orc.OracleCorpus(emb, created, contents)
        self._E, self._consts = {}, None
        with np.errstate(all="ignore"):
            na = _ref_norm(qs)
            self.inv_a = np.where(na > 0, 1.0 / np.sqrt(na), 0.0)
        ladder_rows = np.concatenate([rows for _, rows in self.ladders.values()])
        self.scope_a = np.unique(np.concatenate([np.arange(0, n, 3), ladder_rows]))          # every third row plus the ladders
        self.scope_b = np.unique(np.concatenate([np.arange(1, n, 3), ladder_rows]))

    def E(self, b):
        """The oracle's exact score of every row for query b, computed once."""
        if b not in self._E:
            order, sc = self.corpus.score_all(self.qs[b], self.texts[b], NOW, self.n, threads=8)
            e = np.full(self.n, np.nan)
            e[order] = sc
            assert len(order) == self.n
            self._E[b] = e
        return self._E[b]

    def consts(self):
        if self._consts is None:
            self._consts = self.idx.screen_i8_consts(self.qs)
        return self._consts

    def bound(self, screen, eps1, b):
        """2-norm bound of 0.7 cos for query b and every row, as the screen that ran charges it."""
        if screen in (1, 2):
            c = self.consts()
            with np.errstate(all="ignore"):
                if screen == 1:
                    return _bound_k2j(c["rowf"], c["err2_level1"][b:b + 1], self.inv_a[b:b + 1])[0]
                return _bound_k2i(c["rel_err"], c["rel_hat"], c["err2"][b:b + 1], self.inv_a[b:b + 1])[0]
        return np.full(self.n, float(eps1))

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module")
def case128():
    c = Case(128, 65)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case512():
    c = Case(512, 300)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case192():
    c = Case(192, 40)
    yield c
    c.close()


# ---------------------------------------------------------------------------
# One captured search and its assertions
# ---------------------------------------------------------------------------

def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _search(case, sel, how, topk, groups=None, idx=None):
    idx, n = idx or case.idx, case.n
    q, terms = np.ascontiguousarray(case.qs[sel]), [case.terms[b] for b in sel]
    if how == "plain":
        return idx.search(q, terms, NOW, topk, candidate_limit=n)
    if how == "masked":
        return idx.search_masked(q, terms, NOW, topk, case.scope_a, candidate_limit=n)
    return idx.search_masked_groups(q, terms, NOW, topk, [case.scope_a, case.scope_b], groups, candidate_limit=n)


def _captured(case, sel, how="plain", topk=TOPK, env=None, groups=None, idx=None, capture_first=False):
    """The same search without and with capture (records equal bit for bit), the capture and the kernel statistics.
    capture_first: the captured search runs before the plain one (a handle whose buffers have not grown yet)."""
    idx = idx or case.idx
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        plain = None if capture_first else _search(case, sel, how, topk, groups, idx)
        idx.set_profiling(True)
        idx.reset_search_stats()
        idx.capture_screen(True)
        got = _search(case, sel, how, topk, groups, idx)
        stats, ss = idx.kernel_stats(), idx.search_stats()
        idx.set_profiling(False)
        cap = idx.captured_screen()
        again = _search(case, sel, how, topk, groups, idx)                # disarmed by its one capture: nothing more is recorded
        assert idx.captured_screen()["cnt"].tobytes() == cap["cnt"].tobytes()
        if plain is None:
            plain = again
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for a, b, c in zip(plain, got, again):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c)), "the capture shows in the records"
    return cap, stats, ss


def _checked(B):
    return sorted({0, B - 1} | {b for b in (31, 32, 63, 64, 127, 128, 255, 256) if b < B} | {b for b in PLANTED if b < B})


def _kth_best(values, kth):
    v = np.where(np.isnan(values), -np.inf, values)
    return np.partition(v, len(v) - kth)[len(v) - kth]


def _assert_screen(case, cap, sel, what, part_of=None, checked=None):
    """Every assertion of the module docstring for the checked queries of one capture.  part_of(pos in batch) -> bool [n]: the rows
    that take part for that query besides pos < cap['n'] (None: all)."""
    n, kth, kcap = int(cap["n"]), int(cap["kth"]), int(cap["cap"])
    B = len(sel)
    assert cap["B"] == B and n <= case.n and kth >= 1
    rows_all = np.arange(case.n)
    info, ones_total, filled_total, loose = [], 0, 0, 0
    for i in (checked if checked is not None else _checked(B)):
        b = sel[i]
        E = case.E(b)
        Ecmp = np.where(np.isnan(E), -np.inf, E)
        part = rows_all < n
        if part_of is not None:
            part = part & part_of(i)
        fk, L, cnt = int(cap["floor_key"][i]), float(cap["L"][i]), int(cap["cnt"][i])
        tag = f"{what}, query {i} (pool {b})"
        # ---- the floor
        if fk == 0:
            assert L == -np.inf, (tag, L)
            F, slack = -np.inf, None
        else:
            F = float(_key_score(np.uint64(fk + 1))[0])
            slack = L - F
            assert np.isfinite(L) and np.isfinite(F) and slack > 0, (tag, L, F)
        if int((part & ~np.isnan(E)).sum()) >= kth:                      # (the kth best exact score is a number: see "NaN scores" above)
            best = float(_kth_best(E[part], kth))
            assert L <= best, f"{tag}: the floor L = {L!r} lies above the exact {kth}-th best score {best!r}"
        # ---- the entries
        filled = min(cnt, kcap)
        if part_of is not None and cnt > kcap:
            # mask_survivors compacts an overflowed buffer in place and leaves its count as the overflow signal ("that count
            # stays", csrc/orr_kernels.hip): how many of the cap entries are the compacted ones is not recorded, the tail behind
            # them is stale.  Nothing of such a buffer is read (the query repeats), so only the overflow assertion applies.
            filled = 0
        pos, key = cap["pos"][i, :filled].astype(np.int64), cap["key"][i, :filled]
        assert np.all(pos < n), (tag, pos[pos >= n][:5])
        assert len(np.unique(pos)) == filled, f"{tag}: {filled - len(np.unique(pos))} positions buffered twice"
        assert np.all(key > np.uint64(fk)), (tag, int((key <= np.uint64(fk)).sum()))
        if part_of is not None:
            assert part[pos].all(), f"{tag}: {int((~part[pos]).sum())} buffered rows from outside the query's scope"
        bound = case.bound(int(cap["screen"]), cap["eps1"], b)
        # ---- must keep / overflow
        must = part & ((Ecmp >= L) | np.isnan(E))                         # (a pair without a numeric score is never dropped)
        if cnt <= kcap:
            inbuf = np.zeros(case.n, dtype=bool)
            inbuf[pos] = True
            lost = np.flatnonzero(must & ~inbuf)
            assert lost.size == 0, (f"{tag}: {lost.size} rows with an exact score at or above L = {L!r} are not among the {cnt} survivors; "
                                    f"first: row {lost[0]} (tile {lost[0] // 256}), E {E[lost[0]]!r}, bound {bound[lost[0]]!r}")
        else:
            assert cnt >= min(int(must.sum()), kcap + 1), (tag, cnt, int(must.sum()))
        # ---- the keys against the exact scores
        ones = key == ALL_ONES
        if slack is not None:
            ones_total += int(ones.sum())                                 # (of the queries with a floor: without one, every key may be)
            filled_total += filled
            with np.errstate(all="ignore"):
                e_p, b_p = E[pos], bound[pos]
                finite_b = b_p <= 1.7976931348623157e308
                keeps = e_p + 2.0 * b_p + slack >= F
                # must drop: what the fp64 test of pass 2 kept had to be kept
                bad = ~ones & finite_b & ~keeps
                assert not bad.any(), (f"{tag}: {int(bad.sum())} buffered pairs lie below the floor by more than their bound; first: row "
                                       f"{pos[bad][0]}, E {e_p[bad][0]!r}, bound {b_p[bad][0]!r}, F {F!r}, L {L!r}")
                loose += int((ones & finite_b & ~keeps).sum())            # (kept by pass 1 alone: information)
                ks = _key_score(key[~ones])
                e_k, b_k = e_p[~ones], b_p[~ones]
                low = ~(ks + slack >= e_k) & ~np.isnan(e_k)
                assert not low.any(), f"{tag}: {int(low.sum())} keys lie below the exact score; first: row {pos[~ones][low][0]}, key {ks[low][0]!r}, E {e_k[low][0]!r}"
                high = ~(ks - e_k <= 2.0 * b_k + slack) & (b_k <= 1.7976931348623157e308) & ~np.isnan(e_k)
                assert not high.any(), (f"{tag}: {int(high.sum())} keys lie above the exact score by more than twice the bound; first: row "
                                        f"{pos[~ones][high][0]}, key {ks[high][0]!r}, E {e_k[high][0]!r}, bound {b_k[high][0]!r}")
        info.append(f"{i}:{cnt}")
    share = ones_total / max(1, filled_total)
    print(f"[screen survivors] {what}: screen {cap['screen']} form {cap['tile_form']} floor form {cap['floor_form']} cap {kcap}; survivors per "
          f"query {' '.join(info)}; keys of all ones {share:.4f} of the entries of queries with a floor, {loose} of them below their own bound's reach")


def _assert_kernel(cap, stats, screen, tile_form=None):
    name = SCREEN_NAMES[screen]
    assert cap["screen"] == screen and name in stats and stats[name]["launches"] >= 1, (cap["screen"], sorted(stats))
    if cap["cnt"].max() <= cap["cap"]:                                    # (the repeat of an overflowed query is a pass of its own, in its own form)
        for other in list(SCREEN_NAMES.values()) + ["dot_exact"]:
            assert other == name or other not in stats, (other, sorted(stats))
    if tile_form is not None:
        assert cap["tile_form"] == tile_form, cap["tile_form"]


# ---------------------------------------------------------------------------
# The int8 shadow, dim 128: the stream (K2i) and the eight-wave GEMM
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,screen", [(1, 2), (4, 2), (6, 1), (64, 1)])
def test_int8_screen_at_dim_128_keeps_what_the_floor_demands(case128, B, screen):
    """Links 3 and 4 for the streaming int8 screen (1..4 queries; its floor comes from the stream's own lower-bound keys of the
    sampled prefix) and for the int8 GEMM with fewer than 6 K-tiles, which stays eight-wave whatever the batch."""
    sel = list(range(B))
    cap, stats, _ = _captured(case128, sel)
    _assert_kernel(cap, stats, screen, 0 if screen == 1 else -1)
    assert cap["scope"] == 0 and cap["n"] == N_ROWS
    _assert_screen(case128, cap, sel, f"dim 128, {B} queries")


def test_overflowed_query_counts_at_least_what_it_had_to_keep(case128):
    """Link 4 where the buffer is too small: a query parallel to 20,000 identical rows must count every one of them (cnt beyond
    the capacity sends it to the repeat), and the first pass alone is captured.  On a fresh view of the shard, whose buffers
    still have their first size (a handle's buffers grow with what its searches overflowed): the capture of a view is its own."""
    sel = [0, 1, 2, 3, 4, len(case128.qs) - 1]
    view = case128.idx.view()
    try:
        cap, stats, ss = _captured(case128, sel, idx=view, capture_first=True)
    finally:
        view.close()
    _assert_kernel(cap, stats, 1, 0)
    assert cap["cap"] < len(FLAT_ROWS) < cap["cnt"][5], (cap["cnt"], cap["cap"])
    assert ss["passes"] >= 2, ss                                          # the repeat ran, the capture is the first pass's
    _assert_screen(case128, cap, sel, "dim 128, overflow", checked=[0, 1, 5])


def test_one_product_bf16_screen_keeps_what_the_floor_demands(case128):
    """Links 3 and 4 for gemm_dot_bf16x1_fused (two_stage = 2: no shadow, the fp32 rows converted in the kernel), a kernel that
    exists in fused form only; its bound is the plan's eps1."""
    sel = list(range(40))
    case128.idx.set_option("two_stage", 2)
    try:
        cap, stats, _ = _captured(case128, sel)
    finally:
        case128.idx.set_option("two_stage", 1)
    _assert_kernel(cap, stats, 5)
    assert cap["eps1"] > 0 and cap["eps3"] > 0
    _assert_screen(case128, cap, sel, "dim 128, two_stage 2, 40 queries")


# ---------------------------------------------------------------------------
# The int8 GEMM at dim 512: eight-wave, four-wave and 16 x 16 x 64 forms
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,screen,form", [(4, 2, -1), (64, 1, 0), (70, 1, 1), (128, 1, 1), (130, 1, 2), (256, 1, 2), (300, 1, 2)])
def test_int8_screen_at_dim_512_keeps_what_the_floor_demands(case512, B, screen, form):
    """Links 3 and 4 for every tile form of the int8 screening GEMM (eight-wave to 64 queries, four-wave 32 x 32 x 32 to 128,
    16 x 16 x 64 beyond, 300: several query tiles per row tile and a batch that is no multiple of 32) and the stream at 8
    K-tiles.  The single-K-tile ladders sit in later output tiles and in the partial last tile: a K-tile taken from a
    neighbouring output tile loses or inflates exactly them."""
    sel = list(range(B))
    cap, stats, _ = _captured(case512, sel)
    _assert_kernel(cap, stats, screen, form)
    _assert_screen(case512, cap, sel, f"dim 512, {B} queries")


def test_survivors_do_not_depend_on_the_grid_walk(case512):
    """Link 4 with 8 persistent workgroups (ORR_SCREEN_GRID=8): every workgroup walks three and more output tiles, and every
    assertion holds as with one workgroup per CU."""
    sel = list(range(256))
    cap, stats, _ = _captured(case512, sel, env={"ORR_SCREEN_GRID": "8"})
    _assert_kernel(cap, stats, 1, 2)
    _assert_screen(case512, cap, sel, "dim 512, 256 queries, 8 workgroups")


@pytest.mark.parametrize("env,topk,floor_form", [("1", TOPK, 0), ("2", TOPK, 1), (None, 8, 2)])
def test_every_floor_form_is_valid_and_the_full_ranking_is_tight(case512, env, topk, floor_form):
    """Link 3 for the three floors of the sampled prefix: full ranking (ORR_PREFIX_FULL_RANKING=1), per-lane maxima (=2) and wave
    maxima through select_floor_heads (topK 8: sixteen maxima per segment are 8 k candidates).  Each must be valid; the full
    ranking must also be tight -- the prefix keys are lower bounds approx - bound, so L >= the kth best of E - 2 bound over
    the prefix rows - 2 eps3 - (L - F).  The maxima forms may lie lower: their survivors are printed.  Query 2's ten best rows
    are positions 0..9, one lane's and one wave's rows."""
    sel = list(range(70))
    cap, stats, _ = _captured(case512, sel, topk=topk, env={"ORR_PREFIX_FULL_RANKING": env} if env else None)
    _assert_kernel(cap, stats, 1, 1)
    assert cap["floor_form"] == floor_form and cap["kth"] == topk, (cap["floor_form"], cap["kth"])
    _assert_screen(case512, cap, sel, f"dim 512, 70 queries, floor form {floor_form}")
    if floor_form == 0:
        m = int(cap["prefix_rows"])
        assert 0 < m <= 65_536
        for i in _checked(70):
            fk, L = int(cap["floor_key"][i]), float(cap["L"][i])
            if fk == 0:
                continue
            F = float(_key_score(np.uint64(fk + 1))[0])
            with np.errstate(all="ignore"):
                lower = case512.E(i)[:m] - 2.0 * case512.bound(1, 0.0, i)[:m]
            want = float(_kth_best(lower, topk)) - 2.0 * cap["eps3"] - (L - F)
            assert L >= want, f"query {i}: the full ranking's floor L = {L!r} lies below {want!r}"


def test_masked_screen_keeps_every_in_scope_row_the_floor_demands(case512):
    """Links 3 and 4 under a scope mask (orr_search_batch_masked, every third row plus the ladders): the floor comes from an
    exact re-score of an in-scope sample, the buffers are cleaned by mask_survivors, and must-keep runs over the in-scope rows
    alone."""
    sel = list(range(40))
    in_scope = np.zeros(case512.n, dtype=bool)
    in_scope[case512.scope_a] = True
    case512.idx.set_option("mask_screen", 1)
    try:
        cap, stats, ss = _captured(case512, sel, how="masked")
    finally:
        case512.idx.set_option("mask_screen", 0)
    # (pass_mode is the LAST pass's: the NaN query overflows and repeats on the list path, so the kernels and the capture say it)
    assert ss["pass_mode"] in (4, 5) and "mask_survivors" in stats and "mask_sample_rescore" in stats, (ss, sorted(stats))
    _assert_kernel(cap, stats, 1, 0)
    assert cap["scope"] == 1 and cap["floor_form"] == -1 and 196_608 <= cap["n"] <= N_ROWS
    _assert_screen(case512, cap, sel, "dim 512, masked, 40 queries", part_of=lambda i: in_scope)


def test_grouped_screen_keeps_every_row_of_the_querys_own_group(case512):
    """Links 3 and 4 under two scopes that share one screening pass (orr_search_batch_masked_groups): a row of the other group
    that beat the query's floor must be gone (mask_survivors_grouped), every row of its own group at or above L must be there."""
    sel = list(range(40))
    groups = np.array([b % 2 for b in range(40)], dtype=np.int32)
    masks = []
    for scope in (case512.scope_a, case512.scope_b):
        m = np.zeros(case512.n, dtype=bool)
        m[scope] = True
        masks.append(m)
    case512.idx.set_option("mask_screen", 1)
    try:
        cap, stats, ss = _captured(case512, sel, how="grouped", groups=groups)
    finally:
        case512.idx.set_option("mask_screen", 0)
    assert ss["pass_mode"] in (4, 5, 6) and "mask_survivors_grouped" in stats, (ss, sorted(stats))    # (the last pass's: see the masked test)
    _assert_kernel(cap, stats, 1, 0)
    assert cap["scope"] == 2
    _assert_screen(case512, cap, sel, "dim 512, grouped, 40 queries", part_of=lambda i: masks[groups[i]])


# ---------------------------------------------------------------------------
# The bf16 shadow, dim 192
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,screen", [(3, 3), (8, 3), (40, 4)])
def test_bf16_screen_at_dim_192_keeps_what_the_floor_demands(case192, B, screen):
    """Links 3 and 4 on the bf16 shadow: the stream K2g (1..8 queries), which exists in fused form only, and screen_bf16_fused.
    The bound of every pair is the plan's eps1."""
    sel = list(range(B))
    cap, stats, _ = _captured(case192, sel)
    _assert_kernel(cap, stats, screen)
    assert cap["eps1"] > 0 and cap["tile_form"] == -1
    _assert_screen(case192, cap, sel, f"dim 192, {B} queries")


# ---------------------------------------------------------------------------
# The entry points' own states
# ---------------------------------------------------------------------------

def test_capture_states_on_a_live_handle(case128):
    """Not sealed and nothing captured are ORR_ESTATE; a size that differs from the capture's is ORR_EINVAL with nothing written
    (the NULL checks in front of the handle are tests/test_abi_cpu.py's)."""
    import ctypes as C
    P = case128.P
    N = P.native
    fresh = P.RecallIndex(dim=8)
    fresh.append(np.ones((4, 8), np.float32), np.full(4, NOW, dtype=np.int64), [b"x"] * 4)
    info = N.OrrScreenCapture()
    assert N.hip.orr_index_capture_screen(fresh._h, 1) == N.ORR_ESTATE
    assert N.hip.orr_index_captured_screen(fresh._h, C.byref(info), 0, 0, None, None, None, None, None) == N.ORR_ESTATE
    fresh.seal()
    assert N.hip.orr_index_captured_screen(fresh._h, C.byref(info), 0, 0, None, None, None, None, None) == N.ORR_ESTATE
    fresh.capture_screen(True)
    fresh.search(np.ones((1, 8), np.float32), [[b"x"]], NOW, 2, candidate_limit=4)        # no two-stage pass: nothing to capture
    assert N.hip.orr_index_captured_screen(fresh._h, C.byref(info), 0, 0, None, None, None, None, None) == N.ORR_ESTATE
    fresh.capture_screen(False)
    fresh.close()
    idx = case128.idx
    idx.capture_screen(True)
    idx.search(case128.qs[:6], case128.terms[:6], NOW, TOPK, candidate_limit=case128.n)
    cap = idx.captured_screen()
    B, kcap = cap["B"], cap["cap"]
    arrays = [np.full(B + 1, 7, np.uint64), np.full(B + 1, 7.0), np.full(B + 1, 7, np.uint32), np.full((B + 1) * kcap, 7, np.uint64),
              np.full((B + 1) * kcap, 7, np.uint32)]
    ptrs = [a.ctypes.data for a in arrays]
    info = N.OrrScreenCapture()
    for wrong_b, wrong_cap in ((B + 1, kcap), (B, kcap + 64), (B - 1, kcap)):
        assert N.hip.orr_index_captured_screen(idx._h, C.byref(info), wrong_b, wrong_cap, *ptrs) == N.ORR_EINVAL
        assert info.B == 0 and info.cap == 0 and all((a == 7).all() for a in arrays)
    idx.capture_screen(True)                                             # arming again drops the capture held
    assert N.hip.orr_index_captured_screen(idx._h, C.byref(info), 0, 0, None, None, None, None, None) == N.ORR_ESTATE
    idx.capture_screen(False)
