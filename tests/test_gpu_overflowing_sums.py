"""Dot sums that overflow fp32, through every pass form, against the oracle.

tests/test_overflowing_sums_cpu.py builds the data and proves the preconditions: a query and rows of magnitude 1.5e19 whose fp32
squares and products are finite, whose reference cosine is an ordinary number ((D - 2m) / D), and whose products no fp32
accumulation can sum to a finite value.  An approximate dot kernel returns +inf, -inf or NaN for such a pair -- which of them
depends on the order in which it meets the flipped signs, so the rows come in layouts that put them first, last, evenly spread
and in aligned slices.  Here:

  * what the float kernels return: not finite on every (big query, big row) pair, finite and inside the bound the pass charges
    on every other pair, with a printed table of which value came back per kernel and layout;
  * end to end, every pass form of a small shard (exact, f32-MFMA stream, split GEMM, large k), host- and device-resident
    queries, with the row kinds a batched pass meets (zero, no embedding, NaN, inf, 1e25) in the same shard;
  * the shard entry point: merged records equal the oracle's and are certified, or the query is reported uncertified --
    certified and wrong is the failure;
  * the two-stage forms at 196,608 + 83 rows, with big rows inside the sampled prefix, far behind it and in the last partial
    tile, unmasked and inside a scope of every second row;
  * range search, walked and bulk, at thresholds between the planted cosines.

A score of -inf or NaN from such a dot is the lowest key there is: a pass that ranks by it cuts the true winners, and a
certificate that compares finite numbers on either side of the cut never notices.
"""
import numpy as np
import pytest

import test_gpu_screen_bounds as bounds
import test_overflowing_sums_cpu as data
from helpers import NOW, build_index, oracle_corpus, orc, pkg

pytestmark = pytest.mark.gpu

K = 10
TEXTS = ["", "alpha beta"]


def _label(v):
    return "+inf" if v == np.inf else "-inf" if v == -np.inf else "nan" if v != v else "finite"


def _same(got, want, what):
    """The file's rule: identical rows, order and fp64 score bits (NaN scores equal NaN scores)."""
    rows, scores, count = got
    orow, osc = want[0], want[1]
    assert count == len(orow), (what, count, len(orow))
    assert list(rows[:count]) == list(orow), (what, list(rows[:count]), list(orow))
    a = np.asarray(scores[:count], dtype=np.float64)
    assert ((a.view(np.int64) == np.asarray(osc).view(np.int64)) | (np.isnan(a) & np.isnan(osc))).all(), (what, a, osc)


def _check_batch(got, want, B, checked, what):
    rows, scores, counts = got
    for b in checked:
        _same((rows[b], scores[b], counts[b]), want(b), (what, B, b))


# ---------------------------------------------------------------------------
# 2. What the kernels return
# ---------------------------------------------------------------------------

# (name, fetch, error of the kernel relative to sum |q_k e_k| as the pass charges it, batch sizes)
FLOAT_KERNELS = {
    # gemv_mfma16_kernel up to 16 queries, gemv_mfma_kernel to 32, then a second launch
    "gemv_mfma": (lambda idx, q: idx.pass_dots(q, 0), lambda d: (2.0 * d + 2.0) * bounds.U23, (5, 16, 17, 33, 40)),
    "gemm_dot_bf16x3": (lambda idx, q: idx.pass_dots(q, 1), lambda d: 3.1 * 2.0 ** -16 + 3.06 * d * bounds.U23, (5, 33, 130)),
    "screen_dots": (lambda idx, q: idx.screen_dots(q), lambda d: 2.0 ** -7 * (1 + 2.0 ** -9) + 1.02 * d * bounds.U23, (3, 33, 130)),
}


@pytest.fixture(scope="module", params=[64, 256])
def plain_shard(request):
    """9,000 rows (three selection segments, the last partial): Gaussian rows and the big rows, nothing else."""
    dim = request.param
    emb, where = data.planted_corpus(dim)
    idx = bounds._index(pkg(), emb)
    yield {"dim": dim, "emb": emb, "where": where, "idx": idx, "emb64": emb.astype(np.float64), "shares": {}}
    idx.close()


@pytest.mark.parametrize("kernel", list(FLOAT_KERNELS))
def test_float_kernels_return_no_finite_value_for_a_sum_that_has_none(plain_shard, kernel):
    """On every (big query, big row) pair the dot is not finite; on every other pair it is finite and inside the bound
    tests/test_gpu_screen_bounds.py charges that kernel (its _bounded, with the big pairs taken out)."""
    s = plain_shard
    dim, emb, where, idx = s["dim"], s["emb"], s["where"], s["idx"]
    fetch, eps_of, batches = FLOAT_KERNELS[kernel]
    big_rows = np.array(sorted(where))
    table = {}
    for B in batches:
        qs, kinds = data.query_batch(dim, B, specials=False)
        big_q = np.array([b for b, k in enumerate(kinds) if k == "big"])
        dots = fetch(idx, qs)
        assert dots.shape == (B, len(emb)) and dots.dtype == np.float32
        sub = dots[np.ix_(big_q, big_rows)]
        for j, r in enumerate(big_rows):
            layout, m = where[int(r)]
            for i, b in enumerate(big_q):
                table.setdefault((layout, m), set()).add(_label(sub[i, j]))
        assert not np.isfinite(sub).any(), (kernel, dim, B, [(int(big_q[i]), int(big_rows[j]), where[int(big_rows[j])], float(sub[i, j]))
                                                             for i, j in np.argwhere(np.isfinite(sub))[:6]])
        pair = np.zeros(dots.shape, dtype=bool)
        pair[np.ix_(big_q, big_rows)] = True
        assert np.isfinite(dots[~pair]).all(), (kernel, dim, B, np.argwhere(~np.isfinite(dots) & ~pair)[:6])
        q64 = qs.astype(np.float64)
        want = q64 @ s["emb64"].T
        case = {"dim": dim, "want_g": want, "scale_g": np.abs(q64) @ np.abs(s["emb64"]).T, "shares": s["shares"]}
        bounds._bounded(case, B, np.where(pair, want, dots.astype(np.float64)), eps_of(dim), f"{kernel} beside overflowing sums")
    for (layout, m), seen in sorted(table.items()):
        print(f"[overflowing sums] {kernel}, dim {dim}, layout {layout}, {m} flips: {' '.join(sorted(seen))}")


# ---------------------------------------------------------------------------
# 3. End to end on a small shard
# ---------------------------------------------------------------------------

SPECIAL_ROWS = {10: "zero", 11: "none", 12: "nan", 13: "inf", 14: "1e25", 4100: "zero", 4101: "none", 4102: "nan", 4103: "inf",
                4104: "1e25", 8990: "zero", 8991: "none", 8992: "nan", 8993: "inf", 8994: "1e25"}


def _special_row(kind, e):
    e = e.copy()
    if kind == "zero":
        e[:] = 0.0
    elif kind == "none":
        return None
    elif kind == "nan":
        e[len(e) // 3] = np.nan
    elif kind == "inf":
        e[len(e) // 2] = np.inf
    elif kind == "1e25":
        e[:] = np.where(e < 0, np.float32(-1e25), np.float32(1e25))
    return e


def _small_corpus(dim):
    if dim >= 64:
        emb, where = data.planted_corpus(dim)
    else:                                                                 # the generic exact form: every sign agrees / differs
        emb = np.random.default_rng(1).standard_normal((data.N_ROWS, dim)).astype(np.float32)
        where = {}
        for j, pos in enumerate(data.POSITIONS[:8]):
            emb[pos] = data.big_query(dim) * np.float32(-1.0 if j == 3 else 1.0)
            where[pos] = ("front", dim if j == 3 else 0)
    rows = [emb[r] for r in range(len(emb))]
    for r, kind in SPECIAL_ROWS.items():
        assert r not in where
        rows[r] = _special_row(kind, emb[r])
    rng = np.random.default_rng(5)
    contents = [" ".join(rng.choice(["alpha", "beta", "gamma", "delta"], size=int(rng.integers(0, 4)))) for _ in range(len(emb))]
    return {"emb": rows, "created": np.full(len(emb), NOW, dtype=np.int64), "contents": contents, "dim": dim}, where


_SMALL = {}


def _small(dim):
    if dim not in _SMALL:
        c, where = _small_corpus(dim)
        _SMALL[dim] = {"dim": dim, "c": c, "where": where, "idx": build_index(c), "corpus": oracle_corpus(c), "want": {}}
    return _SMALL[dim]


def _oracle(s, q, text, k, threads=1):
    key = (q.tobytes(), text, k)
    if key not in s["want"]:
        s["want"][key] = s["corpus"].search(q, text, NOW, k, candidate_limit=len(s["c"]["created"]), threads=threads)
    return s["want"][key]


def _checked(kinds):
    """The queries of a batch that are compared with the oracle: every big and every special one, and a few ordinary ones."""
    plain = [b for b, k in enumerate(kinds) if k == "gauss"]
    return sorted({b for b, k in enumerate(kinds) if k != "gauss"} | set(plain[:2]) | set(plain[-1:]))


SMALL_FORMS = [(1, None), (4, None), (5, "gemv_mfma"), (33, "gemv_mfma"), (64, "gemv_mfma"), (65, "gemm_dot_bf16x3"), (130, "gemm_dot_bf16x3")]


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("B,kernel", SMALL_FORMS, ids=[f"B{b}" for b, _ in SMALL_FORMS])
def test_small_shard_every_pass_form_equals_the_oracle(dim, B, kernel):
    """Host-resident batches of 1 and 4 queries (the exact pass: the baseline), 5 / 33 / 64 (the f32-MFMA stream over all rows) and
    65 / 130 (the split GEMM over all rows), the big query at 0, 31, 32 and last: top-10 identical to the oracle's."""
    P = pkg()
    s = _small(dim)
    idx = s["idx"]
    qs, kinds = data.query_batch(dim, B)
    texts = [TEXTS[b % 2] for b in range(B)]
    terms = [P.text.query_terms(t) for t in texts]
    idx.set_profiling(True)
    got = idx.search(qs, terms, NOW, K, candidate_limit=data.N_ROWS)
    stats = idx.kernel_stats()
    idx.set_profiling(False)
    if kernel is None:
        assert "gemv_mfma" not in stats and "gemm_dot_bf16x3" not in stats and "rescore_exact" not in stats, sorted(stats)
    else:
        assert kernel in stats and "rescore_exact" in stats, sorted(stats)
    _check_batch(got, lambda b: _oracle(s, qs[b], texts[b], K), B, _checked(kinds), f"dim {dim}")
    if dim >= 64:                                                         # the planted rows, best first (the CPU file proves the margin)
        want = data.expected_order(dim, s["where"])[:K]
        for b in data.big_positions(B):
            if texts[b] == "":
                assert list(got[0][b]) == want, (dim, B, b)


@pytest.mark.parametrize("B", [1, 4, 5])
def test_small_shard_at_dim_3_takes_the_generic_exact_form(B):
    P = pkg()
    s = _small(3)
    qs, kinds = data.query_batch(3, B)
    texts = [TEXTS[b % 2] for b in range(B)]
    got = s["idx"].search(qs, [P.text.query_terms(t) for t in texts], NOW, K, candidate_limit=data.N_ROWS)
    _check_batch(got, lambda b: _oracle(s, qs[b], texts[b], K), B, range(B), "dim 3")


@pytest.mark.parametrize("dim", [64, 256])
def test_small_shard_top_100_takes_the_large_k_form(dim):
    P = pkg()
    s = _small(dim)
    B = 5
    qs, kinds = data.query_batch(dim, B)
    texts = [TEXTS[b % 2] for b in range(B)]
    s["idx"].set_profiling(True)
    got = s["idx"].search(qs, [P.text.query_terms(t) for t in texts], NOW, 100, candidate_limit=data.N_ROWS)
    stats = s["idx"].kernel_stats()
    s["idx"].set_profiling(False)
    assert "radix_sort_desc" in stats, sorted(stats)
    _check_batch(got, lambda b: _oracle(s, qs[b], texts[b], 100), B, range(B), f"dim {dim}, top 100")


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("B", [5, 15, 16, 33, 130])
def test_small_shard_device_resident_queries_equal_the_oracle(dim, B):
    """The same with the queries in device memory: below 16 their norms come from the host, from 16 on from the device."""
    import torch
    P = pkg()
    s = _small(dim)
    qs, kinds = data.query_batch(dim, B)
    texts = [TEXTS[b % 2] for b in range(B)]
    qd = torch.from_numpy(qs).to("cuda:0")
    got = s["idx"].search(qd, [P.text.query_terms(t) for t in texts], NOW, K, candidate_limit=data.N_ROWS)
    _check_batch(got, lambda b: _oracle(s, qs[b], texts[b], K), B, _checked(kinds), f"dim {dim}, device queries")


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("B", [4, 5, 33, 130])
def test_shard_entry_is_right_or_says_it_is_not_certain(dim, B):
    """orr_search_shard with k' = 32, then orr_merge_candidates: for every query either the merged top-10 is the oracle's and
    the query is certified, or it is reported uncertified.  (A shard pass runs once, at the caller's k': no escalation hides a
    cut winner.)"""
    P = pkg()
    s = _small(dim)
    qs, kinds = data.query_batch(dim, B)
    texts = [TEXTS[b % 2] for b in range(B)]
    terms = [P.text.query_terms(t) for t in texts]
    rec = s["idx"].search_shard(qs, terms, NOW, 32, data.N_ROWS)
    rows, scores, counts, unc, cert = P.index.merge_candidates(rec[None], dim, qs, terms, NOW, K, with_certificates=True)
    assert unc == int((~cert).sum())
    wrong = []
    for b in _checked(kinds):
        if not cert[b]:
            continue
        try:
            _same((rows[b], scores[b], counts[b]), _oracle(s, qs[b], texts[b], K), (dim, B, b))
        except AssertionError as e:
            wrong.append((b, kinds[b], str(e)[:300]))
    print(f"[overflowing sums] shard entry, dim {dim}, {B} queries: {unc} uncertified "
          f"({sorted(set(kinds[b] for b in range(B) if not cert[b]))}), {len(wrong)} certified and wrong")
    assert not wrong, wrong
    assert all(cert[b] for b, k in enumerate(kinds) if k == "gauss"), "ordinary queries lost their certificate"


@pytest.mark.parametrize("dim,B", [(64, 5), (256, 130)])
def test_shard_entry_with_a_list_that_the_kept_rows_fill_is_not_certified(dim, B):
    """k' = 12 against 16 and more rows that are kept whatever their key: the list holds kept rows only, in the order of their
    positions, so what was left out is unknown.  The trailer's cut-off must say so (+inf, not the NaN that stands for "everything
    left out scores NaN as well"): the big query comes back uncertified, and ordinary queries still get certificates."""
    P = pkg()
    s = _small(dim)
    assert len(s["where"]) > 12
    qs, kinds = data.query_batch(dim, B, specials=False)
    terms = [P.text.query_terms("")] * B
    rec = s["idx"].search_shard(qs, terms, NOW, 12, data.N_ROWS)
    rows, scores, counts, unc, cert = P.index.merge_candidates(rec[None], dim, qs, terms, NOW, K, with_certificates=True)
    for b, kind in enumerate(kinds):
        if kind == "big":
            assert not cert[b], (dim, B, b, list(rows[b]))
            assert rec[b, 12]["approx_score"] == np.inf
    plain = [b for b, k in enumerate(kinds) if k == "gauss"]
    assert any(cert[b] for b in plain), "no ordinary query kept its certificate"   # (a near-tie at the cut may cost one its own)
    for b in [b for b in plain if cert[b]][:3]:
        _same((rows[b], scores[b], counts[b]), _oracle(s, qs[b], "", K), (dim, B, b))


# ---------------------------------------------------------------------------
# Two-stage size
# ---------------------------------------------------------------------------

TWO_STAGE_N = 196_608 + 83


def _two_stage_positions(dim, n):
    """Where the big rows go: inside the sampled prefix (the newest rows: the first of the shard), the 3D/4 `back` row among
    them; far behind it (row 150,000 on); in the last partial tile."""
    prefix = iter((0, 5, 63, 64, 300, 1023, 1024, 2047, 3000, 4000))
    far = iter(150_000 + 257 * j for j in range(12))
    last = iter([n - 1] + list(range(n - 80, n - 1, 9)))
    pos = []
    for i, (layout, m) in enumerate(data.planted_rows(dim)):
        pos.append(next(prefix if (m == 3 * dim // 4 or i % 3 == 0) else far if i % 3 == 1 else last))
    assert len(set(pos)) == len(pos) and min(p for p in pos if p > 4096 * 4) >= 150_000
    return pos


_TWO_STAGE = {}


def _two_stage_shard(dim):
    """One shard per dimension, shared by the cases (the options differ, the rows do not)."""
    if dim not in _TWO_STAGE:
        _TWO_STAGE.clear()                                                # (one at a time: 150 MB each)
        n = TWO_STAGE_N
        emb, where = data.planted_corpus(dim, n=n, seed=1, positions=_two_stage_positions(dim, n))
        assert any(p >= 196_608 for p in where) and any(150_000 <= p < 160_000 for p in where)
        assert any(m == 3 * dim // 4 and p < 4096 for p, (_, m) in where.items())
        created = np.full(n, NOW, dtype=np.int64)
        _TWO_STAGE[dim] = {"dim": dim, "emb": emb, "where": where, "n": n, "want": {},
                           "corpus": orc.OracleCorpus(emb, created, ["x"] * n)}
    return _TWO_STAGE[dim]


def _two_stage_oracle(s, q):
    key = q.tobytes()
    if key not in s["want"]:
        s["want"][key] = s["corpus"].search(q, "", NOW, K, candidate_limit=s["n"], threads=8)
    return s["want"][key]


TWO_STAGE_CASES = [(128, 1, 0), (128, 0, 0), (128, 2, 0), (192, 1, 0), (192, 0, 0), (192, 2, 0), (128, 0, 1)]


@pytest.mark.parametrize("dim,two_stage,fuse", TWO_STAGE_CASES, ids=[f"{d}-two_stage{t}" + ("-fused" if f else "") for d, t, f in TWO_STAGE_CASES])
def test_two_stage_forms_keep_rows_whose_sums_overflow(dim, two_stage, fuse):
    """The parametrisation of test_winner_with_subnormal_products_survives_the_screen (int8 shadow, no two-stage pass, in-kernel
    bf16 conversion; the bf16 shadow at 192), and the fused split GEMM behind a sampled prefix once.  1, 4, 6 and 130 queries;
    the big query and two ordinary ones per batch against the oracle."""
    P = pkg()
    s = _two_stage_shard(dim)
    n = s["n"]
    idx = bounds._index(P, s["emb"])
    if two_stage != 1:
        idx.set_option("two_stage", two_stage)
    if fuse:
        idx.set_option("fuse_epilogue", 1)
    want_big = data.expected_order(dim, s["where"])[:K]
    for B in (1, 4, 6, 130):
        qs, kinds = data.query_batch(dim, B, specials=False)
        got = idx.search(qs, [P.text.query_terms("")] * B, NOW, K, candidate_limit=n)
        plain = [b for b, k in enumerate(kinds) if k == "gauss"]
        checked = [0] + plain[:2] + ([B - 1] if B > 1 else [])
        _check_batch(got, lambda b: _two_stage_oracle(s, qs[b]), B, checked, f"dim {dim}, two_stage {two_stage}, fuse {fuse}")
        assert list(got[0][0]) == want_big, (dim, two_stage, B)
    idx.close()


def test_two_stage_masked_search_keeps_rows_whose_sums_overflow():
    """The same search inside a scope of every second row (the masked screen: its floor comes from an in-scope sample)."""
    P = pkg()
    dim, B = 128, 6
    s = _two_stage_shard(dim)
    n = s["n"]
    scope = np.arange(0, n, 2, dtype=np.int64)
    half = orc.OracleCorpus(s["emb"][::2], np.full(len(scope), NOW, dtype=np.int64), ["x"] * len(scope))
    idx = bounds._index(P, s["emb"])
    qs, kinds = data.query_batch(dim, B, specials=False)
    rows, scores, counts = idx.search_masked(qs, [P.text.query_terms("")] * B, NOW, K, scope, candidate_limit=n)
    for b in (0, 1, 2, B - 1):
        orow, osc, _ = half.search(qs[b], "", NOW, K, candidate_limit=len(scope), threads=8)
        _same((rows[b], scores[b], counts[b]), (np.asarray(orow) * 2, osc), ("masked", b))
    in_scope = [p for p in data.expected_order(dim, s["where"]) if p % 2 == 0]
    assert len(in_scope) >= 3 and list(rows[0][:len(in_scope[:K])]) == in_scope[:K]
    idx.close()


# ---------------------------------------------------------------------------
# Range search
# ---------------------------------------------------------------------------

def test_range_search_returns_the_rows_whose_sums_overflow():
    """orr_search_range_cosine and its bulk form with the big query at 0.7 and 0.72 (between the planted cosines 0.6875, 0.71875
    and 0.75 at dim 128): membership, order and cosine bits equal tests/test_gpu_scope_near.py's restatement."""
    import test_gpu_range_cosine as rbase
    import test_gpu_scope_near as nbase
    tbase = nbase.tbase
    n, dim = 20_000, 128
    emb, where = data.planted_corpus(dim, n=n, seed=1)
    _, created, rowbytes = tbase._rows(n, 64)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    idx = tbase._build(emb, created, rowbytes, ids, n)
    model = nbase.Model(emb, created, rowbytes, ids)
    rng = np.random.default_rng(9)
    q = np.stack([data.big_query(dim), data.big_query(dim), rng.standard_normal(dim).astype(np.float32), emb[63]])
    t = np.array([0.7, 0.72, 0.25, 0.7], np.float64)
    c = model.cos(q[0])
    assert sorted(np.flatnonzero(c >= 0.7)) == sorted(p for p, (_, m) in where.items() if (dim - 2 * m) / dim >= 0.7)
    assert (c >= 0.72).sum() < (c >= 0.7).sum() and (c >= 0.72).sum() >= 6
    for form in (1, 2, 0):
        idx.set_option("range_form", form)
        rbase._check(idx.range_cosine(q, t, 64), model, q, t, 64, what=("walked", form))
    rbase._check(idx.range_cosine_bulk(q, t, 64), model, q, t, 64, what="bulk")
    idx.close()
