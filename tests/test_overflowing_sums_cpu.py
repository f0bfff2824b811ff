"""Finite vectors whose dot sum overflows fp32: the planted data, and the arithmetic facts the GPU tests rest on.

With |q_k| = |e_k| = A = 1.5e19 every fp32 square and every fp32 product is 2.25e38 < FLT_MAX, the reference's double sums and
norms are ordinary numbers and the cosine is (D - 2m) / D for a row that differs from the query in m signs -- but two like-signed
products already exceed FLT_MAX, so no fp32 accumulation of them, in whatever order, ends on a finite value.  An approximate dot
kernel hands back +inf, -inf or NaN for such a pair, depending on the order in which it meets the flipped signs; the layouts below
put them first, last, evenly spread and in whole aligned slices so that every order a kernel might use sees each case.

tests/test_gpu_overflowing_sums.py imports the builder; what is asserted here needs no GPU.
"""
import numpy as np
import pytest

from helpers import NOW, orc

A = np.float32(1.5e19)
FLT_MAX = float(np.finfo(np.float32).max)
N_ROWS = 9_000                                                            # three kSelSegRows segments, the last partial
DIMS = (64, 128, 192, 256)
# where the big rows sit: segment and tile borders first, then scattered
POSITIONS = (0, 63, 64, 4095, 4096, 8999, 1000, 2047, 2048, 3333, 5000, 6143, 6144, 7777, 8191, 8192, 8500, 8998, 311, 4500,
             127, 128, 255, 256, 8703, 8704)


def sign_pattern(dim):
    """A fixed +-1 pattern of length dim."""
    return np.where(np.random.default_rng(77).random(dim) < 0.5, -1.0, 1.0).astype(np.float32)


def flipped(dim, layout, m):
    """The m coordinates a layout flips."""
    if layout == "front":
        return np.arange(m)
    if layout == "back":
        return np.arange(dim - m, dim)
    if layout == "every":
        return (np.arange(m) * dim) // m
    g = int(layout.split("-")[1])                                         # "slices-g": aligned groups of g, at 0, D/2, g, D/2 + g, ...
    assert m % g == 0 and (dim // 2) % g == 0
    starts = [(j // 2) * g + (j % 2) * (dim // 2) for j in range(m // g)]
    return np.concatenate([np.arange(s, s + g) for s in starts])


def planted_rows(dim):
    """[(layout, m)] in the order they are placed at POSITIONS: three flip counts near D/8 in every layout, one `back` row with
    3D/4 flips (cosine -0.5; a left-to-right sum is +inf) and three exact copies of the first `front` row."""
    ms = (dim // 8, dim // 8 + 2, dim // 8 + 4)
    kinds = [(layout, m) for m in ms for layout in ("front", "back", "every")]
    kinds += [(f"slices-{g}", m) for g in (4, 8, 16, 32) for m in ms if m % g == 0 and (dim // 2) % g == 0]
    kinds.append(("back", 3 * dim // 4))
    for at in (1, 4, 5):                                                  # the copies: rows 63, 4096 and 8999 (the original: row 0)
        kinds.insert(at, ("front", ms[0]))
    assert len(kinds) <= len(POSITIONS)
    return kinds


def big_row(dim, layout, m):
    t = sign_pattern(dim).copy()
    idx = flipped(dim, layout, m)
    assert len(np.unique(idx)) == m
    t[idx] = -t[idx]
    return (A * t).astype(np.float32)


def big_query(dim):
    return (A * sign_pattern(dim)).astype(np.float32)


def planted_corpus(dim, n=N_ROWS, seed=1, positions=POSITIONS):
    """Standard Gaussian rows with the big rows at `positions`.  Returns (emb [n, dim] fp32, where: position -> (layout, m))."""
    emb = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    where = {}
    for pos, (layout, m) in zip(positions, planted_rows(dim)):
        emb[pos] = big_row(dim, layout, m)
        where[pos] = (layout, m)
    return emb, where


def expected_order(dim, where):
    """The planted rows with a positive cosine, best first: descending cosine, ties by position."""
    return [p for p, (_, m) in sorted(where.items(), key=lambda kv: (kv[1][1], kv[0])) if dim - 2 * m > 0]


def big_positions(B):
    """Where the big query sits in a batch of B: 0, 31, 32 and last."""
    return sorted({p for p in (0, 31, 32, B - 1) if 0 <= p < B})


def query_batch(dim, B, seed=2, specials=True):
    """B queries: the big one at big_positions(B); then (specials) one zero, one NaN-holding and one 1e25-scaled query in the first
    free slots while at least one slot stays ordinary; the rest standard Gaussian.  Returns (qs, kinds [B])."""
    rng = np.random.default_rng(seed + 1000 * dim)
    qs = rng.standard_normal((B, dim)).astype(np.float32)
    kinds = ["gauss"] * B
    for p in big_positions(B):
        qs[p] = big_query(dim)
        kinds[p] = "big"
    if specials:
        free = [b for b in range(B) if kinds[b] == "gauss"]
        for b, kind in zip(free[:max(0, len(free) - 1)], ("zero", "nan", "1e25")):
            kinds[b] = kind
            if kind == "zero":
                qs[b] = 0.0
            elif kind == "nan":
                qs[b, dim // 2] = np.nan
            else:
                with np.errstate(over="ignore"):
                    qs[b] = (qs[b] * np.float32(1e25)).astype(np.float32)
    return qs, kinds


def _seq32(products):
    """Left-to-right fp32 sum of each row of fp32 products."""
    with np.errstate(all="ignore"):
        return np.cumsum(products.astype(np.float32), axis=-1, dtype=np.float32)[..., -1]


def _ref_norm(v):
    with np.errstate(over="ignore"):
        return float(np.cumsum((v * v).astype(np.float64))[-1])


@pytest.fixture(scope="module", params=DIMS)
def case(request):
    dim = request.param
    emb, where = planted_corpus(dim)
    return dim, emb, where, big_query(dim)


def test_squares_products_and_norms_are_finite(case):
    dim, emb, where, q = case
    assert abs(float(A) - 1.5e19) < 1e12
    with np.errstate(over="raise"):
        for pos in where:
            e = emb[pos]
            assert np.all(np.abs(e) == A) and np.all(np.abs(q) == A)
            for prod in (q * q, e * e, q * e):                            # fp32 arithmetic
                assert prod.dtype == np.float32 and np.all(np.isfinite(prod)) and np.all(np.abs(prod) < FLT_MAX)
            assert np.isfinite(_ref_norm(e)) and _ref_norm(e) > 0
    assert np.isfinite(_ref_norm(q)) and _ref_norm(q) == dim * float(A * A)


def test_reference_cosine_is_the_planted_one(case):
    dim, emb, where, q = case
    for pos, (layout, m) in where.items():
        assert abs(orc.cosine(q, emb[pos]) - (dim - 2 * m) / dim) <= 1e-12, (pos, layout, m)
    dup = [p for p, lm in where.items() if lm == ("front", dim // 8)]
    assert len(dup) == 4 and all(np.array_equal(emb[p], emb[dup[0]]) for p in dup)
    assert np.all(np.diff(sorted(dup)) > 1)                               # copies at non-adjacent positions: ties go by position
    assert len({orc.cosine(q, emb[p]) for p in dup}) == 1


def test_no_finite_fp32_value_can_be_the_sum(case):
    dim, emb, where, q = case
    p = float(A * A)
    assert abs(p - 2.25e38) < 1e32 and 2 * p > FLT_MAX
    for pos, (layout, m) in where.items():
        assert abs(dim - 2 * m) * p > FLT_MAX, (layout, m)
        exact = float((q * emb[pos]).astype(np.float64).sum())
        assert exact == (dim - 2 * m) * p and abs(exact) > FLT_MAX


def test_left_to_right_fp32_sum_is_minus_inf_in_front_and_plus_inf_at_the_back(case):
    dim, emb, where, q = case
    seen = set()
    for pos, (layout, m) in where.items():
        s = _seq32(q * emb[pos])
        assert not np.isfinite(s), (layout, m, s)
        if layout == "front":
            assert s == -np.inf, (m, s)
        if layout == "back":
            assert s == np.inf, (m, s)
        seen.add((layout, "+inf" if s == np.inf else "-inf" if s == -np.inf else "nan"))
    assert ("front", "-inf") in seen and ("back", "+inf") in seen
    assert any(m == 3 * dim // 4 for _, m in where.values())


def test_ordinary_rows_stay_finite_and_below_the_planted_cosines(case):
    dim, emb, where, q = case
    plain = np.ones(len(emb), dtype=bool)
    plain[list(where)] = False
    with np.errstate(over="raise"):
        prods = emb[plain] * q[None, :]
    s = _seq32(prods)
    assert np.all(np.isfinite(s))
    partial = np.cumsum(prods.astype(np.float64), axis=1)
    assert np.abs(partial).max() < FLT_MAX / 1e10                         # whatever the order: sum |products| is far from the edge
    assert np.abs(prods.astype(np.float64)).sum(axis=1).max() < FLT_MAX / 1e10
    rows = np.flatnonzero(plain)
    cos = np.array([orc.cosine(q, emb[r]) for r in rows])
    planted = sorted((dim - 2 * m) / dim for _, m in where.values() if dim - 2 * m > 0)
    print(f"[overflowing sums] dim {dim}: largest ordinary cosine {cos.max():.4f}, smallest planted positive cosine {planted[0]:.4f}")
    assert cos.max() < planted[0] - 0.05, (dim, cos.max(), planted[0])
    # the expected top-k of the big query: the planted rows, descending cosine, ties by position
    order = expected_order(dim, where)
    assert len(order) == len(where) - 1 and len(order) > 10      # more than a top-10 holds
    corpus = orc.OracleCorpus(emb, np.full(len(emb), NOW, dtype=np.int64), ["x"] * len(emb))
    got, scores, _ = corpus.search(q, "", NOW, len(order), candidate_limit=len(emb))
    assert list(got) == order and np.all(np.isfinite(scores))


def test_query_batches_hold_the_big_query_where_the_kernels_switch():
    for B, want in ((1, [0]), (4, [0, 3]), (5, [0, 4]), (33, [0, 31, 32]), (64, [0, 31, 32, 63]), (130, [0, 31, 32, 129])):
        qs, kinds = query_batch(64, B)
        assert [b for b, k in enumerate(kinds) if k == "big"] == want
        assert all(np.array_equal(qs[b], big_query(64)) for b in want)
        if B >= 6:
            assert {"zero", "nan", "1e25", "gauss"} <= set(kinds)
            assert np.isinf(_ref_norm(qs[kinds.index("1e25")])) and np.isnan(qs[kinds.index("nan")]).any()
