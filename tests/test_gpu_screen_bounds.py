"""Every screening kernel against the bound its certificate charges.

A fast search is exact only while (a) each approximate dot kernel stays inside its stated bound and (b) the int8 screen's
per-pair Cauchy-Schwarz bound is sound for every (query, row).  End-to-end parity sees a violation of either only when a true
top-k row happens to fall below the floor (tests/test_gpu_i8_gemm_exact.py records what that is worth), so here every
constant, every integer and every approximate dot the certificates rest on is fetched through a diagnostic entry point and
compared with a float64 restatement:

  * the int8 row constants (scale, rel_err, rel_hat, rowf) and query constants (s1, both images, err2, err2_level1):
    sound (>= the true value) and tight (within the factors i8_rel_norms / i8_queries_kernel apply);
  * the streaming int8 screen's (K2i) two accumulators per pair: bit exact, both unit forms, 1..4 queries, and shapes at which
    its grid-stride loop runs twice;
  * the f32-MFMA stream (K2s), the split-bf16 GEMM and the plain-bf16 screening GEMM: bit exact on small integers (a K-slice
    skipped or counted twice cannot hide inside a rounding bound), and inside the bound the pass charges on Gaussian data;
  * the per-pair bound itself, K2i and K2j form, against the cosine in the reference's arithmetic (fp32 products summed in
    double), down to scales at which those products are subnormal;
  * one end-to-end corpus on which a bound that charges subnormal products a relative error provably loses the winner.
"""
import numpy as np
import pytest

from helpers import NOW, orc, pkg

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23
DEN32 = 2.0 ** -149                                                       # the smallest fp32 denormal
MIN_NORM_B = 2.0 ** -96                                                   # kI8MinNormB: below it a row is never screened out
MIN_QUERY_MAX = 2.0 ** -48                                                # kI8MinQueryMax: below it every pair of a query passes


# ---------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------

def _ref_norm(v):
    """sum_k (double) fl32(v_k^2), left to right (RecallSearchService.cs:77-82)."""
    with np.errstate(all="ignore"):
        return np.cumsum((v * v).astype(np.float64), axis=-1)[..., -1]


def _ref_cos(qs, emb):
    """The reference's cosine of every pair, [B, n]: fp32 products, summed in double (numpy's pairwise order differs from the
    reference's by 2^-53 relative per addition: 1e-13 here, and nothing at all where the products are subnormal, whose sums are
    exact in double)."""
    with np.errstate(all="ignore"):
        na, nb = _ref_norm(qs), _ref_norm(emb)
        dot = np.stack([(emb * q[None, :]).astype(np.float64).sum(axis=1) for q in qs])
        cos = dot / (np.sqrt(na)[:, None] * np.sqrt(nb)[None, :])
        return np.where((na <= 0)[:, None] | (nb <= 0)[None, :], 0.0, cos), na, nb


def _ru32(x):
    """float64 -> float32, rounded up."""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float64)
        f = x.astype(np.float32)
        return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def _quantise_rows64(emb):
    """i8_quantise_row restated: scale (fp32), image, and the float64 sums of (e - e^)^2 and e^^2."""
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(emb).all(axis=1)
        mx = np.where(bad, np.float32(0), np.abs(np.where(np.isfinite(emb), emb, np.float32(0))).max(axis=1)).astype(np.float32)
        se = (mx / np.float32(127.0)).astype(np.float32)
        inv = np.where(se > 0, np.float32(1.0) / np.where(se > 0, se, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        q = np.rint((np.where(bad[:, None], np.float32(0), emb) * inv[:, None]).astype(np.float32))
        ie = np.clip(q, -127, 127).astype(np.int8)
        hat = se.astype(np.float64)[:, None] * ie.astype(np.float64)
        d2 = ((emb.astype(np.float64) - hat) ** 2).sum(axis=1)
        h2 = (hat ** 2).sum(axis=1)
    return se, ie, bad, d2, h2


def _quantise_queries64(qs):
    """i8_queries_kernel restated: s1, both int8 levels, and the float64 |q - q^|^2 after one level and after two."""
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(qs).all(axis=1)
        mx = np.abs(qs).max(axis=1).astype(np.float32)
        usable = (mx > 0) & ~bad
        s1 = np.where(usable, (mx / np.float32(127.0)).astype(np.float32), np.float32(0)).astype(np.float32)
        s2 = (s1 / np.float32(254.0)).astype(np.float32)
        safe1 = np.where(usable, s1, np.float32(1))
        a = np.clip(np.rint((qs / safe1[:, None]).astype(np.float32)), -127, 127)
        a = np.where(usable[:, None], a, 0.0)
        r = qs.astype(np.float64) - s1.astype(np.float64)[:, None] * a
        ok2 = usable & (s2 > 0)
        c2 = np.clip(np.rint(r / np.where(ok2, s2, np.float32(1)).astype(np.float64)[:, None]), -127, 127)
        c2 = np.where(ok2[:, None], c2, 0.0)
        dl = r - s1.astype(np.float64)[:, None] * (c2 / 254.0)
        q2 = (qs.astype(np.float64) ** 2).sum(axis=1)
        e1 = np.where(usable, (r * r).sum(axis=1), q2)
        e2 = np.where(usable, (dl * dl).sum(axis=1), q2)
    return s1, a.astype(np.int8), c2.astype(np.int8), e1, e2, bad, mx


def _bound_k2i(rel_err, rel_hat, err2, inv_sqrt_na):
    """screen_gemv_i8_kernel's per-pair bound on 0.7 cos, [B, n]."""
    with np.errstate(all="ignore"):
        re, rh = rel_err.astype(np.float64)[None, :], rel_hat.astype(np.float64)[None, :]
        return 0.7 * 1.000001 * (re * 1.0000003 + (np.sqrt(err2) * inv_sqrt_na)[:, None] * rh + 1.2e-7) + 1e-9


def _rowf_of(rel_err, rel_hat):
    """i8_rowf_of's .y and .z in float64, before the rounding up."""
    with np.errstate(all="ignore"):
        return (0.7 * 1.000002 * (rel_err.astype(np.float64) * 1.0000003 + 2.4e-7) + 1e-9, rel_hat.astype(np.float64) * 1.000001)


def _bound_k2j(rowf, err2_level1, inv_sqrt_na):
    """The int8 screening GEMM's per-pair bound on 0.7 cos: rowf.y + qf.w rowf.z, qf.w restated from fused_query_const_of."""
    with np.errstate(all="ignore"):
        qw = _ru32(0.7 * 1.000001 * np.sqrt(err2_level1) * inv_sqrt_na).astype(np.float64)
        return rowf[:, 1].astype(np.float64)[None, :] + qw[:, None] * rowf[:, 2].astype(np.float64)[None, :]


def _inside(value, true, factor):
    """true <= value <= true * factor + one fp32 denormal, elementwise (inf == inf passes)."""
    with np.errstate(all="ignore"):
        value, true = np.asarray(value, dtype=np.float64), np.asarray(true, dtype=np.float64)
        return (value >= true) & (value <= true * factor + DEN32)


def _index(P, emb):
    n, dim = emb.shape
    idx = P.RecallIndex(dim=dim)
    idx.append(emb, np.full(n, NOW, dtype=np.int64), [b"x"] * n)
    idx.seal()
    return idx


# ---------------------------------------------------------------------------
# Row and query families
# ---------------------------------------------------------------------------

def _row_families(rng, dim, scale=1.0):
    sign = rng.choice([-1.0, 1.0], dim)
    g = rng.standard_normal((5, dim))
    fam = {"gauss 1e-3": g[0] * 1e-3, "gauss": g[1], "gauss 50": g[2] * 50.0, "zero": np.zeros(dim)}
    for k in (0, dim - 1):
        v = np.zeros(dim)
        v[k] = -2.5
        fam[f"one-hot {k}"] = v
    fam["equal magnitude"] = sign * 1.0
    v = rng.choice([-1.0, 1.0], dim)
    v[dim // 3] = 1e4
    fam["one coordinate 1e4 times the rest"] = v
    v = (rng.integers(-127, 127, dim) + 0.5) * 2.0 ** -7                  # half-steps (j + 0.5) se with se = 2^-7 ...
    v[5] = 127 * 2.0 ** -7                                                # ... because max|e| = 127 se
    fam["half steps"] = v
    v = g[3].copy()
    v[7] = np.inf
    fam["inf"] = v
    v = g[4].copy()
    v[dim - 2] = np.nan
    fam["nan"] = v
    with np.errstate(all="ignore"):
        return {k: (v * scale).astype(np.float32) for k, v in fam.items()}


def _huge_families(rng, dim):
    """Finite rows and queries at the large end: every fp32 square and product of the equal-magnitude one is 2.25e38 (finite), its
    norms and the reference's double sums are finite, and no fp32 sum of two like-signed products is
    (tests/test_overflowing_sums_cpu.py); the Gaussian one holds coordinates whose fp32 squares overflow."""
    return {"gauss 1e19": (rng.standard_normal(dim) * 1e19).astype(np.float32),
            "equal magnitude 1.5e19": (rng.choice([-1.0, 1.0], dim) * 1.5e19).astype(np.float32)}


def _place(rng, n, dim, fam, scale=1.0):
    """Gaussian rows with every family row in the first tile, a middle tile and the partial last tile."""
    emb = (rng.standard_normal((n, dim)) * scale).astype(np.float32)
    where = {}
    for t, base in enumerate((3, 256 + 17, 2 * 256 + 9)):
        for j, (name, v) in enumerate(fam.items()):
            emb[base + 3 * j] = v
            where[(name, t)] = base + 3 * j
    return emb, where


N_CONST = 2 * 256 + 100


# ---------------------------------------------------------------------------
# Quantisation constants
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 3072])
def test_int8_row_constants_are_sound_and_tight(dim):
    """scale, rel_err, rel_hat and rowf of the int8 shadow against a float64 restatement of the quantisation: never below the
    true relative norms (a rel_err that is too small drops rows silently), never above them by more than the factors
    i8_rel_norms applies (1.000001, then one rounding up to fp32).  Rows whose norm is 0 hold 0 / 0, rows with a non-finite
    coordinate inf / 0, and so do rows whose norm is positive but below 2^-96, where the bound's relative charge for the
    reference's fp32 products no longer holds."""
    P = pkg()
    rng = np.random.default_rng(1000 + dim)
    fam = _row_families(rng, dim)
    sign = rng.choice([-1.0, 1.0], dim)
    fam["equal magnitude 3e-21"] = (sign * 3e-21).astype(np.float32)      # normB = D 9e-42 < 2^-96
    fam["equal magnitude 2^-48"] = (sign * 2.0 ** -48).astype(np.float32)  # normB = D 2^-96: the bounded route
    for name, s in (("one-hot 2^-48", np.float32(2.0 ** -48)), ("one-hot below 2^-48", np.nextafter(np.float32(2.0 ** -48), np.float32(0)))):
        v = np.zeros(dim, dtype=np.float32)
        v[dim // 2] = s                                                   # normB = 2^-96 exactly / just below it
        fam[name] = v
    fam.update(_huge_families(rng, dim))
    emb, where = _place(rng, N_CONST, dim, fam)
    idx = _index(P, emb)
    c = idx.screen_i8_consts()
    _, _, ie = idx.screen_i8_dots(emb[:1], 0)
    idx.close()

    se, ie_ref, bad, d2, h2 = _quantise_rows64(emb)
    nb = _ref_norm(emb)
    assert np.array_equal(ie, ie_ref), "the int8 images differ from the restated quantisation"
    assert np.array_equal(c["scale"], se), "the scales differ from the restated quantisation"
    with np.errstate(all="ignore"):
        true_err, true_hat = np.sqrt(d2 / nb), np.sqrt(h2 / nb)
    zero = ~(nb > 0)                                                      # (a NaN norm as well: the score is NaN whatever the dot)
    never = ~zero & (bad | (nb < MIN_NORM_B))
    plain = ~zero & ~never
    assert zero.sum() >= 6 and never.sum() >= 9 and plain.sum() >= N_CONST - 60
    for t in range(3):
        assert zero[where[("zero", t)]] and zero[where[("nan", t)]]
        assert never[where[("inf", t)]] and never[where[("equal magnitude 3e-21", t)]] and never[where[("one-hot below 2^-48", t)]]
        assert plain[where[("one-hot 2^-48", t)]] and plain[where[("equal magnitude 2^-48", t)]]
        assert plain[where[("equal magnitude 1.5e19", t)]] and np.isfinite(nb[where[("equal magnitude 1.5e19", t)]])
    assert np.all(c["rel_err"][zero] == 0) and np.all(c["rel_hat"][zero] == 0), "zero-norm rows: 0 / 0"
    assert np.all(np.isposinf(c["rel_err"][never])) and np.all(c["rel_hat"][never] == 0), "never-screened-out rows: inf / 0"
    factor = (1 + 1e-6) * (1 + U23)
    for name, got, true in (("rel_err", c["rel_err"], true_err), ("rel_hat", c["rel_hat"], true_hat)):
        ok = _inside(got[plain], true[plain], factor)
        worst = np.flatnonzero(plain)[~ok]
        assert ok.all(), f"{name}: rows {worst[:8]}: {got[worst[:8]]} against true {true[worst[:8]]}"
    # rowf = i8_rowf_of(scale, rel_err, rel_hat): each term rounded up once
    y, z = _rowf_of(c["rel_err"], c["rel_hat"])
    rowf = c["rowf"]
    assert np.array_equal(rowf[:, 0], c["scale"]) and np.all(rowf[:, 3] == 0)
    assert _inside(rowf[:, 1], y, 1 + U23).all() and _inside(rowf[:, 2], z, 1 + U23).all()
    assert np.all(np.isposinf(rowf[never, 1]))


@pytest.mark.parametrize("dim", [128, 3072])
def test_int8_query_constants_are_exact_sound_and_tight(dim):
    """s1 and both int8 levels of the queries bit for bit; err2 (two levels: the stream's) and err2_level1 (one level: the
    screening GEMM's) within [true, true (1 + 1e-6)(1 + 2^-52 D)] of the float64 |q - q^|^2; +inf for a query with a
    non-finite coordinate and for one whose largest coordinate is below 2^-48 (every pair of such a query passes)."""
    P = pkg()
    rng = np.random.default_rng(2000 + dim)
    fam = _row_families(rng, dim)
    fam["equal magnitude 3e-21"] = (rng.choice([-1.0, 1.0], dim) * 3e-21).astype(np.float32)
    fam["gauss 1e-19"] = (rng.standard_normal(dim) * 1e-19).astype(np.float32)
    v = np.zeros(dim, dtype=np.float32)
    v[dim // 2] = 2.0 ** -48
    fam["one-hot 2^-48"] = v
    v = (rng.standard_normal(dim) * 1e-30).astype(np.float32)
    v[3] = np.nextafter(np.float32(2.0 ** -48), np.float32(0))
    fam["largest just below 2^-48"] = v
    fam.update(_huge_families(rng, dim))
    names = list(fam)
    qs = np.stack([fam[k] for k in names] + [rng.standard_normal(dim).astype(np.float32) for _ in range(4)])
    emb = rng.standard_normal((300, dim)).astype(np.float32)
    idx = _index(P, emb)
    c = idx.screen_i8_consts(qs)
    _, iq1, _ = idx.screen_i8_dots(qs, 0)
    idx.close()

    s1, a, c2, e1, e2, bad, mx = _quantise_queries64(qs)
    differ = np.flatnonzero(c["s1"] != s1)
    assert differ.size == 0, f"s1 differs from the restated quantisation for {[(names + ['gauss'] * 4)[i] for i in differ]}: {c['s1'][differ]!r} != {s1[differ]!r}"
    assert np.array_equal(iq1, a), "the first int8 level differs from the restated quantisation"
    assert np.array_equal(c["iq2"], c2), "the second int8 level differs from the restated quantisation"
    unbounded = bad | ((mx > 0) & (mx < MIN_QUERY_MAX))
    for k in ("inf", "nan", "equal magnitude 3e-21", "gauss 1e-19", "largest just below 2^-48"):
        assert unbounded[names.index(k)], k
    for k in ("zero", "one-hot 0", f"one-hot {dim - 1}", "one-hot 2^-48", "gauss 1e-3", "half steps", "gauss 1e19", "equal magnitude 1.5e19"):
        assert not unbounded[names.index(k)], k
    assert np.all(np.isposinf(c["err2"][unbounded])) and np.all(np.isposinf(c["err2_level1"][unbounded]))
    factor = (1 + 1e-6) * (1 + 2.0 ** -52 * dim)
    for name, got, true in (("err2", c["err2"], e2), ("err2_level1", c["err2_level1"], e1)):
        lo, hi = true[~unbounded], true[~unbounded] * factor
        g = got[~unbounded]
        assert np.all((g >= lo) & (g <= hi)), f"{name}: {g} outside [{lo}, {hi}]"
    assert c["err2"][names.index("zero")] == 0 and c["err2_level1"][names.index("zero")] == 0
    assert np.all(e2[~unbounded] <= e1[~unbounded])                       # (the second level only ever helps)


# ---------------------------------------------------------------------------
# K2i: the streaming int8 screen's integers, bit exact
# ---------------------------------------------------------------------------

def _extreme_rows(rng, n, dim):
    """Gaussian rows plus the rows that drive the accumulators to their extremes (tests/test_gpu_i8_gemm_exact.py), in the first
    tile, in a later tile and in the partial last tile."""
    emb = rng.standard_normal((n, dim), dtype=np.float32)
    for r in (0, 256 * 9 + 5, n - 3):
        emb[r] = 1.0
        emb[r + 1] = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0)
    emb[7] = 0.0
    for r in (300, n - 40):
        emb[r] = 0.0
        emb[r, dim - 1] = 5.0                                             # one coordinate only, in the LAST K-tile
    for r in (600, n - 50):
        emb[r] = 0.0
        emb[r, 0] = -3.0                                                  # ... in the FIRST K-tile
    return emb


# The launch caps the grid at 512 workgroups of 4 units: 1025 tiles of two 128-row units and 129 tiles of sixteen 16-row units are
# the smallest shards at which the kernel's grid-stride loop runs a second time.  (The 16-row-unit form needs D % 1024 == 0.)
K2I_SHAPES = [(6244, 128, (False,)), (6244, 384, (False,)), (6244, 1024, (True,)), (6244, 3072, (False, True)),
              (1025 * 256 - 156, 128, (False,)), (129 * 256 - 156, 1024, (True,))]


@pytest.mark.parametrize("n,dim,forms", K2I_SHAPES, ids=[f"{n}x{d}" for n, d, _ in K2I_SHAPES])
def test_streaming_int8_screen_accumulators_bit_exact(n, dim, forms):
    """(I1, I2) of screen_gemv_i8_kernel = numpy's integer products of the int8 images, for 1..4 queries in both unit forms:
    two accumulators per pair, a clamped prefetch and a cross-lane reduction that no other test looks at."""
    P = pkg()
    rng = np.random.default_rng(3000 + n + dim)
    emb = _extreme_rows(rng, n, dim)
    idx = _index(P, emb)
    qs = rng.standard_normal((4, dim)).astype(np.float32)
    qs[0] = 1.0                                                           # with row 0: I1 = D 127^2, the largest there is
    qs[1] = emb[n - 40] + 0.001 * qs[1]                                   # mostly second-level digits outside the last K-tile
    qs[2, : dim - 64] = 0.0                                               # the last K-tile only
    _, iq1, ie = idx.screen_i8_dots(qs, 0)
    iq2 = idx.screen_i8_consts(qs)["iq2"]
    se, ie_ref, _, _, _ = _quantise_rows64(emb)
    assert np.array_equal(ie, ie_ref)
    ie64 = ie.astype(np.float64)
    # exact in binary64: |sum| <= 3072 * 127^2 < 2^53
    want = np.stack([iq1.astype(np.float64) @ ie64.T, iq2.astype(np.float64) @ ie64.T], axis=1).astype(np.int64)   # [4][2][n]
    assert np.abs(want[:, 1]).max() > 0
    for unit16 in forms:
        for nq in (1, 2, 3, 4):
            for q0 in ((0, 4 - nq) if nq < 4 else (0,)):                  # (every query also runs as a launch's first)
                got = idx.screen_i8_stream_dots(qs[q0:q0 + nq], unit16=unit16)
                what = f"{n} rows x {dim}, {'16' if unit16 else '128'}-row units, queries {q0}..{q0 + nq - 1}"
                assert not np.any(got.view(np.uint32) == 0xABABABAB), f"{what}: elements never written"
                g = got.astype(np.int64)
                if not np.array_equal(g, want[q0:q0 + nq]):
                    bad = np.argwhere(g != want[q0:q0 + nq])
                    b, lv, r = bad[0]
                    raise AssertionError(f"{what}: {len(bad)} of {g.size} accumulators differ; first at query {q0 + b}, level "
                                         f"{lv + 1}, row {r} (tile {r // 256}): {g[b, lv, r]} != {want[q0 + b, lv, r]}")
    assert want[0, 0, 0] == dim * 127 * 127
    if dim % 1024 != 0:
        with pytest.raises(P.native.OrrError):                            # no 16-row-unit form at this dimension
            idx.screen_i8_stream_dots(qs[:1], unit16=True)
    with pytest.raises(P.native.OrrError):
        idx.screen_i8_stream_dots(np.concatenate([qs, qs[:1]]), unit16=False)   # five queries: not this kernel's
    idx.close()


# ---------------------------------------------------------------------------
# The float kernels: K2s (f32 MFMA stream), the split-bf16 GEMM, the plain-bf16 screening GEMM
# ---------------------------------------------------------------------------

N_FLOAT = 6244                                                            # a multiple of neither 64, 128 nor 256
B_K2S = (1, 5, 16, 17, 32, 33)                                            # gemv_mfma16_kernel up to 16, gemv_mfma_kernel to 32, then a second launch
B_SPLIT = (5, 255, 256, 257, 300)
B_SCREEN = (3, 70, 300)
# K2s's grid is capped at 4096 workgroups of 256 rows: its grid-stride loop needs more than a million rows to run twice, which is
# left to the scale tests.


@pytest.fixture(scope="module", params=[64, 192, 3072])
def float_case(request):
    """One integer corpus and one Gaussian corpus per dimension, with their float64 references, shared by the tests below."""
    P = pkg()
    dim = request.param
    rng = np.random.default_rng(4000 + dim)
    ints = rng.integers(-8, 9, (N_FLOAT, dim)).astype(np.float32)
    ints[N_FLOAT - 1] = 8.0
    qi = rng.integers(-8, 9, (300, dim)).astype(np.float32)
    qi[0] = 8.0                                                           # with the last row: 64 D, the largest sum there is
    qi[4, : dim - 1] = 0.0                                                # the last coordinate only
    qi[4, dim - 1] = 1.0
    gauss = (rng.standard_normal((N_FLOAT, dim)) * rng.choice([1e-3, 1.0, 50.0], (N_FLOAT, 1))).astype(np.float32)
    qg = rng.standard_normal((300, dim)).astype(np.float32)
    qg[0] = gauss[N_FLOAT - 1]
    qg[4] = gauss[100]
    case = {"dim": dim, "ints": _index(P, ints), "gauss": _index(P, gauss), "qi": qi, "qg": qg,
            "want_i": (qi.astype(np.float64) @ ints.astype(np.float64).T).astype(np.float32),     # integers below 2^24: exact
            "want_g": qg.astype(np.float64) @ gauss.astype(np.float64).T,
            "scale_g": np.abs(qg).astype(np.float64) @ np.abs(gauss).astype(np.float64).T, "shares": {}}
    yield case
    for k in ("ints", "gauss"):
        case[k].close()
    for name, share in sorted(case["shares"].items()):
        print(f"[screen bounds] dim {dim}: {name}: largest error {share:.3f} of its bound")


def _exact(case, B, dots, what):
    """Integers in [-8, 8] are exact in bf16 and every partial sum is at most 3072 * 64 < 2^24, so whatever the order of
    summation the dots equal the integer product bit for bit.  At D = 3072 a rounding bound of (2 D + 2) 2^-23 cannot see a
    dropped coordinate (1 / D of sum |q_k e_k|); this can.  What it cannot see: every bf16 lo half of such integers is zero, so
    of the split GEMM only hi * hi is exercised here.  A skipped hi * lo or lo * hi product shows in the Gaussian bound test
    alone, and by magnitude only at D = 64 and 192 (2^-9 / sqrt(D) of sum |q_k e_k| against a bound that grows with D): the
    small dimensions must stay."""
    want = case["want_i"][:B]
    if not np.array_equal(dots, want):
        bad = np.argwhere(dots != want)
        b, r = bad[0]
        raise AssertionError(f"{what}, dim {case['dim']}, {B} queries: {len(bad)} of {dots.size} dots differ; first at query {b}, "
                             f"row {r}: {dots[b, r]} != {want[b, r]}")
    assert dots[0, N_FLOAT - 1] == 64 * case["dim"] and dots.shape == (B, N_FLOAT)


def _bounded(case, B, dots, eps, what):
    err = np.abs(dots.astype(np.float64) - case["want_g"][:B])
    share = float((err / (eps * case["scale_g"][:B] + 1e-300)).max())
    case["shares"][what] = max(case["shares"].get(what, 0.0), share)
    print(f"[screen bounds] {what}, dim {case['dim']}, {B} queries: largest error {share:.3f} of the bound")
    assert share <= 1.0, (what, case["dim"], B, share)


@pytest.mark.parametrize("B", B_K2S)
def test_f32_mfma_stream_dots_exact_on_small_integers(float_case, B):
    _exact(float_case, B, float_case["ints"].pass_dots(float_case["qi"][:B], 0), "f32 MFMA stream")


@pytest.mark.parametrize("B", B_K2S)
def test_f32_mfma_stream_dots_stay_inside_the_bound_the_certificate_charges(float_case, B):
    """Error against float64, relative to sum |q_k e_k|: D products and D additions charged one unit in the last place each."""
    eps = (2.0 * float_case["dim"] + 2.0) * U23
    _bounded(float_case, B, float_case["gauss"].pass_dots(float_case["qg"][:B], 0), eps, "f32 MFMA stream")


@pytest.mark.parametrize("B", B_SPLIT)
def test_split_bf16_gemm_dots_exact_on_small_integers(float_case, B):
    _exact(float_case, B, float_case["ints"].pass_dots(float_case["qi"][:B], 1), "split-bf16 GEMM")


@pytest.mark.parametrize("B", B_SPLIT)
def test_split_bf16_gemm_dots_stay_inside_the_bound_the_certificate_charges(float_case, B):
    """3 D additions of exact products, the dropped lo * lo and the split's second-order residuals (u = 2^-8)."""
    eps = 3.1 * 2.0 ** -16 + 3.06 * float_case["dim"] * U23
    _bounded(float_case, B, float_case["gauss"].pass_dots(float_case["qg"][:B], 1), eps, "split-bf16 GEMM")


@pytest.mark.parametrize("B", B_SCREEN)
def test_plain_bf16_screening_dots_exact_on_small_integers(float_case, B):
    """(Its bound is checked by test_screening_dots_stay_inside_the_bound_the_two_stage_pass_uses.)"""
    _exact(float_case, B, float_case["ints"].screen_dots(float_case["qi"][:B]), "plain-bf16 screening GEMM")


# ---------------------------------------------------------------------------
# The per-pair bound against the reference's cosine
# ---------------------------------------------------------------------------

BOUND_SCALES = [1.0, 1e-19, 3e-20, 1e-20, 3e-21, 1e18, 2.0 ** -48]       # 2^-48: the smallest at which equal-magnitude vectors keep a finite bound


@pytest.mark.parametrize("scale", BOUND_SCALES, ids=[f"{s:g}" for s in BOUND_SCALES])
def test_per_pair_bound_covers_the_reference_cosine(scale):
    """|0.7 cos_ref - 0.7 cos^| <= the bound the screen adds, for every pair, with the bound built in numpy from the constants and
    integers the library hands back: the stream's form (K2i) and the screening GEMM's (K2j: rowf.y + qf.w rowf.z).  cos_ref is the
    reference's: fp32 products summed in double.  The bound charges those products 1.2e-7 relative, which stops holding once
    they are subnormal: rows of equal magnitude 3e-21 against themselves are off by 580 times the bound, so such rows and
    queries must come back with an infinite bound instead (never screened out).  Which scales judge what: at 1, 1e18 and 2^-48
    nearly every pair has a finite bound that has to hold; at 1e-19 ... 3e-21 every scaled row has normB < 2^-96, so what is
    checked there is that the library no longer hands back a finite bound for them (the pairs of unit-scale queries with those
    rows included) -- 2^-48 is the scale that tests finite bounds next to the thresholds."""
    P = pkg()
    dim = 128
    rng = np.random.default_rng(5000)
    fam = _row_families(rng, dim, scale)
    fam.update(_huge_families(rng, dim))                                  # (whatever the scale of the rest)
    emb, where = _place(rng, N_CONST, dim, fam, scale)
    names = list(fam)
    with np.errstate(all="ignore"):
        extra = [rng.standard_normal(dim) * scale, rng.standard_normal(dim) * 30.0 * scale, rng.choice([-1.0, 1.0], dim) * scale]
        for k in (0, dim - 1):
            v = np.zeros(dim)
            v[k] = scale
            extra.append(v)
        scaled = np.stack([fam[k] for k in names] + [np.asarray(v).astype(np.float32) for v in extra]).astype(np.float32)
    unit = np.stack([v for k, v in _row_families(rng, dim).items() if k not in ("inf", "nan", "zero")])   # the same against queries of scale 1
    qs = scaled if scale == 1.0 else np.concatenate([scaled, unit])
    idx = _index(P, emb)
    c = idx.screen_i8_consts(qs)
    I, iq1, ie = idx.screen_i8_dots(qs, 0)
    I12 = np.concatenate([idx.screen_i8_stream_dots(qs[b:b + 4]) for b in range(0, len(qs), 4)])
    idx.close()
    assert np.array_equal(I, iq1.astype(np.int64) @ ie.astype(np.int64).T)
    assert np.array_equal(I12[:, 0], I)

    cos_ref, na, nb = _ref_cos(qs, emb)
    with np.errstate(all="ignore"):
        inv_a = np.where(na > 0, 1.0 / np.sqrt(na), 0.0)
        inv_b = np.where(nb > 0, 1.0 / np.sqrt(nb), 0.0)                  # row_consts_of: normB <= 0 -> cosine 0
        s = (c["s1"].astype(np.float64) * inv_a)[:, None] * (c["scale"].astype(np.float64) * inv_b)[None, :]
        forms = {"K2i": (0.7 * s * (I12[:, 0] + I12[:, 1] / 254.0), _bound_k2i(c["rel_err"], c["rel_hat"], c["err2"], inv_a)),
                 "K2j": (0.7 * s * I, _bound_k2j(c["rowf"], c["err2_level1"], inv_a))}
        judged = np.isfinite(cos_ref) & (na > 0)[:, None] & np.isfinite(inv_a)[:, None]   # (use_cos is off for a query of norm 0)
        own = (names.index("equal magnitude"), where[("equal magnitude", 1)])     # the pair the relative charge fails first
        assert judged[own] and abs(cos_ref[own] - 1) < 1e-12
        huge = (names.index("equal magnitude 1.5e19"), where[("equal magnitude 1.5e19", 1)])   # finite norms, a dot no fp32 sum holds
        assert judged[huge] and abs(cos_ref[huge] - 1) < 1e-12
        for form, (approx, bound) in forms.items():
            diff = np.abs(0.7 * cos_ref - np.where(inv_b[None, :] == 0, 0.0, approx))
            ok = ~judged | (diff <= bound) | ~(bound <= 1.7976931348623157e308)   # (a bound that is not finite: the pair is kept)
            finite = judged & (bound <= 1.7976931348623157e308)
            share = float((diff[finite] / bound[finite]).max()) if finite.any() else 0.0
            print(f"[screen bounds] scale {scale:g}, {form}: {int(finite.sum())} of {judged.size} pairs with a finite bound, "
                  f"largest error {share:.3f} of it")
            if not ok.all():
                b, r = np.argwhere(~ok)[0]
                raise AssertionError(f"scale {scale:g}, {form}: {int((~ok).sum())} of {int(judged.sum())} pairs exceed their bound, by up "
                                     f"to {float((diff[~ok] / bound[~ok]).max()):.1f} times; first: query {b}, row {r}: "
                                     f"|{0.7 * cos_ref[b, r]!r} - {approx[b, r]!r}| > {bound[b, r]!r}")
    if scale == 1.0:                                                      # at an ordinary scale the bound is finite wherever the data are
        eq = [where[("equal magnitude", t)] for t in range(3)]
        assert np.all(np.isfinite(forms["K2i"][1][names.index("equal magnitude"), eq]))


# ---------------------------------------------------------------------------
# End to end: a corpus on which a relative charge for subnormal products loses the winner
# ---------------------------------------------------------------------------

def _tiny_magnitude():
    """The fp32 s in [sqrt(20) , sqrt(40)) 2^-74.5 whose square rounds UP the most in fp32 (a subnormal of 20..40 units): normA of a
    query of magnitude s is then overstated by some 2 %, and with it every cos^ the screen forms is understated."""
    best, best_rel = None, 0.0
    for m in range(20, 40):
        s = np.float32(np.sqrt((m + 0.55) * DEN32))
        rel = (float(s * s) - float(s) ** 2) / float(s) ** 2
        if rel > best_rel:
            best, best_rel = s, rel
    assert best_rel > 0.01
    return best


E2E_N = 196_608 + 77
E2E_K = 10


@pytest.mark.parametrize("dim,two_stage", [(128, 1), (128, 0), (128, 2), (192, 1), (192, 0), (192, 2)])
def test_winner_with_subnormal_products_survives_the_screen(dim, two_stage):
    """Row X has equal magnitudes of about 5e-22 and equals query 0: its reference cosine is 1 and it wins.  The screen's cos^ of
    it is 2 % low (the reference's normA is a sum of subnormal squares that round up), which a bound charging 1.2e-7 relative
    does not cover; rows Y in the sampled prefix sit on the int8 grid, so their lower bounds are tight and the floor they set
    lies above X's upper bound.  Both preconditions are asserted on the CPU from a numpy restatement of the bound WITHOUT the
    thresholds (so the test cannot go vacuous); the search must return X first all the same, for 1, 4, 6 and 130 queries.
    (128, 1) is the int8 shadow, where the thresholds hand the query's pairs to the exact re-score.  The other combinations run
    the bf16 shadow, the in-kernel bf16 conversion, the f32-MFMA stream and the split GEMM, which have no such value: there
    plan_form sends a host-resident batch with such a query down the exact pass (without that, (128, 2), (192, 1) and (192, 2)
    return rows 0..9 for 6 and 130 queries).  Every batch runs a second time with the queries in device memory, where the plan
    cannot look at them: the norm the device computes (below 16 queries: the host's, of the downloaded copy) marks the query,
    every pair of it is kept, and the query climbs the escalation ladder to the exact pass."""
    P = pkg()
    rng = np.random.default_rng(6000 + dim)
    n, k = E2E_N, E2E_K
    emb = rng.standard_normal((n, dim), dtype=np.float32)
    sign = rng.choice([-1.0, 1.0], dim)
    s = _tiny_magnitude()
    x_row = 150_000                                                       # far behind the sampled prefix (at most 16,384 rows)
    emb[x_row] = (sign * float(s)).astype(np.float32)
    n_y = k + 2
    for j in range(n_y):                                                  # the newest rows: (127 - d) 2^-7 along sign, d small integers
        emb[j] = sign * (127.0 - (np.arange(dim) % (j + 2))) * 2.0 ** -7
    qs = rng.standard_normal((130, dim)).astype(np.float32)
    qs[0] = emb[x_row]

    # preconditions, from the restated quantisation and the bound as it stood without the thresholds
    rows = np.concatenate([emb[:n_y], emb[x_row:x_row + 1]])
    se, ie, _, d2, h2 = _quantise_rows64(rows)
    nb = _ref_norm(rows)
    rel_err, rel_hat = _ru32(np.sqrt(d2 / nb) * 1.000001), _ru32(np.sqrt(h2 / nb) * 1.000001)
    assert np.all(rel_err[:n_y] == 0)                                     # on the grid: quantised exactly
    s1, a, c2, e1, e2, _, _ = _quantise_queries64(qs[:1])
    na = _ref_norm(qs[:1])
    inv_a, inv_b = 1.0 / np.sqrt(na), 1.0 / np.sqrt(nb)
    sc = (s1.astype(np.float64) * inv_a)[:, None] * (se.astype(np.float64) * inv_b)[None, :]
    I1, I2 = a.astype(np.float64) @ ie.astype(np.float64).T, c2.astype(np.float64) @ ie.astype(np.float64).T
    rowf = np.stack([se, _ru32(_rowf_of(rel_err, rel_hat)[0]), _ru32(_rowf_of(rel_err, rel_hat)[1]), np.zeros_like(se)], axis=1)
    for form, approx, bound in (("K2i", 0.7 * sc * (I1 + I2 / 254.0), _bound_k2i(rel_err, rel_hat, e2 * 1.000001, inv_a)),
                                ("K2j", 0.7 * sc * I1, _bound_k2j(rowf, e1 * 1.000001, inv_a))):
        upper_x = (approx + bound)[0, n_y]
        lower_y = np.sort((approx - bound)[0, :n_y])[::-1]
        assert upper_x < lower_y[k - 1], (form, upper_x, lower_y)         # X's upper bound lies below the floor k of the Y set
    exact = np.array([orc.cosine(qs[0], r) for r in rows])
    assert exact[n_y] > exact[:n_y].max() and exact[n_y] > 1 - 1e-12      # and yet X is the winner

    idx = _index(P, emb)
    if two_stage != 1:
        idx.set_option("two_stage", two_stage)
    corpus = orc.OracleCorpus(emb, np.full(n, NOW, dtype=np.int64), ["x"] * n)
    want = [corpus.search(qs[b], "", NOW, k, candidate_limit=n, threads=8) for b in range(len(qs))]
    assert want[0][0][0] == x_row
    terms = [P.text.query_terms("")] * len(qs)
    import torch
    qd = torch.from_numpy(qs).to("cuda:0")
    for B in (1, 4, 6, 130):
        for where_q, q in (("host", qs[:B]), ("device", qd[:B])):
            got_rows, got_scores, counts = idx.search(q, terms[:B], NOW, k, candidate_limit=n)
            for b in range(B):
                orow, osc, _ = want[b]
                assert counts[b] == len(orow)
                assert list(got_rows[b, :counts[b]]) == list(orow), (B, where_q, b, got_rows[b], orow)
                assert np.array_equal(got_scores[b, :counts[b]], osc), (B, where_q, b)
    idx.close()
