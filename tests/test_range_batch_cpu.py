"""Range search for batches, the host half.

1. The BAND of the shared pass (include/mvdb.h: mvdb_range_band).  The pass names, per query, every row
   whose fp16 nomination score a(x) is not provably below the threshold: a(x) >= threshold - band.  It is exact only if

       |a(x) - s(x)| <= band(d, |q|, max|x|)        for every stored row x,

   s(x) being the fp32 score the exact scans compute — in THEIR summation order, which is not the matrix cores'.  The
   nomination is emulated in numpy (fp16 rounding of s_q q and s_x x, fp32 accumulation in the kernel's chains — one chain of
   d products up to d = 512, chains of 128 products added up in order beyond —, the exact power-of-two rescale) and
   compared against fp32 dot products summed sequentially, pairwise and in the scans' chunk / butterfly order.  The bound is
   PROVEN for the scans' order (the only one the library computes scores in); the other two orders are measured here.

2. The Python layer over a scripted index: scalar and per-query thresholds, count_similar_batch.
"""
import numpy as np
import pytest

from oracle import flat
from test_range_cpu import RangeOracleIndex, make_db, same
from test_split_bound import _fp16_image, _fp32_chain, _pow2_scale

DIMS = [128, 512, 1024]
SHAPES = {128: (32, 1), 512: (64, 2), 1024: (64, 4)}     # choose_shape(d / 4): G lanes per row, C chunks per lane


def chain(d):
    """Products one fp32 accumulator of range_nominate_h16_kernel takes: all d up to d = 512, 128 beyond (NACC = d / 128)."""
    return d if d <= 512 else 128


def range_eps(d):
    """Restatement of half_scan.hip: half_range_eps (per unit |q| max|x|): operand rounding, fp16 underflow, worst-case fp32
    accumulation of one chain on the matrix cores (any order, additions truncated) plus the <= 8 in-order additions of the
    partial sums, and the scan's own tree: 4 C fmaf + log2 G butterfly additions <= 4 ceil(d / 128) + 6 roundings."""
    u11, u23, u24 = 2.0 ** -11, 2.0 ** -23, 2.0 ** -24
    e_op = 2 * u11 + u11 * u11
    e_uf = np.sqrt(float(d)) * 2.0 ** -27 * (1 + u11) + d * 2.0 ** -56
    n = chain(d) + 8.0
    e_acc = n * u23 / (1 - n * u23) * (1 + u11) ** 2
    depth = (d + 127) // 128 * 4 + 6
    e_scan = depth * u24 / (1 - depth * u24)
    return (e_op + e_uf + e_acc + e_scan) * (1 + 1e-5) + 4 * u24


def nominate(products, d, mode):
    """fp32 accumulation as the kernel does it: every chain a sequential fp32 sum (`mode`: the matrix cores' additions rounded
    to nearest or truncated), the partial sums added in order (VALU: round to nearest)."""
    c = chain(d)
    total = _fp32_chain(products[..., :c], mode)
    for lo in range(c, d, c):
        total = (total + _fp32_chain(products[..., lo:lo + c], mode)).astype(np.float32)
    return total


def _fma_step(acc, a, b):
    """fp32 fmaf(a, b, acc): the product of two fp32 values is exact in float64; one rounding to fp32."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def dot_sequential(q, x):
    acc = np.zeros(x.shape[0], np.float32)
    for i in range(x.shape[1]):
        acc = _fma_step(acc, x[:, i], q[:, i])
    return acc


def dot_pairwise(q, x):
    p = (q * x).astype(np.float32)
    while p.shape[1] > 1:
        if p.shape[1] % 2:
            p = np.concatenate([p, np.zeros((p.shape[0], 1), np.float32)], axis=1)
        p = (p[:, 0::2] + p[:, 1::2]).astype(np.float32)
    return p[:, 0]


def dot_scan_order(q, x, G, C):
    """range_scan_kernel / flat_scan_kernel: lane t of G takes the 4-element chunks t, t + G, ..., C x 4 fmaf in chunk order,
    then the G/2 ... 1 xor butterfly (lane 0's sum)."""
    n, d = x.shape
    assert d == 4 * G * C
    xs = x.reshape(n, C, G, 4)
    qs = q.reshape(n, C, G, 4)
    acc = np.zeros((n, G), np.float32)
    for c in range(C):
        for e in range(4):
            acc = _fma_step(acc, xs[:, c, :, e], qs[:, c, :, e])
    m = G // 2
    while m >= 1:
        acc = (acc + acc[:, np.arange(G) ^ m]).astype(np.float32)
        m //= 2
    return acc[:, 0]


def _cases(d):
    rs = np.random.RandomState(900 + d)
    unit = lambda a: (a / np.linalg.norm(a.astype(np.float64), axis=-1, keepdims=True)).astype(np.float32)
    g = unit(rs.randn(16, d))
    yield "random rows", unit(rs.randn(16, d)), g
    yield "all-positive rows", unit(rs.rand(16, d) + 0.5), unit(rs.rand(16, d) + 0.5)
    # adversarial: every product has the same sign and every operand sits just below an fp16 rounding midpoint, so the
    # operand errors and the accumulation errors all push the same way
    m = np.float32(1.0) + np.float32(2.0 ** -11) * (1 - 2.0 ** -10)
    sign = np.where(rs.rand(4, d) < 0.5, -1.0, 1.0).astype(np.float32)
    mags = (m * 2.0 ** rs.randint(-3, 1, (4, d))).astype(np.float32)
    yield "sign-aligned fp16 midpoints", unit(sign * mags), unit(sign * mags[::-1])
    yield "parallel", g, g
    wide = rs.randn(16, d) * 10.0 ** rs.randint(-9, 1, (16, d))            # many elements below fp16's normal range
    yield "elements below fp16's normal range", unit(wide), unit(rs.randn(16, d) * 10.0 ** rs.randint(-9, 1, (16, d)))
    yield "raw rows and queries (norms 30 and 7)", (g * np.float32(7.0)).astype(np.float32), \
        (unit(rs.randn(16, d)) * np.float32(30.0)).astype(np.float32)


@pytest.mark.parametrize("d", DIMS)
def test_library_band_is_the_documented_formula(d):
    from minivectordb_amd import _native
    assert _native.range_band(d, 1.0, 1.0) == pytest.approx(range_eps(d), rel=1e-12)
    assert _native.range_band(d, 3.0, 0.5) == pytest.approx(1.5 * range_eps(d), rel=1e-12)     # linear in |q| and in max|x|
    assert _native.range_band(d, 0.0, 1.0) == 0.0
    # operand rounding + one chain's accumulation + the scan's tree, nothing fitted away
    G, C = SHAPES[d]
    assert _native.range_band(d, 1.0, 1.0) > 2.0 ** -10 + chain(d) * 2.0 ** -23 + (4 * C + int(np.log2(G))) * 2.0 ** -24


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("mode", ["rne", "trunc"])
@pytest.mark.parametrize("flush", [False, True])
def test_band_covers_emulated_nomination_against_every_fp32_order(d, mode, flush):
    from minivectordb_amd import _native
    G, C = SHAPES[d]
    worst = 0.0
    for name, q, x in _cases(d):
        xnorm = np.linalg.norm(x.astype(np.float64), axis=-1)
        bound = np.float32(xnorm.max() * (1 + 4e-6))                       # the index's row-norm bound
        sx = _pow2_scale(bound)
        sq = np.array([_pow2_scale(np.abs(r).max()) for r in q])
        qh = np.stack([_fp16_image(q[i], sq[i], flush) for i in range(q.shape[0])])
        xh = _fp16_image(x, sx, flush)
        approx = nominate(qh * xh, d, mode).astype(np.float64) / (sq * sx)
        qnorm = np.sqrt((q.astype(np.float32) ** 2).sum(axis=-1, dtype=np.float32))      # |q| as the device has it: fp32
        band = np.array([_native.range_band(d, float(qn), float(bound)) for qn in qnorm])
        for order, s in (("sequential", dot_sequential(q, x)), ("pairwise", dot_pairwise(q, x)),
                         ("scan order", dot_scan_order(q, x, G, C))):
            diff = np.abs(approx - s.astype(np.float64))
            print(f"[band] d={d} {mode} flush={flush} {name} / {order}: worst {float((diff / band).max()):.4f} of the band")
            assert np.all(diff <= band), (name, order, float((diff / band).max()))
            worst = max(worst, float((diff / band).max()))
    assert 0 < worst <= 1


@pytest.mark.parametrize("d", [128, 384, 512, 1024])
def test_allowance_for_the_two_normalised_query_images(d):
    """With normalize_q the nomination reads queries normalised by normalize_rows_kernel while the exact kernels normalise in
    their prologue.  Both sum the squares lane by lane and then over a butterfly (depth 4 C + log2 G <= 4 ceil(d / 128) + 6) and
    multiply by 1 / sqrt: each image is within ((depth + 1) / 2 + 3) 2^-24 of the real-number one, element by element.  The
    band's coefficient allows (d + 8) 2^-24 for their difference (mvdb.hip: range_shared_phase) — checked here against images
    whose sums of squares are taken in the scan's order, sequentially and pairwise (a worse order than either kernel's)."""
    G, C = {128: (32, 1), 384: (32, 3), 512: (64, 2), 1024: (64, 4)}[d]
    assert (4 * C + int(np.log2(G)) + 7) < d + 8
    rs = np.random.RandomState(40 + d)
    q = np.concatenate([rs.randn(8, d), rs.rand(8, d) + 0.5, rs.randn(8, d) * 10.0 ** rs.randint(-6, 3, (8, d))]).astype(np.float32)

    def image(nr):
        inorm = (np.float32(1.0) / np.sqrt(nr.astype(np.float32))).astype(np.float32)
        return (q * inorm[:, None]).astype(np.float32)

    images = [image(dot_scan_order(q, q, G, C)), image(dot_sequential(q, q)), image(dot_pairwise(q, q))]
    exact = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    allowance = (d + 8) * 2.0 ** -24
    for a in images:
        for b in images:
            rel = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.abs(exact)
            assert rel.max() <= allowance, (d, float(rel.max()), allowance)


def test_band_stays_useful_at_d_1024():
    """band < 1e-3 |q| max|x| at d = 1024.  Rounding both operands to fp16 alone costs (1 + 2^-11)^2 - 1 = 9.768e-4, so the
    accumulation may cost next to nothing: the wide shapes of the kernel add at most 128 products into one accumulator
    (136 2^-23 = 1.6e-5 worst case instead of 1028 2^-23 = 1.2e-4) and the exact side is bounded by the scan's tree (38 2^-24)
    instead of any order of 1,024 additions."""
    from minivectordb_amd import _native
    for d in DIMS:
        print(f"[band] d={d}: {_native.range_band(d, 1.0, 1.0):.6e} per unit |q| max|x|")
    assert _native.range_band(1024, 1.0, 1.0) < 1e-3


# ---- the Python layer over a scripted index ------------------------------------------------------------------------------
class EachOracleIndex(RangeOracleIndex):
    """RangeOracleIndex whose range calls take one threshold or one per query, and note which form reached them."""
    forms = []

    def _range(self, q, threshold, rowset, normalize_q):
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        type(self).forms.append(type(threshold))
        if np.ndim(threshold) == 0:
            return RangeOracleIndex._range(self, q, threshold, rowset, normalize_q)
        assert isinstance(threshold, np.ndarray) and threshold.dtype == np.float32 and threshold.shape == (q.shape[0],)
        return [RangeOracleIndex._range(self, q[i:i + 1], threshold[i], rowset, normalize_q)[0] for i in range(q.shape[0])]


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    EachOracleIndex.forms = []
    monkeypatch.setattr(_native, "FlatIndex", EachOracleIndex)


FILTERS = [{}, {"metadata_filter": {"bucket": 3}}, {"exclude_filter": {"bucket": 1}}, {"metadata_filter": {"rare": "yes"}}]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_scalar_and_sequence_thresholds(backend, tmp_path, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(7, 16, 77)
    scores = [0.3, -1.0, 0.05, 0.9, 0.2, 0.0, 0.45]
    for f in FILTERS:
        EachOracleIndex.forms = []
        one = db.find_all_similar_batch(q, 0.2, **f)
        assert all(t is float for t in EachOracleIndex.forms)              # a scalar reaches the index as a Python float
        EachOracleIndex.forms = []
        for form in (scores, tuple(scores), np.asarray(scores, np.float64)):
            many = db.find_all_similar_batch(q, form, **f)
            assert len(many) == len(q)
            for i in range(len(q)):
                same(many[i], db.find_all_similar(q[i], scores[i], **f), (f, i))
        assert np.ndarray in EachOracleIndex.forms or not EachOracleIndex.forms     # (no rows selected: the index is not asked)
        same(one[4], many[4], f)                                           # scores[4] == 0.2
        counts = db.count_similar_batch(q, scores, **f)
        assert counts == [db.count_similar(q[i], scores[i], **f) for i in range(len(q))]
        assert counts == [len(m[0]) for m in many] and all(type(c) is int for c in counts)
        assert db.count_similar_batch(q, 0.2, **f) == [len(m[0]) for m in one]
    assert db.count_similar_batch(np.empty((0, 16), np.float32), 0.2) == []
    assert db.find_all_similar_batch(np.empty((0, 16), np.float32), []) == []


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_bad_threshold_sequences(backend, tmp_path, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(4, 16, 78)
    for call in (db.find_all_similar_batch, db.count_similar_batch):
        with pytest.raises(ValueError):
            call(q, [0.1, 0.2, 0.3])                                        # one short
        with pytest.raises(ValueError):
            call(q, [0.1, 0.2, 0.3, 0.4, 0.5])
        with pytest.raises(ValueError):
            call(q, [0.1, float("nan"), 0.3, 0.4])
        with pytest.raises(ValueError):
            call(q, float("nan"))
        with pytest.raises(ValueError):
            call(q, np.zeros((4, 1), np.float32))


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_bad_threshold_sequences_on_an_empty_database_and_an_empty_batch(backend, tmp_path, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    empty = VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat" else \
        ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64)
    full = make_db(kind, tmp_path)
    q = flat.synth(4, 16, 79)
    none = np.empty((0, 16), np.float32)
    for db, qs in ((empty, q), (full, none)):
        nq = qs.shape[0]
        assert db.find_all_similar_batch(qs, [0.1] * nq) == [([], [], [])] * nq
        assert db.count_similar_batch(qs, [0.1] * nq) == [0] * nq
        for call in (db.find_all_similar_batch, db.count_similar_batch):
            with pytest.raises(ValueError):
                call(qs, [0.1] * (nq + 1))
            with pytest.raises(ValueError):
                call(qs, float("nan"))
            if nq:
                with pytest.raises(ValueError):
                    call(qs, [0.1, float("nan"), 0.3, 0.4])


def test_native_threshold_forms():
    """_native.FlatIndex._range_thresholds: None for a scalar, float32[nq] for a sequence, ValueError otherwise (no device)."""
    from minivectordb_amd import _native
    f = _native.FlatIndex._range_thresholds
    assert f(0.5, 3) is None and f(np.float32(0.5), 3) is None
    t = f([0.1, 0.2, -np.inf], 3)
    assert t.dtype == np.float32 and t.tolist() == [np.float32(0.1), np.float32(0.2), -np.inf]
    for bad in ([0.1, 0.2], [0.1, 0.2, float("nan")], np.zeros((3, 1))):
        with pytest.raises(ValueError):
            f(bad, 3)
