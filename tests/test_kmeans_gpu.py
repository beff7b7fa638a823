"""Spherical k-means on the device (mvdb_index_kmeans, csrc/assign_scan.hpp): every comparison is exact.  The oracle is the
loop of tests/kmeans_oracle.py fed the library's own single-query bits: in every iteration, for each centre j, the full ranking
idx.search / search_rowset of c[j] alone over the selected rows, scattered into a [C, n] matrix.  Centres and scores are
compared as bits, labels, counts and iterations as integers.

Corpus (2,214 rows, two slices of the list build, stored in shuffled order): five planted directions with 256, 257, 700, 1,000
and 1 member rows — a cluster of exactly one chunk, of one chunk and one row, of three chunks, of four, and of one row — and a
sixth centre opposite to the first direction, which no row is nearest to: it stays empty and must come back unchanged.

The initial centres are normalised by the scan's prologue.  The test gets those bits from the library itself: k-means under an
EMPTY row set labels nothing, updates nothing and returns the initial centres as the loop first holds them."""
import numpy as np
import pytest

from kmeans_oracle import assign, kmeans
from maxsim_oracle import MISSING

pytestmark = pytest.mark.gpu

SIZES = [256, 257, 700, 1000, 1]
N = sum(SIZES)
C = len(SIZES) + 1
DIMS = [100, 512]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_WORLDS = {}


class World:
    def __init__(self, d):
        from minivectordb_amd import _native
        rng = np.random.default_rng(500 + d)
        true = rng.standard_normal((len(SIZES), d))
        true /= np.linalg.norm(true, axis=1, keepdims=True)
        owner = np.repeat(np.arange(len(SIZES)), SIZES)
        rng.shuffle(owner)
        x = (true[owner] + 0.3 / np.sqrt(d) * rng.standard_normal((N, d))).astype(np.float32)
        self.d, self.owner = d, owner
        self.idx = _native.FlatIndex(d)
        self.idx.add(x, normalize=True)
        self.stored = self.idx.get_rows(0, N)
        self.stored.setflags(write=False)
        far = -3.0 * true[:1]
        # "planted": a centre near every direction — the first labels are the planted partition
        near = 2.0 * (true + 0.1 / np.sqrt(d) * rng.standard_normal(true.shape))
        self.inits = {"planted": np.concatenate([near, far]).astype(np.float32)}
        # "rough": stored rows; two from the cluster of 1,000, none from the cluster of 700 — memberships move for a few iterations
        pick = [np.flatnonzero(owner == 0)[0], np.flatnonzero(owner == 1)[0], np.flatnonzero(owner == 3)[0],
                np.flatnonzero(owner == 3)[1], np.flatnonzero(owner == 4)[0]]
        self.inits["rough"] = np.concatenate([self.stored[pick], far.astype(np.float32)]).astype(np.float32)
        self.empty = self.idx.rowset(np.empty(0, np.int64))
        self.sets = {None: (None, np.arange(N, dtype=np.int64))}
        rows = np.random.default_rng(9).permutation(N)[:1500].astype(np.int64)
        self.sets["unsorted"] = (self.idx.rowset(rows), rows)
        gone = np.flatnonzero(owner == 2)[:200].astype(np.int64)
        self.sets["excluded"] = (self.idx.rowset(gone, excluded=True), np.setdiff1d(np.arange(N, dtype=np.int64), gone))
        self._oracle = {}

    def normalised(self, init):
        """The initial centres as the loop first holds them, from the library: a run under the empty set."""
        centres, labels, scores, counts, its = self.idx.kmeans(init, 3, rowset=self.empty)
        assert (labels == -1).all() and (scores == MISSING).all() and (counts == 0).all() and its == 1
        return centres

    def scores_of(self, kind):
        rs, selected = self.sets[kind]
        m = len(selected)

        def scores(centres):
            s = np.full((centres.shape[0], N), np.nan, np.float32)
            for j in range(centres.shape[0]):
                if rs is None:
                    D, I = self.idx.search(centres[j:j + 1], m, normalize_q=False)
                else:
                    D, I = self.idx.search_rowset(centres[j:j + 1], m, rs, normalize_q=False)
                s[j, I[0][I[0] >= 0]] = D[0][I[0] >= 0]
            return s
        return scores

    def oracle(self, name, kind, max_iter):
        key = (name, kind, max_iter)
        if key not in self._oracle:
            self._oracle[key] = kmeans(self.scores_of(kind), self.stored, self.normalised(self.inits[name]), max_iter)
        return self._oracle[key]


def world(d):
    if d not in _WORLDS:
        _WORLDS[d] = World(d)
    return _WORLDS[d]


def same(got, want, what):
    for g, w, name in zip(got, want, ("centres", "labels", "scores", "counts", "iterations")):
        if name == "iterations":
            assert g == w, (what, name, g, w)
        elif w.dtype == np.float32:
            assert g.dtype == np.float32 and g.shape == w.shape, (what, name)
            assert np.array_equal(bits(g), bits(w)), (what, name, np.argwhere(bits(g) != bits(w))[:10])
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g, w)


@pytest.mark.parametrize("d", DIMS)
def test_planted_memberships_chunk_edges_and_the_empty_cluster(gpu, d):
    w = world(d)
    init = w.inits["planted"]
    got = w.idx.kmeans(init, 25)
    want = w.oracle("planted", None, 25)
    print(f"d={d} planted: iterations {got[4]} counts {got[3].tolist()}")
    same(got, want, ("planted", d))
    centres, labels, scores, counts, its = got
    assert np.array_equal(labels, w.owner) and counts.tolist() == SIZES + [0]          # forced: the planted partition
    assert its == 1                                                                      # one update, then nothing changed
    start = w.normalised(init)
    assert np.array_equal(bits(centres[C - 1]), bits(start[C - 1]))                      # the empty cluster kept its centre
    assert not np.array_equal(bits(centres[:C - 1]), bits(start[:C - 1]))
    lone = np.flatnonzero(w.owner == 4)[0]                                               # the cluster of one: its row, normalised again
    assert np.abs(centres[4] - w.stored[lone]).max() < 1e-6
    # the returned labels / scores are the assignment of the returned centres; the initial centres were normalised by the prologue
    again = w.idx.assign(centres, normalize_c=False)
    assert np.array_equal(again[0], labels) and np.array_equal(bits(again[1]), bits(scores))
    a = w.idx.assign(init, normalize_c=True)
    b = w.idx.assign(start, normalize_c=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    # twice: the same bits
    same(w.idx.kmeans(init, 25), got, ("planted again", d))


@pytest.mark.parametrize("d", DIMS)
def test_memberships_that_move_max_iter_and_early_stop(gpu, d):
    w = world(d)
    init = w.inits["rough"]
    full = w.idx.kmeans(init, 25)
    want = w.oracle("rough", None, 25)
    print(f"d={d} rough: iterations {full[4]} counts {full[3].tolist()}")
    same(full, want, ("rough", d))
    assert 2 <= full[4] < 25 and full[3].sum() == N                                      # it converged early, after labels moved
    same(w.idx.kmeans(init, 25), full, ("rough again", d))
    again = w.idx.assign(full[0], normalize_c=False)
    assert np.array_equal(again[0], full[1]) and np.array_equal(bits(again[1]), bits(full[2]))
    # max_iter = 1 and 2: the loop runs out — that many updates, then the labels of the centres as they are
    for max_iter in (1, 2):
        got = w.idx.kmeans(init, max_iter)
        same(got, w.oracle("rough", None, max_iter), ("rough", d, max_iter))
        assert got[4] == max_iter
        again = w.idx.assign(got[0], normalize_c=False)
        assert np.array_equal(again[0], got[1]) and np.array_equal(bits(again[1]), bits(got[2]))
    # max_iter = the iterations it took: the same result, whether the loop stops or runs out
    assert w.idx.kmeans(init, full[4])[4] == full[4]


@pytest.mark.parametrize("kind", ["unsorted", "excluded"])
@pytest.mark.parametrize("d", DIMS)
def test_unselected_rows_never_move_a_centre(gpu, d, kind):
    w = world(d)
    rs, selected = w.sets[kind]
    assert rs.is_bitmap == (kind == "excluded")
    for name in ("planted", "rough"):
        got = w.idx.kmeans(w.inits[name], 25, rowset=rs)
        same(got, w.oracle(name, kind, 25), (name, d, kind))
        unselected = np.setdiff1d(np.arange(N), selected)
        assert (got[1][unselected] == -1).all() and (got[2][unselected] == MISSING).all() and got[3].sum() == len(selected)
        assert not np.array_equal(bits(got[0]), bits(w.idx.kmeans(w.inits[name], 25)[0]))    # other members, other centres


def test_argument_errors(gpu):
    from minivectordb_amd import _native
    w = world(100)
    init = w.inits["planted"]
    with pytest.raises(ValueError, match="max_iter"):
        w.idx.kmeans(init, 0)
    with pytest.raises(ValueError, match="C <= 4096"):
        w.idx.kmeans(np.zeros((4097, 100), np.float32), 3)
    with pytest.raises(ValueError, match="another index"):
        w.idx.kmeans(init, 3, rowset=world(512).sets["unsorted"][0])
    l2 = _native.FlatIndex(100, metric=1)
    l2.add(np.asarray(w.stored[:50]))
    with pytest.raises(ValueError, match="inner-product"):
        l2.kmeans(init, 3)
    l2.close()
    empty = _native.FlatIndex(100)
    centres, labels, scores, counts, its = empty.kmeans(init, 3)
    assert labels.shape == (0,) and (counts == 0).all() and its == 1 and np.array_equal(bits(centres), bits(w.normalised(init)))
    empty.close()


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_cluster_embeddings_under_a_metadata_filter(gpu, tmp_path, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    w = world(100)
    n = 900
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=256)
    ids = [f"id{i}" for i in range(n)]
    db.store_embeddings_batch(ids, np.asarray(w.stored[:n]), [{"keep": i % 3 != 0, "i": i} for i in range(n)])
    got_ids, labels, scores, centroids = db.cluster_embeddings(4, max_iter=10, seed=2, metadata_filter={"keep": True})
    rows = np.array([i for i in range(n) if i % 3 != 0], dtype=np.int64)
    assert list(got_ids) == [ids[i] for i in rows]
    idx = db.index
    picked = np.random.default_rng(2).choice(rows, 4, replace=False)
    init = np.concatenate([idx.get_rows(int(r), 1) for r in picked])
    rs = idx.rowset(rows)
    start = idx.kmeans(init, 1, rowset=idx.rowset(np.empty(0, np.int64)))[0]
    stored = idx.get_rows(0, n)

    def scores_of(centres):
        s = np.full((4, n), np.nan, np.float32)
        for j in range(4):
            D, I = idx.search_rowset(centres[j:j + 1], len(rows), rs, normalize_q=False)
            s[j, I[0][I[0] >= 0]] = D[0][I[0] >= 0]
        return s

    want = kmeans(scores_of, stored, start, 10)
    assert np.array_equal(bits(centroids), bits(want[0])) and centroids.shape == (4, 100)
    assert labels.dtype == np.int32 and np.array_equal(labels, want[1][rows]) and np.array_equal(bits(scores), bits(want[2][rows]))
    # and the labels alone, through assign_to_nearest
    a_ids, a_labels, a_scores = db.assign_to_nearest(centroids, metadata_filter={"keep": True})
    assert list(a_ids) == list(got_ids) and np.array_equal(a_labels, labels)
    whole = db.assign_to_nearest(centroids)
    assert list(whole[0]) == ids and np.array_equal(whole[1][rows], labels)
