"""update_embedding / update_embeddings_batch on the CPU oracle stand-in: the host half (id index, metadata list, inverted
index, value index, row-set caches, shard files, atomicity).  After any mix of stores, updates and deletes the database must
answer as one rebuilt from scratch with the final contents: the same oracle arithmetic runs on both sides."""
import hashlib
import os

import numpy as np
import pytest

from oracle import flat
from oracle_backend import OracleIndex

N, D = 300, 16


class UpdatableOracleIndex(OracleIndex):
    """OracleIndex + set_rows as the C-ABI states it: distinct rows inside [0, ntotal), overwritten in place (normalised as
    add normalises), nothing renumbered.  (+ search_grouped as a loop, so find_most_similar_each takes its grouped route.)"""

    def set_rows(self, rows, x, normalize=False):
        rows = np.asarray(rows, dtype=np.int64)
        x = np.ascontiguousarray(x, dtype=np.float32).copy()
        if x.ndim != 2 or x.shape != (rows.shape[0], self.d):
            raise ValueError("bad shape")
        if rows.size and (rows.min() < 0 or rows.max() >= self.x.shape[0] or len(set(rows.tolist())) != len(rows)):
            raise ValueError("row out of range or listed twice")
        if normalize:
            flat.normalize_l2(x)
        self.x[rows] = x
        self.calls.append(("set_rows", len(rows)))

    def search_grouped(self, q, k, rowsets, normalize_q=False):
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        Ds = np.empty((q.shape[0], k), np.float32)
        Is = np.empty((q.shape[0], k), np.int64)
        for i, rs in enumerate(rowsets):
            if rs is None:
                Ds[i:i + 1], Is[i:i + 1] = OracleIndex.search(self, q[i:i + 1], k, normalize_q=normalize_q)
            elif len(rs) == 0:
                Ds[i], Is[i] = -3.4028234663852886e38, -1
            else:
                Ds[i:i + 1], Is[i:i + 1] = OracleIndex.search_rowset(self, q[i:i + 1], k, rs, normalize_q=normalize_q)
        return Ds, Is


@pytest.fixture(autouse=True)
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", UpdatableOracleIndex)


def new_db(kind, where):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    os.makedirs(where, exist_ok=True)
    if kind == "flat":
        return VectorDatabase(storage_file=str(where / "db.pkl"))
    return ShardedVectorDatabase(storage_dir=str(where / "shards"), shard_size=64)


def meta_of(i, salt=0):
    m = {"bucket": (i + salt) % 7, "rank": i}
    if (i + salt) % 50 == 0:
        m["rare"] = "yes"
    if (i + salt) % 60 == 0:
        m["tags"] = ["a", i % 3]     # an unhashable value
    return m


def make_db(kind, where, n=N):
    db = new_db(kind, where)
    db.store_embeddings_batch(list(range(n)), flat.synth(n, D, 5), [meta_of(i) for i in range(n)])
    return db


FILTERS = [
    {},
    {"metadata_filter": {"bucket": 0}},
    {"metadata_filter": {"bucket": 3}},
    {"exclude_filter": {"bucket": 3}},
    {"or_filters": [{"bucket": 4}, {"rare": "yes"}]},
    {"metadata_filter": {"rank": {"$gte": 250}}},
    {"metadata_filter": {"rare": "yes"}},
    {"metadata_filter": {"tags": ["a", 0]}},
    {"metadata_filter": {"gone": 1}},
    {"metadata_filter": {"fresh": "x"}},
]


def answers(db, queries, k=8):
    out = []
    for f in FILTERS:
        for q in queries:
            ids, scores, metas = db.find_most_similar(q, k=k, **f)
            out.append((list(ids), [float(v) for v in scores], list(metas)))
    return out


def assert_same_state(db, twin, queries):
    assert list(db._ids.uids) == list(twin._ids.uids)
    assert db.metadata == twin.metadata
    assert {k: set(v) for k, v in db.inverted_index.items()} == {k: set(v) for k, v in twin.inverted_index.items()}
    assert answers(db, queries) == answers(twin, queries)


def assert_same_contents(db, twin, queries):
    """For an instance reopened from storage: shard files stack in shard order and a pickled matrix holds rows that were
    already normalised once, so row order and the last bit of a score may differ — ids, metadata and ranking may not."""
    assert dict(zip(db._ids.uids, db.metadata)) == dict(zip(twin._ids.uids, twin.metadata))
    assert {k: set(v) for k, v in db.inverted_index.items()} == {k: set(v) for k, v in twin.inverted_index.items()}
    for got, want in zip(answers(db, queries), answers(twin, queries)):
        assert got[0] == want[0] and got[2] == want[2]
        assert np.allclose(got[1], want[1], rtol=0, atol=1e-6)


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_mixed_sequences_equal_a_rebuild(tmp_path, kind):
    """store / filter (builds the value index) / update / delete / update again, against a database built from the final
    contents — ids, metadata, inverted index, value index (through the filters) and the rows (through the scores)."""
    q = flat.synth(3, D, 6)
    db = make_db(kind, tmp_path / "a")
    x = flat.synth(N, D, 5).copy()
    meta = {i: meta_of(i) for i in range(N)}
    answers(db, q)                                   # flushes the rows, builds the value index for every filtered key
    y = flat.synth(N, D, 77)
    # embedding + metadata, embedding only, metadata only; singles and a batch
    db.update_embedding(5, y[5], {"bucket": 3, "rank": 5, "fresh": "x"})
    x[5], meta[5] = y[5], {"bucket": 3, "rank": 5, "fresh": "x"}
    db.update_embedding(0, embedding=q[0])           # row 0 becomes a copy of query 0
    x[0] = q[0]
    db.update_embedding(50, metadata_dict={"rank": 50})   # loses "rare", "bucket"
    meta[50] = {"rank": 50}
    db.update_embedding(60, metadata_dict={"bucket": 3, "rank": 60, "tags": ["a", 0]})
    meta[60] = {"bucket": 3, "rank": 60, "tags": ["a", 0]}
    ids = list(range(100, 160))
    db.update_embeddings_batch(ids, y[100:160], [meta_of(i, salt=1) for i in ids])
    for i in ids:
        x[i], meta[i] = y[i], meta_of(i, salt=1)
    assert db.find_most_similar(q[0], k=1)[0][0] == 0
    for uid in (7, 100, 299):
        if kind == "flat":
            db.delete_embedding(uid)
        else:
            db.delete_embeddings_batch([uid])
        del meta[uid]
    # rows stored after the flush are still pending on the host: update one of them and one synced row in a single batch
    db.store_embeddings_batch([1000, 1001], flat.synth(2, D, 8), [{"bucket": 0, "rank": 1000}, {"bucket": 1, "rank": 1001}])
    x = np.vstack([x, flat.synth(2, D, 8)])
    meta[1000], meta[1001] = {"bucket": 0, "rank": 1000}, {"bucket": 1, "rank": 1001}
    db.update_embeddings_batch([1001, 3], [y[1], y[3]], [{"bucket": 3, "rank": 1001, "rare": "yes"}, {"rank": 3}])
    x[N + 1], x[3] = y[1], y[3]
    meta[1001], meta[3] = {"bucket": 3, "rank": 1001, "rare": "yes"}, {"rank": 3}
    every_rare_gone = [i for i in meta if "rare" in meta[i] and i != 1001]
    db.update_embeddings_batch(every_rare_gone, metadata_dicts=[{"rank": i} for i in every_rare_gone])
    for i in every_rare_gone:
        meta[i] = {"rank": i}
    assert db.inverted_index["rare"] == {1001}

    alive = [i for i in list(range(N)) + [1000, 1001] if i in meta]
    rows = [i if i < N else N + (i - 1000) for i in alive]
    twin = new_db(kind, tmp_path / "b")
    twin.store_embeddings_batch(alive, x[rows], [meta[i] for i in alive])
    assert_same_state(db, twin, q)
    # a key nobody holds any more disappears, as after a delete
    db.update_embedding(1001, metadata_dict={"rank": 1001})
    assert "rare" not in db.inverted_index
    # what a fresh instance reads back from the storage
    if kind == "flat":
        db.persist_to_disk()
    twin.update_embedding(1001, metadata_dict={"rank": 1001})
    again = new_db(kind, tmp_path / "a")
    assert_same_contents(again, twin, q)


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_pending_and_flushed_rows_behave_alike(tmp_path, kind):
    q = flat.synth(1, D, 6)[0]
    early, late = make_db(kind, tmp_path / "a"), make_db(kind, tmp_path / "b")
    early.update_embedding(17, embedding=q)          # before the first query: the row still waits on the host
    assert not any(c[0] == "set_rows" for c in (early.index.calls if early.index is not None else []))
    late.find_most_similar(q, k=1)                   # uploads
    late.update_embedding(17, embedding=q)
    assert late.index.calls.count(("set_rows", 1)) == 1
    a, b = early.find_most_similar(q, k=5), late.find_most_similar(q, k=5)
    assert a[0][0] == b[0][0] == 17 and list(a[0]) == list(b[0]) and list(a[1]) == list(b[1])
    if kind == "flat":
        want = q.copy()[None, :]
        flat.normalize_l2(want)
        assert np.array_equal(early.get_vector(17), want[0]) and np.array_equal(late.get_vector(17), want[0])
    else:
        assert np.array_equal(early.get_vector(17), q) and np.array_equal(late.get_vector(17), q)   # shards keep raw rows


def test_row_store_keeps_no_mirror_of_synced_rows(tmp_path):
    db = make_db("flat", tmp_path)
    q = flat.synth(1, D, 6)[0]
    db.find_most_similar(q, k=1)
    store = db._mat
    assert store.synced == N and store.pending == [] and store._cache is None
    _ = db.embeddings                                 # materialises the cache
    assert store._cache is not None
    db.update_embeddings_batch([1, 2, 3], flat.synth(3, D, 9))
    assert store._cache is None and store.pending == [] and store.npending == 0 and store.synced == N
    assert db.index.calls.count(("set_rows", 3)) == 1   # ONE call for the batch
    host_arrays = [v for v in vars(store).values() if isinstance(v, np.ndarray)]
    assert host_arrays == []


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_cache_invalidation_rules(tmp_path, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(25, D, 6)
    f = {"metadata_filter": {"bucket": 2}}
    db.find_most_similar(q[0], k=3, **f)
    tenants = [{"metadata_filter": {"bucket": t % 7}} for t in range(20)]
    db.find_most_similar_each(q[:20], tenants, k=3)
    made = sum(c[0] == "rowset" for c in db.index.calls)
    gen = db._write_gen
    held, held_each = dict(db._rowsets), dict(db._rowsets_each)
    assert held and held_each
    # embedding only: no row number and no filter result moved — the caches stay, no new row set is built
    member = db.find_most_similar(q[0], k=1, **f)[0][0]
    db.update_embedding(member, embedding=-q[0])
    assert db._write_gen == gen and db._rowsets == held and dict(db._rowsets_each) == held_each
    after = db.find_most_similar(q[0], k=3, **f)
    assert member not in after[0]
    each = db.find_most_similar_each(q[:20], tenants, k=3)
    assert sum(c[0] == "rowset" for c in db.index.calls) == made
    for i, t in enumerate(tenants):
        one = db.find_most_similar(q[i], k=3, **t)
        assert list(each[i][0]) == list(one[0]) and list(each[i][1]) == list(one[1])
    # metadata: filter results moved — the caches go, as after a store
    db.update_embedding(member, metadata_dict={"bucket": 5, "rank": member})
    assert db._write_gen == gen + 1 and db._rowsets == {} and len(db._rowsets_each) == 0
    assert member not in db.find_most_similar(-q[0], k=N, **f)[0]
    assert member in db.find_most_similar(-q[0], k=N, metadata_filter={"bucket": 5})[0]
    assert sum(c[0] == "rowset" for c in db.index.calls) > made


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_a_failing_call_changes_nothing(tmp_path, kind):
    db = make_db(kind, tmp_path / "a")
    twin = make_db(kind, tmp_path / "b")
    q = flat.synth(3, D, 6)
    answers(db, q)
    y = flat.synth(4, D, 9)
    calls = len(db.index.calls)
    files = shard_digests(tmp_path / "a" / "shards") if kind == "sharded" else None
    bad = [
        dict(unique_ids=[1, 2]),                                              # nothing to update
        dict(unique_ids=[1, 9999], embeddings=y[:2]),                         # unknown id
        dict(unique_ids=[1, 2, 1], embeddings=y[:3]),                         # repeated id
        dict(unique_ids=[1, 2], embeddings=[y[0], np.zeros(D + 1, np.float32)]),   # wrong width
        dict(unique_ids=[1, 2], embeddings=np.zeros((2, D - 1), np.float32)),
        dict(unique_ids=[1, 2], embeddings=y[:3]),                            # length mismatch
        dict(unique_ids=[1, 2], embeddings=y[:2], metadata_dicts=[{"bucket": 1}]),
        dict(unique_ids=[1, 2], metadata_dicts=[{"bucket": 1}, "not a dict"]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            db.update_embeddings_batch(**kw)
    with pytest.raises(ValueError):
        db.update_embedding(1)
    with pytest.raises(ValueError):
        db.update_embedding("nobody", embedding=y[0])
    assert [c for c in db.index.calls[calls:] if c[0] == "set_rows"] == []
    assert_same_state(db, twin, q)
    if kind == "sharded":
        assert shard_digests(tmp_path / "a" / "shards") == files
    # storing an existing id still raises, as before
    with pytest.raises(ValueError):
        db.store_embedding(1, y[0])
    db.update_embeddings_batch([], embeddings=[])      # an empty batch is a no-op
    assert_same_state(db, twin, q)


def shard_digests(folder):
    return {name: hashlib.sha256(open(os.path.join(folder, name), "rb").read()).hexdigest() for name in sorted(os.listdir(folder))}


def test_only_the_owning_shard_files_change(tmp_path):
    import pickle
    db = make_db("sharded", tmp_path)
    folder = tmp_path / "shards"
    before = shard_digests(folder)
    assert len(before) == 5                                     # 300 ids, 64 per shard
    y = flat.synth(3, D, 9)
    ids = [3, 70, 71]                                           # shards 0 and 1
    db.update_embeddings_batch(ids, y, [{"bucket": 6, "rank": -1, "fresh": "x"}] * 3)
    after = shard_digests(folder)
    changed = sorted(name for name in before if before[name] != after[name])
    assert changed == ["shard_0.pkl", "shard_1.pkl"]
    shard = pickle.load(open(folder / "shard_1.pkl", "rb"))
    at = shard["unique_ids"].index(70)
    assert np.array_equal(shard["embeddings"][at], y[1])        # the raw row, in place
    assert shard["metadata"][at] == {"bucket": 6, "rank": -1, "fresh": "x"}
    assert shard["inverted_index"]["fresh"] == {70, 71} and type(shard["inverted_index"]) is dict
    assert 70 not in shard["inverted_index"].get("rare", set())
    assert shard["unique_ids"] == list(range(64, 128)) and shard["embeddings"].shape == (64, D)
    # the file is what a delete + store of the same contents would hold, apart from the order inside the shard
    assert {u for holders in shard["inverted_index"].values() for u in holders} <= set(shard["unique_ids"])
    for key, holders in shard["inverted_index"].items():
        assert holders == {u for u, m in zip(shard["unique_ids"], shard["metadata"]) if key in m}, key
    # embedding only: metadata bytes of the shard stay, only that file moves
    mid = shard_digests(folder)
    db.update_embedding(200, embedding=y[0])
    assert sorted(n for n in mid if mid[n] != shard_digests(folder)[n]) == ["shard_3.pkl"]


def test_batch_equals_single_updates(tmp_path):
    a, b = make_db("flat", tmp_path / "a"), make_db("flat", tmp_path / "b")
    q = flat.synth(3, D, 6)
    answers(a, q), answers(b, q)
    ids = list(range(0, N, 3))
    y = flat.synth(len(ids), D, 11)
    metas = [meta_of(i, salt=2) for i in ids]
    a.update_embeddings_batch(ids, y, metas)
    for i, v, m in zip(ids, y, metas):
        b.update_embedding(i, v, m)
    assert_same_state(a, b, q)
    assert np.array_equal(a.embeddings, b.embeddings)
