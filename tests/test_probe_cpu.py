"""tests/probe_oracle.py against an inline float64 brute force on small inputs.  No device: these pass with or without the
probed search itself, like the k-means oracle's tests."""
import numpy as np

from probe_oracle import MISSING, image, probe_search, probes, ranking


def brute(coarse, fine, labels, k, nprobe, selected=None):
    """The contract with sorted() over Python tuples; scores compared as float64 (exact images of the float32 values)."""
    C, n = len(coarse), len(fine)
    order = sorted((j for j in range(C) if coarse[j] == coarse[j]), key=lambda j: (-float(coarse[j]), j))
    P = order[:nprobe]
    rows = [r for r in range(n) if labels[r] in P and labels[r] >= 0 and (selected is None or r in selected)]
    best = sorted((r for r in rows if fine[r] == fine[r]), key=lambda r: (-float(fine[r]), r))[:k]
    D = [float(fine[r]) for r in best] + [float(MISSING)] * (k - len(best))
    I = best + [-1] * (k - len(best))
    return D, I, P


def world(seed, n=300, C=9, d=12):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    c = rng.standard_normal((C, d))
    q = rng.standard_normal(d)
    labels = np.argmax(x @ c.T, axis=1).astype(np.int32)
    return (c @ q).astype(np.float32), (x @ q).astype(np.float32), labels


def check(coarse, fine, labels, k, nprobe, selected=None):
    D, I, P = probe_search(coarse, fine, labels, k, nprobe, selected)
    bD, bI, bP = brute(coarse, fine, labels, k, nprobe, None if selected is None else set(int(r) for r in selected))
    assert P.tolist() == bP and I.tolist() == bI and D.astype(np.float64).tolist() == bD
    return D, I, P


def test_random_worlds_every_k_and_nprobe():
    for seed in range(5):
        coarse, fine, labels = world(seed)
        for nprobe in (1, 3, 9):
            for k in (1, 10, 64):
                check(coarse, fine, labels, k, nprobe)
        sel = np.random.default_rng(seed).permutation(300)[:200]
        check(coarse, fine, labels, 10, 3, np.sort(sel))
        check(coarse, fine, labels, 10, 3, np.empty(0, np.int64))


def test_nprobe_equal_to_the_lists_is_the_exact_ranking_of_the_labelled_rows():
    coarse, fine, labels = world(11)
    labels[::7] = -1
    D, I, P = check(coarse, fine, labels, 64, 9)
    assert sorted(P.tolist()) == list(range(9))
    want = ranking(fine, np.flatnonzero(labels >= 0))[:64]
    assert I.tolist() == want.tolist() and not (labels[I] == -1).any()


def test_ties_go_to_the_lower_centre_and_the_lower_row():
    coarse, fine, labels = world(3)
    coarse[7] = coarse[2] = coarse.max() + 1          # twin centres at the top: nprobe = 1 probes centre 2
    assert probes(coarse, 1).tolist() == [2] and probes(coarse, 2).tolist() == [2, 7]
    labels[:] = 0
    labels[10], labels[200] = 2, 7                    # twin rows in different lists
    fine[10] = fine[200] = fine.max() + 1
    D, I, _ = check(coarse, fine, labels, 2, 2)
    assert I.tolist() == [10, 200] and D[0] == D[1]
    D, I, _ = check(coarse, fine, labels, 2, 1)
    assert I.tolist() == [10, -1] and D[1] == MISSING                 # list 7 is not probed: fewer than k rows, padding


def test_nan_is_never_a_candidate_and_an_empty_list_takes_its_slot():
    coarse, fine, labels = world(4)
    coarse[0] = np.nan
    fine[5] = np.nan
    labels[labels == 3] = 4                           # list 3 is empty
    coarse[3] = coarse[~np.isnan(coarse)].max() + 1   # ... and ranks first
    D, I, P = check(coarse, fine, labels, 10, 1)
    assert P.tolist() == [3] and (I == -1).all() and (D == MISSING).all()
    D, I, P = check(coarse, fine, labels, 64, 9)
    assert 0 not in P.tolist() and len(P) == 8 and 5 not in I.tolist()
    allnan = np.full_like(coarse, np.nan)
    D, I, P = check(allnan, fine, labels, 5, 9)
    assert len(P) == 0 and (I == -1).all()


def test_the_order_of_the_keys():
    s = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, np.nan, -1.0], np.float32)
    assert ranking(s).tolist() == [2, 4, 0, 1, 6, 3]                 # -0.0 below +0.0, NaN left out
    img = image(s[[3, 6, 1, 0, 4, 2]]).astype(np.int64)
    assert (np.diff(img) > 0).all() and img[0] == 0x007FFFFF
