"""CPU: the mask classes of a dedupe group (csrc/uvrt_dedupe.h "mask classes", reached through the host-only hook
uvrt_dedupe_classes) against the numpy brute force of tests/test_dedupe_cpu.py.

The hook returns the class list a batch gives a group -- found from a thin sample of the group's keys, so it is held here to
what a list must be (deterministic, multi-bit masks only, no duplicate, no longer than asked for), never to a particular
content -- and the atomics the group's traced rays issue with that list.  That figure is restated from the brute-force masks:
an owner deposits once when its mask has one bit or a class, else once per bit.  The fold is restated in numpy as well: launch
planes plus class planes give the per-launch totals that one deposit per bit gives."""
import numpy as np
import pytest

from test_dedupe_cpu import brute_masks, lamp0, np_seed_input, seed_chain, stepped_chain, tie_chain  # noqa: F401 (lamp0: a fixture)

PLANE_FORM, CLASS_FORM, PLANE_INDEX = 1 << 30, 1 << 29, 0xFFFF


def popcount(a):
    a = np.asarray(a, dtype=np.uint32)
    return sum(((a >> np.uint32(b)) & np.uint32(1)).astype(np.int64) for b in range(32))


def owners_of(lamp, prev, nxt, mode, first_gid, n):
    gids = first_gid + np.arange(n, dtype=np.int64)
    h = np.stack([np_seed_input(gids, lamp, prev[k], nxt[k], mode) for k in range(len(prev))])
    masks, _ = brute_masks(h)
    return masks[masks != 0]


def expected_deposits(owner_masks, classes):
    pc = popcount(owner_masks)
    once = (pc == 1) | np.isin(owner_masks, np.asarray(classes, dtype=np.uint32))
    return int(np.where(once, 1, pc).sum())


def check_list(classes, max_classes):
    assert len(classes) <= max_classes
    assert len(set(int(m) for m in classes)) == len(classes), "a mask has two classes"
    assert all(int(m) & (int(m) - 1) for m in classes), "a single-bit mask needs no class"
    assert all(int(m) < (1 << 30) for m in classes)


GROUPS = [  # (K, first gid, n)
    (8, 0, 4096), (8, 1200000, 4096), (8, 2000000, 4096), (2, 0, 4096), (5, 1000000, 6000), (17, 500000, 3000), (30, 700000, 2000),
]


@pytest.mark.parametrize("K,first_gid,n", GROUPS)
def test_class_list_and_deposit_count(pkg, lamp0, K, first_gid, n):
    """the list is the same on every call and well formed; the deposit figure is the brute-force masks' with that list"""
    capi = pkg.capi
    lamp, length = lamp0
    prev, nxt = seed_chain(capi, lamp, length, K, 0, 0)
    own = owners_of(lamp, prev, nxt, 0, first_gid, n)
    for mc in (1, 4, capi.dedupe_classes_default(), capi.DEDUPE_CLASS_MAX):
        if mc == 0:
            continue
        classes, dep = capi.dedupe_classes(lamp, prev, nxt, 0, first_gid, n, mc)
        again, dep2 = capi.dedupe_classes(lamp, prev, nxt, 0, first_gid, n, mc)
        assert np.array_equal(classes, again) and dep == dep2
        check_list(classes, mc)
        assert dep == expected_deposits(own, classes)
        # a longer list starts with the shorter one: most frequent first
        longer, _ = capi.dedupe_classes(lamp, prev, nxt, 0, first_gid, n, capi.DEDUPE_CLASS_MAX)
        assert np.array_equal(longer[:len(classes)], classes)
    # classes off: one deposit per set bit, which is one per occurrence
    classes, dep = capi.dedupe_classes(lamp, prev, nxt, 0, first_gid, n, 0)
    assert len(classes) == 0 and dep == int(popcount(own).sum()) == K * n


def test_seed_mode_1(pkg, lamp0):
    capi = pkg.capi
    length = lamp0[1]
    lamp = (-2000.0, 1.25, -1500.0)          # the first ~2 500 sums are negative: key 0 many times over, each traced alone
    prev, nxt = seed_chain(capi, lamp, length, 5, 0x1234, 1)
    for first_gid in (0, 2000):
        own = owners_of(lamp, prev, nxt, 1, first_gid, 6000)
        classes, dep = capi.dedupe_classes(lamp, prev, nxt, 1, first_gid, 6000, 4)
        check_list(classes, 4)
        assert dep == expected_deposits(own, classes)


def test_headline_group_deposits_once_per_ray(pkg, lamp0):
    """lamp 0, 8 x 2 073 600 from SEED 0 at the default maximum: 8 418 915 owners (tests/test_dedupe_cpu.py holds that figure)
    issue at most 0.1 % more atomics than there are owners -- 32 classes cover 0.9995 of them.  Classes off: 16 588 800."""
    capi = pkg.capi
    lamp, length = lamp0
    prev, nxt = seed_chain(capi, lamp, length, 8, 0, 0)
    assert nxt[-1] == 0xbf71c277
    if capi.dedupe_classes_default() > 0:
        classes, dep = capi.dedupe_classes(lamp, prev, nxt, 0, 0, 2073600)
        check_list(classes, capi.dedupe_classes_default())
        print("headline: %d classes, %d deposits for 8 418 915 owners (%+.4f %%)" % (len(classes), dep, 100.0 * (dep - 8418915) / 8418915))
        assert 8418915 <= dep <= 8418915 * 1.001
    classes, dep = capi.dedupe_classes(lamp, prev, nxt, 0, 0, 2073600, capi.DEDUPE_CLASS_MAX)
    assert 8418915 <= dep <= 8418915 * 1.001
    _, dep0 = capi.dedupe_classes(lamp, prev, nxt, 0, 0, 2073600, 0)
    assert dep0 == 8 * 2073600


def test_31_launches_keep_the_masks(pkg, lamp0):
    """bit 30 is a launch in a group of 31, so the word has no room for the plane form: no classes, one deposit per bit"""
    capi = pkg.capi
    lamp, length = lamp0
    prev, nxt = seed_chain(capi, lamp, length, 31, 0, 0)
    classes, dep = capi.dedupe_classes(lamp, prev, nxt, 0, 300000, 1500, capi.DEDUPE_CLASS_MAX)
    assert len(classes) == 0 and dep == 31 * 1500
    prev, nxt = prev[:30], nxt[:30]
    classes, dep = capi.dedupe_classes(lamp, prev, nxt, 0, 300000, 1500, capi.DEDUPE_CLASS_MAX)
    assert len(classes) > 0 and dep < 30 * 1500


KEYS_TWICE = [("past_2_28", 16000000, 8192, 0), ("ties_2_27", 9000000, 4000, 16), ("ties_2_27b", 15000000, 4000, 16),
              ("ties_low", 5000000, 4000, 8), ("ties_lower", 1100000, 4000, 2)]


@pytest.mark.parametrize("case,first_gid,n,grid", KEYS_TWICE, ids=[c[0] for c in KEYS_TWICE])
def test_keys_held_twice_stay_single_bit(pkg, lamp0, case, first_gid, n, grid):
    """a key some launch holds twice is traced by every occurrence alone, with its own bit: such rays deposit once in their
    launch's plane and never meet a class"""
    capi = pkg.capi
    if grid == 0:
        lamp, length = lamp0
        K = 8
        prev, nxt = seed_chain(capi, lamp, length, K, 0, 0)
    else:
        lamp, length, K = (-1.5, 1.25, 2.0), 1.0, 6
        prev, nxt = tie_chain(K, grid, 0x02468ace)
    gids = first_gid + np.arange(n, dtype=np.int64)
    h = np.stack([np_seed_input(gids, lamp, prev[k], nxt[k], 0) for k in range(K)])
    masks, distinct = brute_masks(h)
    own = masks[masks != 0]
    if grid in (0, 16):                      # (further down the ties meet no second gid: tests/test_dedupe_cpu.py asserts none there either)
        assert own.size > distinct, "the case holds no key twice"
    for mc in (4, capi.DEDUPE_CLASS_MAX):
        classes, dep = capi.dedupe_classes(lamp, prev, nxt, 0, first_gid, n, mc)
        check_list(classes, mc)
        assert dep == expected_deposits(own, classes)


def np_deposit_word(mask, classes, first_class_plane):
    """csrc/uvrt_dedupe.h dedupe_deposit_word with a class list (an empty list: classes off)"""
    if len(classes) == 0:
        return mask
    if mask & (mask - 1) == 0:
        return PLANE_FORM | (mask.bit_length() - 1)
    if mask in classes:
        return PLANE_FORM | CLASS_FORM | (first_class_plane + classes.index(mask))
    return mask


@pytest.mark.parametrize("K", [2, 8, 17, 30])
def test_fold_restated(K):
    """Deposits by word into launch planes and class planes (replicas: 3 for a launch plane, 2 for a class plane), then the
    fold's rule -- a launch's total = its own plane's replicas + the replicas of every class whose mask holds it -- against one
    deposit per set bit.  One class holds bit K - 1 (bit 29 at K = 30); some masks have no class and take the per-bit form."""
    rng = np.random.default_rng(1000 + K)
    T, R, RC, rays = 37, 3, 2, 5000
    full = (1 << K) - 1
    pool = sorted({int(m) for m in rng.integers(1, full + 1, size=40, dtype=np.int64)} | {full, (1 << (K - 1)) | 1})
    multi = [m for m in pool if m & (m - 1)]
    classes = ([(1 << (K - 1)) | 1] + [m for m in multi if m != ((1 << (K - 1)) | 1)][:5]) if K > 2 else [3]
    assert any(m >> (K - 1) & 1 for m in classes)
    singles = [1 << int(b) for b in rng.integers(0, K, size=6)]
    masks = rng.choice(np.array(pool + singles, dtype=np.int64), size=rays)
    tris = rng.integers(0, T, size=rays)
    blocks = rng.integers(0, 1000, size=rays)                     # the workgroup that traces the ray picks the replica
    want = np.zeros((K, T), dtype=np.int64)
    launch = np.zeros((K, R, T), dtype=np.int64)
    cls = np.zeros((len(classes), R, T), dtype=np.int64)          # allocated like a launch plane, RC replicas in use
    for m, t, b in zip(masks.tolist(), tris.tolist(), blocks.tolist()):
        for j in range(K):
            if m >> j & 1:
                want[j, t] += 1
        w = np_deposit_word(m, classes, K)
        if w & PLANE_FORM:
            idx = w & PLANE_INDEX
            if w & CLASS_FORM:
                cls[idx - K, b % RC, t] += 1
            else:
                launch[idx, b % R, t] += 1
        else:
            for j in range(K):
                if w >> j & 1:
                    launch[j, b % R, t] += 1
    assert cls[:, RC:, :].sum() == 0 and cls.sum() > 0 and launch.sum() > 0
    folded = launch.sum(axis=1)
    for c, m in enumerate(classes):
        total = cls[c, :RC].sum(axis=0)                            # read once per triangle ...
        for j in range(K):
            if m >> j & 1:
                folded[j] += total                                 # ... added to every launch of the mask
    assert np.array_equal(folded, want)
    # classes off: the words are the masks, the class planes stay empty
    assert all(np_deposit_word(int(m), [], K) == int(m) for m in masks[:50])
