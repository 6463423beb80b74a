"""A numpy model of how a pooled leaf round of k_trace deals its work items to the lanes of one wave (trace_body's leaf_issue,
DESIGN.md section 4), in the form it had and in the form it has.  It is a documented model of the scheme: it proves the scheme,
not the kernel (tests/test_gpu_leaf_issue.py holds the kernel to the oracle on rounds of known shape).

A parked lane ("owner") has a leaf of 1..8 triangles.  Owners are served in lane order while their whole leaf fits into the wave's
64 items; item i is triangle k of owner o's leaf and is tested by lane i.

Before: lf_pre = the exclusive prefix sum of the counts, lf_served = parked and lf_pre + count <= 64, every served owner stored its
lane number into s_map[lf_pre .. lf_pre + count), item i read o = s_map[i] and took k = i - lf_pre[o] by a shuffle.

Now: a served owner stores ONE word, ((lf_pre << 6) | lane) + 1, into the slot of its first item, every other slot holds 0, and an
inclusive maximum over the lanes at and below i -- six DPP steps -- hands item i the word of the last owner that starts at or below i:
served owners' lf_pre and lane numbers both rise in lane order.  o and k = i - start are fields of that word.  This is the kernel's word
(KK_BITS = 0 below).

The second parametrisation, KK_BITS = 7, is NOT in the kernel: it is the variant of tools/patches/leaf_issue_kk_word.patch, whose word
((lf_pre << 13) | (lane << 7) | kk) + 1 also carries the seven axis / kind bits of the owner's ray below its lane number, where they
order nothing because two owners never share lf_pre or a lane.  It was measured and not kept; the model holds it to
the same mapping so that the patch stays a proven one."""
import numpy as np
import pytest


def prefix(counts):
    """(lf_pre, lf_served, lf_items) for a batch of count vectors, shape (n, 64); count 0 = not parked."""
    counts = np.asarray(counts, np.int64)
    pre = np.cumsum(counts, axis=1) - counts
    served = (counts > 0) & (pre + counts <= 64)
    items = np.where(served, pre + counts, 0).max(axis=1)       # lf_pre + count of the last served owner
    return pre, served, items


def old_map(counts):
    """Owner and in-leaf index of every item by the fill loop.  -1 where no owner stored anything."""
    counts = np.asarray(counts, np.int64)
    pre, served, items = prefix(counts)
    n = counts.shape[0]
    s_map = np.full((n, 64), -1, np.int64)
    rows = np.arange(n)[:, None].repeat(64, 1)
    lanes = np.arange(64)[None, :].repeat(n, 0)
    for k in range(8):
        m = served & (k < counts)
        s_map[rows[m], (pre + k)[m]] = lanes[m]
    valid = np.arange(64)[None, :] < items[:, None]
    owner = np.where(valid, s_map, 0)
    k = np.arange(64)[None, :] - np.take_along_axis(pre, owner, 1)          # the shuffle of the owner's lf_pre
    return owner, k, valid


def row_shr(x, n):
    """DPP row_shr:n, bound_ctrl off, old = 0: lane l of a row of 16 reads lane l - n of its row, or 0 when that is outside the row."""
    y = np.zeros_like(x)
    lane = np.arange(64)
    ok = (lane % 16) >= n
    y[:, ok] = x[:, lane[ok] - n]
    return y


def row_bcast(x, src_lane, row_mask):
    """DPP row_bcast:15 / row_bcast:31 with a row mask, old = 0: row_bcast:15 hands lane 15 of each row to every lane of the NEXT row,
    row_bcast:31 hands lane 31 to rows 2 and 3; rows outside row_mask take 0 (the identity of max)."""
    y = np.zeros_like(x)
    for row in range(4):
        if not (row_mask >> row) & 1:
            continue
        src = 16 * row - 1 if src_lane == 15 else 31
        if src >= 0:
            y[:, 16 * row:16 * row + 16] = x[:, src:src + 1]
    return y


def wave_max_scan(x):
    for n in (1, 2, 4, 8):
        x = np.maximum(x, row_shr(x, n))
    x = np.maximum(x, row_bcast(x, 15, 0xA))
    x = np.maximum(x, row_bcast(x, 31, 0xC))
    return x


def new_map(counts, kk, kk_bits):
    """kk_bits = 0: the kernel's word; 7: the kk-word variant (kk below the lane number)."""
    counts = np.asarray(counts, np.int64)
    pre, served, items = prefix(counts)
    n = counts.shape[0]
    slots = np.zeros((n, 64), np.int64)
    rows = np.arange(n)[:, None].repeat(64, 1)
    lanes = np.arange(64)[None, :].repeat(n, 0)
    word = ((pre << (6 + kk_bits)) | (lanes << kk_bits) | (kk if kk_bits else 0)) + 1
    assert word[served].max(initial=0) < 2 ** 32
    slots[rows[served], pre[served]] = word[served]
    w = wave_max_scan(slots) - 1
    valid = np.arange(64)[None, :] < items[:, None]
    owner, start, kk_item = (w >> kk_bits) & 63, w >> (6 + kk_bits), w & ((1 << kk_bits) - 1)
    return owner, np.arange(64)[None, :] - start, kk_item, valid


def check(counts):
    counts = np.atleast_2d(np.asarray(counts, np.int64))
    rng = np.random.default_rng(counts.shape[0])
    kk = rng.integers(0, 128, counts.shape)
    o0, k0, v0 = old_map(counts)
    assert (o0[v0] >= 0).all()                               # the fill loop covered every valid item
    assert (k0[v0] >= 0).all() and (k0[v0] < np.take_along_axis(counts, o0, 1)[v0]).all()
    for kk_bits in (0, 7):                                   # the kernel's word, then the kk-word variant of tools/patches
        o1, k1, kk1, v1 = new_map(counts, kk, kk_bits)
        assert np.array_equal(v0, v1)
        assert np.array_equal(o0[v0], o1[v0]) and np.array_equal(k0[v0], k1[v0])
        if kk_bits:
            assert np.array_equal(kk1[v0], np.take_along_axis(kk, o0, 1)[v0])
    return v0.sum(axis=1)


def test_max_scan_is_an_inclusive_maximum():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 2 ** 20, (2000, 64)) * (rng.random((2000, 64)) < 0.3)
    assert np.array_equal(wave_max_scan(x), np.maximum.accumulate(x, axis=1))


@pytest.mark.parametrize("s", range(1, 9))
def test_every_lane_parked_with_one_count(s):
    """First items on lanes 0, s, 2s, ...: over the eight counts every lane of rows 0-3 is a first item and leaves straddle lanes 16, 32 and 48."""
    items = check(np.full(64, s))
    assert items[0] == 64 // s * s


def test_first_items_reach_every_lane():
    first = set()
    for s in range(1, 9):
        first |= set(range(0, 64 // s * s, s))
    assert first == set(range(64))


def test_exact_fits_of_64_items():
    for c in ([8] * 8, [1] * 64, [7] * 8 + [8], [3, 5] * 8, [8, 7, 6, 5, 4, 3, 2, 1] + [4] * 7, [2] * 32):
        v = np.zeros(64, np.int64)
        v[:len(c)] = c
        assert v.sum() == 64 and check(v)[0] == 64
    # the same owners spread out over the wave, with lanes in between that are not parked
    v = np.zeros(64, np.int64)
    v[3::8] = 8
    assert check(v)[0] == 64


def test_a_leaf_that_straddles_item_64_stays_parked():
    v = np.zeros(64, np.int64)
    v[:9] = 7                    # nine owners make 63 items
    v[9] = 2                     # 63 + 2 > 64
    v[10] = 1                    # would fit, but owners are served in lane order: nobody after a leaf that does not fit
    pre, served, items = prefix(v[None])
    assert served[0, :9].all() and not served[0, 9:].any() and items[0] == 63
    assert check(v)[0] == 63
    assert check(np.full(64, 7))[0] == 63


def test_one_parked_lane():
    for lane in (0, 63):
        for s in range(1, 9):
            v = np.zeros(64, np.int64)
            v[lane] = s
            assert check(v)[0] == s


def test_only_the_last_row_parked():
    rng = np.random.default_rng(3)
    for _ in range(50):
        v = np.zeros(64, np.int64)
        v[48:] = rng.integers(1, 9, 16)
        check(v)
    v = np.zeros(64, np.int64)
    v[48:] = 4
    assert check(v)[0] == 64


def test_random_vectors():
    rng = np.random.default_rng(20000)
    p = rng.random((20000, 1))                                    # a parked share per vector, from nearly nobody to everybody
    counts = rng.integers(1, 9, (20000, 64)) * (rng.random((20000, 64)) < p)
    items = check(counts)
    assert items.min() == 0 and items.max() == 64
