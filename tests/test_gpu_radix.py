"""The stable LSD radix sort under order, sort and both category builds (cs::radix_sort_pairs64, cs_radix.hip), by itself,
against numpy.

cs_debug_radix_sort_pairs64 sorts n (uint64 key, int32 item) pairs on the device in place.  Keys and items are compared for
EXACT equality with

    perm = argsort(keys, kind="stable");  keys[perm], items[perm]

The items are random int32 values, so a payload that does not travel with its key shows.  Both arrays carry 8 sentinels
behind n.  The key families and sizes are in radix_cases.py; tests/test_radix_cases_cpu.py checks without a GPU that they
reach every digit position, every pass count from 0 to 8 (odd: the result is copied back from the scratch buffers), skipped
digits that are not zero, and runs of one digit value over a whole 1024-pair chunk of a wave."""
import numpy as np
import pytest

import gpuutil
import radix_cases as rc

pytestmark = pytest.mark.gpu

GUARD = 8
KEY_SENTINEL = np.uint64(0x5EA7ED5EA7ED5EA7)
ITEM_SENTINEL = np.int32(-0x12345678)


def upload(keys, items):
    import torch

    n = len(keys)
    k = np.concatenate([keys.astype(np.uint64), np.full(GUARD, KEY_SENTINEL, dtype=np.uint64)])
    i = np.concatenate([items.astype(np.int32), np.full(GUARD, ITEM_SENTINEL, dtype=np.int32)])
    return torch.from_numpy(k.view(np.int64)).cuda(), torch.from_numpy(i).cuda(), n


def download(dk, di, n, what):
    k, i = dk.cpu().numpy().view(np.uint64), di.cpu().numpy()
    assert (k[n:] == KEY_SENTINEL).all(), what + ": wrote behind keys[n]"
    assert (i[n:] == ITEM_SENTINEL).all(), what + ": wrote behind items[n]"
    return k[:n], i[:n]


def sort_on_device(dk, di, n, stream=None):
    L = gpuutil.lib()
    L.check(L.lib.cs_debug_radix_sort_pairs64(dk.data_ptr(), di.data_ptr(), n, stream))


def compare(got_keys, got_items, keys, items, what):
    want_keys, want_items = rc.reference(keys, items)
    bad = np.flatnonzero((got_keys != want_keys) | (got_items != want_items))
    assert bad.size == 0, "%s: %d pairs differ, the first at %d: (%#x, %d), expected (%#x, %d)" % (
        what, bad.size, bad[0], int(got_keys[bad[0]]), int(got_items[bad[0]]), int(want_keys[bad[0]]), int(want_items[bad[0]]))


def check(keys, items, what, stream=None):
    import torch

    dk, di, n = upload(keys, items)
    torch.cuda.synchronize()
    sort_on_device(dk, di, n, stream)
    got_keys, got_items = download(dk, di, n, what)
    compare(got_keys, got_items, keys, items, what)


@pytest.mark.parametrize("name", list(rc.FAMILIES))
def test_gpu_radix_sort(name):
    """Every size of the family (radix_cases.sizes: around one ballot step, one wave's chunk, one and two tiles; the families
    marked large also a last tile of one pair and 18 tiles; full random 300 000 pairs)."""
    for n in rc.sizes(name):
        check(rc.keys_of(name, n), rc.items_of(name, n), "%s n %d" % (name, n))


@pytest.mark.parametrize("name", ["live_digit_0_of_2_values", "live_digit_7_of_2_values", "order_keys", "all_equal_mixed", "two_keys_99_to_1"])
def test_gpu_radix_sort_keeps_equal_keys_in_index_order(name):
    """The payload is the index: behind the sort the items of every run of equal keys ascend."""
    import torch

    n = 8193
    keys, items = rc.keys_of(name, n), np.arange(n, dtype=np.int32)
    dk, di, _ = upload(keys, items)
    torch.cuda.synchronize()
    sort_on_device(dk, di, n)
    got_keys, got_items = download(dk, di, n, name)
    assert (got_keys[1:] >= got_keys[:-1]).all(), name + ": keys not ascending"
    broken = np.flatnonzero((got_keys[1:] == got_keys[:-1]) & (got_items[1:] <= got_items[:-1]))
    if broken.size:
        at = int(broken[0])
        pytest.fail("%s: index order broken among equal keys, first at %d: key %#x, items %d then %d" % (
            name, at, int(got_keys[at]), int(got_items[at]), int(got_items[at + 1])))
    compare(got_keys, got_items, keys, items, name)


@pytest.mark.parametrize("side_stream", [False, True], ids=["default_stream", "side_stream"])
def test_gpu_radix_sort_of_65_pairs_right_after_70001(side_stream):
    """The scratch of the large sort comes back from the pool for the small one (buffers far larger than it needs)."""
    import torch

    big, small = rc.LARGE_N[-1], 65
    stream = torch.cuda.Stream() if side_stream else None
    handle = stream.cuda_stream if side_stream else None
    cases = [("full_random", big), ("full_random", small), ("3_live_digits", small)]
    dev = [upload(rc.keys_of(nm, n), rc.items_of(nm, n)) for nm, n in cases]
    torch.cuda.synchronize()
    for dk, di, n in dev:
        sort_on_device(dk, di, n, handle)
    for (nm, n), (dk, di, _) in zip(cases, dev):
        what = "%s n %d after %d%s" % (nm, n, big, " on a side stream" if side_stream else "")
        got_keys, got_items = download(dk, di, n, what)
        compare(got_keys, got_items, rc.keys_of(nm, n), rc.items_of(nm, n), what)


def test_gpu_radix_sort_entry_point_arguments():
    import torch

    L = gpuutil.lib()
    f = L.lib.cs_debug_radix_sort_pairs64
    keys, items = np.sort(rc.keys_of("full_random", 4))[::-1].copy(), rc.items_of("full_random", 4)  # (descending: a sort would show)
    dk, di, _ = upload(keys, items)
    torch.cuda.synchronize()
    assert f(dk.data_ptr(), di.data_ptr(), -1, None) == L.CS_ERR_INVALID_ARG
    for n in (1, 4):
        assert f(None, di.data_ptr(), n, None) == L.CS_ERR_INVALID_ARG
        assert f(dk.data_ptr(), None, n, None) == L.CS_ERR_INVALID_ARG
        assert f(None, None, n, None) == L.CS_ERR_INVALID_ARG
    assert f(None, None, 0, None) == L.CS_OK
    for n in (0, 1):  # nothing to sort: nothing is touched (the four pairs stay as they were, unsorted)
        assert f(dk.data_ptr(), di.data_ptr(), n, None) == L.CS_OK
        got_keys, got_items = download(dk, di, 4, "n %d" % n)
        assert np.array_equal(got_keys, keys) and np.array_equal(got_items, items), n
