"""What tests/test_gpu_size_boundaries.py shares (profiles/size_boundaries.txt): the launch plan's arithmetic restated, so that a test
can assert that it hands a persistent kernel several items per resident lane; the big batch made of a small base set by a seeded random index; and
the two exact comparisons - copy i of base row b against the small call's row b (explicit keys), windows of the big call against small calls over
the same rows with key_base + a (no keys). The answers stay on the device: a comparison is one kernel over their 32-bit words."""
import numpy as np

WG = 256          # SOL_WG: the lanes of a workgroup of the persistent kernels
CU_LANES = 2048   # a CU holds at most 32 waves of 64 lanes, whatever the occupancy query answers
WINDOW = 257      # rows of a window: four waves and one row
SWITCH_BELOW = (0, 8, 64)
SETTINGS = tuple((bpc, sb) for bpc in (1, 0) for sb in SWITCH_BELOW)  # (SOL_OPT_MAX_BLOCKS_PER_CU, SOL_OPT_SWITCH_BELOW)


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def resident_lanes(bpc):
    """The most lanes sol_launch_plan's grid can hold: n_cu x blocks_per_cu x 256. SOL_OPT_MAX_BLOCKS_PER_CU = 1: one workgroup per CU; 0: what the
    occupancy query allows, which is at most the CU's 2048 lanes."""
    return n_cu() * (WG if bpc == 1 else CU_LANES)


def items_wanted(bpc):
    """Eight items per resident lane under one workgroup per CU, four per lane the CU can hold under the default."""
    return (8 if bpc == 1 else 4) * resident_lanes(bpc)


def plan_items(n, samples=None, per_sample=False):
    """The items of one launch over n rows as sol_gather_launch / query_launch count them: n for a query; chunks x groups x 64 for chunk sums
    (chunks of 16 samples, groups of 64 rows); samples x groups x 64 per sample."""
    if samples is None:
        return n
    groups = -(-n // 64)
    return (samples if per_sample else -(-samples // 16)) * groups * 64


def rows_for(bpc, items_per_row, at_least=0):
    """The fewest rows whose launch has items_wanted(bpc) items, plus 65: a last group of one row."""
    n = max(-(-items_wanted(bpc) // items_per_row), at_least)
    return (n + 63) // 64 * 64 + 65


def assert_refills(items, bpc):
    """The launch has several items per lane of the largest grid the plan can give it: lanes end their item and take another while their neighbours
    are mid-search, reservoirs run dry between refills, and the counter runs past the items."""
    assert items >= items_wanted(bpc) and items >= 2 * resident_lanes(bpc), (items, items_wanted(bpc), resident_lanes(bpc), bpc)


def apply(ds, bpc, switch_below):
    from solstrale_amd import _abi
    ds.set_option(_abi.OPT_MAX_BLOCKS_PER_CU, bpc)
    ds.set_option(_abi.OPT_SWITCH_BELOW, switch_below)


# ---- device arrays ------------------------------------------------------------------------------------------------------------------------------
def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def keys_to_dev(keys):
    return to_dev(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32))


def words(rows):
    """The answers of a call, a device tensor or a host array of any 32-bit type and shape [n, ..], as an [n, words] int32 device tensor."""
    import torch
    if not hasattr(rows, "data_ptr"):
        a = np.ascontiguousarray(rows)
        rows = torch.from_numpy(a.view(np.int32).reshape(len(a), -1)).cuda()
    rows = rows.contiguous()
    return rows.view(torch.int32).reshape(rows.shape[0], -1)


def distinct_rows(w):
    return len(np.unique(w.cpu().numpy(), axis=0))


def rows_off(got, want):
    """(rows that differ in any word, the first few of them)."""
    import torch
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (got != want).any(dim=1)
    return int(bad.sum()), torch.nonzero(bad).flatten()[:6].tolist()


def random_index(n_base, n, seed):
    """n seeded random rows of the base set, every one of them at least once: neighbouring lanes hold different rows."""
    idx = np.random.default_rng(seed).integers(0, n_base, n)
    assert len(np.unique(idx)) == n_base
    return idx


def window_spans(n, boundaries, seed):
    """(start, length) of the windows of a call over n rows: the start, the end, a seeded place, and each side of every boundary inside the call."""
    assert n > 3 * WINDOW
    starts = {0, n - WINDOW, int(np.random.default_rng(seed).integers(WINDOW, n - 2 * WINDOW))}
    for b in boundaries:
        if WINDOW <= b < n:
            starts |= {b - WINDOW, b}
    return [(a, min(WINDOW, n - a)) for a in sorted(starts)]


# ---- the two comparisons ----------------------------------------------------------------------------------------------------------------------------
def assert_copies_equal_the_small_call(call, base, base_keys, small, n, seed, what):
    """call(rows, keys, key_base) over n random copies of the base rows, each with its base row's key: row i is the small call's row idx[i], word
    for word. base, base_keys, small: device tensors. Returns the index."""
    idx = random_index(len(base), n, seed)
    at = to_dev(idx)
    big = words(call(base[at], None if base_keys is None else base_keys[at], 0))
    off, where = rows_off(big, small[at])
    assert off == 0, (what, "rows that differ from the small call's", off, n, where)
    return idx


def assert_windows_equal_small_calls(call, rows, key_base, boundaries, seed, what, host=False):
    """call(rows, None, key_base) over the whole batch, row i drawing from key_base + i; every window [a, a + 257) of it against the call over just
    those rows with key_base + a. rows: a device tensor (host: a numpy array). Returns the whole call's words."""
    n = rows.shape[0]
    big = words(call(rows, None, key_base))
    for a, k in window_spans(n, boundaries, seed):
        part = words(call(rows[a:a + k] if host else rows[a:a + k].contiguous(), None, key_base + a))
        off, where = rows_off(part, big[a:a + k])
        assert off == 0, (what, "window at", a, "rows that differ", off, where)
    return big
