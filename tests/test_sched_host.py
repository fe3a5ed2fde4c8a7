"""CPU-only checks around the scheduler tests: sched_oracle's own arithmetic (the sort's bins against a restatement in Python
integers, the interval pull-up on hand-made rows), the two scheduler hooks in the header and the signature table, and what they
refuse without a context."""
import ctypes

import numpy as np

from sched_oracle import cost_class, f32_round, lpt_bins, lpt_bins_integer, pull_up
from test_binding_host import Prototype, prototypes

INVALID = -1


def test_f32_round_is_numpy_float32():
    rng = np.random.default_rng(7)
    for v in [1, 3, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, 0xFFFFFFFF, 0xFFFFFF7F, 0xFFFFFF80,
              *rng.integers(1, 1 << 32, 200).tolist()]:
        assert float(f32_round(v)) == float(np.float32(np.uint32(v))), v
    for a, b in [(255, 3), (255, 4000), (255, 0xFFFFFFFF), (255, 1234), (255, 7)]:
        assert float(f32_round(f32_round(a) / f32_round(b))) == float(np.float32(a) / np.float32(b)), (a, b)


def test_lpt_bins_against_the_integer_restatement():
    rng = np.random.default_rng(11)
    cases = [np.zeros(5, dtype=np.uint32), np.full(9, 1234, dtype=np.uint32), np.arange(1, 600, dtype=np.uint32) * 7,
             rng.integers(0, 4001, 500).astype(np.uint32), rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32),
             np.array([0xFFFFFFFF, 0, 1, (1 << 24) + 1, 0xFFFFFF7F, 0x80000000, 0x7FFFFFFF], dtype=np.uint32),
             np.array([3, 1, 2], dtype=np.uint32), np.array([1], dtype=np.uint32)]
    for costs in cases:
        assert lpt_bins(costs).tolist() == lpt_bins_integer(costs.tolist())
    # by hand: the heaviest tile is in bin 0, an idle one in bin 255, half the maximum in the middle
    assert lpt_bins([4000, 0, 2000, 4000]).tolist() == [0, 255, 128, 0]
    assert lpt_bins([0, 0]).tolist() == [255, 255]
    assert lpt_bins([]).size == 0


def test_cost_class():
    assert cost_class([1.0, 255.9, 256.0, 300.0, 304.4, 304.5, 2.0 ** 15.75, 3.0e38, 0.0]).tolist() == [0, 0, 0, 0, 0, 1, 31, 31, 0]
    assert cost_class(2.0 ** 10 * (1 - 1e-6), 1e-3) == 8 and cost_class(2.0 ** 10 * (1 - 1e-6), 0.0) == 7
    assert cost_class(2.0 ** 10 * (1 + 1e-6), -1e-3) == 7


def test_pull_up_on_hand_made_rows():
    # one heavy tile pulls its two row neighbours to one class below it, and nobody else
    assert pull_up([0, 0, 9, 0, 0]).tolist() == [0, 8, 9, 8, 0]
    # all lanes at once, from the classes before the pull-up: no chain
    assert pull_up([9, 0, 0, 0]).tolist() == [9, 8, 0, 0]
    assert pull_up([5, 5, 6, 3]).tolist() == [5, 5, 6, 5]
    # blocks of 64 tile indices: lane 63 has no right neighbour, lane 0 no left one
    row = np.zeros(130, dtype=np.int64)
    row[64] = 20
    row[127] = 10
    want = row.copy()
    want[65] = 19                   # (63 is in the block before: untouched)
    want[126] = 9                   # (128 is in the block behind)
    assert pull_up(row).tolist() == want.tolist()
    # lanes past the last tile carry the class of the start cost (0): they pull nobody up
    assert pull_up([3]).tolist() == [3] and pull_up([0, 31]).tolist() == [30, 31]
    # intervals, bound by bound: lo with the neighbours' lo, hi with their hi, and lo <= hi survives
    lo, hi = np.array([2, 2, 7, 2]), np.array([2, 4, 12, 2])
    assert pull_up(lo).tolist() == [2, 6, 7, 6] and pull_up(hi).tolist() == [3, 11, 12, 11]
    rng = np.random.default_rng(3)
    for _ in range(50):
        lo = rng.integers(0, 32, 200)
        hi = np.minimum(31, lo + rng.integers(0, 6, 200) * (rng.random(200) < 0.2))
        mid = rng.integers(lo, hi + 1)
        a, b, c = pull_up(lo), pull_up(mid), pull_up(hi)
        assert (a <= b).all() and (b <= c).all()


def test_the_hooks_are_in_the_header_and_the_table(host):
    by_name = {p.name: p for p in prototypes()}
    assert by_name["rt_debug_tile_order"] == Prototype("int", "rt_debug_tile_order",
                                                       ["rt_context *ctx", "uint32_t *out", "int cap", "int *nTiles", "int *policy"])
    assert by_name["rt_debug_lpt_sort"] == Prototype("int", "rt_debug_lpt_sort",
                                                     ["rt_context *ctx", "uint32_t *costs", "int nTiles", "uint32_t *order", "uint32_t *accum"])
    u32p, intp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)
    assert host.SIGNATURES["rt_debug_tile_order"] == (ctypes.c_int, [ctypes.c_void_p, u32p, ctypes.c_int, intp, intp])
    assert host.SIGNATURES["rt_debug_lpt_sort"] == (ctypes.c_int, [ctypes.c_void_p, u32p, ctypes.c_int, u32p, u32p])
    names = list(host.SIGNATURES)
    at = names.index("rt_debug_predicted_classes")
    assert names[at + 1: at + 3] == ["rt_debug_tile_order", "rt_debug_lpt_sort"]


def test_the_hooks_refuse_a_null_context(host):
    """Before anything else is looked at, and without a device."""
    e = host.load_library().entry
    buf = (ctypes.c_uint32 * 4)()
    n, policy = ctypes.c_int(7), ctypes.c_int(7)
    assert e["rt_debug_tile_order"](None, buf, 4, ctypes.byref(n), ctypes.byref(policy)) == INVALID
    assert e["rt_debug_tile_order"](None, None, 0, None, None) == INVALID
    assert (n.value, policy.value) == (7, 7)
    assert e["rt_debug_lpt_sort"](None, buf, 4, buf, None) == INVALID
    assert e["rt_debug_lpt_sort"](None, None, 0, None, None) == INVALID
