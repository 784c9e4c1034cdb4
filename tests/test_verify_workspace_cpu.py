"""The handle-less workspace queries of the verification entry points (csrc/verify_common.h holds their shared plan): the
documented products of include/dlwp_hip.h, restated here in Python and compared over a small table.  A NULL handle counts 256 CUs,
the launches aim at 8 blocks per CU.  No GPU."""
import ctypes
import itertools

import pytest

from dlwp_amd import _lib

NULL = ctypes.c_void_p(0)
LL = ctypes.c_longlong
BLOCKS = 256 * 8                       # blocks of a launch without a handle
CELLS = ((1, 1), (3, 2), (40, 5), (2049, 1))
WIDTHS = (4, 180, 512)
ROWS = (1, 45, 64)
SPLITS = (0, 1, 3)
COUNTS = (1, 5, 1000)


def _ceil(a, b):
    return -(-a // b)


def _tiles(row):
    """256-thread column tiles of the route with the fewer of them: 16-byte units where row % 4 == 0"""
    return _ceil(row // 4 if row % 4 == 0 else row, 256)


@pytest.mark.parametrize('leads,groups', CELLS)
def test_error_workspace_is_cells_times_blocks_rounded_up_times_24_bytes(leads, groups):
    f = _lib.lib.dlwp_verify_error_workspace
    assert f(NULL, leads, groups) == leads * groups * _ceil(BLOCKS, leads * groups) * 3 * 8
    assert f(NULL, 0, groups) == 0 and f(NULL, leads, 0) == 0 and f(NULL, -1, -1) == 0


@pytest.mark.parametrize('leads,groups', CELLS)
def test_spectrum_workspace_is_cells_times_blocks_rounded_up_times_the_partial(leads, groups):
    f = _lib.lib.dlwp_verify_spectrum_workspace
    for width in WIDTHS:
        partial = (4 * (width // 2 + 1) + 2) * 8
        assert f(NULL, leads, groups, width) == leads * groups * _ceil(BLOCKS, leads * groups) * partial, width
    for bad in ((0, groups, 180), (leads, 0, 180), (leads, groups, 3), (leads, groups, 513), (leads, groups, 0)):
        assert f(NULL, *bad) == 0, bad


@pytest.mark.parametrize('leads', [c[0] for c in CELLS])
def test_skill_map_workspace_is_the_chunk_planes_of_the_documented_split(leads):
    f = _lib.lib.dlwp_verify_skill_map_workspace
    for count0, row, split in itertools.product((0,) + COUNTS, ROWS, SPLITS):
        chunks = split if split else max(1, BLOCKS // (leads * _tiles(row)))
        chunks = max(1, min(chunks, count0))
        want = leads * chunks * 9 * row * 8 if chunks > 1 else 0
        assert f(NULL, leads, count0, LL(row), split) == want, (count0, row, split)
    assert f(NULL, 0, 5, LL(64), 0) == 0 and f(NULL, leads, 5, LL(0), 0) == 0 and f(NULL, leads, 5, LL(64), -1) == 0


@pytest.mark.parametrize('n_labels', [1, 3, 12, 64])
def test_label_nanmean_workspace_is_a_sum_and_a_count_per_label_chunk_and_column(n_labels):
    f = _lib.lib.dlwp_verify_label_nanmean_workspace
    for count, row in itertools.product(COUNTS + (14608,), ROWS + (63360,)):
        split = min(max(1, BLOCKS // (n_labels * _tiles(row))), count)
        assert f(NULL, count, LL(row), n_labels) == n_labels * split * row * (8 + 4), (count, row)
    for bad in ((0, 64, n_labels), (5, 0, n_labels), (5, 64, 0), (5, 64, 65), (5, 64, 2049)):
        assert f(NULL, bad[0], LL(bad[1]), bad[2]) == 0, bad
