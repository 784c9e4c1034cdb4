"""The data-movement kernels of dlwp_amd/csrc/halo.hip -- pad2d forward / backward, maxpool2, upsample2, copy_channels and
series_merge_time -- on EVERY route their host code can take, not only the ones torch-aligned tensors of the U-Net's sizes
happen to take.

The host picks a kernel by pointer alignment, row length, `inner` (channels-last), LDS fit and a grid cap, and reports nothing
about its choice, so `pad_route` below restates that dispatch line for line (halo.hip:686-734 forward, 755-819 backward).  One
case list, CASES, names the route every shape is meant to reach; a CPU test checks the list against the restatement at
lds_bytes = 65536 / 256 CUs and that it reaches every route; the GPU tests check it again with the device's own numbers, then
compare the kernels with the float64 oracle (oracle/np_ref.py): the forward bit for bit, the backward inside a DERIVED bound
(m float32 additions in any order) and bit for bit on integer-valued gradients.  Nothing here is tuned to what the kernels give."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_ref

ZERO, WRAP, EDGE, REFLECT, SYMMETRIC = 0, 1, 2, 3, 4
MODES = (ZERO, WRAP, EDGE, REFLECT, SYMMETRIC)
MODE_PAIRS = [(mh, mw) for mh in MODES for mw in MODES]
LDS0, CU0 = 65536, 256             # the numbers the case list is written for; the GPU tests use the device's own

# ----------------------------------------------------------------------------------------------------------------- #
# 1. the host dispatch of dlwp_pad2d_fwd / dlwp_pad2d_bwd, restated
# ----------------------------------------------------------------------------------------------------------------- #

# family: 'flat' (pad2d_*_flat_kernel), 'rows' (pad2d_fwd_kernel / pad2d_bwd_rows_kernel), 'elementwise' (pad2d_bwd_kernel)
# or 'refused'; vec: floats per load / store; rows: rows per wave and trip; capped: the grid was cut to 8 * cu_count blocks (the
# grid-stride loop then repeats); instance: which instantiation of a flat kernel ('zero_wrap': the compile-time composite halo)
Route = collections.namedtuple('Route', 'family vec rows capped instance')


def _pad_flat_rows(row_floats):                              # halo.hip:662
    return 16 if row_floats <= 80 else (8 if row_floats <= 160 else 4)


def _rows_vec(ri, ro, a_mod16, b_mod16):                     # halo.hip:720-721 / 795-796
    if ri % 4 == 0 and ro % 4 == 0 and a_mod16 == 0 and b_mod16 == 0:
        return 4
    if ri % 2 == 0 and ro % 2 == 0 and a_mod16 % 8 == 0 and b_mod16 % 8 == 0:
        return 2
    return 1


def _instance(mode_h, mode_w):                               # halo.hip:699 / 770
    return 'zero_wrap' if (mode_h, mode_w) == (ZERO, WRAP) else 'generic'


def pad_route(direction, outer, H, W, inner, pads, modes, in_mod16, out_mod16, lds_bytes, cu_count):
    """The kernel dlwp_pad2d_fwd ('fwd': in = x, out = y) or dlwp_pad2d_bwd ('bwd': in = dy, out = dx) launches.  *_mod16: the
    pointer's address modulo 16."""
    top, bottom, left, right = pads
    Ho, Wo = H + top + bottom, W + left + right              # :684 / :756
    RI, RO = W * inner, Wo * inner                           # :685 / :787
    cap = cu_count * 8
    both16 = in_mod16 == 0 and out_mod16 == 0
    if direction == 'fwd':
        if inner == 1 and both16 and Wo <= 4096:             # :686
            rows = _pad_flat_rows(min(W, Wo))                # :687
            flat_lds = (RI + 6) // 4 * 4 + 4                 # :688
            nbytes = flat_lds * 4 * rows * 4 + 4 * rows * 8  # :689
            if nbytes <= 64 * 1024 and nbytes <= lds_bytes:  # :690
                groups = (outer * Ho + rows - 1) // rows     # :691
                grid = (groups + 3) // 4                     # :692
                return Route('flat', 4, rows, grid > cap, _instance(*modes))      # :693-707
        row_lds = (RI + 3) // 4 * 4                          # :713
        if row_lds * 4 * 4 * 4 > lds_bytes:                  # :714-715  (no 64 KB condition here: see test 4)
            return Route('refused', 0, 0, False, None)
        grid = (outer * Ho + 15) // 16                       # :716-717
        return Route('rows', _rows_vec(RI, RO, in_mod16, out_mod16), 4, grid > cap, None)     # :718-734
    assert direction == 'bwd'
    if inner == 1 and both16 and Wo <= 4096:                 # :755
        rows = _pad_flat_rows(W)                             # :757
        flat_lds = (Wo + 6) // 4 * 4 + 4                     # :758
        nbytes = flat_lds * 4 * rows * 4 + 4 * rows * (8 + 4)                     # :759
        if nbytes <= 64 * 1024 and nbytes <= lds_bytes:      # :760
            groups = (outer * H + rows - 1) // rows          # :761
            grid = (groups + 3) // 4                         # :762
            return Route('flat', 4, rows, grid > cap, _instance(*modes))          # :763-778
    row_lds = (RO + 3) // 4 * 4                              # :788
    nbytes = row_lds * 4 * 4 * 4                             # :789
    if nbytes <= lds_bytes and nbytes <= 64 * 1024:          # :790
        grid = (outer * H + 15) // 16                        # :791-792
        return Route('rows', _rows_vec(RI, RO, in_mod16, out_mod16), 4, grid > cap, None)     # :793-809
    want = (outer * H * W * inner + 255) // 256              # :815-816, grid_for (:19-24)
    return Route('elementwise', 1, 0, max(want, 1) > cap, None)


# ----------------------------------------------------------------------------------------------------------------- #
# the case list
# ----------------------------------------------------------------------------------------------------------------- #

def _r(family, vec, rows, capped=False):
    return (family, vec, rows, capped)


F16, F8, F4 = _r('flat', 4, 16), _r('flat', 4, 8), _r('flat', 4, 4)
R4, R2, R1 = _r('rows', 4, 4), _r('rows', 2, 4), _r('rows', 1, 4)
EW, REFUSED = _r('elementwise', 1, 0), _r('refused', 0, 0)
F16C, R1C = _r('flat', 4, 16, True), _r('rows', 1, 4, True)

# layout 'nchw': shape (N, C, H, W), inner = 1; 'nhwc': shape (N, H, W, C), inner = C.
# pads: (top, bottom, left, right), cut per mode to what the axis admits; 'max': as large as every mode admits on both axes;
#   'maxh': as large as admitted on the rows, (3, 2) on the columns.
# offs: (a, b) floats by which the unpadded tensor (x / dx) and the padded one (y / dy) are moved off a 16-byte boundary.
# fwd / bwd: (family, vec, rows per wave, capped) the case is meant to reach at lds_bytes = 65536 and 256 CUs.
Case = collections.namedtuple('Case', 'name layout shape pads offs fwd bwd')
P = (2, 1, 3, 2)
Q = (2, 1, 3, 1)      # W and Wo of the same parity: rows of whole 8- or 16-byte units on both sides

# the last W of a (1, 1, 3, W) tensor under pads P whose flat LDS request fits in 64 KB (4 rows per wave):
#   forward   ((W + 6) // 4 * 4 + 4) * 64 + 128 <= 65536   <=>  W <= 1013
#   backward  ((W + 5 + 6) // 4 * 4 + 4) * 64 + 192 <= 65536  <=>  W <= 1008
FWD_EDGE_W, BWD_EDGE_W = 1013, 1008

CASES = [
    # flat: rows per wave change at row lengths 80 / 81 and 160 / 161
    Case('flat_w77', 'nchw', (1, 2, 5, 77), P, (0, 0), F16, F16),
    Case('flat_w78', 'nchw', (1, 2, 5, 78), P, (0, 0), F16, F16),
    Case('flat_w80', 'nchw', (1, 2, 5, 80), P, (0, 0), F16, F16),
    Case('flat_w81', 'nchw', (1, 2, 5, 81), P, (0, 0), F8, F8),
    Case('flat_w157', 'nchw', (1, 2, 5, 157), P, (0, 0), F8, F8),
    Case('flat_w158', 'nchw', (1, 2, 5, 158), P, (0, 0), F8, F8),
    Case('flat_w160', 'nchw', (1, 2, 5, 160), P, (0, 0), F8, F8),
    Case('flat_w161', 'nchw', (1, 2, 5, 161), P, (0, 0), F4, F4),
    # flat: the last row length whose LDS request fits, and the next one (forward and backward leave at different lengths)
    Case('edge_bwd_last', 'nchw', (1, 1, 3, BWD_EDGE_W), P, (0, 0), F4, F4),
    Case('edge_bwd_next', 'nchw', (1, 1, 3, BWD_EDGE_W + 1), P, (0, 0), F4, R1),
    Case('edge_fwd_last', 'nchw', (1, 1, 3, FWD_EDGE_W), P, (0, 0), F4, R1),
    Case('edge_fwd_next', 'nchw', (1, 1, 3, FWD_EDGE_W + 1), P, (0, 0), R1, R1),
    # rows, inner == 1: a pointer off the 16-byte boundary, or (V = 4) aligned rows too long for the flat kernels
    Case('rows_w12_x2', 'nchw', (2, 3, 7, 12), Q, (2, 0), R2, R2),
    Case('rows_w12_y2', 'nchw', (2, 3, 7, 12), Q, (0, 2), R2, R2),
    Case('rows_w12_x1', 'nchw', (2, 3, 7, 12), Q, (1, 0), R1, R1),
    Case('rows_w12_y1', 'nchw', (2, 3, 7, 12), Q, (0, 1), R1, R1),
    Case('rows_w10_x2', 'nchw', (2, 3, 7, 10), Q, (2, 0), R2, R2),
    Case('rows_w10_xy2', 'nchw', (2, 3, 7, 10), Q, (2, 2), R2, R2),
    Case('rows_w9_y1', 'nchw', (2, 3, 7, 9), P, (0, 1), R1, R1),
    Case('rows_w9_x2', 'nchw', (2, 3, 7, 9), P, (2, 0), R1, R1),
    Case('rows_w1016_v4', 'nchw', (1, 1, 3, 1016), Q, (0, 0), R4, R4),
    # rows, inner > 1 (channels-last): W * C and Wo * C a multiple of 4, of 2, or odd; C = 1 is the flat route again
    Case('nhwc_c4', 'nhwc', (2, 5, 6, 4), P, (0, 0), R4, R4),
    Case('nhwc_c2', 'nhwc', (2, 5, 6, 2), P, (0, 0), R2, R2),
    Case('nhwc_c3', 'nhwc', (2, 5, 6, 3), P, (0, 0), R1, R1),
    Case('nhwc_c1', 'nhwc', (2, 5, 6, 1), P, (0, 0), F16, F16),
    Case('nhwc_c4_y2', 'nhwc', (2, 5, 6, 4), P, (0, 2), R2, R2),
    Case('nhwc_c4_x1', 'nhwc', (2, 5, 6, 4), P, (1, 0), R1, R1),
    # capped grids (more than 8 * 256 blocks wanted): the grid-stride loop runs a second trip
    Case('capped_flat', 'nchw', (1, 9000, 13, 6), P, (0, 0), F16C, F16),
    Case('capped_rows', 'nchw', (1, 9000, 13, 6), P, (1, 0), R1C, R1C),
    Case('capped_flat_bwd', 'nchw', (1, 9000, 15, 6), P, (0, 0), F16C, F16C),
    # padding as large as the mode admits (wrap = axis, REFLECT = axis - 1, SYMMETRIC = axis); one-row and one-column axes
    Case('max_3x4', 'nchw', (1, 2, 3, 4), 'max', (0, 0), F16, F16),
    Case('max_3x4_x1', 'nchw', (1, 2, 3, 4), 'max', (1, 0), R1, R1),
    Case('max_one_row', 'nchw', (1, 2, 1, 5), 'max', (0, 0), F16, F16),
    Case('max_one_col', 'nchw', (1, 2, 4, 1), 'max', (0, 0), F16, F16),
    Case('max_one_col_y1', 'nchw', (1, 2, 4, 1), 'max', (0, 1), R1, R1),
    Case('max_nhwc', 'nhwc', (1, 3, 4, 2), 'max', (0, 0), R4, R4),
    # rows longer than 1024 floats: the backward falls back to the element-wise kernel, the forward refuses at 64 KB of LDS
    # (what it does with more is test_pad2d_fwd_long_rows')
    Case('long_1030', 'nchw', (1, 1, 3, 1030), P, (0, 0), REFUSED, EW),
    Case('long_1030_x1', 'nchw', (1, 1, 3, 1030), P, (1, 0), REFUSED, EW),
    Case('long_1030_maxh', 'nchw', (1, 1, 3, 1030), 'maxh', (0, 0), REFUSED, EW),
    Case('long_2x4x1440', 'nchw', (1, 2, 4, 1440), P, (0, 0), REFUSED, EW),
    Case('long_2x4x1440_y2', 'nchw', (1, 2, 4, 1440), P, (0, 2), REFUSED, EW),
    Case('long_nhwc_1200', 'nhwc', (1, 3, 400, 3), P, (0, 0), REFUSED, EW),
    Case('long_nhwc_1200_x1', 'nhwc', (1, 3, 400, 3), P, (1, 0), REFUSED, EW),
    Case('long_1440', 'nchw', (1, 1, 3, 1440), P, (0, 0), REFUSED, EW),
    Case('long_2600', 'nchw', (1, 1, 3, 2600), P, (0, 0), REFUSED, EW),
]
CASE_IDS = [c.name for c in CASES]

# every name above, once more: the rows of the issue's table.  A case dropped from CASES fails test_case_list_... below.
REQUIRED_CASES = (
    'flat_w77 flat_w78 flat_w80 flat_w81 flat_w157 flat_w158 flat_w160 flat_w161 edge_bwd_last edge_bwd_next edge_fwd_last '
    'edge_fwd_next rows_w12_x2 rows_w12_y2 rows_w12_x1 rows_w12_y1 rows_w10_x2 rows_w10_xy2 rows_w9_y1 rows_w9_x2 rows_w1016_v4 '
    'nhwc_c4 nhwc_c2 nhwc_c3 nhwc_c1 nhwc_c4_y2 nhwc_c4_x1 capped_flat capped_rows capped_flat_bwd max_3x4 max_3x4_x1 '
    'max_one_row max_one_col max_one_col_y1 max_nhwc long_1030 long_1030_x1 long_1030_maxh long_2x4x1440 long_2x4x1440_y2 '
    'long_nhwc_1200 long_nhwc_1200_x1 long_1440 long_2600').split()


def geometry(case):
    """(outer, H, W, inner) as ops.pad2d hands them to the library"""
    if case.layout == 'nhwc':
        n, h, w, c = case.shape
        return n, h, w, c
    n, c, h, w = case.shape
    return n * c, h, w, 1


def _limit(n, mode):
    """the largest padding a mode admits on an axis of n (zero / edge admit any: n stands in)"""
    return n - 1 if mode == REFLECT else n


def pads_for(case, mode_h, mode_w):
    _, H, W, _ = geometry(case)
    want = {'max': (H, H, W, W), 'maxh': (H, H, 3, 2)}.get(case.pads, case.pads)
    lh, lw = _limit(H, mode_h), _limit(W, mode_w)
    return (min(want[0], lh), min(want[1], lh), min(want[2], lw), min(want[3], lw))


def padded_shape(case, pads):
    t, b, l, r = pads
    if case.layout == 'nhwc':
        n, h, w, c = case.shape
        return (n, h + t + b, w + l + r, c)
    n, c, h, w = case.shape
    return (n, c, h + t + b, w + l + r)


def case_route(case, direction, modes, lds_bytes, cu_count, mods=None):
    """mods: (address of the unpadded tensor mod 16, of the padded one); None: what case.offs asks for"""
    a, b = mods if mods is not None else (4 * case.offs[0], 4 * case.offs[1])
    outer, H, W, inner = geometry(case)
    in_mod, out_mod = (a, b) if direction == 'fwd' else (b, a)
    return pad_route(direction, outer, H, W, inner, pads_for(case, *modes), modes, in_mod, out_mod, lds_bytes, cu_count)


def test_case_list_reaches_every_route_of_the_pad_dispatch():
    assert sorted(CASE_IDS) == sorted(REQUIRED_CASES) and len(set(CASE_IDS)) == len(CASES)
    for direction in ('fwd', 'bwd'):
        reached = set()
        for case in CASES:
            inner = geometry(case)[3]
            for modes in MODE_PAIRS:
                r = case_route(case, direction, modes, LDS0, CU0)
                want = case.fwd if direction == 'fwd' else case.bwd
                assert tuple(r[:4]) == want, (case.name, direction, modes, r)
                reached.add((r.family, r.vec, r.rows, r.instance, inner > 1))
                if r.capped:
                    reached.add((r.family, 'capped'))
        for rows in (16, 8, 4):
            for inst in ('zero_wrap', 'generic'):
                assert ('flat', 4, rows, inst, False) in reached, (direction, rows, inst)
        for vec in (4, 2, 1):
            for nhwc in (False, True):
                assert ('rows', vec, 4, None, nhwc) in reached, (direction, vec, nhwc)
        assert ('flat', 'capped') in reached and ('rows', 'capped') in reached, direction
        if direction == 'bwd':
            assert ('elementwise', 1, 0, None, False) in reached and ('elementwise', 1, 0, None, True) in reached
        else:
            assert ('refused', 0, 0, None, False) in reached


def test_flat_route_ends_where_the_derivation_says():
    """FWD_EDGE_W / BWD_EDGE_W are the last flat row lengths of (1, 1, 3, W) under pads P, by search through the restated dispatch"""
    for direction, edge in (('fwd', FWD_EDGE_W), ('bwd', BWD_EDGE_W)):
        fams = [pad_route(direction, 1, 3, w, 1, P, (EDGE, EDGE), 0, 0, LDS0, CU0).family for w in range(900, 1100)]
        last = max(w for w, f in zip(range(900, 1100), fams) if f == 'flat')
        assert last == edge and all(f == 'flat' for f in fams[:edge - 900 + 1]), (direction, last)


# ----------------------------------------------------------------------------------------------------------------- #
# 6. the oracle itself
# ----------------------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('shape', [(1, 2, 3, 4), (2, 1, 1, 5), (1, 2, 4, 1), (2, 3, 5, 7)])
def test_oracle_pad_grad_is_the_exact_adjoint_in_all_25_mode_pairs(shape):
    """sum(pad(x) * dy) == sum(x * grad(dy)) EXACTLY on integer-valued float64 data, at the largest admissible paddings and at P"""
    rng = np.random.default_rng(17)
    x = rng.integers(-50, 51, size=shape).astype(np.float64)
    for case in (Case('max', 'nchw', shape, 'max', (0, 0), None, None), Case('p', 'nchw', shape, P, (0, 0), None, None)):
        for mh, mw in MODE_PAIRS:
            pads = pads_for(case, mh, mw)
            y = np_ref.pad2d_modes(x, pads, mh, mw)
            dy = rng.integers(-50, 51, size=y.shape).astype(np.float64)
            dx = np_ref.pad2d_modes_grad(dy, shape, pads, mh, mw)
            assert dx.shape == x.shape and (y * dy).sum() == (x * dx).sum(), (pads, mh, mw)


# ----------------------------------------------------------------------------------------------------------------- #
# GPU plumbing
# ----------------------------------------------------------------------------------------------------------------- #

@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def device_numbers():
    """(lds_bytes, cu_count) of the library's handle -- what halo.hip's dispatch compares with"""
    from dlwp_amd import _lib
    cu, lds = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib.dlwp_device_info(_lib.handle(torch.cuda.current_device()), ctypes.byref(cu), ctypes.byref(lds), None, 0))
    assert cu.value > 0 and lds.value > 0
    assert cu.value == torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return lds.value, cu.value


SENTINEL = np.float32(-7.25e11)
GUARD = 8           # floats in front of and behind every slab (a multiple of 4: the guard does not move the alignment)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Slab(object):
    """A float32 tensor that is buf[k : k + numel].view(shape) of a larger flat buffer, `off` floats off a 16-byte boundary, with
    sentinel floats on both sides that a kernel must leave bit-identical."""

    def __init__(self, shape, off=0, values=None):
        n = int(np.prod(shape))
        self.lo, self.n, self.shape = GUARD + off, n, tuple(shape)
        self.buf = torch.full((self.lo + n + GUARD,), float(SENTINEL), dtype=torch.float32, device='cuda')
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[self.lo:self.lo + n].view(self.shape)
        if values is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (4 * off) % 16

    @property
    def mod16(self):
        return self.t.data_ptr() % 16

    def read(self):
        """the tensor on the host; asserts the sentinels first"""
        torch.cuda.synchronize()
        a = self.buf.cpu().numpy()
        assert np.all(_bits(a[:self.lo]) == _bits(SENTINEL)), 'wrote in front of the tensor'
        assert np.all(_bits(a[self.lo + self.n:]) == _bits(SENTINEL)), 'wrote behind the tensor'
        return a[self.lo:self.lo + self.n].reshape(self.shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool(np.all(_bits(self.buf.cpu().numpy()) == _bits(SENTINEL)))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def pad_bwd_into(ops, dy, dx, case, pad):
    """dlwp_pad2d_bwd through the C ABI, into a dx of the caller's (ops.pad2d_bwd allocates its own, always aligned)"""
    from dlwp_amd import _lib
    outer, H, W, inner = geometry(case)
    _lib.check(_lib.lib.dlwp_pad2d_bwd(_lib.handle(torch.cuda.current_device()), _vp(dy), _vp(dx), outer, H, W, inner, pad, _lib.F32,
                                       _stream()))


def ref_pad(case, x, pads, mh, mw):
    if case.layout == 'nhwc':
        return np.ascontiguousarray(np_ref.pad2d_modes(x.transpose(0, 3, 1, 2), pads, mh, mw).transpose(0, 2, 3, 1))
    return np_ref.pad2d_modes(x, pads, mh, mw)


def ref_pad_grad(case, dy, pads, mh, mw):
    """float64"""
    if case.layout == 'nhwc':
        n, h, w, c = case.shape
        g = np_ref.pad2d_modes_grad(dy.transpose(0, 3, 1, 2), (n, c, h, w), pads, mh, mw)
        return np.ascontiguousarray(g.transpose(0, 2, 3, 1))
    return np_ref.pad2d_modes_grad(dy, case.shape, pads, mh, mw)


def distinct(shape):
    """arange-based float32: every element distinct and exactly representable, so a misrouted element is a wrong integer"""
    n = int(np.prod(shape))
    assert n < 2 ** 24
    return (np.arange(n, dtype=np.float32) + 1).reshape(shape)


# ----------------------------------------------------------------------------------------------------------------- #
# 2. pad forward, bit-exact
# ----------------------------------------------------------------------------------------------------------------- #

@pytest.mark.gpu
@pytest.mark.parametrize('case', [c for c in CASES if c.fwd != REFUSED], ids=lambda c: c.name)
def test_pad2d_fwd_on_its_route_is_bit_exact(ops, case):
    lds, cu = device_numbers()
    x = distinct(case.shape)
    xs = Slab(case.shape, case.offs[0], x)
    for mh, mw in MODE_PAIRS:
        pads = pads_for(case, mh, mw)
        ys = Slab(padded_shape(case, pads), case.offs[1])
        r = case_route(case, 'fwd', (mh, mw), lds, cu, (xs.mod16, ys.mod16))
        assert tuple(r[:4]) == case.fwd, 'expected route %r, the dispatch gives %r (lds_bytes %d, %d CUs)' % (case.fwd, r, lds, cu)
        got = ops.pad2d(xs.t, ops.make_pad(*pads, mh, mw), channels_last=case.layout == 'nhwc', out=ys.t)
        assert got.data_ptr() == ys.t.data_ptr()
        assert np.array_equal(ys.read(), ref_pad(case, x, pads, mh, mw)), (pads, mh, mw, r)
    assert np.array_equal(xs.read(), x)


@pytest.mark.gpu
def test_pad2d_refuses_one_more_than_each_limit(ops):
    from dlwp_amd._lib import DlwpError
    x = torch.zeros((1, 2, 3, 4), device='cuda')
    dy = torch.zeros((1, 2, 16, 16), device='cuda')
    for pads, mh, mw, fwd_msg, bwd_msg in [
            ((4, 0, 0, 0), WRAP, ZERO, 'periodic row padding', 'periodic rows exceed H'),
            ((0, 4, 0, 0), WRAP, ZERO, 'periodic row padding', 'periodic rows exceed H'),
            ((0, 0, 5, 0), ZERO, WRAP, 'periodic column padding', 'periodic cols exceed W'),
            ((0, 0, 0, 5), ZERO, WRAP, 'periodic column padding', 'periodic cols exceed W'),
            ((3, 0, 0, 0), REFLECT, ZERO, 'mirror padding exceeds the axis', 'mirror padding exceeds the axis'),
            ((0, 0, 0, 4), ZERO, REFLECT, 'mirror padding exceeds the axis', 'mirror padding exceeds the axis'),
            ((0, 4, 0, 0), SYMMETRIC, ZERO, 'mirror padding exceeds the axis', 'mirror padding exceeds the axis'),
            ((0, 0, 5, 0), ZERO, SYMMETRIC, 'mirror padding exceeds the axis', 'mirror padding exceeds the axis')]:
        p = ops.make_pad(*pads, mh, mw)
        with pytest.raises(DlwpError, match=fwd_msg):
            ops.pad2d(x, p)
        with pytest.raises(DlwpError, match=bwd_msg):
            ops.pad2d_bwd(dy, (1, 2, 3, 4), p)


# ----------------------------------------------------------------------------------------------------------------- #
# 3. pad backward, against the float64 adjoint
# ----------------------------------------------------------------------------------------------------------------- #

U = 2.0 ** -24


def summands(case, pads, mh, mw):
    """m = pad2d_modes_grad(ones): how many dy elements fold onto each dx element (the same in every image: one is folded)"""
    t, b, l, r = pads
    _, H, W, _ = geometry(case)
    m = np_ref.pad2d_modes_grad(np.ones((1, 1, H + t + b, W + l + r), np.float32), (1, 1, H, W), pads, mh, mw)
    return m[0, 0][None, :, :, None] if case.layout == 'nhwc' else m


def check_adjoint(dx, dy, ref_grad, m, what):
    """dx (float32, from the kernel) against the float64 fold of dy.  m = the number of float32 summands of an element, S = the
    same fold of |dy|.  m == 1: the element is a copy, bit for bit.  Otherwise |dx - ref| <= gamma_m * S with
    gamma_m = m u / (1 - m u), u = 2^-24: the bound of m float32 additions in ANY order plus the final rounding."""
    ref = ref_grad(dy)
    m = np.broadcast_to(m, ref.shape)
    S = ref_grad(np.abs(dy))
    assert dx.shape == ref.shape and dx.dtype == np.float32
    one = m == 1
    assert np.array_equal(dx[one].astype(np.float64), ref[one]), what
    gamma = m * U / (1.0 - m * U)
    err = np.abs(dx.astype(np.float64) - ref)
    bad = err > gamma * S
    assert not bad.any(), (what, float(err[bad].max()), int(bad.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_pad2d_bwd_on_its_route_against_the_float64_adjoint(ops, case):
    lds, cu = device_numbers()
    rng = np.random.default_rng(len(case.name) + sum(case.shape))
    pool = {}                                   # gradients per padded shape: a few shapes serve all 25 mode pairs
    for mh, mw in MODE_PAIRS:
        pads = pads_for(case, mh, mw)
        pshape = padded_shape(case, pads)
        if pshape not in pool:
            pool[pshape] = (rng.standard_normal(pshape).astype(np.float32),
                            rng.integers(-1000, 1001, size=pshape).astype(np.float32))
        pad = ops.make_pad(*pads, mh, mw)
        for kind, dy in zip(('normal', 'integer'), pool[pshape]):
            dys = Slab(pshape, case.offs[1], dy)
            if case.offs[0]:
                dxs = Slab(case.shape, case.offs[0])
                dx_mod = dxs.mod16
            else:
                dxs, dx_mod = None, 0
            r = case_route(case, 'bwd', (mh, mw), lds, cu, (dx_mod, dys.mod16))
            assert tuple(r[:4]) == case.bwd, 'expected route %r, the dispatch gives %r (lds_bytes %d, %d CUs)' % (case.bwd, r, lds, cu)
            if dxs is not None:
                pad_bwd_into(ops, dys.t, dxs.t, case, pad)
                dx = dxs.read()
            else:
                t = ops.pad2d_bwd(dys.t, case.shape, pad, channels_last=case.layout == 'nhwc')
                assert t.data_ptr() % 16 == 0
                torch.cuda.synchronize()
                dx = t.cpu().numpy()
            assert np.array_equal(dys.read(), dy)

            def ref_grad(g):
                return ref_pad_grad(case, g, pads, mh, mw)
            if kind == 'integer':              # |dy| <= 1000, at most a few hundred summands: every partial sum is exact
                assert np.array_equal(dx.astype(np.float64), ref_grad(dy)), (pads, mh, mw, r)
            else:
                check_adjoint(dx, dy, ref_grad, summands(case, pads, mh, mw), (pads, mh, mw, r))


# ----------------------------------------------------------------------------------------------------------------- #
# 4. the forward above 1024 floats per row
# ----------------------------------------------------------------------------------------------------------------- #

@pytest.mark.gpu
@pytest.mark.parametrize('case', [c for c in CASES if c.fwd == REFUSED], ids=lambda c: c.name)
def test_pad2d_fwd_long_rows_launch_bit_exact_or_are_refused_untouched(ops, case):
    """Rows of more than 1024 floats never fit the flat kernel; the row-staged forward asks for 64 bytes of LDS per row float and
    is refused only against the handle's lds_bytes (halo.hip:713-715).  With lds_bytes = 65536 every case here is refused; with
    more, rows up to lds_bytes / 64 floats launch with a dynamic LDS request above 64 KB.  Whatever the device says: a case the
    restated dispatch sends to 'rows' must come out bit-exact, a refused one must raise the LDS message and leave the output
    alone.

    MEASURED on the MI355X: the handle reports lds_bytes = 163840.  (1, 1, 3, 1030) -> rows, V = 1, a dynamic LDS
    request of 66048 bytes; (1, 1, 3, 1440) -> rows, V = 1, 92160 bytes; both launch WITHOUT hipFuncSetAttribute and are bit-exact
    in all 25 mode pairs (so are the 1200-float channels-last rows and the misaligned variants); (1, 1, 3, 2600) -> refused
    (166400 bytes), output untouched.  No 64 KB guard was added to this route: it would refuse calls that work."""
    from dlwp_amd._lib import DlwpError
    lds, cu = device_numbers()
    x = distinct(case.shape)
    xs = Slab(case.shape, case.offs[0], x)
    for mh, mw in MODE_PAIRS:
        pads = pads_for(case, mh, mw)
        ys = Slab(padded_shape(case, pads), case.offs[1])
        r = case_route(case, 'fwd', (mh, mw), lds, cu, (xs.mod16, ys.mod16))
        if (mh, mw) == MODE_PAIRS[0]:
            print('%s %r: lds_bytes %d -> %s V=%d' % (case.name, case.shape, lds, r.family, r.vec))
        assert r.family in ('rows', 'refused'), r
        pad = ops.make_pad(*pads, mh, mw)
        if r.family == 'refused':
            with pytest.raises(DlwpError, match='does not fit in LDS'):
                ops.pad2d(xs.t, pad, channels_last=case.layout == 'nhwc', out=ys.t)
            assert ys.untouched()
        else:
            ops.pad2d(xs.t, pad, channels_last=case.layout == 'nhwc', out=ys.t)
            assert np.array_equal(ys.read(), ref_pad(case, x, pads, mh, mw)), (pads, mh, mw, r)


# ----------------------------------------------------------------------------------------------------------------- #
# 5. upsample2, maxpool2, copy_channels, series_merge_time
# ----------------------------------------------------------------------------------------------------------------- #

@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 3, 5, 6), (1, 1, 1, 2), (1, 2, 3, 1)])
def test_upsample2_pair_and_scalar_kernels(ops, shape):
    """even W, everything aligned: the pair kernels; the input 1 float or the output 2 floats off a 16-byte boundary, or an odd W:
    the scalar ones.  The forward copies; the backward's four-term sums of integers are exact: both bit for bit."""
    from dlwp_amd import _lib
    x = distinct(shape)
    want = np_ref.upsample2(x)
    for x_off, y_off in ((0, 0), (1, 0), (0, 2), (1, 2), (2, 0)):
        xs, ys = Slab(shape, x_off, x), Slab(want.shape, y_off)
        ops.upsample2(xs.t, out=ys.t)
        assert np.array_equal(ys.read(), want), (x_off, y_off)
    rng = np.random.default_rng(shape[-1])
    dy = rng.integers(-1000, 1001, size=want.shape).astype(np.float32)
    ref = np_ref.upsample2_grad(dy)
    for dy_off, dx_off in ((0, 0), (2, 0), (0, 1), (0, 2), (2, 1)):
        dys = Slab(dy.shape, dy_off, dy)
        if dx_off == 0:
            t = ops.upsample2_bwd(dys.t)
            torch.cuda.synchronize()
            dx = t.cpu().numpy()
        else:
            dxs = Slab(shape, dx_off)
            _lib.check(_lib.lib.dlwp_upsample2_bwd(_lib.handle(torch.cuda.current_device()), _vp(dys.t), _vp(dxs.t),
                                                   _lib.Shape4(*shape), _lib.F32, _stream()))
            dx = dxs.read()
        assert np.array_equal(dx.astype(np.float64), ref), (dy_off, dx_off)
        assert np.array_equal(dys.read(), dy)


@pytest.mark.gpu
def test_upsample2_refuses_a_4_byte_aligned_high_resolution_tensor(ops):
    from dlwp_amd._lib import DlwpError
    xs, ys = Slab((1, 2, 3, 4), 0, distinct((1, 2, 3, 4))), Slab((1, 2, 6, 8), 1)
    with pytest.raises(DlwpError, match='output must be 8-byte aligned'):
        ops.upsample2(xs.t, out=ys.t)
    assert ys.untouched()
    with pytest.raises(DlwpError, match='dy must be 8-byte aligned'):
        ops.upsample2_bwd(ys.t)


POOL_SHAPES = [(1, 2, 5, 6), (1, 2, 6, 5), (1, 2, 5, 5), (1, 1, 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', POOL_SHAPES)
def test_maxpool2_odd_maps_and_misaligned_pointers(ops, shape):
    """odd H and / or W: the last row / column is in no window and gets a zero gradient; (1, 1, 1, 1): the pooled map is empty"""
    n, c, h, w = shape
    rng = np.random.default_rng(h * 10 + w)
    x = rng.permutation(n * c * h * w).astype(np.float32).reshape(shape) - 7
    x[:, :, -1, :] += 100 * (h % 2)           # the rows / columns outside every window hold the largest values
    x[:, :, :, -1] += 100 * (w % 2)
    want = np_ref.maxpool2(x)
    dy = distinct(want.shape)
    dx_ref = np_ref.maxpool2_grad(x, dy)
    for x_off, y_off in ((0, 0), (1, 0), (0, 1), (1, 3)):
        xs = Slab(shape, x_off, x)
        if want.size:
            ys = Slab(want.shape, y_off)
            ops.maxpool2(xs.t, out=ys.t)
            assert np.array_equal(ys.read(), want), (x_off, y_off)
            dys = Slab(want.shape, y_off, dy).t
        else:
            y = ops.maxpool2(xs.t)
            assert tuple(y.shape) == want.shape
            dys = torch.empty(want.shape, dtype=torch.float32, device='cuda')
        t = ops.maxpool2_bwd(xs.t, dys)
        torch.cuda.synchronize()
        dx = t.cpu().numpy()
        assert np.array_equal(dx.astype(np.float64), dx_ref), (x_off, y_off)
        if h % 2:
            assert not dx[:, :, -1, :].any()
        if w % 2:
            assert not dx[:, :, :, -1].any()
        assert np.array_equal(xs.read(), x)


@pytest.mark.gpu
def test_maxpool2_bwd_ties_in_every_position_of_the_window(ops):
    """one window per non-empty subset of the four positions holding the (tied) maximum, plus an all-equal window, on an odd map:
    the gradient goes to the first maximum in row-major order"""
    x = np.full((1, 1, 9, 9), 50, np.float32)
    x[:, :, :8, :8] = -1
    for i in range(1, 16):
        r, cidx = 2 * (i // 4), 2 * (i % 4)
        for pos in range(4):
            if i >> pos & 1:
                x[0, 0, r + pos // 2, cidx + pos % 2] = 3
    dy = distinct((1, 1, 4, 4))
    ref = np_ref.maxpool2_grad(x, dy)
    got = ops.maxpool2_bwd(Slab(x.shape, 1, x).t, Slab(dy.shape, 1, dy).t)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(got.astype(np.float64), ref)
    assert (got != 0).sum() == 16 and not got[0, 0, 8].any() and not got[0, 0, :, 8].any()
    for i in range(1, 16):                    # the lowest set bit of the subset is the first maximum
        first = [pos for pos in range(4) if i >> pos & 1][0]
        assert got[0, 0, 2 * (i // 4) + first // 2, 2 * (i % 4) + first % 2] == dy[0, 0, i // 4, i % 4]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', POOL_SHAPES)
def test_maxpool2_bfloat16_odd_maps(ops, shape):
    """against float32 pooling of the widened values: the maximum of bfloat16 values is one of them"""
    rng = np.random.default_rng(sum(shape))
    xb = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda().to(torch.bfloat16)
    wide = xb.float().cpu().numpy()
    y = ops.maxpool2(xb)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == np_ref.maxpool2(wide).shape
    assert np.array_equal(y.float().cpu().numpy(), np_ref.maxpool2(wide))


def _copy_case(ops, n, c, h, w, src_total, src_off, dst_total, dst_off, src_shift=0, dst_shift=0):
    src = distinct((n, src_total, h, w))
    ss = Slab(src.shape, src_shift, src)
    ds = Slab((n, dst_total, h, w), dst_shift)
    ds.t.fill_(float('nan'))
    ops.copy_channels(ss.t, ds.t, c, src_off, dst_off)
    got = ds.read()
    assert np.array_equal(got[:, dst_off:dst_off + c], src[:, src_off:src_off + c])
    outside = np.ones(dst_total, bool)
    outside[dst_off:dst_off + c] = False
    assert np.isnan(got[:, outside]).all()
    assert np.array_equal(ss.read(), src)


@pytest.mark.gpu
def test_copy_channels_scalar_against_vector_route(ops):
    # hw = 6, channel offset 1: run 12, strides 24 and 36 -- every count a multiple of 4, the pointers 24 bytes in: scalar
    _copy_case(ops, 3, 2, 2, 3, 4, 1, 6, 1)
    _copy_case(ops, 3, 2, 2, 3, 4, 0, 6, 1)           # only the destination off the boundary
    _copy_case(ops, 3, 2, 2, 3, 4, 1, 6, 0)           # only the source
    # hw = 5, channel offset 4: the pointers 80 bytes in (aligned), the run of 15 floats is no multiple of 4: scalar
    _copy_case(ops, 2, 3, 1, 5, 8, 4, 9, 4)
    # the vector route with differing strides: hw = 8, offsets of 16 and 8 floats, strides 32 and 48
    _copy_case(ops, 3, 2, 2, 4, 4, 2, 6, 1)
    # the same counts, the source / the destination a view 1 or 2 floats off: scalar
    _copy_case(ops, 3, 2, 2, 4, 4, 2, 6, 1, src_shift=1)
    _copy_case(ops, 3, 2, 2, 4, 4, 2, 6, 1, dst_shift=2)


@pytest.mark.gpu
def test_copy_channels_second_grid_stride_trip(ops):
    """one copy of more than 8 * CUs * 256 threads * 4 floats: the vector kernel's grid is capped and its loop repeats"""
    _, cu = device_numbers()
    n, c, h, w = 4, 64, 96, 96
    assert n * c * h * w > 8 * cu * 256 * 4
    _copy_case(ops, n, c, h, w, 64, 0, 96, 16)


@pytest.mark.gpu
def test_series_merge_time_scalar_route_and_empty_series(ops):
    t, n, td, v, h, w = 3, 2, 2, 2, 2, 4             # run = v * h * w = 16: a multiple of 4
    s = distinct((t, n, td * v, h, w))
    want = np_ref._merge_time(s, t, n, td, (td * v, h, w), False)
    for off in (0, 1, 2):                            # off 0: the vector kernel; 1, 2: the input is misaligned, scalar
        ss = Slab(s.shape, off, s)
        got = ops.series_merge_time(ss.t, td)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want), off
        assert np.array_equal(ss.read(), s)
    for shape in ((0, n, td * v, h, w), (t, 0, td * v, h, w)):
        out = ops.series_merge_time(torch.empty(shape, dtype=torch.float32, device='cuda'), td)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (shape[0] * td, shape[1], v, h, w)
