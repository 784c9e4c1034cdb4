"""The case table of the pinned RowConnected2D suite (tests/rowconv_cases.py), checked without a GPU: every row's geometry, the
exactness condition of family (a), the float64 oracle on exact inputs against its own float32 rounding, and the ROUTES -- the
host-only launch report (dlwp_rowconv2d_launch_info, the decision the three entry points launch from) names the instance each row
names, the table reaches every compiled instance, every vector kernel and every fall-back reason, and a sweep over the planners'
inputs never sees an instance outside the compiled set."""
import ctypes

import numpy as np
import pytest

from dlwp_amd import _lib, ops
from tests import rowconv_cases as rc

ROW_IDS = [r['name'] for r in rc.ROWS]


@pytest.mark.parametrize('row', rc.ROWS, ids=ROW_IDS)
def test_geometry_is_valid(row):
    (H, W), (Hp, Wp), (ho, wo) = rc.geometry(row)
    kh, kw = row['k']
    t, b, l, r = row['pads']
    assert ho >= 1 and wo >= 1 and row['n'] >= 1
    for pad_lo, pad_hi, size, mode in ((t, b, H, row['modes'][0]), (l, r, W, row['modes'][1])):
        assert 0 <= mode <= 4
        assert max(pad_lo, pad_hi) <= (size - 1 if mode == 3 else size)      # a mirror halo without the border needs one more
    for (off, total), c in ((row['in_win'], row['cin']), (row['out_win'], row['cout'])):
        assert 0 <= off and off + c <= total
    cd, xs = rc.descriptor(ops, row)
    ys = ops.conv_out_shape(_lib.Shape4(*xs), cd)                            # the library agrees
    assert (ys.n, ys.c, ys.h, ys.w) == (row['n'], row['cout'], ho, wo)
    assert (row['expect']['dgrad'] is None) == bool(row['src'])              # no data gradient through the up-sampling loader
    d = rc.inputs(row, 'exact')
    assert d['x'].shape == (row['n'], row['in_win'][1], row['h'], row['w']) and d['dz'].shape == (row['n'], row['out_win'][1], ho, wo)
    assert d['k'].shape == (ho, kh, kw, row['cin'], row['cout']) and (d['bias'] is not None) == row['bias']


def test_the_table_has_the_rows_the_suite_relies_on():
    names = set(ROW_IDS)
    assert len(names) == len(ROW_IDS)
    windowed = [r for r in rc.ROWS if r['in_win'][0] > 0 and r['in_win'][0] + r['cin'] < r['in_win'][1] and
                r['out_win'][0] > 0 and r['out_win'][0] + r['cout'] < r['out_win'][1]]
    assert len(windowed) >= 3                                                # foreign channels in front of AND behind both windows
    assert any(r['src'] == 1 for r in rc.ROWS) and any(r['n'] == 1 for r in rc.ROWS)
    assert any(set(r['modes']) & {3, 4} and len(set(r['pads'])) > 2 and r['extra'].get('dgrad_fold') for r in rc.ROWS)
    b5 = rc.row_named('batch5-groups')                                       # more samples than a workgroup takes, a ragged last group
    for p in ('fwd', 'dgrad'):
        s = b5['extra'][p + '_samples']
        assert b5['n'] > s and b5['n'] % s != 0


@pytest.mark.parametrize('row', rc.ROWS, ids=ROW_IDS)
def test_exact_family_stays_inside_float32(row):
    """every pass: the worst sum of |terms| is below LIMIT / ROOM units, the inputs are multiples of the unit -- and the float64
    oracle's results on these inputs survive a round trip through float32 bit for bit"""
    d = rc.inputs(row, 'exact')
    for key in ('x', 'dz', 'k', 'dw0', 'db0'):
        assert np.array_equal(d[key], np.round(d[key]))
    if d['bias'] is not None:
        assert np.array_equal(d['bias'] / rc.BIAS_UNIT, np.round(d['bias'] / rc.BIAS_UNIT))
    cond = rc.exact_condition(row)
    assert set(cond) == {p for p in rc.PASSES if row['expect'][p] is not None}
    for p, c in cond.items():
        assert 0 < c <= rc.LIMIT / rc.ROOM, (p, c)
    assert rc.amplitude(row) >= 2                                            # (integers that use more than a sign)
    for act in ('linear', 'relu'):
        ref = rc.reference(row, 'exact', act)
        for key, v in ref.items():
            if v is not None:
                assert np.array_equal(v.astype(np.float32).astype(np.float64), v), (act, key)
                assert np.isfinite(v).all()


@pytest.mark.parametrize('row', rc.ROWS, ids=ROW_IDS)
def test_launch_report_names_the_rows_instance(row):
    rep = rc.reports(ops, row)
    for p, info in rep.items():
        assert rc.instance_name(p, info) == row['expect'][p], (p, info)
        assert info['grid'] >= 1 and info['block'] in (128, 256)
        assert (info['lds'] > 0) == (info['kind'] == 'mfma') and info['lds'] <= 96 * 1024
        assert ops.rowconv2d_uses_matrix_cores(rc.descriptor(ops, row)[1], rc.descriptor(ops, row)[0], rc.PASSES.index(p)) == \
            (info['kind'] == 'mfma')
        if info['kind'] == 'mfma':
            rows_of_grid = {'fwd': rc.geometry(row)[2][0], 'wgrad': rc.geometry(row)[2][0] * row['k'][0],
                            'dgrad': row['h'] if info['circ'] else rc.geometry(row)[1][0]}[p]
            assert info['grid'] == rows_of_grid * info['n_cb'] * info['n_sg'] * info['n_cg'] * info['n_mg']
        if p != 'dgrad':
            assert not info['circ'] and not info['fold']
        else:
            assert info['fold'] == (any(row['pads']) and not info['circ'])
    for key, want in row['extra'].items():
        p, field = key.split('_', 1)
        assert rep[p][field] == want, (key, rep[p])


def test_table_reaches_every_instance_and_every_fall_back_reason():
    seen = {p: set() for p in rc.PASSES}
    for row in rc.ROWS:
        for p, info in rc.reports(ops, row).items():
            seen[p].add(rc.instance_name(p, info))
        for p, info in rc.reports(ops, row, n=0).items():                   # the empty batch of every row
            assert rc.instance_name(p, info) == '%s_simple: empty batch' % p
            assert info['grid'] == (0 if p != 'wgrad' else max(1, -(-rc.inputs(row, 'exact')['k'].size // 256)))
            seen[p].add(rc.instance_name(p, info))
    for p, xs, cout, k, pads in rc.OFFSET_PROBES:                            # tensors of 2 GB: the report only
        cd = ops.make_conv(cout, k[0], k[1], 1, ops.make_pad(*pads))
        seen[p].add(rc.instance_name(p, ops.rowconv2d_launch_info(xs, cd, rc.PASSES.index(p))))
    assert rc.UNREACHABLE == []
    for p in rc.PASSES:
        want = set(rc.COMPILED[p]) | {'%s_simple: %s' % (p, why) for why in rc.REASONS[p]}
        assert seen[p] == want, (p, sorted(want - seen[p]), sorted(seen[p] - want))


def test_compiled_set_is_the_dispatch_of_the_source():
    """COMPILED lists exactly the instances the entry points of csrc/rowconv.hip can launch"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'rowconv.hip')).read()
    src = src.replace('kMaxSlots', str(rc.K_MAX_SLOTS))
    found = {p: set() for p in rc.PASSES}
    for p, a, b in re.findall(r'launch\(rowconv2d_(fwd|wgrad)_mfma<(\d+), (\d+)>\)', src):
        found[p].add('%s_mfma<%s,%s>' % (p, a, b))
    for a in re.findall(r'hipLaunchKernelGGL\(rowconv2d_dgrad_mfma<(\d+)>', src):
        found['dgrad'].add('dgrad_mfma<%s>' % a)
    assert found == {p: set(v) for p, v in rc.COMPILED.items()}


def test_no_geometry_of_the_sweep_names_an_instance_outside_the_compiled_set():
    """Cout 1 .. 64, Wo 1 .. 512, Cin in {1, 4, 5, 8, 64}, kh 1 .. 5, N in {1, 2, 7} (3 kernel columns, no halo): the forward report
    names the five compiled instances and its vector kernel, never <kMaxSlots, 2> -- more than 4 column slots leave plan_fwd 4 planes
    per staging round, i.e. one sample of 4 channels, never 8.  The gradients, on every 7th width: compiled instances only."""
    fn = _lib.lib.dlwp_rowconv2d_launch_info
    info = _lib.RowconvLaunchInfo()
    pinfo = ctypes.byref(info)
    seen = {p: set() for p in rc.PASSES}
    for cout in range(1, 65):
        for kh in range(1, 6):
            cd = ops.make_conv(cout, kh, 3)
            pcd = ctypes.byref(cd)
            for cin in (1, 4, 5, 8, 64):
                for n in (1, 2, 7):
                    for wo in range(1, 513):
                        xs = _lib.Shape4(n, cin, kh + 1, wo + 2)
                        assert fn(None, xs, pcd, 0, pinfo) == 0
                        seen['fwd'].add((info.kind, info.targ[0], info.targ[1], info.reason))
                        if wo % 7 == 1:
                            for which in (1, 2):
                                assert fn(None, xs, pcd, which, pinfo) == 0
                                seen[rc.PASSES[which]].add((info.kind, info.targ[0], info.targ[1], info.reason))
    names = {p: {rc.instance_name(p, dict(kind='mfma' if k else 'simple', targ=(a, b), reason=ops.ROWCONV_REASONS[why]))
                 for (k, a, b, why) in v} for p, v in seen.items()}
    for p in rc.PASSES:
        allowed = set(rc.COMPILED[p]) | {'%s_simple: %s' % (p, why) for why in rc.REASONS[p]}
        assert names[p] <= allowed, (p, sorted(names[p] - allowed))
    assert set(rc.COMPILED['fwd']) <= names['fwd']                          # (the sweep is wide enough to see all five)
    assert 'fwd_mfma<%d,2>' % rc.K_MAX_SLOTS not in names['fwd']


def test_launch_report_validates_without_a_device():
    cd = ops.make_conv(4, 3, 3)
    with pytest.raises(_lib.DlwpError):
        ops.rowconv2d_launch_info((1, 4, 8, 8), cd, 3)                       # no such pass
    with pytest.raises(_lib.DlwpError):
        ops.rowconv2d_launch_info((1, 4, 8, 8), ops.make_conv(4, 3, 3, 2), 0)          # dilation 2: not a row-connected layer
    with pytest.raises(_lib.DlwpError):
        ops.rowconv2d_launch_info((1, 4, 8, 8), ops.make_conv(4, 3, 3, src_mode=ops.SRC_UPSAMPLE2), 1)     # no data gradient there
    assert ops.rowconv2d_launch_info((1, 4, 8, 8), ops.make_conv(4, 3, 3, src_mode=ops.SRC_UPSAMPLE2), 2)['kind'] == 'mfma'
