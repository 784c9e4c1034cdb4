"""tests/conv_fwd_cases.py without a GPU: the exactness condition on the arrays every table row generates, a float32 restatement of
Winograd F(2x2, 3x3) that returns the float64 sums to the bit under that condition (the claim tests/test_gpu_conv_fwd.py rests on,
proved apart from any kernel), the reference's NaN masks under the poison patterns, and the table's form."""
import numpy as np
import pytest

from oracle import np_ref
from tests import conv_fwd_cases as cases

ROWS = cases.ROWS
IDS = [r['name'] for r in ROWS]

# F(2x2, 3x3) as in csrc/conv_fwd_wino_kernel.h (tests/test_conv_grads_cpu.py holds the weight-gradient form's matrices)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float32)
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float32)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float32)


def winograd_f32(row, x, w, b, act, pool):
    """the row's layer (dilation 1) on 2x2 output tiles, every operation in float32: U = G g G^T, V = B^T d B, M = sum_c U V,
    Y = A^T M A"""
    assert row['k'] == 3 and row['dil'] == 1
    xp = np_ref.pad2d_modes(cases.source(row, x), row['pads'], row['mh'], row['mw']).astype(np.float32)
    n, c, hp, wp = xp.shape
    ho, wo = hp - 2, wp - 2
    th, tw = -(-ho // 2), -(-wo // 2)
    full = np.zeros((n, c, 2 * th + 2, 2 * tw + 2), np.float32)
    full[:, :, :hp, :wp] = xp
    d = np.stack([np.stack([full[:, :, i:i + 2 * th:2, j:j + 2 * tw:2] for j in range(4)], -1) for i in range(4)], -2)
    u = np.einsum('ij,jkco,lk->ilco', G, np.asarray(w, np.float32), G)
    v = np.einsum('ij,nctsjk,lk->nctsil', BT, d, BT)
    m = np.einsum('nctsil,ilco->notsil', v, u)
    y = np.einsum('ij,notsjk,lk->notsil', AT, m, AT)
    assert u.dtype == v.dtype == m.dtype == y.dtype == np.float32
    y = y.transpose(0, 1, 2, 4, 3, 5).reshape(n, -1, 2 * th, 2 * tw)[:, :, :ho, :wo] + np.asarray(b, np.float32)[None, :, None, None]
    if act == 'relu':
        y = np.maximum(y, np.float32(0))
    if pool:
        y = np_ref.maxpool2(y)
    assert y.dtype == np.float32
    return y


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_exactness_measure_stays_below_the_limit(row):
    """on the very arrays the GPU test uploads (both seeds)"""
    for seed in (0, 1):
        x, w, b = cases.exact_inputs(row, seed)
        assert set(np.unique(x)) <= {-2., -1., 1., 2.} and np.all(w != 0) and np.all(b != 0)
        assert np.array_equal(np_ref.round_bf16(x), x) and np.array_equal(np_ref.round_bf16(w), w), 'exact in bfloat16'
        m = cases.exact_measure(row, x, w, b)
        assert 0 < m < cases.LIMIT, (row['name'], m)


@pytest.mark.parametrize('name', ['tiles-wino-k3d1', 'ragged-c13-d1-s1', 'flat-9x33'])
@pytest.mark.parametrize('act,pool', [('linear', False), ('relu', True)])
def test_float32_winograd_restatement_equals_the_float64_reference_to_the_bit(name, act, pool):
    row = cases.BY_NAME[name]
    x, w, b = cases.exact_inputs(row)
    assert cases.exact_measure(row, x, w, b) < cases.LIMIT
    want = cases.reference(row, x, w, b, act, pool)
    got = winograd_f32(row, x, w, b, act, pool)
    assert got.shape == want.shape == (cases.N,) + cases.out_shape(row, pool)
    assert np.array_equal(got.astype(np.float64), want)
    # and it is a statement about the integers: scaled so that the sums leave the 24 bits, the same code rounds
    big = winograd_f32(row, x * np.float32(2.0 ** 12 + 1), w * np.float32(2.0 ** 11 + 1), b, 'linear', False)
    ref = cases.reference(row, x * np.float32(2.0 ** 12 + 1), w * np.float32(2.0 ** 11 + 1), b, 'linear', False)
    assert not np.array_equal(big.astype(np.float64), ref)


@pytest.mark.parametrize('row', ROWS, ids=IDS)
@pytest.mark.parametrize('act', ['linear', 'relu'])
def test_reference_nan_masks_under_the_poison_patterns(row, act):
    """(p1): sample 1 all NaN, samples 0 and 2 as without it.  (p2): NaN exactly on the receptive-field footprint -- through the
    source transforms, the wrap / edge / reflect halos and a pooled epilogue --, NaN under relu and max-pool too, not 0."""
    x, w, b = cases.exact_inputs(row)
    pools = (False, True) if row['pools'] == 'auto' else row['pools']
    for pool in pools:
        clean = cases.reference(row, x, w, b, act, pool)
        assert np.isfinite(clean).all()
        p1 = cases.reference(row, cases.poison_p1(x), w, b, act, pool)
        assert np.isnan(p1[1]).all() and np.array_equal(p1[[0, 2]], clean[[0, 2]])
        p2 = cases.reference(row, cases.poison_p2(row, x), w, b, act, pool)
        assert np.array_equal(p2[[0, 2]], clean[[0, 2]])
        nan = np.isnan(p2[1])
        foot = cases.footprint(row, pool)
        if row['d2s']:                                           # every phase channel of a poisoned pixel: its whole 2x2 block
            foot = foot.repeat(2, axis=0).repeat(2, axis=1)
        assert foot.any() and not foot.all()
        assert np.array_equal(nan, np.broadcast_to(foot, nan.shape)), (row['name'], act, pool, int(nan[0].sum()), int(foot.sum()))
        assert np.array_equal(p2[1][~nan], clean[1][~nan])


def test_footprint_cases_cover_sources_halos_and_pooling():
    seen = set()
    for row in ROWS:
        seen.add(('src', row['src']))
        seen.add(('mode', row['mh']))
        seen.add(('mode', row['mw']))
        if row['pools'] != (False,):
            seen.add('pooled')
    assert {('src', 0), ('src', 1), ('src', 2), ('mode', 0), ('mode', 1), ('mode', 2), ('mode', 3), 'pooled'} <= seen


def test_table_is_well_formed():
    assert len(set(IDS)) == len(IDS)
    for row in ROWS:
        assert cases.halos_fit(row), row['name']
        assert (row['route'] is None) != (row['force'] is None), row['name']
        assert row['route'] is None or isinstance(row['route'], str) or row['route'] < 0
        c, ho, wo = cases.out_shape(row, False)
        assert c > 0 and ho > 1 and wo > 1
        for extra in (cases.EXTRA, 8):
            wide = cases.store_wide(np.zeros((cases.N, row['cin'], 2, 2), np.float32), extra, np.nan)
            assert wide.shape[1] == row['cin'] + 2 * extra and np.isnan(wide[:, :extra]).all() and np.isnan(wide[:, -extra:]).all()
            assert not np.isnan(wide[:, extra:extra + row['cin']]).any()
        # every tensor of the GPU test stays small
        e2 = 2 * cases.extra_of(row)
        assert 4 * cases.N * (row['cin'] + e2) * row['h'] * row['w'] < 1.5e6 and 4 * cases.N * (c + e2) * ho * wo < 1.5e6, row['name']
    ch, pix = cases.p2_pixels(ROWS[0])
    assert pix[0] == (0, 0) and 0 < pix[1][0] < ROWS[0]['h'] - 1 and 0 < pix[1][1] < ROWS[0]['w'] - 1


def test_forced_rows_partition_a_registry():
    """forced_configs on a registry as the library reports it (the shape of ops.conv_configs()): every plain instance belongs to
    exactly one forced row of its geometry, cell-update instances to none"""
    lds = 0
    reg = [(3, 1, 8, 32, 4, 4, 2, 16, 0, lds, 0), (3, 1, 8, 32, 4, 4, 2, 8, 1, lds, 0), (3, 1, 8, 64, 4, 2, -4, 8, 0, lds, 0),
           (3, 1, 8, 32, 4, 0, 2, 8, 0, lds, 32), (3, 1, 8, 32, 4, 0, 4, 8, 0, lds, 32), (3, 1, 8, 32, 4, 0, 1, 8, 0, lds, 1),
           (3, 1, 8, 32, 4, 0, 1, 8, 0, lds, 5), (3, 1, 8, 32, 4, 4, 2, 32, 2, lds, 0), (3, 1, 8, 32, 4, 4, 2, 16, 3, lds, 0),
           (3, 2, 8, 32, 4, 4, 2, 8, 3, lds, 0), (3, 1, 8, 32, 4, 4, 2, 32, 2, lds, 24), (3, 1, 8, 32, 4, 4, 2, 16, 3, lds, 16),
           (3, 1, 8, 32, 4, 4, 4, 16, 3, lds, 2), (3, 1, 8, 32, 4, 4, 4, 16, 2, lds, 26)]
    fams = [cases.family_of(c) for c in reg]
    assert fams == ['direct', 'pooled-loader', 'packed-n', 'wino', 'wino', 'wino-split', 'wino', 'bf16', 'bf16', 'bf16', 'octet',
                    'octet', 'cell-update', 'cell-update']
    owners = [[r['name'] for r in ROWS if r['force'] and 'tile' not in r['force'] and i in cases.forced_configs(r, reg)]
              for i in range(len(reg))]
    assert all(len(o) == 1 for o in owners[:12]) and owners[12] == owners[13] == [], owners
