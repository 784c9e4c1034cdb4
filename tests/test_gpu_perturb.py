"""The ensemble member generator on the device (csrc/perturb.hip behind dlwp_amd.ops.ens_perturb and dlwp_amd.model.ensemble) against
the independent float64 restatement of tests/perturb_cases.py.

Required, per tensor: with x = 0 the output is the perturbation p and |got - want| <= 1e-5 max|want| (the FWD_TOL form of
tests/test_gpu_eltwise.py; the float32 evaluation of the Box-Muller pair sits at about 3 % of it); with x != 0 the bar gains
2^-24 |x + p| for the final sum.  Every call writes into a NaN-filled buffer between NaN guards, runs twice (identical bits), with
operands 0 to 3 floats past a 16-byte boundary.  Sizes: widths and heights around the 32 x 64 tile of the smoothed path (31, 33, 63,
65), quads cut by the end of a row (5, 7, 45), radii 0, 1, 6, 16 including R_y > H and R_x = W, 1 to 33 members (33 splits into
member chunks on the white path).  Run with -s to see error / bound of every case."""
import numpy as np
import pytest
import torch

from dlwp_amd import ops
from dlwp_amd.model import ensemble
from tests import perturb_cases as pc
from tests.nets import cnn2_layers

pytestmark = pytest.mark.gpu

GUARD = 64
#: correlation lengths with R = ceil(3 L) = 0, 1, 6, 16
LEN = {0: 0.0, 1: 0.3, 6: 2.0, 16: 5.3}


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def bits(t):
    return t.contiguous().view(torch.int32)


def place(a, off):
    """a (numpy float32) on the device, `off` floats past a 16-byte boundary"""
    a = np.array(a, dtype=np.float32)                    # a copy: a broadcast view is not writable
    store = torch.empty(a.size + 8, dtype=torch.float32, device='cuda')
    assert store.data_ptr() % 16 == 0
    t = store[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * off
    return t


def guarded(numel, off):
    """a NaN-filled buffer of numel floats, `off` floats past a 16-byte boundary, between two NaN guards"""
    store = torch.full((numel + 2 * GUARD + 4,), float('nan'), dtype=torch.float32, device='cuda')
    assert store.data_ptr() % 16 == 0
    return store, store[GUARD + off:GUARD + off + numel]


def generate(x, sigma, members, lengths, offs=(0, 0, 0), **kw):
    """ops.ens_perturb twice into guarded buffers; returns the device result (S, M, K, H, W) or (M, S, K, H, W)"""
    taps_y, taps_x = ensemble.smoothing_taps(lengths[0])[1], ensemble.smoothing_taps(lengths[1])[1]
    xd = place(x, offs[0])
    sd = place(np.broadcast_to(np.asarray(sigma, np.float32), (x.shape[1],)), offs[1])
    runs = []
    for _ in range(2):
        store, out = guarded(x.size * members, offs[2])
        res = ops.ens_perturb(xd, sd, members, taps_y=taps_y, taps_x=taps_x, out=out, **kw)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        n = out.numel()
        assert torch.isnan(store[:GUARD + offs[2]]).all() and torch.isnan(store[GUARD + offs[2] + n:]).all()      # nothing outside
        runs.append(res)
    assert torch.equal(bits(runs[0]), bits(runs[1]))
    return runs[0]


#: (S, K, H, W), M, (R_y, R_x), control, antithetic, first_member, member_axis, (x, sigma, out) offsets
CASES = [
    ((1, 1, 1, 5), 1, (0, 0), False, False, 0, 2, (0, 0, 0)),
    ((2, 3, 2, 7), 2, (0, 0), True, False, 0, 2, (1, 2, 3)),
    ((1, 3, 9, 45), 5, (0, 0), True, True, 2, 1, (0, 0, 0)),
    ((2, 1, 9, 180), 33, (0, 0), True, True, 0, 2, (0, 1, 0)),          # 16-byte accesses, four member chunks
    ((2, 1, 9, 180), 33, (0, 0), False, False, 7, 1, (0, 0, 2)),        # the same row length on the element path
    ((1, 1, 1, 5), 2, (1, 1), False, False, 0, 2, (3, 0, 1)),           # R_y > H
    ((2, 3, 2, 7), 5, (6, 6), True, True, 0, 2, (0, 0, 0)),             # R_y > H, quads cut by the wrap on both sides
    ((1, 1, 9, 45), 2, (16, 16), True, False, 0, 1, (2, 3, 0)),
    ((1, 3, 9, 180), 5, (6, 1), True, False, 4, 2, (0, 0, 0)),          # three column tiles, the last 52 wide
    ((1, 1, 33, 65), 2, (6, 6), False, True, 0, 2, (1, 0, 0)),          # one row and one column past the tile
    ((1, 1, 31, 63), 1, (1, 6), False, False, 0, 2, (0, 0, 3)),         # one short of it
    ((1, 1, 2, 16), 2, (0, 16), False, False, 0, 2, (0, 0, 0)),         # R_x = W: every column twice in the halo
    ((2, 1, 9, 6), 2, (1, 6), True, False, 0, 1, (0, 2, 0)),            # R_x = W
    ((1, 1, 2, 7), 33, (1, 1), True, True, 0, 2, (0, 0, 1)),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s-M%d-R%d.%d' % ('x'.join(map(str, c[0])), c[1], c[2][0], c[2][1]))
def test_perturbation_against_float64(case):
    dims, members, radii, control, antithetic, first, member_axis, offs = case
    lengths = (LEN[radii[0]], LEN[radii[1]])
    sigma = (0.5 + 0.25 * np.arange(dims[1])).astype(np.float32)
    kw = dict(first_member=first, seed=2016 + members, control=control, antithetic=antithetic, member_axis=member_axis)
    want = pc.perturbation64(dims, members, sigma, lengths, 2016 + members, control, antithetic, first)

    def second(t):
        return t.cpu().numpy().astype(np.float64) if member_axis == 2 else np.moveaxis(t.cpu().numpy().astype(np.float64), 0, 1)
    got = second(generate(np.zeros(dims, np.float32), sigma, members, lengths, offs, **kw))
    bar = 1e-5 * np.abs(want).max()
    err = np.abs(got - want).max()
    print('x = 0: error / bound %.3f' % (err / bar if bar else 0.0))
    assert not np.isnan(got).any() and err <= bar
    x = np.random.default_rng(members).standard_normal(dims).astype(np.float32)
    got = second(generate(x, sigma, members, lengths, offs, **kw))
    full = x.astype(np.float64)[:, None] + want
    ratio = np.abs(got - full) / (bar + 2.0 ** -24 * np.abs(full))
    print('x != 0: error / bound %.3f' % ratio.max())
    assert not np.isnan(got).any() and ratio.max() <= 1.0
    if control and first == 0:
        assert np.array_equal(got[:, 0].astype(np.float32).view(np.int32), x.view(np.int32))


@pytest.mark.parametrize('length', [0.0, (0.0, 2.0)], ids=['white', 'smoothed'])
def test_dense_state(length):
    """(2, 1030): one channel, one row of 1030 = 16 tiles + 6 columns"""
    want = pc.perturbation64((2, 1, 1, 1030), 5, 0.25, length, 3)
    got = ensemble.perturb_members(torch.zeros((2, 1030), device='cuda'), 5, stddev=0.25, length=length, seed=3)
    assert got.is_cuda and tuple(got.shape) == (10, 1030)
    err, bar = np.abs(got.cpu().numpy().reshape(want.shape) - want).max(), 1e-5 * np.abs(want).max()
    print('dense: error / bound %.3f' % (err / bar))
    assert err <= bar
    host = ensemble.perturb_members(np.zeros((2, 1030), np.float32), 5, stddev=0.25, length=length, seed=3)
    assert np.abs(host.reshape(want.shape) - want).max() <= bar


@pytest.mark.parametrize('radii', [(0, 0), (1, 6)], ids=['white', 'smoothed'])
@pytest.mark.parametrize('width', [8, 7])
def test_bit_for_bit_identities(radii, width):
    dims = (2, 3, 9, width)
    lengths = (LEN[radii[0]], LEN[radii[1]])
    rng = np.random.default_rng(31)
    x = rng.standard_normal(dims).astype(np.float32)
    sigma = np.array([0.5, 0.1, 2.0], np.float32)
    zero = np.zeros(dims, np.float32)
    full = generate(x, sigma, 8, lengths, seed=5)
    assert torch.equal(bits(full[:, 0]), bits(torch.from_numpy(x).cuda()))                                  # the control member
    assert not torch.equal(full[:, 1], full[:, 0])
    still = generate(x, 0.0, 3, lengths, seed=5)                                                           # stddev 0
    assert all(torch.equal(bits(still[:, m]), bits(full[:, 0])) for m in range(3))
    anti = generate(zero, sigma, 7, lengths, seed=5, antithetic=True)                                      # +/- pairs at x = 0
    for m in (1, 3, 5):
        assert torch.equal(bits(anti[:, m + 1]), bits(-anti[:, m])) and float(anti[:, m].abs().max()) > 0
    a = generate(x, sigma, 3, lengths, seed=5)                                                             # [0, 8) = [0, 3) + [3, 8)
    b = generate(x, sigma, 5, lengths, seed=5, first_member=3)
    assert torch.equal(bits(torch.cat([a, b], dim=1)), bits(full))
    pa = generate(x, sigma, 4, lengths, seed=5, antithetic=True)                                           # a split inside a pair
    pb = generate(x, sigma, 4, lengths, seed=5, antithetic=True, first_member=4)
    assert torch.equal(bits(torch.cat([pa, pb], dim=1)), bits(generate(x, sigma, 8, lengths, seed=5, antithetic=True)))
    first = generate(x, sigma, 8, lengths, seed=5, member_axis=1)                                          # the two layouts
    assert tuple(first.shape) == (8,) + dims and torch.equal(bits(first.transpose(0, 1)), bits(full))
    for offs in ((1, 0, 0), (0, 0, 2), (3, 1, 1)):                                                         # misaligned operands
        assert torch.equal(bits(generate(x, sigma, 8, lengths, offs, seed=5)), bits(full))
    assert not torch.equal(generate(x, sigma, 8, lengths, seed=6)[:, 1], full[:, 1])                       # the seed matters


def test_nan_stays_local_and_the_public_paths_agree():
    x = np.random.default_rng(41).standard_normal((2, 2, 1, 6, 9)).astype(np.float32)                      # (S, time, var, H, W)
    x[1, 0, 0, 2, 3] = np.nan
    for length in (0.0, 1.0):
        dev = ensemble.perturb_members(torch.from_numpy(x).cuda(), 4, stddev=[0.1, 0.2], length=length, seed=8)
        assert dev.is_cuda and tuple(dev.shape) == (8, 2, 1, 6, 9)
        nan = torch.isnan(dev.view(2, 4, 2, 1, 6, 9))
        assert int(nan.sum()) == 4 and bool(nan[1, :, 0, 0, 2, 3].all())
        up = ensemble.perturb_members(x, 4, stddev=[0.1, 0.2], length=length, seed=8, device='cuda')       # numpy in, device out
        assert up.is_cuda and torch.equal(bits(torch.nan_to_num(up)), bits(torch.nan_to_num(dev)))
        host = ensemble.perturb_members(x, 4, stddev=[0.1, 0.2], length=length, seed=8)
        # the host's z is the float64 pair rounded once, the kernel evaluates the pair in float32: a few roundings of max|z| apart
        assert np.nanmax(np.abs(host - dev.cpu().numpy())) <= 0.2 * 1e-5 * 5.77
    with pytest.raises(ValueError, match='more than one wrap'):
        ensemble.perturb_members(torch.from_numpy(x).cuda(), 2, length=(0.0, 3.2))
    with pytest.raises(ValueError, match='sigma holds'):
        ops.ens_perturb(torch.zeros((1, 2, 3, 4), device='cuda'), torch.ones(3, device='cuda'), 2)


def test_ensemble_forecast_generates_rolls_out_and_feeds_the_scores():
    """tests.nets.cnn2_layers on an 8 x 12 grid, 2 samples x 5 members, 3 steps: equal, bit for bit, to perturb_members plus
    predict_timeseries composed by hand; both views; scored where it is"""
    from dlwp_amd.model import DLWPNeuralNet
    np.random.seed(0)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=1, scaler_type=None, scale_targets=False)
    d.build_model(cnn2_layers((4, 8, 12)), loss='mse', optimizer='adam')
    rng = np.random.default_rng(51)
    x0 = rng.standard_normal((2, 4, 8, 12)).astype(np.float32)
    kw = dict(stddev=0.05, length=1.0, seed=9)
    ens = ensemble.ensemble_forecast(d, x0, 3, 5, **kw).clone()          # a device series may live in the rollout's own buffer
    assert ens.is_cuda and tuple(ens.shape) == (3, 2, 5, 4, 8, 12)
    members = ensemble.perturb_members(x0, 5, device='cuda', **kw)
    assert tuple(members.shape) == (10, 4, 8, 12)
    by_hand = d.predict_timeseries(members, 3, return_device=True)
    assert torch.equal(bits(ens), bits(by_hand.view(3, 2, 5, 4, 8, 12)))
    assert torch.equal(bits(ens[0, :, 0]), bits(d.predict_timeseries(x0, 1, return_device=True)[0]))       # the control member
    first = ensemble.ensemble_forecast(d, torch.from_numpy(x0).cuda(), 3, 5, member_axis=1, **kw).clone()
    assert tuple(first.shape) == (3, 5, 2, 4, 8, 12)
    hand1 = d.predict_timeseries(ensemble.perturb_members(x0, 5, member_axis=1, device='cuda', **kw), 3, return_device=True)
    assert torch.equal(bits(first), bits(hand1.view(3, 5, 2, 4, 8, 12)))
    valid = ens.mean(dim=2) + 0.05 * torch.from_numpy(rng.standard_normal((3, 2, 4, 8, 12)).astype(np.float32)).cuda()
    for forecast, axis in ((ens, 2), (first, 1)):
        res = ensemble.ensemble_scores(forecast, valid, member_axis=axis)
        assert res.count.tolist() == [2 * 4 * 8 * 12] * 3 and res.rank_hist.shape == (3, 6)
        assert (res.rank_hist.sum(axis=-1) == res.count).all()
        assert np.isfinite(res.crps).all() and (res.spread > 0).all()
