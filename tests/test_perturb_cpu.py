"""The ensemble member generator without a GPU: the numpy statement of the definition in dlwp_amd/model/ensemble.py
against Random123's known answers, against the independent float64 restatement of tests/perturb_cases.py, its statistics, its
bit-level identities and its refusals; and the C ABI of dlwp_ens_perturb as far as it answers without a device."""
import math
import os
import re

import numpy as np
import pytest

from dlwp_amd import _lib, ops
from dlwp_amd.model import ensemble
from tests import perturb_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: Random123 kat_vectors, philox4x32 10 rounds: (counter, key, expected)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_philox_known_answers():
    for c, k, want in KAT:
        assert tuple(int(v) for v in ensemble.philox4x32_10(c, k)) == want
        assert pc.philox(c, k) == want                              # the restatement's own rounds
        assert tuple(int(v) for v in pc.philox_np(np.uint64(c[0]), c[1], c[2], c[3], k[0], k[1])) == want
    # vectorised over the first counter word: element n is the scalar answer of counter (n, 7, 8, 9)
    w = ensemble.philox4x32_10((np.arange(5), 7, 8, 9), (1, 2))
    for n in range(5):
        assert tuple(int(v[n]) for v in w) == pc.philox((n, 7, 8, 9), (1, 2))


def test_uniforms_are_float32_values_and_normals_are_bounded():
    words = np.array([0, 1, 255, 256, 511, 512, 0x7fffffff, 0x80000000, 0xfffffe00, 0xffffffff], np.uint32)
    rng = np.random.default_rng(5)
    words = np.concatenate([words, rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)])
    u1, u2 = ensemble.pair_uniforms(words, words)
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    assert u1.min() == 2.0 ** -24 and u1.max() == 1.0 - 2.0 ** -24 and u2.min() == 0.0 and u2.max() == 1.0 - 2.0 ** -24
    top = math.sqrt(48.0 * math.log(2.0))
    assert abs(top - 5.77) < 0.01 and math.sqrt(-2.0 * math.log(u1.min())) <= top * (1 + 1e-15)
    z = ensemble.white_noise(3, 0, 0, 0, np.arange(-16, 104), 180)
    assert np.isfinite(z).all() and np.abs(z).max() <= top


def test_white_noise_equals_the_restatement():
    for seed, d, s, k, rows, width in [(0, 0, 0, 0, range(3), 8), (2016, 5, 1, 2, range(-16, 4), 7), ((1 << 63) + 12345, 70000, 3, 65535, [-32767, 0, 32767], 45)]:
        got = ensemble.white_noise(seed, d, s, k, np.asarray(list(rows)), width)
        want = pc.white64(seed, d, s, k, list(rows), width)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize('length', [0.0, 0.3, 2.0, (5.0, 0.0), (0.0, 1.7), (4.0, 1.0)], ids=str)
def test_host_path_equals_the_restatement(length):
    """x = 0, sigma = 1: the output is zeta.  White noise is the float64 value rounded once; smoothed fields are within the float32
    accumulation bound of perturb_cases.smoothing_bound."""
    dims = (2, 3, 9, 7)
    got = ensemble.perturb_members(np.zeros(dims, np.float32), 4, length=length, seed=11, control=False).reshape((2, 4) + dims[1:])
    want = pc.perturbation64(dims, 4, 1.0, length, 11, control=False)
    ly, lx = length if isinstance(length, tuple) else (length, length)
    if ly == 0.0 and lx == 0.0:
        assert np.array_equal(got, want.astype(np.float32))
        assert np.abs(got - want).max() <= 2.0 ** -24 * np.abs(want).max()
    else:
        err, bound = np.abs(got - want).max(), pc.smoothing_bound(ly, lx)
        print('length %s: error %.3g, bound %.3g' % (length, err, bound))
        assert err <= bound


@pytest.mark.parametrize('seed', [0, 1, 2016])
def test_white_statistics(seed):
    z = np.concatenate([ensemble.white_noise(seed, d, 0, 0, np.arange(88), 180).ravel() for d in range(16)])
    n = z.size
    assert n == 16 * 88 * 180
    print('seed %d: mean %.2f, var %.2f sigma units' % (seed, z.mean() * math.sqrt(n), (z.var() - 1) / math.sqrt(2.0 / n)))
    assert abs(z.mean()) <= 4.0 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 4.0 * math.sqrt(2.0 / n)


def test_smoothed_statistics():
    """L = 2 over 64 draws of 88 x 180: unit variance and the lag-1 autocorrelation sum g_a g_{a+1} on both axes, within
    4 sqrt(2 (2R + 1)^2 / n) (a smoothed field has about n / (2R + 1)^2 independent values)"""
    x = np.zeros((1, 1, 88, 180), np.float32)
    f = ensemble.perturb_members(x, 64, length=2.0, seed=0, control=False).reshape(64, 88, 180).astype(np.float64)
    radius, g = ensemble.smoothing_taps(2.0)
    assert radius == 6 and abs(float((g.astype(np.float64) ** 2).sum()) - 1.0) < 1e-6
    n = f.size
    bound = 4.0 * math.sqrt(2.0 * (2 * radius + 1) ** 2 / n)
    g64 = g.astype(np.float64)
    theory = float((g64[:-1] * g64[1:]).sum())
    var = (f * f).mean()
    lag_y = (f[:, 1:] * f[:, :-1]).mean()
    lag_x = (f * np.roll(f, -1, axis=2)).mean()
    print('var %.4f, lag-1 %.4f (y) %.4f (x), theory %.4f, bound %.4f' % (var, lag_y, lag_x, theory, bound))
    assert abs(var - 1.0) <= bound
    assert abs(lag_y - theory) <= bound and abs(lag_x - theory) <= bound


def test_bit_level_identities():
    rng = np.random.default_rng(21)
    x = rng.standard_normal((2, 3, 5, 8)).astype(np.float32)
    kw = dict(length=(1.0, 0.5), seed=99)
    full = ensemble.perturb_members(x, 8, stddev=0.1, **kw)
    assert full.shape == (16, 3, 5, 8) and full.dtype == np.float32
    v = full.reshape(2, 8, 3, 5, 8)
    assert np.array_equal(bits(v[:, 0]), bits(x))                                           # the control member
    assert not np.array_equal(v[:, 1], x)
    zero = ensemble.perturb_members(x, 4, stddev=0.0, **kw).reshape(2, 4, 3, 5, 8)
    assert all(np.array_equal(bits(zero[:, m]), bits(x)) for m in range(4))                 # stddev 0
    anti = ensemble.perturb_members(np.zeros_like(x), 7, stddev=0.3, antithetic=True, **kw).reshape(2, 7, 3, 5, 8)
    for m in (1, 3, 5):                                                                     # members 1|2, 3|4, 5|6 share a draw
        assert np.array_equal(bits(anti[:, m + 1]), bits(-anti[:, m])) and np.abs(anti[:, m]).max() > 0
    assert not np.array_equal(anti[:, 1], anti[:, 3])
    plain = ensemble.perturb_members(np.zeros_like(x), 3, stddev=0.3, antithetic=True, control=False, **kw).reshape(2, 3, 3, 5, 8)
    assert np.array_equal(bits(plain[:, 1]), bits(-plain[:, 0])) and np.array_equal(bits(plain[:, 0]), bits(anti[:, 1]))
    a = ensemble.perturb_members(x, 3, stddev=0.1, **kw).reshape(2, 3, 3, 5, 8)             # [0, 8) = [0, 3) + [3, 8)
    b = ensemble.perturb_members(x, 5, stddev=0.1, first_member=3, **kw).reshape(2, 5, 3, 5, 8)
    assert np.array_equal(bits(np.concatenate([a, b], axis=1)), bits(v))
    first = ensemble.perturb_members(x, 8, stddev=0.1, member_axis=1, **kw)                 # the two layouts
    assert first.shape == (16, 3, 5, 8)
    assert np.array_equal(bits(np.moveaxis(first.reshape(8, 2, 3, 5, 8), 0, 1)), bits(v))
    sig = np.array([0.5, 0.0, 2.0], np.float32)                                             # a per-channel stddev
    per = ensemble.perturb_members(np.zeros_like(x), 3, stddev=sig, control=False, **kw).reshape(2, 3, 3, 5, 8)
    one = ensemble.perturb_members(np.zeros_like(x), 3, stddev=1.0, control=False, **kw).reshape(2, 3, 3, 5, 8)
    for k in range(3):
        assert np.array_equal(bits(per[:, :, k]), bits(np.float32(0.0) + sig[k] * one[:, :, k]))      # the sum with x = 0 turns -0 into +0
    # the time steps of a recurrent state count as channels, and a dense state is one row
    rec = ensemble.perturb_members(x.reshape(2, 3, 1, 5, 8), 8, stddev=0.1, **kw)
    assert rec.shape == (16, 3, 1, 5, 8) and np.array_equal(bits(rec.reshape(full.shape)), bits(full))
    dense = ensemble.perturb_members(x.reshape(2, 120), 3, stddev=0.1, seed=99)
    grid = ensemble.perturb_members(x.reshape(2, 1, 1, 120), 3, stddev=0.1, seed=99)
    assert dense.shape == (6, 120) and np.array_equal(bits(dense), bits(grid.reshape(6, 120)))


def test_nan_stays_local():
    x = np.zeros((1, 2, 6, 9), np.float32)
    x[0, 1, 2, 3] = np.nan
    out = ensemble.perturb_members(x, 4, length=1.0, seed=3).reshape(1, 4, 2, 6, 9)
    where = np.isnan(out)
    assert where.sum() == 4 and where[0, :, 1, 2, 3].all()


def test_refusals():
    x = np.zeros((1, 2, 6, 9), np.float32)
    with pytest.raises(ValueError, match="'members' must be >= 1"):
        ensemble.perturb_members(x, 0)
    with pytest.raises(ValueError, match='at most 16'):
        ensemble.perturb_members(x, 2, length=5.5)                       # R = 17
    ensemble.perturb_members(np.zeros((1, 1, 2, 16), np.float32), 2, length=(0.0, 16.0 / 3.0))      # R_x = 16 = W is allowed
    with pytest.raises(ValueError, match='more than one wrap'):
        ensemble.perturb_members(x, 2, length=(0.0, 3.2))                # R_x = 10 > W = 9
    with pytest.raises(ValueError, match="'stddev' holds 3 values for 2 channels"):
        ensemble.perturb_members(x, 2, stddev=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="'length' must be >= 0"):
        ensemble.perturb_members(x, 2, length=-1.0)
    with pytest.raises(ValueError, match="'first_member' must be >= 0"):
        ensemble.perturb_members(x, 2, first_member=-1)
    with pytest.raises(ValueError, match="'member_axis' must be 1 or 2"):
        ensemble.perturb_members(x, 2, member_axis=0)


def test_abi_symbol_is_declared_bound_and_untaped():
    assert 'dlwp_ens_perturb' in _lib.declared_symbols()
    fn = _lib.lib.dlwp_ens_perturb
    assert fn.argtypes is not None and len(fn.argtypes) == 6 and fn.argtypes[4] is _lib.EnsPerturb
    # the descriptor's layout as include/dlwp_hip.h declares it: 6 ints, the seed, 2 ints, 2 x 33 floats, 2 ints, 2 long longs
    assert _lib.EnsPerturb.seed.offset == 24 and _lib.EnsPerturb.taps_y.offset == 40 and _lib.EnsPerturb.control.offset == 40 + 264
    assert ctypes_sizeof(_lib.EnsPerturb) == 328
    src = open(os.path.join(ROOT, 'dlwp_amd', 'csrc', 'perturb.hip')).read()
    m = re.search(r'^int dlwp_ens_perturb\(([^)]*)\)\s*\{', src, re.M | re.S)
    assert m and 'void* stream' in m.group(1)
    body = src[m.end():src.index('\n}\n', m.end())]
    assert 'DLWP_UNTAPED(dlwp_ens_perturb)' in body
    # Dropout and the generator share one Philox
    assert '#include "philox.h"' in src and '#include "philox.h"' in open(os.path.join(ROOT, 'dlwp_amd', 'csrc', 'dense.hip')).read()


def ctypes_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_argument_checks_answer_with_a_null_handle():
    """every refusal comes before the handle is looked at: a null handle and null pointers reach only the last two checks"""
    def call(x=1, sigma=1, out=1, **kw):
        args = dict(samples=1, channels=2, height=6, width=9, members=3, first_member=0, seed=0, taps_y=[1.0], taps_x=[1.0], control=True,
                    antithetic=False, sample_stride=3 * 108, member_stride=108)
        args.update(kw)
        d = ops.ens_perturb_desc(**args)
        rc = _lib.lib.dlwp_ens_perturb(None, 16 * x or None, 16 * sigma or None, 16 * out or None, d, None)
        assert rc != 0
        return _lib.lib.dlwp_last_error().decode()
    assert 'must all be >= 1' in call(width=0)
    assert 'members 0' in call(members=0)
    assert 'first_member -1' in call(first_member=-1)
    assert 'radius_x 10 wraps' in call(taps_x=np.ones(21))
    assert 'at most 65535' in call(channels=65536)
    assert 'expected < 32768' in call(height=32767, taps_y=np.ones(3))
    assert 'overlap' in call(member_stride=107)
    assert 'overlap' in call(samples=2, sample_stride=2 * 108)
    assert 'negative' in call(member_stride=-108)
    assert 'null pointer' in call(x=0) and 'null pointer' in call(sigma=0) and 'null pointer' in call(out=0)
    assert 'null handle' in call()
    assert 'null handle' in call(sample_stride=108, member_stride=108)             # samples inside members, one sample
    d = ops.ens_perturb_desc(1, 1, 1, 4, 1, 0, 0, [1.0], [1.0], True, False, 4, 4)
    d.radius_y = 17
    assert _lib.lib.dlwp_ens_perturb(None, 16, 16, 16, d, None) != 0 and 'expected 0 .. 16' in _lib.lib.dlwp_last_error().decode()
    with pytest.raises(ValueError, match='expected an odd count'):
        ops.ens_perturb_desc(1, 1, 1, 4, 1, 0, 0, [1.0, 1.0], [1.0], True, False, 4, 4)
