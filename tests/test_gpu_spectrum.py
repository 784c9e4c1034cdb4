"""Zonal power spectra on the device (csrc/spectrum.hip behind verify.forecast_spectrum / persistence_spectrum / spectrum_sums) against
the float64 restatement of tests/spectrum_cases.py, inside the bounds derived there: every sum within its worst-case
bound, sum w within 2^-40, equal counts, identical bits on repeated calls, forecast_spectrum bit-equal to finish_spectrum of the
device sums, device and host Spectrum inside the same propagated bounds.  Shapes are the smallest at which each mechanism can go wrong:
W = 4 and 5 (one matrix step and a half), 30, 45 (odd: scalar loads, no Nyquist term), 180 (K = 91: three wavenumber tiles, the last
ragged; many blocks per cell), 360 (two tiles per wave), 512 (K = 257: nine tiles, the largest LDS image), row counts below one 32-row
tile and not a multiple of one, one group and several, a plain series whose last leads have few or no pairs, persistence, weights and
none, a base one float off alignment, planted non-finite rows, an offset field.  Run with -s to see error / bound of every case; for the
red input at W >= 180 the bound exceeds the smallest coefficients, and the test shows only that the error stays inside it."""
import numpy as np
import pytest
import torch

from dlwp_amd import ops
from dlwp_amd.model import verify
from tests.spectrum_cases import CASES, axis_of, case, check_spectrum, check_sums

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def cuda(x, misalign=False):
    """x on the device; misalign: the same values one float into a storage, so the address is 4 (mod 16)"""
    t = torch.from_numpy(np.array(x, dtype=np.float32, order='C')).cuda()          # a copy: the shared case arrays are read-only
    if not misalign:
        assert t.data_ptr() % 16 == 0
        return t
    store = torch.empty(t.numel() + 4, dtype=torch.float32, device='cuda')
    assert store.data_ptr() % 16 == 0
    out = store[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def device_sums(name, misalign=False):
    fc, va, weights, grouped, n_fhour, ref = case(name)
    axis = axis_of(fc, va, grouped, n_fhour)
    sums, norm = verify.spectrum_sums(cuda(fc, misalign), cuda(va, misalign), weights, axis, n_fhour=n_fhour or None)
    return sums, norm, ref


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_sums_inside_the_derived_bounds(name):
    sums, norm, ref = device_sums(name)
    check_sums(sums, norm, ref, 'device ' + name)
    if name.startswith('series'):
        assert not sums[5:].any() and not norm[5:].any()         # leads without pairs: no work, zeros
    if name == 'nonfinite':
        assert norm[..., 1].tolist() == [[16, 17], [17, 16]]


@pytest.mark.parametrize('name', ['w180', 'w30', 'w512', 'offset', 'nonfinite'])
def test_scalar_route_from_a_misaligned_base_has_the_same_results(name):
    """W % 4 == 0 here, so only the base address takes these cases off the 16-byte route: the same bits, not merely the same bounds"""
    sums, norm, ref = device_sums(name, misalign=True)
    check_sums(sums, norm, ref, 'misaligned ' + name)
    aligned = device_sums(name)
    assert np.array_equal(sums, aligned[0]) and np.array_equal(norm, aligned[1])


@pytest.mark.parametrize('name', ['w180', 'w45', 'series_groups'])
def test_two_calls_give_identical_bits(name):
    a, b = device_sums(name), device_sums(name)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('name', ['w5', 'w180', 'w180_red', 'w360_red', 'series', 'series_groups', 'persistence', 'offset', 'nonfinite'])
def test_spectrum_on_cuda_tensors_is_the_finish_of_the_device_sums_and_agrees_with_the_host(name):
    fc, va, weights, grouped, n_fhour, ref = case(name)
    axis = axis_of(fc, va, grouped, n_fhour)
    if n_fhour:
        got = verify.persistence_spectrum(cuda(fc), cuda(va), n_fhour, weights, axis)
        host = verify.persistence_spectrum(fc, va, n_fhour, weights, axis)
    else:
        got = verify.forecast_spectrum(cuda(fc), cuda(va), weights, axis)
        host = verify.forecast_spectrum(fc, va, weights, axis)
    sums, norm, _ = device_sums(name)
    want = verify.finish_spectrum(sums, norm, grouped)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    check_spectrum(got, ref, grouped, 'device ' + name)
    check_spectrum(host, ref, grouped, 'host ' + name)
    assert np.array_equal(got.count, host.count)
    if name.startswith('series'):
        assert (got.count[5:] == 0).all() and np.isnan(got.power_valid[5:]).all() and np.isnan(got.ratio[5:]).all()


def test_numpy_arguments_with_device_take_the_kernel():
    fc, va, weights, grouped, _, ref = case('w45')
    axis = axis_of(fc, va, grouped)
    sums, norm = verify.spectrum_sums(np.array(fc), np.array(va), weights, axis, device='cuda')      # copies: the case arrays are read-only
    check_sums(sums, norm, ref, 'numpy + device w45')
    again = device_sums('w45')
    assert np.array_equal(sums, again[0]) and np.array_equal(norm, again[1])


def test_a_perfect_forecast_and_a_pure_wave_on_the_device():
    fc, va, weights, grouped, _, _ = case('w180')
    got = verify.forecast_spectrum(cuda(va), cuda(va), weights, axis_of(fc, va, grouped))
    assert np.array_equal(got.power_error, np.zeros_like(got.power_error)) and np.array_equal(got.power_forecast, got.power_valid)
    assert np.array_equal(got.ratio, np.ones_like(got.ratio)) and np.array_equal(got.coherence, np.ones_like(got.coherence))
    j = np.arange(180)
    wave = np.broadcast_to(np.cos(2 * np.pi * 45 * j / 180), (1, 2, 1, 3, 180)).astype(np.float32)
    got = verify.forecast_spectrum(torch.zeros(wave.shape, device='cuda'), cuda(wave))
    want = np.zeros(91)
    want[45] = 0.5
    assert np.abs(got.power_valid[0] - want).max() < 1e-6 and np.abs(got.power_error[0] - want).max() < 1e-6


def test_wrapper_refuses_addressing_out_of_range_and_wide_rows_without_a_launch():
    x = torch.zeros(2 * 3 * 24, device='cuda')
    ok = dict(leads=2, count0=3, count_dec=0, groups=1, run=24, width=8)
    sums, norm = ops.verify_spectrum_sums(x, (72, 24, 0), x, (72, 24, 0), **ok)
    assert sums.shape == (2, 1, 4, 5) and norm.shape == (2, 1, 2) and norm[..., 1].tolist() == [[9.0], [9.0]]
    with pytest.raises(ValueError, match='operand fc holds 144 elements, the strides address 168'):
        ops.verify_spectrum_sums(x, (72, 24, 0), x, (72, 24, 0), **dict(ok, count0=4))
    with pytest.raises(ValueError, match='operand ob holds 144 elements, the strides address 168'):
        ops.verify_spectrum_sums(x, (72, 24, 0), x, (72, 24, 1), **ok)
    with pytest.raises(ValueError, match='operand fc holds'):
        ops.verify_spectrum_sums(x, (72, 24, 0), x, (72, 24, 0), **dict(ok, groups=2))
    with pytest.raises(ValueError, match='4 .. 512'):
        ops.verify_spectrum_sums(x, (0, 0, 0), x, (0, 0, 0), 1, 1, 0, 1, 513, 513)
    with pytest.raises(ValueError, match='4 .. 512'):
        ops.verify_spectrum_sums(x, (0, 0, 0), x, (0, 0, 0), 1, 1, 0, 1, 24, 3)
    with pytest.raises(ValueError, match='do not divide a run'):
        ops.verify_spectrum_sums(x, (72, 24, 0), x, (72, 24, 0), **dict(ok, width=5))
    with pytest.raises(ValueError, match='weights do not divide'):
        ops.verify_spectrum_sums(x, (72, 24, 0), x, (72, 24, 0), weights=np.ones(2), **ok)
    with pytest.raises(ValueError, match='negative|>= 0'):
        ops.verify_spectrum_sums(x, (72, -24, 0), x, (72, 24, 0), **ok)
    wide = torch.zeros((1, 1, 2, 516), device='cuda')
    with pytest.raises(ValueError, match='at most 512'):
        verify.forecast_spectrum(wide, wide)                     # a resident series is never downloaded silently
