"""dlwp_convlstm_gates_bwd -- the one hand-written backward without a torch twin -- against autograd of the float64 gate function
(oracle/torch_ref.convlstm_gates) with upstream gradients dh and dc_in:  loss = (h * dh).sum() + (c * dc_in).sum();  dz is the
gradient with respect to zx (identical for zh), dc_prev with respect to c_prev.

Kinks.  hard_sigmoid has kinks at |z| = 2.5, relu at 0, and the kernel adds zx + zh in float32.  The inputs come from
tests/test_oracle_conv.kink_free_gate_inputs: the float32 sum is exact, z is an odd multiple of 2^-7 -- never 0, never +-2.5, at
least 2^-7 away from every kink.  So NO element is excluded (no mask, no isclose filter: the test asserts the distance instead),
and it asserts that the linear part and each saturated side of hard_sigmoid hold at least 5 % of the gate values.  The cell
state handed to the kernel is the oracle's c rounded to float32 (rounding keeps its sign; relu at an exact 0 has gradient 0 on
both sides).

Tolerance.  The device tanh is exp2 + rcp hardware approximations and the sigmoid uses __expf, so no ulp count follows from the
source: the bar is the project's stated float32 parity bar, 1e-5 relative to the output scale (FWD_TOL), per output
tensor, with dh, dc_in, c_prev unit normal.  A wrong derivative branch is an error of order 0.1."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import torch_ref
from tests.test_oracle_conv import kink_free_gate_inputs

pytestmark = pytest.mark.gpu

BWD_TOL = 1e-5
ACTS = ('linear', 'tanh', 'relu')
RECS = ('hard_sigmoid', 'sigmoid')
#: (n, f, h, w): hw % 4 != 0 (5 x 7) and == 0 (16 x 24), f in {1, 3, 24}, n in {1, 3}
SHAPES = [(1, 1, 5, 7), (3, 3, 5, 7), (1, 24, 5, 7), (3, 1, 16, 24), (1, 3, 16, 24), (3, 24, 16, 24)]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def make_case(rng, n, f, h, w, first, with_dc_in):
    """float64 inputs, all exactly representable in float32"""
    zx, zh = kink_free_gate_inputs(rng, (n, 4 * f, h, w), first)
    r32 = lambda shape: rng.standard_normal(shape).astype(np.float32).astype(np.float64)  # noqa: E731
    cp = None if first else r32((n, f, h, w))
    dh = r32((n, f, h, w))
    dc_in = r32((n, f, h, w)) if with_dc_in else None
    return zx, zh, cp, dh, dc_in


def check_kink_free(zx, zh, shares):
    """the float32 sum is exact, z is an odd multiple of 2^-7, at least 2^-7 from 0 and from +-2.5; counts the hard_sigmoid
    branches of the i, f, o gate values into `shares`"""
    z = zx + (0 if zh is None else zh)
    z32 = zx.astype(np.float32) + (0 if zh is None else zh.astype(np.float32))
    assert z32.dtype == np.float32 and np.array_equal(z32.astype(np.float64), z)
    k = z * 128
    assert np.array_equal(k, np.round(k)) and np.all(np.abs(k) % 2 == 1)
    assert min(np.abs(z).min(), np.abs(np.abs(z) - 2.5).min()) >= 2.0 ** -7
    f = z.shape[1] // 4
    gates = np.concatenate([z[:, :2 * f].ravel(), z[:, 3 * f:].ravel()])
    shares += np.array([(gates < -2.5).sum(), (np.abs(gates) < 2.5).sum(), (gates > 2.5).sum(), gates.size])


def oracle(zx, zh, cp, dh, dc_in, act, rec):
    """(c, dz, dc_prev | None) in float64 by autograd"""
    t = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)  # noqa: E731
    zx_t = t(zx).requires_grad_(True)
    cp_t = None if cp is None else t(cp).requires_grad_(True)
    c, h = torch_ref.convlstm_gates(zx_t, t(zh), cp_t, act, rec)
    loss = (h * t(dh)).sum()
    if dc_in is not None:
        loss = loss + (c * t(dc_in)).sum()
    loss.backward()
    return c.detach().numpy(), zx_t.grad.numpy(), None if cp is None else cp_t.grad.numpy()


def kernel_direct(zx, zh, cp, c, dh_full, dc_in, f, h_c_off, act, rec, want_dc_prev):
    """the C entry point on outputs PRE-FILLED with NaN: whatever it does not write stays NaN"""
    from dlwp_amd import _lib
    n, _, h, w = zx.shape
    dz = torch.full_like(zx, float('nan'))
    dcp = torch.full_like(c, float('nan')) if (cp is not None and want_dc_prev) else None
    ptr = lambda a: ctypes.c_void_p(0 if a is None else a.data_ptr())  # noqa: E731
    _lib.check(_lib.lib.dlwp_convlstm_gates_bwd(_lib.handle(torch.cuda.current_device()), ptr(zx), ptr(zh), ptr(cp), ptr(c),
                                                ptr(dh_full), ptr(dc_in), ptr(dz), ptr(dcp), n, f, h * w, h_c_off,
                                                dh_full.shape[1], act, rec, _lib.F32,
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return dz, dcp


def run_case(ops, case, f, act, rec, want_dc_prev):
    """Runs the wrapper and the C entry point on one case; returns {'dz': error / scale, 'dc_prev': ...}."""
    zx, zh, cp, dh, dc_in = case
    first = zh is None
    c64, dz_want, dcp_want = oracle(zx, zh, cp, dh, dc_in, act, rec)
    n, _, h, w = zx.shape
    # dh is channels [f, 2f) of a (n, 3f, h, w) tensor; the other channels hold NaN and must not reach the result
    dh_full = np.full((n, 3 * f, h, w), np.nan, dtype=np.float32)
    dh_full[:, f:2 * f] = dh
    d = [dev(a) for a in (zx, zh, cp, c64, dh_full, dc_in)]
    act_code, rec_code = ops.ACTIVATIONS[act], ops.REC_HARD_SIGMOID if rec == 'hard_sigmoid' else ops.REC_SIGMOID
    dz, dcp = ops.convlstm_gates_bwd(d[0], d[1], d[2], d[3], d[4], d[5], f, h_c_off=f, act=act_code, rec_act=rec_code,
                                     want_dc_prev=want_dc_prev)
    dz2, dcp2 = kernel_direct(d[0], d[1], d[2], d[3], d[4], d[5], f, f, act_code, rec_code, want_dc_prev)
    torch.cuda.synchronize()
    assert tuple(dz.shape) == zx.shape and torch.isfinite(dz2).all() and torch.equal(dz, dz2)      # fully written
    got = dz.cpu().numpy()
    errs = {'dz': float(np.abs(got - dz_want).max() / max(1.0, np.abs(dz_want).max()))}
    if first:
        assert dcp is None and dcp2 is None
        assert np.all(got[:, f:2 * f] == 0)                 # no c_prev: the forget block is exactly 0
    elif want_dc_prev:
        assert torch.isfinite(dcp2).all() and torch.equal(dcp, dcp2)
        errs['dc_prev'] = float(np.abs(dcp.cpu().numpy() - dcp_want).max() / max(1.0, np.abs(dcp_want).max()))
    else:
        assert dcp is None and dcp2 is None
    return errs


@pytest.mark.parametrize('rec', RECS)
@pytest.mark.parametrize('act', ACTS)
def test_gates_backward_matches_float64_autograd(ops, act, rec):
    """Every (activation, recurrent activation) pair: first step (zh, c_prev None) and later step, dc_in None and given,
    want_dc_prev True and False, over SHAPES; dh read through a channel window between NaN channels."""
    rng = np.random.default_rng(11)
    worst = {}
    for first in (True, False):
        shares = np.zeros(4)
        for n, f, h, w in SHAPES:
            for with_dc_in in (False, True):
                for want_dc_prev in ((True,) if first else (True, False)):
                    case = make_case(rng, n, f, h, w, first, with_dc_in)
                    check_kink_free(case[0], case[1], shares)
                    errs = run_case(ops, case, f, act, rec, want_dc_prev)
                    for k, e in errs.items():
                        assert e <= BWD_TOL, '%s/%s %s: %.3e (first %r, shape %r, dc_in %r)' % (
                            act, rec, k, e, first, (n, f, h, w), with_dc_in)
                        key = '%s %s' % ('first' if first else 'later', k)
                        worst[key] = max(worst.get(key, 0.0), e)
        # no branch of hard_sigmoid goes unvisited: the draws give about 7 % per saturated side (19 % on the first step)
        assert np.all(shares[:3] >= 0.05 * shares[3]), shares
    print('\nMEASURED gates_bwd %s/%s: %s (bar %.0e)' % (act, rec, ', '.join('%s %.2e' % kv for kv in sorted(worst.items())),
                                                         BWD_TOL))


@pytest.mark.parametrize('act,rec', [('tanh', 'sigmoid'), ('relu', 'hard_sigmoid')])
def test_gates_backward_beyond_the_grid_cap(ops, act, rec):
    """n * f * hw above this kernel's grid cap of 16 * cu_count blocks of 256 threads: the grid-stride loop repeats"""
    from tests.test_gpu_optimizers import cu_count
    f, h, w = 24, 96, 120
    n = (16 * cu_count() * 256) // (f * h * w) + 1
    assert n * f * h * w > 16 * cu_count() * 256
    rng = np.random.default_rng(12)
    shares = np.zeros(4)
    case = make_case(rng, n, f, h, w, False, True)
    check_kink_free(case[0], case[1], shares)
    assert np.all(shares[:3] >= 0.05 * shares[3])
    errs = run_case(ops, case, f, act, rec, True)
    print('\nMEASURED gates_bwd %s/%s, %d elements: %s' % (act, rec, n * f * h * w, errs))
    assert errs['dz'] <= BWD_TOL and errs['dc_prev'] <= BWD_TOL


def test_gates_backward_of_an_empty_batch(ops):
    z = torch.empty((0, 12, 5, 7), device='cuda')
    c = torch.empty((0, 3, 5, 7), device='cuda')
    dz, dcp = ops.convlstm_gates_bwd(z, z, c, c, torch.empty((0, 9, 5, 7), device='cuda'), c, 3, h_c_off=3)
    torch.cuda.synchronize()
    assert tuple(dz.shape) == (0, 12, 5, 7) and tuple(dcp.shape) == (0, 3, 5, 7)
