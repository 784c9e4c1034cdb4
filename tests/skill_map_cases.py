"""Shared by tests/test_skill_map_cpu.py and tests/test_gpu_skill_map.py: the float64 restatement of forecast_skill_map /
persistence_skill_map and the checker.  Nothing is restated twice: a sample row of P points is handed to the per-lead restatement of
tests/skill_cases.py as P groups of one element, without weights (w = 1), so `forecast64` / `persistence64` reduce over the samples
alone and their bounds (derived in that module's docstring) hold per point:
  mse, rmse, mae 2^-22 relative; bias 2^-23 mae_ref + 2^-24 |bias_ref|; acc 2^-21 absolute; acc_centered 2^-21 kappa with kappa taken
  per point from the reference and asserted <= 2 wherever the reference is not NaN; NaN where the reference is NaN; equal where it is
  0 or infinite; counts equal.
kappa <= 2 is a condition on the inputs: a lead of these tests has 0, 1 or at least 63 counted samples per point (one sample has a
variance of exactly zero on both sides: NaN on both)."""
import numpy as np
import torch

from dlwp_amd.model import verify
from tests.skill_cases import Ref, check_skill, forecast64, persistence64


def _points(x, lead_axes):
    """(*lead_axes, *inner) -> (*lead_axes, P, 1): every point its own group"""
    return None if x is None else x.reshape(x.shape[:lead_axes] + (-1, 1))


def _table_points(table, inner):
    if table is None:
        return None
    return _points(table, 0) if table.shape == tuple(inner) else _points(table, 1)


def _maps(ref, leads, inner):
    return Ref(*(np.asarray(v).reshape((leads,) + tuple(inner)) for v in ref))


def forecast_map64(fc, va, table=None, labels=None):
    per_lead = fc.ndim == va.ndim
    inner = va.shape[2 if per_lead else 1:]
    ref = forecast64(_points(fc, 2), _points(va, 2 if per_lead else 1), _table_points(table, inner), labels, None, True)
    return _maps(ref, fc.shape[0], inner)


def persistence_map64(pr, va, n_fhour, table=None, labels=None):
    inner = va.shape[1:]
    ref = persistence64(_points(pr, 1), _points(va, 1), n_fhour, _table_points(table, inner), labels, None, True)
    return _maps(ref, n_fhour, inner)


def to_host(skill):
    """a Skill of CUDA tensors as a Skill of numpy arrays (the 28 bytes per point)"""
    return verify.Skill(*(v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in skill))


def check_skill_map(got, ref, what, on_device=None):
    """got: a Skill of maps (numpy, or CUDA tensors when on_device); ref: a Ref of maps.  Asserts where the result lives, then the
    bounds of tests/skill_cases.check_skill at every point"""
    assert isinstance(got, verify.Skill), what
    if on_device is not None:
        for v in got:
            assert isinstance(v, torch.Tensor) and v.is_cuda if on_device else isinstance(v, np.ndarray), (what, type(v))
    got = to_host(got)
    assert got.count.shape == ref.count.shape, (what, got.count.shape, ref.count.shape)
    check_skill(got, ref, what)
    return got


# -- the planes against the per-lead sums of dlwp_verify_skill_sums ------------------------------------------------------------------ #
def weighted_plane_sums(sums, w_e):
    """(leads, 9) + inner planes -> (leads, 10) in the order of dlwp_verify_skill_sums: sum over points of w_e x plane"""
    s = (np.asarray(sums, np.float64) * w_e).reshape(sums.shape[0], 9, -1).sum(axis=2)
    return np.concatenate([s[:, 8:], s[:, :8], np.asarray(sums, np.float64).reshape(sums.shape[0], 9, -1)[:, 8].sum(axis=1)[:, None]],
                          axis=1)


def term_magnitudes(fc, va, table, labels, w_e):
    """(leads, 10): sum |term| of every sum of dlwp_verify_skill_sums for a per-lead `valid`, from float32 d, fa, oa in float64"""
    out = np.zeros((fc.shape[0], 10))
    for f in range(fc.shape[0]):
        c = table[np.maximum(labels[f], 0)] if table is not None else np.float32(0)
        with np.errstate(invalid='ignore'):
            d, fa, oa = fc[f] - va[f], fc[f] - c, va[f] - c
        ok = ~(np.isnan(d) | np.isnan(fa) | np.isnan(oa))
        if table is not None:
            ok &= (labels[f] >= 0).reshape((-1,) + (1,) * (fc.ndim - 2))
        d, fa, oa = (np.where(ok, v, 0).astype(np.float64) for v in (d, fa, oa))
        w = ok * w_e
        out[f] = [np.sum(np.abs(t)) for t in (w, w * d, w * d * d, w * d, w * fa, w * oa, w * fa * oa, w * fa * fa, w * oa * oa, ok)]
    return out
