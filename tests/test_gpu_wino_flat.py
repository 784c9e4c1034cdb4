"""The Winograd forward on runs of 64 consecutive tiles (csrc/conv_fwd_wino_flat.hip, DLWP_OPT_WINO_FLAT): the same bits as the
8 x 32 instances it replaces -- per launch on the U-Net's 22 x 45 layers, ragged batches, odd and even widths, every halo mode it
accepts, channel windows and activations; the float64 oracle; the whole 28-forward rollout -- and a clean loop in the ISA."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import np_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_RTOL = 1e-5
ACTS = {'linear': 0, 'tanh': 1, 'relu': 2}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


CASES = [
    # (n, stored channels, cin window (offset, count), h, w of the STORED input, cout, output window (offset, total), mode_h,
    #  mode_w, src_mode, act)
    (256, 64, (0, 64), 22, 45, 128, (0, 0), 0, 1, 0, 'tanh'),       # U-Net layer 3
    (256, 128, (0, 128), 22, 45, 64, (0, 0), 0, 1, 1, 'tanh'),      # U-Net layer 4: up-sampled source, 9 live positions
    (1, 64, (0, 64), 22, 45, 128, (0, 0), 0, 1, 0, 'relu'),
    (3, 128, (0, 128), 22, 45, 64, (0, 0), 1, 1, 1, 'linear'),
    (63, 64, (0, 64), 22, 45, 128, (0, 0), 2, 2, 0, 'tanh'),
    (63, 128, (0, 128), 22, 45, 64, (0, 0), 2, 0, 1, 'relu'),
    (3, 16, (0, 16), 21, 46, 32, (0, 0), 1, 0, 0, 'tanh'),         # even width, odd height: a half-used last tile row
    (5, 16, (0, 16), 9, 33, 64, (0, 0), 0, 2, 1, 'tanh'),           # up-sampled, 64 channels per block
    (4, 16, (0, 16), 13, 32, 32, (0, 0), 2, 1, 1, 'linear'),        # up-sampled, 32 channels per block
    (3, 24, (0, 24), 17, 41, 64, (32, 96), 1, 1, 0, 'tanh'),        # output channel windows
    (2, 32, (0, 32), 11, 45, 64, (64, 128), 0, 1, 1, 'relu'),
]


def _ref(x, w, b, mh, mw, act, src):
    xs = np.asarray(x, np.float64)
    if src == 1:
        xs = np_ref.upsample2(xs)
    xp = np_ref.pad2d_modes(xs, (1, 1, 1, 1), mh, mw)
    return np_ref.conv2d(xp, w, b, 1, act)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_flat_runs_give_the_bits_of_the_rectangle_instances(ops, case):
    n, ct, (coff, cin), h, w, cout, (ooff, otot), mh, mw, src, act = case
    rng = np.random.default_rng(9100 + CASES.index(case))
    x = rng.standard_normal((n, ct, h, w)).astype(np.float32)
    wt = np_ref.glorot_uniform((3, 3, cin, cout), rng)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    cd = ops.make_conv(cout, 3, 3, 1, ops.make_pad(1, 1, 1, 1, mh, mw), ACTS[act], in_c_off=coff, in_c_total=ct,
                       out_c_off=ooff, out_c_total=otot, src_mode=src)
    xd, wd, bd = dev(x), dev(wt), dev(b)
    tot = otot or cout
    ho, wo = (2 * h, 2 * w) if src == 1 else (h, w)
    outs, infos = [], []
    prev = ops.set_wino_flat(0)
    try:
        for mode in (0, 2):
            ops.set_wino_flat(mode)
            infos.append(ops.conv_launch_info(x.shape, cd))
            y = torch.full((n, tot, ho, wo), 7.0, device='cuda')
            ops.conv2d(xd, wd, bd, cd, out=y, x_channels=cin)
            outs.append(y)
    finally:
        ops.set_wino_flat(prev)
    # the flat kernel stands in for the 8 x 32 Winograd instances (which the headline layers take); elsewhere it must not run
    cfg = ops.conv_configs()[infos[0][0][0]] if infos[0][0][0] >= 0 else None
    rect = cfg is not None and cfg[:6] == (3, 1, 8, 32, 4, 0) and cfg[7] == 8 and not (cfg[10] & 1)
    if case in CASES[:2]:
        assert rect, infos
    assert infos[0][0][0] != -4 and (infos[1][0][0] == -4) == rect, infos
    if rect:
        runs = -(-((ho + 1) // 2) * ((wo + 1) // 2) // 64)
        bnf = 4 if src == 1 and cout % 64 == 0 else cfg[6]          # (up-sampled sources: 64-channel runs whenever Cout allows)
        assert infos[1][0][1] == n * runs * (cout // (16 * bnf)), infos
    assert torch.equal(outs[1], outs[0]), (case, float((outs[1] - outs[0]).abs().max()))
    got = outs[1].cpu().numpy()
    keep = [c for c in range(tot) if not ooff <= c < ooff + cout]
    assert np.all(got[:, keep] == 7.0), 'channels outside the output window were written'
    if n <= 8:
        want = _ref(x[:, coff:coff + cin], wt, b, mh, mw, act, src)
        sub = got[:, ooff:ooff + cout]
        scale = max(1.0, float(np.abs(want).max()))
        assert float(np.abs(sub - want).max()) <= CONV_RTOL * scale


@pytest.mark.gpu
def test_flat_runs_are_taken_by_default_on_the_headline_layers_only_from_a_full_chip(ops):
    cd3 = ops.make_conv(128, 3, 3, 1, ops.make_pad(1, 1, 1, 1, 0, 1), ACTS['tanh'])
    cd4 = ops.make_conv(64, 3, 3, 1, ops.make_pad(1, 1, 1, 1, 0, 1), ACTS['tanh'], src_mode=1)
    assert ops.conv_launch_info((256, 64, 22, 45), cd3)[0][0] == -4
    info4 = ops.conv_launch_info((256, 128, 22, 45), cd4)[0]
    assert info4[0] == -4 and info4[1] == 256 * 16
    # executed matrix work: 16 runs of 64 tiles x 9 positions x 64 channels x 128 input channels per sample
    assert info4[3] == 2.0 * 256 * 16 * 64 * 9 * 64 * 128
    info4 = ops.conv_launch_info((128, 128, 22, 45), cd4)[0]          # (one of the rollout's two member chains)
    assert info4[0] == -4 and info4[1] == 128 * 16
    assert ops.conv_launch_info((1, 128, 22, 45), cd4)[0][0] != -4
    assert ops.conv_launch_info((256, 64, 44, 90), cd3)[0][0] != -4     # too wide for the staged rows


@pytest.mark.gpu
def test_rollout_is_bit_identical_with_and_without_flat_runs(ops):
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.presets import unet_layers
    grid, cin, members, forwards = (88, 180), 4, 256, 28
    g = torch.Generator().manual_seed(0)
    base = torch.randn((1, cin) + grid, generator=g)
    state0 = (base + 0.01 * torch.randn((members, cin) + grid, generator=g)).cuda()
    series = []
    prev = ops.set_wino_flat(0)
    try:
        for mode in (0, 1):
            ops.set_wino_flat(mode)
            np.random.seed(1234)
            d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
            d.build_model(unet_layers((cin,) + grid), loss='mse', optimizer='adam', metrics=['mae'], gpus=1)
            series.append(d.model.rollout_on_device(state0, forwards).clone())
            torch.cuda.synchronize()
            del d
    finally:
        ops.set_wino_flat(prev)
    assert torch.isfinite(series[0]).all()
    assert torch.equal(series[1], series[0]), float((series[1] - series[0]).abs().max())


def test_flat_kernels_have_no_wait_behind_their_prefetch_loads():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_waits as w
    path = os.path.join(ROOT, 'dlwp_amd', 'csrc', 'build', 'conv_fwd_wino_flat.o')
    if not os.path.exists(path) or not os.path.exists(w.LLVM + '/llvm-objdump'):
        pytest.skip('conv_fwd_wino_flat.o is not built here (or no llvm-objdump)')
    ks = [(name, lines) for name, lines in w.kernels(w.disassemble(path)) if 'conv2d_fwd_wino_flat_f32' in name]
    assert len(ks) == 3, [n for n, _ in ks]
    for name, lines in ks:
        mf = [i for i, l in enumerate(lines) if 'v_mfma' in l]
        assert mf, name
        falls = sum(1 for i, l in enumerate(lines[:-1]) if l.startswith('s_xor_b64 exec') and lines[i + 1].startswith('s_cbranch_execnz'))
        inside = [hit for hit in w.scan(lines, 6) if mf[0] < hit[0] < mf[-1]]
        scratch = sum(1 for i, l in enumerate(lines) if l.startswith('scratch_') and mf[0] < i < mf[-1])
        assert not inside and falls == 0 and scratch == 0, (name, inside[:3], falls, scratch)
