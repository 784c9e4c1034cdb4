"""The set-up of a workgroup of the Winograd forward kernels (csrc/conv_fwd_wino_kernel.h: conv2d_fwd_wino_body): which
block it is (reciprocal multiplies on the scalar unit instead of divisions) and where its first two chunks come from and where they
land in LDS (loads issued ahead of the rest of the set-up).  None of it touches the arithmetic: on the smallest shapes that can
break a block's coordinates the results are compared with the float64 oracle and, bit for bit, with the position-split COMPAT
instances of csrc/conv_fwd_wino2_kernel.h (another kernel, which this set-up is not part of); the build's register counts are
checked from the objects.

Two things differ from the plan this file was written to.  (1) A plain-source layer of 5 - 8 input channels and whole 32-channel
tiles belongs to the direct family at every batch size (conv_fwd.hip: few_family), so the one-chunk case -- the second staged chunk
is the clamped dummy -- reaches the body only on an up-sampled source: 8 channels of 4 x 16 -> 8 x 32 (one block) and of 5 x 17 ->
10 x 34 (ragged both ways).  (2) The wave-priority option measured slower on every launch and was left out, so there
are no priority settings to compare."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import np_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_RTOL = 1e-5          # the suite's forward tolerance (tests/test_gpu_wino_flat.py, tests/test_gpu_kernels.py)
BATCHES = (2, 3)

# (name, cin, cout, h, w of the STORED input, up-sampled source, pooled epilogue, how the launch is chosen)
#   'rect': the 8 x 32 four-wave 32-channel instance, forced;  'auto': the library's own choice;  'flat': DLWP_OPT_WINO_FLAT = 2
SHAPES = [
    ('one-block-c8', 8, 32, 4, 16, 1, False, 'rect'),        # one chunk: the second staged chunk is the clamped dummy (see above)
    ('one-block-c16', 16, 32, 8, 32, 0, False, 'rect'),
    ('one-block-c24', 24, 32, 8, 32, 0, False, 'rect'),
    ('ragged-c8', 8, 32, 5, 17, 1, False, 'rect'),           # ragged both ways: 2 x 2 tiles (10 x 34 out)
    ('ragged-c16', 16, 32, 9, 33, 0, False, 'rect'),
    ('ragged-c24', 24, 32, 9, 33, 0, False, 'rect'),
    ('pairs-12x64', 16, 64, 12, 64, 0, True, 'rect'),        # column pairs + edge pairs, pooled epilogue
    ('pairs-44x90', 16, 64, 44, 90, 0, True, 'rect'),
    ('odd-22x45-rect', 16, 32, 22, 45, 0, False, 'rect'),    # odd width: element loader
    ('odd-22x45-auto', 16, 32, 22, 45, 0, False, 'auto'),    # ... whatever Winograd instance the library takes at this batch
    ('flat-22x45', 16, 32, 22, 45, 0, False, 'flat'),
    ('flat-ups-22x45', 16, 64, 22, 45, 1, False, 'flat'),    # up-sampled source 22 x 45 -> 44 x 90
    ('flat-22x45-wide', 16, 384, 22, 45, 0, False, 'flat'),  # enough channel tiles for the 8 x 32 instance -- which a flat launch
                                                             # stands in for -- to be the library's choice at two samples
    ('nine-blocks', 16, 32, 8, 96, 0, False, 'rect'),        # batch 3: 9 blocks, odd and no multiple of 8 (the XCD remap's ragged case)
]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rect_config(ops):
    idx = [i for i, c in enumerate(ops.conv_configs()) if c[:8] == (3, 1, 8, 32, 4, 0, 2, 8) and not (c[10] & 1)]
    assert len(idx) == 1, idx
    return idx[0]


def _compat_configs(ops):
    return [i for i, c in enumerate(ops.conv_configs()) if c[0] == 3 and c[1] == 1 and c[5] == 0 and (c[10] & 5) == 5]


_cache = {}


def _case(shape, n):
    """inputs and the float64 reference of one (shape, batch), computed once"""
    key = (shape[0], n)
    if key not in _cache:
        name, cin, cout, h, w, src, pool, how = shape
        rng = np.random.default_rng(3900 + 16 * [s[0] for s in SHAPES].index(name) + n)
        x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
        wt = np_ref.glorot_uniform((3, 3, cin, cout), rng)
        b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        xs = np.asarray(x, np.float64)
        if src == 1:
            xs = np_ref.upsample2(xs)
        want = np_ref.conv2d(np_ref.pad2d_modes(xs, (1, 1, 1, 1), 0, 1), wt, b, 1, 'tanh')   # zero halo on rows, periodic on columns
        if pool:
            want = np_ref.maxpool2(want)
        _cache[key] = (x, wt, b, want)
    return _cache[key]


def cd0(ops, shape):
    name, cin, cout, h, w, src, pool, how = shape
    return ops.make_conv(cout, 3, 3, 1, ops.make_pad(1, 1, 1, 1, 0, 1), ops.ACT_TANH, src_mode=src, out_pool=pool)


def _run(ops, shape, n):
    """the launch under test: (output, launch info)"""
    name, cin, cout, h, w, src, pool, how = shape
    x, wt, b, _ = _case(shape, n)
    cd = ops.make_conv(cout, 3, 3, 1, ops.make_pad(1, 1, 1, 1, 0, 1), ops.ACT_TANH, src_mode=src, out_pool=pool)
    prev_flat = ops.set_wino_flat(2 if how == 'flat' else 0)
    try:
        if how == 'rect':
            ops.force_conv_config(_rect_config(ops))
        info = ops.conv_launch_info(x.shape, cd)
        y = ops.conv2d(dev(x), dev(wt), dev(b), cd)
        torch.cuda.synchronize()
    finally:
        ops.force_conv_config(-1)
        ops.set_wino_flat(prev_flat)
    return y, info


@pytest.mark.gpu
@pytest.mark.parametrize('n', BATCHES)
@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
def test_block_setup_keeps_the_oracle_and_the_compat_bits(ops, shape, n):
    from dlwp_amd import _lib
    name, cin, cout, h, w, src, pool, how = shape
    x, wt, b, want = _case(shape, n)
    out, info = _run(ops, shape, n)
    print(name, n, info)
    # the launch really is the kernel under test
    cfgs = ops.conv_configs()
    if how == 'flat':
        # flat runs stand in for the 8 x 32 four-wave instance where the library would take that one (never for a forced
        # configuration); at these batch sizes it may prefer another instance, and then the launch is that instance's
        prev_flat = ops.set_wino_flat(0)
        try:
            auto = ops.conv_launch_info(x.shape, cd0(ops, shape))[0][0]
        finally:
            ops.set_wino_flat(prev_flat)
        rect = auto >= 0 and cfgs[auto][:6] == (3, 1, 8, 32, 4, 0) and cfgs[auto][7] == 8 and not (cfgs[auto][10] & 1)
        print('   without flat runs: config %d %r' % (auto, cfgs[auto] if auto >= 0 else None))
        assert (info[0][0] == -4) == rect, (info, auto)
    elif how == 'rect':
        assert info[0][0] == _rect_config(ops), info
    else:
        assert info[0][0] >= 0 and cfgs[info[0][0]][0] == 3 and cfgs[info[0][0]][5] == 0, info
    if name.startswith('pairs-'):
        assert info[0][5] == 5, info                  # column pairs (1) + edge pairs (4)
    if name.startswith('odd-') and how == 'rect':
        assert info[0][5] & 3 == 0, info              # element by element
    if name == 'nine-blocks' and n == 3:
        assert info[0][1] == 9, info
    # float64 oracle
    got = out.cpu().numpy()
    assert got.shape == want.shape
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print('   oracle error %.3g of scale %.3g' % (err, scale))
    assert err <= CONV_RTOL * scale, (name, n, err)
    # an independent kernel with the same arithmetic, where the geometry has one
    cd = ops.make_conv(cout, 3, 3, 1, ops.make_pad(1, 1, 1, 1, 0, 1), ops.ACT_TANH, src_mode=src, out_pool=pool)
    witnesses = 0
    prev_flat = ops.set_wino_flat(0)
    try:
        for i in _compat_configs(ops):
            ops.force_conv_config(i)
            try:
                ref = ops.conv2d(dev(x), dev(wt), dev(b), cd)
            except _lib.DlwpError:
                continue
            witnesses += 1
            assert torch.equal(ref, out), (name, n, i, float((ref - out).abs().max()))
    finally:
        ops.force_conv_config(-1)
        ops.set_wino_flat(prev_flat)
    print('   COMPAT witnesses: %d' % witnesses)
    if src == 0:
        assert witnesses >= 1, 'no position-split COMPAT instance took a plain-source layer with whole 32-channel tiles'


def test_reciprocal_multiply_is_an_exact_division_below_2_to_the_31():
    """wino_reciprocal / wino_div of conv_fwd_wino_kernel.h restated: l = ceil(log2 d), sh = 31 + l, m = ceil(2^sh / d) fits 32 bits
    and (n m) >> sh == n // d for every 0 <= n < 2^31 -- checked at the places a wrong multiplier would show first (multiples of d
    and their predecessors, the top of the range) for every divisor a block decomposition can meet here and a spread of large ones."""
    rng = np.random.default_rng(5)
    divisors = list(range(1, 2050)) + [int(v) for v in rng.integers(2050, 2 ** 31 - 1, 400)] + [2 ** 31 - 1, 2 ** 30, 2 ** 30 + 1, 65535, 65537]
    top = 2 ** 31 - 1
    for d in divisors:
        l = (d - 1).bit_length()
        sh = 31 + l
        m = ((1 << sh) + d - 1) // d
        assert m < 2 ** 32, d
        q = top // d
        ns = {0, 1, d - 1, d, d + 1, top, top - 1, q * d, q * d - 1, max(q - 1, 0) * d, (q // 2) * d, (q // 2) * d + d - 1}
        ns.update(int(v) for v in rng.integers(0, top, 8))
        for n in ns:
            if 0 <= n <= top:
                assert (n * m) >> sh == n // d, (n, d)


def test_headline_instances_keep_their_registers_and_use_no_scratch():
    """The four headline launches run three instances of conv2d_fwd_wino_body; their set-up was re-ordered around early loads and
    pinned accumulator clears, which must not cost a register over the parent's build (214 for the dominant instance -- two waves
    per SIMD either way, but the loop's own need is the yardstick; 225 / 247 for the flat runs) nor spill."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_prologue as ip
    build = os.path.join(ROOT, 'dlwp_amd', 'csrc', 'build')
    objs = [os.path.join(build, 'conv_fwd_k3d1.o'), os.path.join(build, 'conv_fwd_wino_flat.o')]
    if not all(os.path.exists(p) for p in objs) or not os.path.exists(ip.LLVM + 'llvm-objdump'):
        pytest.skip('the Winograd objects are not built here (or no llvm-objdump)')
    limits = {'WinoCfg<1, 8, 32, 4, 2, 8, false, false, false, false, false, true, false, true>': (objs[0], 214),
              'WinoFlatCfg<false, 2>': (objs[1], 225),
              'WinoFlatCfg<true, 4>': (objs[1], 247)}
    for pat, (path, vgprs) in limits.items():
        ks = ip.kernels(path, pat)
        assert len(ks) == 1, (pat, list(ks))
        k = list(ks.values())[0]
        assert k['vgpr'] is not None and k['vgpr'] <= vgprs and k['scratch'] == 0, (pat, k['vgpr'], k['scratch'])
        first, last = ip.window(k['ins'])
        assert first is not None and not any(o.startswith('scratch_') for o, _ in k['ins']), pat
        pro = [o for o, _ in k['ins'][:first]]
        # the block decomposition no longer divides on the vector ALU
        assert not any(o.startswith('v_rcp') for o in pro), pat
