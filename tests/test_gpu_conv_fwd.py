"""dlwp_conv2d_fwd, _fwd_direct, _fwd_prepared and _fwd_pool2 on every forward route (tests/conv_fwd_cases.py) against the float64
reference, on guarded slabs:
 1. route  -- dlwp_conv2d_launch_info reports the route the row names; the table reaches every compiled configuration;
 2. exact  -- integer inputs: the float64 sums TO THE BIT (`==`), linear and relu, with and without the pooled epilogue, nothing
              written outside the output window, no NaN left inside it;
 3. tanh   -- random reals inside FWD_TOL of max(1, max |reference|) (bfloat16 outputs: one bfloat16 ulp, as tests/test_gpu_kernels.py
              holds them); `-s` prints the worst error / bound ratio per family as MEASURED;
 4. containment -- NaN in the stored channels outside the input window, an output tensor wider than the window, a NaN sample next
              to clean ones: the clean results keep their bits;
 5. no NaN lost -- where the reference is NaN the kernel is; it may spread inside the poisoned sample (a Winograd tile, a flat
              run: printed as SPREAD), never out of it.
Every tensor lies between guard elements, outputs start as NaN, every call runs twice -- the second time with every operand 1 to 3
floats past a 16-byte boundary -- and must return the same bits.  DESIGN.md (section 4) holds the contract and the measured figures."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import np_ref
from tests import conv_fwd_cases as cases
from tests.test_gpu_train_ops import GUARD, Slab, same_bits

pytestmark = pytest.mark.gpu

ROWS = cases.ROWS
IDS = [r['name'] for r in ROWS]
N = cases.N
GUARD16 = np.uint16(0xD329)              # a finite negative bfloat16
SECOND = dict(x=1, w=2, b=3, y=3, y2=1, z=2, c=1, c_out=2)       # floats past a 16-byte boundary in the second call
WORST, SPREAD, REACHED, POOLED, FORMS, WHOLE_STEP, STEP_RAN = {}, {}, set(), {}, {}, set(), []


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from dlwp_amd import ops as _ops
    return _ops


def bf16_bits(values):
    """float32 values that bfloat16 holds exactly (or NaN) -> their 16 bits"""
    u = np.ascontiguousarray(values, np.float32).view(np.uint32)
    assert np.all((u & 0xffff) == 0), 'not a bfloat16 value'
    return (u >> 16).astype(np.uint16)


class Slab16(object):
    """tests/test_gpu_train_ops.py: Slab, for a bfloat16 tensor: `align` FLOATS past a 16-byte boundary, guards on both sides"""

    def __init__(self, values, align=0, shape=None):
        if values is None:
            values = np.full(shape, np.nan, dtype=np.float32)
        bits = bf16_bits(values)
        n, off = bits.size, 2 * (GUARD + align)
        host = np.full(n + 4 * GUARD + 8, GUARD16, dtype=np.uint16)
        host[off:off + n] = bits.reshape(-1)
        self.host, self.off, self.n, self.shape = host, off, n, bits.shape
        self.buf = torch.from_numpy(host.view(np.int16).copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[off:off + n].view(torch.bfloat16).view(bits.shape)

    def read(self):
        torch.cuda.synchronize()
        now = self.buf.cpu().numpy().view(np.uint16)
        lo, hi = self.off, self.off + self.n
        assert np.array_equal(now[:lo], self.host[:lo]), 'guard below the tensor was written'
        assert np.array_equal(now[hi:], self.host[hi:]), 'guard above the tensor was written'
        return (now[lo:hi].astype(np.uint32) << 16).view(np.float32).reshape(self.shape).copy()

    def unchanged(self):
        torch.cuda.synchronize()
        return np.array_equal(self.buf.cpu().numpy().view(np.uint16), self.host)


def to_o8(a):
    n, c, h, w = a.shape
    return np.ascontiguousarray(a.reshape(n, c // 8, 8, h, w).transpose(0, 1, 3, 4, 2)).reshape(n, c, h, w)


def from_o8(a):
    n, c, h, w = a.shape
    return np.ascontiguousarray(a.reshape(n, c // 8, h, w, 8).transpose(0, 1, 4, 2, 3)).reshape(n, c, h, w)


def slab(values, storage, align, shape=None):
    """a tensor in its storage: 'f32', 'bf16' or 'o8' (bfloat16 channel octets); values None: an output, NaN"""
    if values is not None and storage == 'o8':
        values = to_o8(np.asarray(values, np.float32))
    return (Slab if storage == 'f32' else Slab16)(values, align, shape)


def read(s, storage):
    got = s.read()
    return from_o8(got) if storage == 'o8' else got


@contextlib.contextmanager
def options(ops, row, cfg):
    setters = dict(few_stream=ops.set_few_stream, few_wino=ops.set_few_wino, wino_flat=ops.set_wino_flat, splitk=ops.set_splitk,
                   wino_xloader=ops.set_wino_xloader, bf16_mfma=ops.set_bf16_mfma)
    prev = {}
    try:
        for k, v in row['opts'].items():
            prev[k] = setters[k](v)
        ops.force_conv_config(-1 if cfg is None else cfg)
        yield
    finally:
        ops.force_conv_config(-1)
        for k, v in prev.items():
            setters[k](v)


def desc(ops, row, act, pool, extra_in, extra_out):
    oc = cases.out_shape(row, pool)[0]
    return ops.make_conv(row['cout'], row['k'], row['k'], row['dil'], ops.make_pad(*row['pads'], row['mh'], row['mw']),
                         ops.ACTIVATIONS[act], in_c_off=extra_in, in_c_total=row['cin'] + 2 * extra_in if extra_in else 0,
                         out_c_off=extra_out, out_c_total=oc + 2 * extra_out if extra_out else 0, src_mode=row['src'],
                         out_pool=pool, out_d2s=row['d2s'])


def io_dtype(row, c):
    from dlwp_amd import _lib
    code = dict(f32=_lib.F32, bf16=_lib.BF16, o8=_lib.BF16_O8)
    sin, sout = cases.storage_of(row, c)
    return _lib.dtype_io(code[sin], code[sout], row['compute_bf16'])


def launch(ops, row, c, x, w, b, act, pool, entry='fwd', extra=0, foreign=np.nan, second=False):
    """One call on fresh slabs.  x: the (n, cin, h, w) window's values; extra > 0: stored with that many foreign channels on each side,
    `foreign` in them (p3), and written into the window of an output that much wider (p4).  Returns (window, whole output, pooled
    second output's window | None), or None where the entry point has nothing for this layer (and must then have written nothing)."""
    from dlwp_amd._lib import DlwpError
    sin, sout = cases.storage_of(row, c)
    al = SECOND if second else dict.fromkeys(SECOND, 0)
    n = x.shape[0]
    oc, ho, wo = cases.out_shape(row, pool)
    xs = slab(cases.store_wide(x, extra, foreign) if extra else x, sin, al['x'])
    ws, bs = Slab(w, al['w']), Slab(b, al['b'])
    ys = slab(None, sout, al['y'], (n, oc + 2 * extra, ho, wo))
    cd = desc(ops, row, act, pool, extra, extra)
    kw = dict(x_channels=row['cin'], compute_bf16=row['compute_bf16'], in_o8=sin == 'o8', out_o8=sout == 'o8')
    y2 = None
    if entry == 'prepared':
        prep = ops.conv2d_prepare(xs.t, ws.t, cd, out_dtype=ys.t.dtype, **kw)
        if prep is None:
            return None                                            # (this route reads the HWIO weights)
        ops.conv2d(xs.t, ws.t, bs.t, cd, out=ys.t, prepared=prep, **kw)
    elif entry == 'pool2':
        y2 = Slab(None, al['y2'], (n, oc + 2 * extra, ho // 2, wo // 2))
        try:
            ran = ops.conv2d(xs.t, ws.t, bs.t, cd, out=ys.t, out_pool2=y2.t, **kw) is not None
        except DlwpError as e:              # (a forced instance without that store phase, a loader that rounds: refused by name)
            assert 'does not match the layer' in str(e) or 'no other epilogue option' in str(e), str(e)
            ran = False
        if not ran:
            assert ys.unchanged() and y2.unchanged(), 'a refused two-output launch wrote something'
            return None
    else:
        ops.conv2d(xs.t, ws.t, bs.t, cd, out=ys.t, direct=entry == 'direct', **kw)
    full = read(ys, sout)
    assert xs.unchanged() and ws.unchanged() and bs.unchanged(), 'an input was written'
    lo, hi = extra, extra + oc
    assert np.isnan(full[:, :lo]).all() and np.isnan(full[:, hi:]).all(), 'channels outside the output window were written'
    p2 = None
    if y2 is not None:
        f2 = y2.read()
        assert np.isnan(f2[:, :lo]).all() and np.isnan(f2[:, hi:]).all(), 'pooled output: channels outside the window were written'
        p2 = f2[:, lo:hi]
    return full[:, lo:hi], full, p2


def twice(ops, row, c, x, w, b, act, pool, **kw):
    """the call, then the call with every operand off the 16-byte boundary: the same bits"""
    r0 = launch(ops, row, c, x, w, b, act, pool, **kw)
    r1 = launch(ops, row, c, x, w, b, act, pool, second=True, **kw)
    if r0 is None or r1 is None:
        assert r0 is None and r1 is None
        return None
    assert same_bits(r0[1], r1[1]), 'the call on operands off the 16-byte boundary returned other bits'
    assert (r0[2] is None) == (r1[2] is None) and (r0[2] is None or same_bits(r0[2], r1[2]))
    return r0


def stored(want, sout):
    """the float64 reference as the output storage holds it"""
    return want if sout == 'f32' else np_ref.round_bf16(want)


def equal64(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), '%s: exact inputs, yet %d of %d elements differ (%d NaN), worst by %r' % (
        what, int((got != want).sum()), got.size, int(np.isnan(got).sum()),
        float(np.nanmax(np.abs(got - want))) if np.isfinite(got).any() else 'nan')


def note(table, name, value):
    table[name] = max(table.get(name, 0.0), float(value))


def family_name(row):
    return row['force']['family'] if row['force'] else row['name'].rsplit('-', 1)[0] if row['name'].startswith('ragged') else row['name']


def route_of(ops, row, c, idx, cfgs, pool, extra=0):
    """what dlwp_conv2d_launch_info reports for this launch: None where it names another route than the row's (or refuses)"""
    from dlwp_amd._lib import DlwpError
    cd = desc(ops, row, 'linear', pool, extra, extra)
    try:
        info = ops.conv_launch_info((N, row['cin'], row['h'], row['w']), cd, dtype=io_dtype(row, c))
    except DlwpError:
        return None
    got = info[0][0]
    if idx is not None:
        ok = got == idx
    elif isinstance(row['route'], str):
        ok = got >= 0 and cases.family_of(cfgs[got]) == row['route']
    else:
        ok = got == row['route']
    return info if ok else None


def pool_variants(ops, row, c, idx, cfgs):
    """without and with the pooled epilogue, where the row's route has one"""
    if row['pools'] != 'auto':
        return row['pools']
    if row['d2s'] or route_of(ops, row, c, idx, cfgs, True) is None:
        return (False,)
    if idx is None and not ops.supports_out_pool((row['cin'], row['h'], row['w']), desc(ops, row, 'linear', True, 0, 0)):
        return (False,)
    return (False, True)


def run_config(ops, row, idx, cfgs, refs):
    """every step for one launch route: the row's own, or the forced configuration idx"""
    c = None if idx is None else cfgs[idx]
    who = '%s%s' % (row['name'], '' if idx is None else ' config %d %r' % (idx, c))
    sin, sout = cases.storage_of(row, c)
    extra = cases.extra_of(row, c)
    fam = family_name(row)
    main = row['entries'][0]
    vector = main == 'direct'
    xe, we, be = refs['exact']
    xr, wr, br = refs['real']

    def ref(key, x, w, act, pool):
        k = (key, act, pool)
        if k not in refs:
            refs[k] = cases.reference(row, x, w, be if key != 'real' else br, act, pool)
            refs[k].setflags(write=False)
        return stored(refs[k], sout)
    pools = pool_variants(ops, row, c, idx, cfgs)
    POOLED.setdefault(fam, set()).update(pools)
    for pool in pools:
        # 1. route
        if not vector:
            info = route_of(ops, row, c, idx, cfgs, pool, extra)
            assert info is not None, '%s pool %d: dlwp_conv2d_launch_info names another route than the row: %r' % (
                who, pool, ops.conv_launch_info((N, row['cin'], row['h'], row['w']), desc(ops, row, 'linear', pool, extra, extra),
                                                dtype=io_dtype(row, c)))
            assert route_of(ops, row, c, idx, cfgs, pool, 0) is not None, who + ': another route without the channel windows'
            if row['split'] is not None:
                cd = desc(ops, row, 'linear', pool, extra, extra)
                assert ops.conv_split_count((N, row['cin'], row['h'], row['w']), cd, dtype=io_dtype(row, c)) == row['split'], who
            if row['loader'] is not None:
                assert info[0][5] == row['loader'], (who, info)
            elif 'wino_xloader' in row['opts']:
                print('LOADER %s: %d' % (who, info[0][5]))
        # 2. exact: the plain tensors once, then inside wider tensors with NaN around the windows (p3, p4)
        equal64(twice(ops, row, c, xe, we, be, 'linear', pool, entry=main)[0], ref('exact', xe, we, 'linear', pool), who + ' exact linear')
        x1, w1, b1 = refs['exact1']
        if ('exact1', 'relu', pool) not in refs:
            refs[('exact1', 'relu', pool)] = cases.reference(row, x1, w1, b1, 'relu', pool)
        equal64(twice(ops, row, c, x1, w1, b1, 'relu', pool, entry=main)[0], stored(refs[('exact1', 'relu', pool)], sout),
                who + ' exact relu, second seed')
        clean = {}
        for act in ('linear', 'relu'):
            res = twice(ops, row, c, xe, we, be, act, pool, entry=main, extra=extra)
            equal64(res[0], ref('exact', xe, we, act, pool), '%s exact %s in windows' % (who, act))
            clean[act] = res[0]
            # 4. (p3) finite numbers in the foreign channels: the same bits
            fin = launch(ops, row, c, xe, we, be, act, pool, entry=main, extra=extra, foreign=1.5)
            assert same_bits(fin[0], res[0]), who + ': the foreign input channels reach the result'
        entries = row['entries'][1:]
        if not pool and not vector and not row['d2s'] and (sin, sout) == ('f32', 'f32') and 'pool2' not in entries:
            entries += ('pool2',)               # the two-output launch: wherever the route stores both (else refused, nothing written)
        for entry in entries:
            res = twice(ops, row, c, xe, we, be, 'relu', pool, entry=entry, extra=extra)
            FORMS.setdefault((fam, entry), set()).add(res is not None)
            if res is None:
                assert not (entry == 'pool2' and entry in row['entries']), who + ': the row names the two-output launch'
                continue
            equal64(res[0], ref('exact', xe, we, 'relu', pool), '%s exact relu, %s' % (who, entry))
            if entry == 'pool2':
                equal64(res[2], np_ref.maxpool2(ref('exact', xe, we, 'relu', pool)), who + ' exact relu, pooled second output')
        # 3. tanh on random reals (and p3 / p4 once more, on values with round-off)
        ref('real', xr, cases.multiplied_weights(row, wr), 'tanh', pool)
        want = refs[('real', 'tanh', pool)]                      # (unrounded: a bfloat16 output is held to one ulp of it, as today)
        res = twice(ops, row, c, xr, wr, br, 'tanh', pool, entry=main, extra=extra)
        fin = launch(ops, row, c, xr, wr, br, 'tanh', pool, entry=main, extra=extra, foreign=-2.5)
        assert same_bits(fin[0], res[0]), who + ': the foreign input channels reach the tanh result'
        err = np.abs(res[0].astype(np.float64) - want)
        if sout == 'f32':
            ratio = err.max() / (cases.FWD_TOL * max(1.0, np.abs(want).max()))
        else:
            ratio = (err / (2.0 ** -8 * np.abs(want) + 2e-6)).max()
        note(WORST, '%s%s tanh error / %s' % (fam, ' pooled' if pool else '', 'FWD_TOL' if sout == 'f32' else 'bf16 ulp'), ratio)
        assert ratio <= 1.0, (who, pool, ratio)
        # 4. / 5. a poisoned sample between two clean ones
        two = launch(ops, row, c, xe[[0, 2]], we, be, 'relu', pool, entry=main, extra=extra)
        assert same_bits(two[0], clean['relu'][[0, 2]]), who + ': samples 0 and 2 as a batch of 2 differ from the batch of 3'
        for pat, act in (('p1', 'linear'), ('p1', 'relu'), ('p2', 'relu')):
            xp = cases.poison_p1(xe) if pat == 'p1' else cases.poison_p2(row, xe)
            want = ref(pat, xp, we, act, pool)
            got = twice(ops, row, c, xp, we, be, act, pool, entry=main, extra=extra)[0]
            nan_w, nan_g = np.isnan(want), np.isnan(got)
            assert not nan_g[[0, 2]].any(), '%s %s %s: NaN left the poisoned sample' % (who, pat, act)
            assert same_bits(got[[0, 2]], clean[act][[0, 2]]), '%s %s %s: the clean samples changed' % (who, pat, act)
            lost = int((nan_w & ~nan_g).sum())
            assert lost == 0, '%s %s %s pool %d: %d of %d NaN of the reference came out finite (first values %r)' % (
                who, pat, act, pool, lost, int(nan_w.sum()), got[nan_w & ~nan_g][:4])
            if pat == 'p1':
                assert nan_g[1].all()
            equal64(got[~nan_g], want[~nan_g], '%s %s %s: beside the NaN' % (who, pat, act))
            if pat == 'p2':
                share = float((nan_g[1] & ~nan_w[1]).sum()) / nan_g[1].size
                note(SPREAD, '%s%s' % (fam, ' pooled' if pool else ''), share)
                if vector:
                    print('MASKS %s: dlwp_conv2d_fwd_direct NaN mask %s the reference mask' % (
                        who, 'equals' if np.array_equal(nan_g, nan_w) else 'differs from'))
    REACHED.add(-1 if vector else idx if idx is not None else ops.conv_launch_info(
        (N, row['cin'], row['h'], row['w']), desc(ops, row, 'linear', pools[0], 0, 0), dtype=io_dtype(row, c))[0][0])


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_forward_route(ops, row):
    cfgs = ops.conv_configs()
    xe, we, be = cases.exact_inputs(row)
    assert cases.exact_measure(row, xe, we, be) < cases.LIMIT
    refs = dict(exact=(xe, we, be), exact1=cases.exact_inputs(row, 1), real=cases.real_inputs(row))
    forced = cases.forced_configs(row, cfgs) if row['force'] else [None]
    assert forced, 'no compiled configuration of this family'
    failed = []
    for idx in forced:
        with options(ops, row, idx):
            try:
                run_config(ops, row, idx, cfgs, refs)
            except AssertionError as e:                         # (every configuration of the family is tried: all findings at once)
                failed.append('%s' % (str(e)[:600],))
    torch.cuda.synchronize()
    assert not failed, '%d of %d routes:\n%s' % (len(failed), len(forced), '\n'.join(failed))


# ---- the two ConvLSTM2D pins: containment under (p1); what sample 1 becomes is printed (the hard-sigmoid clamp turns NaN into 0) ---- #

LSTM_ROWS = [(16, (16, 24), False, 1), (16, (16, 24), False, 2), (24, (20, 72), True, 2), (16, (16, 24), True, 1)]


def lstm_row_of(c):
    """the pin that forces cell-update instance c"""
    for r in LSTM_ROWS:
        if c[1] == r[3] and (c[8] == 3) == r[2]:
            return r
    return None


def lstm_launch(ops, row, c, x, w, b, zadd, cprev, second):
    f, (h, w_), first, dil = row
    in8, sw = bool(c is not None and c[10] & 8), bool(c is not None and c[10] & 16)
    al = SECOND if second else dict.fromkeys(SECOND, 0)
    n = x.shape[0]
    halo = (dil, dil, dil, dil, 0, 1) if first else (dil, dil, dil, dil, 0, 0)
    cd = ops.make_conv(4 * f, 3, 3, dil, ops.make_pad(*halo), ops.ACT_TANH, out_c_off=8, out_c_total=f + 16, lstm_f=f)
    xs = slab(x, 'f32' if first else ('o8' if in8 else 'bf16'), al['x'])
    ws, bs = Slab(w, al['w']), Slab(b, al['b'])
    hs = slab(None, 'o8' if sw else 'bf16', al['y'], (n, f + 16, h, w_))
    cs = Slab(None, al['c_out'], (n, f, h, w_))
    zs = None if zadd is None else slab(zadd, 'o8' if sw else 'bf16', al['z'])
    cp = None if cprev is None else Slab(to_o8(cprev) if sw else cprev, al['c'])
    ops.convlstm_conv(xs.t, ws.t, bs.t, cd, hs.t, cs.t, z_add=None if zs is None else zs.t, c_prev=None if cp is None else cp.t,
                      compute_bf16=first, in_o8=in8, out_o8=sw)
    hh, cc = read(hs, 'o8' if sw else 'bf16'), cs.read()
    cc = from_o8(cc) if sw else cc
    assert xs.unchanged() and ws.unchanged() and bs.unchanged() and (zs is None or zs.unchanged()) and (cp is None or cp.unchanged())
    assert np.isnan(hh[:, :8]).all() and np.isnan(hh[:, 8 + f:]).all(), 'h channels outside the window were written'
    return hh[:, 8:8 + f], cc


@pytest.mark.parametrize('row', LSTM_ROWS, ids=['f%d-%dx%d-%s-d%d' % (r[0], r[1][0], r[1][1], 'input' if r[2] else 'recurrent', r[3])
                                                for r in LSTM_ROWS])
def test_convlstm_conv_keeps_a_nan_sample_to_itself(ops, row):
    """ops.convlstm_conv, the heuristic's instance and every compiled cell-update instance of the geometry (octet layouts included):
    with sample 1 of the input all NaN, samples 0 and 2 of h and c keep the bits of the clean run"""
    from dlwp_amd._lib import DlwpError
    f, (h, w_), first, dil = row
    rng = np.random.default_rng([f, h, int(first), dil])
    cin = 6 if first else f
    x = np_ref.round_bf16(rng.standard_normal((N, cin, h, w_))).astype(np.float32)
    w = np.asarray(np_ref.glorot_uniform((3, 3, cin, 4 * f), rng), np.float32)
    b = (0.1 * rng.standard_normal(4 * f)).astype(np.float32)
    zadd = None if first else np_ref.round_bf16(0.5 * rng.standard_normal((N, 4 * f, h, w_))).astype(np.float32)
    cprev = None if first else rng.standard_normal((N, f, h, w_)).astype(np.float32)
    cfgs = ops.conv_configs()
    todo = [None] + [i for i, c in enumerate(cfgs) if cases.family_of(c) == 'cell-update' and lstm_row_of(c) == row]
    assert len(todo) > 1
    failed = []
    for idx in todo:
        c = None if idx is None else cfgs[idx]
        try:
            ops.force_conv_config(-1 if idx is None else idx)
            try:
                runs = [[lstm_launch(ops, row, c, xx, w, b, zadd, cprev, second) for second in (False, True)]
                        for xx in (x, cases.poison_p1(x))]
            except DlwpError as e:
                if idx is not None and 'does not match the layer' in str(e):
                    WHOLE_STEP.add(idx)                       # (test_case_table_reaches_every_route accounts for these)
                else:
                    failed.append('config %r %r refused the layer: %s' % (idx, c, str(e)[:200]))
                continue
            for (h0, c0), (h1, c1) in runs:
                assert same_bits(h0, h1) and same_bits(c0, c1), 'operands off the 16-byte boundary: other bits'
            (hc, cc), (hp, cp) = runs[0][0], runs[1][0]
            assert np.isfinite(hc).all() and np.isfinite(cc).all()
            assert same_bits(hp[[0, 2]], hc[[0, 2]]) and same_bits(cp[[0, 2]], cc[[0, 2]]), 'config %r: the clean samples changed' % (idx,)
            print('LSTM %r config %r: poisoned sample 1 becomes h %d NaN of %d (others in [%g, %g]), c %d NaN of %d' % (
                row, idx, int(np.isnan(hp[1]).sum()), hp[1].size, np.nanmin(hp[1]) if np.isfinite(hp[1]).any() else np.nan,
                np.nanmax(hp[1]) if np.isfinite(hp[1]).any() else np.nan, int(np.isnan(cp[1]).sum()), cp[1].size))
            if idx is not None:
                REACHED.add(idx)
        except AssertionError as e:
            failed.append('config %r: %s' % (idx, str(e)[:300]))
        finally:
            ops.force_conv_config(-1)
    assert not failed, '\n'.join(failed)


@pytest.mark.parametrize('f,cx,h,w', cases.LSTM_STEP_ROWS)
def test_convlstm_step_keeps_a_nan_sample_to_itself(ops, f, cx, h, w):
    """ops.convlstm_step (one launch: recurrent + input convolution + cell update, octet layout) under (p1) on the state x"""
    rng = np.random.default_rng(100 + f)
    x = rng.standard_normal((N, 2 * cx, h, w)).astype(np.float32)
    hseq = np_ref.round_bf16(0.5 * rng.standard_normal((N, 2 * f, h, w))).astype(np.float32)
    cp = rng.standard_normal((N, f, h, w)).astype(np.float32)
    w_h = np.asarray(np_ref.glorot_uniform((3, 3, f, 4 * f), rng), np.float32)
    w_x = np.asarray(np_ref.glorot_uniform((3, 3, cx, 4 * f), rng), np.float32)
    b = (0.1 * rng.standard_normal(4 * f)).astype(np.float32)

    def run(xx, second):
        al = SECOND if second else dict.fromkeys(SECOND, 0)
        cd_h = ops.make_conv(4 * f, 3, 3, 1, ops.make_pad(1, 1, 1, 1, 0, 0), ops.ACT_TANH, in_c_off=0, in_c_total=2 * f, out_c_off=f,
                             out_c_total=2 * f, lstm_f=f, lstm_rec_act=0)
        cd_x = ops.make_conv(4 * f, 3, 3, 2, ops.make_pad(2, 2, 2, 2, 0, 1), ops.ACT_LINEAR, in_c_off=cx, in_c_total=2 * cx)
        assert ops.convlstm_step_supported((f, h, w), cd_h, (cx, h, w), cd_x)
        hs, xs = slab(hseq, 'o8', al['y']), Slab(xx, al['x'])
        whs, wxs, bs = Slab(w_h, al['w']), Slab(w_x, al['z']), Slab(b, al['b'])
        cps, cs = Slab(to_o8(cp), al['c']), Slab(None, al['c_out'], (N, f, h, w))
        ops.convlstm_step(hs.t, xs.t, whs.t, wxs.t, bs.t, cd_h, cd_x, cps.t, cs.t, cx)
        hh, cc = read(hs, 'o8'), from_o8(cs.read())
        assert xs.unchanged() and whs.unchanged() and wxs.unchanged() and bs.unchanged() and cps.unchanged()
        assert same_bits(hh[:, :f], hseq[:, :f]), 'the step wrote outside its window of the h sequence'
        return hh[:, f:], cc
    clean, clean2 = run(x, False), run(x, True)
    pois, pois2 = run(cases.poison_p1(x), False), run(cases.poison_p1(x), True)
    assert same_bits(clean[0], clean2[0]) and same_bits(clean[1], clean2[1]) and same_bits(pois[0], pois2[0]) and same_bits(pois[1], pois2[1])
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
    assert same_bits(pois[0][[0, 2]], clean[0][[0, 2]]) and same_bits(pois[1][[0, 2]], clean[1][[0, 2]]), 'the clean samples changed'
    STEP_RAN.append(f)
    print('LSTM step f=%d: poisoned sample 1 becomes h %d NaN of %d, c %d NaN of %d' % (
        f, int(np.isnan(pois[0][1]).sum()), pois[0][1].size, int(np.isnan(pois[1][1]).sum()), pois[1][1].size))


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
def test_maxpool2_propagates_nan_from_every_window_position(ops, storage):
    """ops.maxpool2 at (2, 3, 5, 7): a NaN in each of the four window positions in turn comes out as NaN, as np.max gives it"""
    rng = np.random.default_rng(5)
    base = cases.DENSE_VALUES[rng.integers(0, 4, size=(2, 3, 5, 7))]
    for a in (0, 1):
        for b in (0, 1):
            x = base.copy()
            x[:, :, a:4:2, b:6:4] = np.nan                 # windows (0..1, 0) and (0..1, 2) of every plane
            x[1, 2, 2 + a, 2 + b] = np.nan
            want = np_ref.maxpool2(x.astype(np.float64))
            assert np.isnan(want).sum() == 2 * 3 * 4 + 1
            outs = []
            for second in (False, True):
                xs = slab(x, storage, SECOND['x'] if second else 0)
                ys = slab(None, storage, SECOND['y'] if second else 0, (2, 3, 2, 3))
                ops.maxpool2(xs.t, out=ys.t)
                outs.append(read(ys, storage))
                assert xs.unchanged()
            assert same_bits(outs[0], outs[1])
            assert np.array_equal(np.isnan(outs[0]), np.isnan(want)), (storage, a, b, outs[0], want)
            ok = ~np.isnan(want)
            assert np.array_equal(outs[0][ok].astype(np.float64), want[ok])


def test_model_with_a_relu_layer_keeps_a_nan_sample_to_itself(ops):
    """The preset U-Net with one ReLU layer swapped in, 16 x 36, batch of 3: predict with sample 1 all NaN returns an all-NaN sample
    1 and the bits of the clean run for samples 0 and 2; the same through rollout_on_device for 2 forwards."""
    from dlwp_amd.model import DLWPNeuralNet
    from dlwp_amd.presets import unet_layers
    cs = (4, 16, 36)
    layers = [list(l) for l in unet_layers(cs)]
    convs = [i for i, l in enumerate(layers) if l[0] == 'Conv2D']
    layers[convs[1]][2] = dict(layers[convs[1]][2], activation='relu')           # the 32 -> 64 layer behind the first MaxPooling2D
    np.random.seed(7)
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=2, scaler_type=None, scale_targets=False)
    d.build_model(tuple(tuple(l) for l in layers), loss='mse', optimizer='adam', metrics=['mae'])
    rng = np.random.default_rng(8)
    x = rng.standard_normal((3,) + cs).astype(np.float32)
    xp = cases.poison_p1(x)
    clean, pois = d.predict(x), d.predict(xp)
    assert np.isfinite(clean).all()
    assert np.isnan(pois[1]).all(), '%d of %d values of the NaN sample came out finite' % (int(np.isfinite(pois[1]).sum()), pois[1].size)
    assert same_bits(pois[[0, 2]], clean[[0, 2]])
    sc = d.model.rollout_on_device(torch.from_numpy(x).cuda(), 2).cpu().numpy()
    sp = d.model.rollout_on_device(torch.from_numpy(xp).cuda(), 2).cpu().numpy()
    assert sc.shape[:2] == (2, 3) and np.isfinite(sc).all()
    assert np.isnan(sp[:, 1]).all() and same_bits(sp[:, [0, 2]], sc[:, [0, 2]])


def test_case_table_reaches_every_route(ops):
    """Every index of conv_configs() belongs to a forced row of the table -- the ConvLSTM2D cell-update instances to a pin above --
    and every negative route code the table names is there.  With the whole file run, every one of them was launched and had
    reported itself (a row that silently fell back to another kernel fails here); the cell-update instances that
    dlwp_convlstm_conv_fwd refuses are the whole-step ones, which only dlwp_convlstm_step_fwd launches (the step pin)."""
    cfgs = ops.conv_configs()
    owned = {}
    for row in ROWS:
        if row['force']:
            for i in cases.forced_configs(row, cfgs):
                owned.setdefault(i, []).append(row['name'])
    for i, c in enumerate(cfgs):
        if cases.family_of(c) == 'cell-update':
            assert lstm_row_of(c) is not None, (i, c)
        else:
            assert i in owned, 'configuration %d %r belongs to no row of the table' % (i, c)
    named = {r['route'] for r in ROWS if isinstance(r['route'], int)}
    assert named == {cases.R_VECTOR, cases.R_FEW_STREAM, cases.R_FLAT, cases.R_FEW_WINO}
    if len(REACHED) > len(named):                                # (the parametrised tests above ran in this session)
        print('WHOLE-STEP instances (dlwp_convlstm_step_fwd only): %r' % sorted(WHOLE_STEP))
        missing = [i for i in range(len(cfgs)) if i not in REACHED and i not in WHOLE_STEP] + [r for r in named if r not in REACHED]
        assert not missing, 'never launched: %r' % missing
        assert all(cfgs[i][10] & 24 == 24 for i in WHOLE_STEP) and (not WHOLE_STEP or STEP_RAN), 'whole-step instances: octets in and out'


def test_report():
    """prints this session's worst tanh error / bound ratios and NaN spread shares per family (`-s`)"""
    for k in sorted(WORST):
        print('MEASURED %s: %.4g' % (k, WORST[k]))
    for k in sorted(SPREAD):
        print('SPREAD %s: NaN beyond the reference footprint on at most %.4g of the poisoned sample' % (k, SPREAD[k]))
    for k in sorted(FORMS):
        print('ENTRY %s, %s: %s' % (k[0], k[1], 'ran' if FORMS[k] == {True} else 'no such form' if FORMS[k] == {False} else
                                    'ran on some routes of the family'))
    for k in sorted(POOLED):
        print('POOLED %s: %s' % (k, 'with and without the pooled epilogue' if len(POOLED[k]) == 2 else
                                 ('pooled only' if True in POOLED[k] else 'no pooled epilogue')))
