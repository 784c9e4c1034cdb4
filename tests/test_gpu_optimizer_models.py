"""The Keras optimizers and gradient clipping through compile() / train_on_batch on a small model (config 1's two 5 x 5 convolutions,
2 x 12 x 16, 4 samples): the update the trainer issues against the float64 oracles of tests/test_keras_optimizers_cpu.py, which
optimizers replay as a recorded step and which stay eager, clipnorm on the whole gradient, and save -> load -> continue.
Reference: compile(optimizer=...) of examples/train.py:240 with any keras.optimizers class; Keras 2.2.4 get_updates / get_gradients."""
import numpy as np
import pytest
import torch

from tests.nets import cnn2_layers
from tests.test_gpu_model import _build, _weights_of
from tests.test_keras_optimizers_cpu import KINDS, NAMES, clip_oracle, oracle, step_scalars
from tests.test_optimizers_cpu import U, f32, worst_ratio

pytestmark = pytest.mark.gpu

CS = (2, 12, 16)
N = 4
STEPS = 5                      # steps 1-2 eager (graph_after = 2), step 3 recorded (+ validated by a replay), steps 4-5 replayed


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _optimizers():
    from dlwp_amd import training as T
    return {'sgd_nesterov': lambda: T.SGD(lr=0.01, momentum=0.9, nesterov=True), 'rmsprop': T.RMSprop, 'adagrad': T.Adagrad,
            'adadelta': T.Adadelta, 'adam_amsgrad': lambda: T.Adam(amsgrad=True), 'adamax': T.Adamax, 'nadam': T.Nadam,
            'rmsprop_clipped': lambda: T.RMSprop(clipnorm=1e-2, clipvalue=1e-3),
            'adam_clipvalue': lambda: T.Adam(clipvalue=1e-3), 'sgd_clipnorm': lambda: T.SGD(momentum=0.9, clipnorm=1e-2),
            'rmsprop_decay': lambda: T.RMSprop(decay=1e-3)}


REPLAYED = ('sgd_nesterov', 'rmsprop', 'adagrad', 'adadelta', 'rmsprop_clipped', 'sgd_clipnorm')
EAGER = ('adam_amsgrad', 'adamax', 'nadam', 'adam_clipvalue', 'rmsprop_decay')


def _batches(seed, count=STEPS):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((N,) + CS).astype(np.float32), rng.standard_normal((N,) + CS).astype(np.float32))
            for _ in range(count)]


def _model(name, seed=3):
    d = _build(cnn2_layers(CS, hidden=8), time_dim=2, seed=seed, optimizer=_optimizers()[name]())
    _weights_of(d.model, np.random.default_rng(30))
    return d


def _env(monkeypatch, form):
    for k in ('DLWP_TRAIN_GRAPH', 'DLWP_TRAIN_STEP', 'DLWP_TRAIN_LANES'):
        monkeypatch.delenv(k, raising=False)
    if form == 'eager':
        monkeypatch.setenv('DLWP_TRAIN_GRAPH', '0')
    else:
        monkeypatch.setenv('DLWP_TRAIN_STEP', form)


def _hyper(opt):
    """(kind name, float32-rounded hyper-parameters as the oracle takes them, decay, m_schedule) of an optimizer object"""
    args = dict(opt.step_args())
    ms = args.pop('m_schedule', 1.0)
    decay = f32(args.pop('decay', 0.0))
    return KINDS[opt.step_kind()], {k: f32(v) for k, v in args.items()}, decay, ms


@pytest.mark.parametrize('name', sorted(_optimizers()))
def test_one_eager_step_is_the_oracle_step_on_the_steps_own_gradient(monkeypatch, name):
    """train_on_batch once, launch by launch: the parameters after it equal the float64 oracle applied to the parameters before, the
    step's flat gradient and zero slots, inside the kernel's derived bounds; the slots too; the counters advanced."""
    _env(monkeypatch, 'eager')
    d = _model(name)
    tr, opt = d.model._trainer, d.model.optimizer
    p0 = tr.flat_params.cpu().numpy().copy()
    x, y = _batches(50, 1)[0]
    d.model.train_on_batch(x, y)
    torch.cuda.synchronize()
    kind, hyper, decay, ms = _hyper(_optimizers()[name]())
    g = tr.flat_grads.cpu().numpy().copy()
    assert np.abs(g).max() > 0 and len(tr.opt_state) == opt.n_slots()
    clipnorm, clipvalue = opt.clips()
    factor = None
    if clipnorm > 0:
        got = tr._clip_out.cpu().numpy()
        want, bound = clip_oracle(g, 1.0, f32(clipnorm))
        assert want[1] > 10 * clipnorm                                  # the threshold is far below the norm
        for a, w, b in zip(got, want, bound):
            assert abs(float(a) - w) <= b
        factor = got[0]
    sc = step_scalars(kind, hyper, decay, 0, ms)
    want, bound = oracle(kind, p0, [np.zeros_like(p0)] * opt.n_slots(), g, sc, hyper, 1.0, f32(clipvalue), factor)
    got = [tr.flat_params.cpu().numpy()] + [s.cpu().numpy() for s in tr.opt_state]
    worst = {}
    for nm, a, w, b in zip(NAMES[kind], got, want, bound):
        worst[nm] = worst_ratio(a, w, b, '%s %s' % (name, nm))
        assert worst[nm] <= 1.0, (name, nm, worst[nm])
    print('\nMEASURED %s model step: worst error/bound %s' % (name, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert not np.array_equal(got[0], p0) and opt.iterations == 1
    if name == 'nadam':
        assert opt.m_schedule == pytest.approx(0.9 * (1 - 0.5 * 0.96 ** 0.004), rel=1e-6)


def _run(monkeypatch, name, form, batches):
    _env(monkeypatch, form)
    d = _model(name)
    tr = d.model._trainer
    logs = [d.model.train_on_batch(x, y) for x, y in batches]
    torch.cuda.synchronize()
    return {'weights': [w.copy() for w in d.model.get_weights()], 'logs': logs, 'slots': [s.cpu().numpy().copy() for s in tr.opt_state],
            'iterations': d.model.optimizer.iterations, 'last_grads': tr.flat_grads.cpu().numpy().copy(), 'trainer': tr}


def _assert_same(got, ref, what):
    """(the comparison of tests/test_gpu_train_steps.py::_assert_same)"""
    assert got['iterations'] == ref['iterations'] == STEPS
    for a, b in zip(got['logs'], ref['logs']):
        assert np.allclose(a, b, rtol=1e-5, atol=1e-7), (what, a, b)
    for a, b in zip(got['weights'], ref['weights']):
        assert np.abs(a - b).max() <= 2e-7 * STEPS, what
    assert len(got['slots']) == len(ref['slots']) > 0
    for a, b in zip(got['slots'], ref['slots']):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), what
    assert np.abs(got['last_grads'] - ref['last_grads']).max() <= 1e-5 * np.abs(ref['last_grads']).max(), what


@pytest.mark.parametrize('name', REPLAYED)
def test_step_independent_optimizers_replay_as_a_recorded_step(monkeypatch, name):
    """Five steps under DLWP_TRAIN_STEP=graph against DLWP_TRAIN_GRAPH=0: the step was recorded (update and clip pass on the tape,
    the factor on the device), validated and replayed, and leaves what the eager steps leave."""
    batches = _batches(60)
    ref = _run(monkeypatch, name, 'eager', batches)
    assert not ref['trainer']._graphs
    got = _run(monkeypatch, name, 'graph', batches)
    tr = got['trainer']
    ents = [e for k, e in tr._graphs.items() if k[0] == N and e.get('step') is not None]
    assert len(ents) == 1, 'the step was not recorded (refused: %r)' % (tr._no_tape,)
    assert tr._graph_ok(N) == 'graph'
    _assert_same(got, ref, name)
    assert not all(np.array_equal(a, b) for a, b in zip(got['weights'], _model(name).model.get_weights()))


@pytest.mark.parametrize('name', EAGER)
def test_step_dependent_optimizers_stay_eager(monkeypatch, name):
    """Adamax, Nadam, amsgrad or clipped Adam and anything with decay > 0 carry step-dependent launch arguments: asked for the graph
    form they still run launch by launch -- nothing recorded, nothing refused -- with the bits of the DLWP_TRAIN_GRAPH=0 run."""
    batches = _batches(61)
    ref = _run(monkeypatch, name, 'eager', batches)
    got = _run(monkeypatch, name, 'graph', batches)
    tr = got['trainer']
    assert tr._graph_ok(N) is False and not tr._graphs and not tr._no_tape
    assert got['iterations'] == STEPS
    for a, b in zip(got['weights'] + got['slots'], ref['weights'] + ref['slots']):
        assert np.array_equal(a, b)


def test_a_changed_hyper_parameter_never_replays_the_old_arguments(monkeypatch):
    """rho and clipnorm are launch arguments of the recorded step: changing either makes a new key, the steps run eagerly again
    until the new shape is recorded, and the result is that of a run that was eager throughout."""
    from dlwp_amd import training as T
    batches = _batches(62, 8)

    def run(form):
        _env(monkeypatch, form)
        d = _build(cnn2_layers(CS, hidden=8), time_dim=2, seed=3, optimizer=T.RMSprop(clipnorm=1e-2))
        _weights_of(d.model, np.random.default_rng(30))
        for i, (x, y) in enumerate(batches):
            if i == 4:
                d.model.optimizer.rho = 0.5
                d.model.optimizer.clipnorm = 2e-2
            d.model.train_on_batch(x, y)
        torch.cuda.synchronize()
        return d
    ref, got = run('eager'), run('graph')
    keys = [k for k, e in got.model._trainer._graphs.items() if e.get('step') is not None]
    assert len(keys) == 2 and keys[0][3] != keys[1][3]
    for a, b in zip(got.model.get_weights(), ref.model.get_weights()):
        assert np.abs(a - b).max() <= 2e-7 * len(batches)


def test_clipnorm_far_below_the_gradient_norm_sets_the_norm_of_the_update(monkeypatch):
    """SGD(lr=1, momentum=0) writes v = -g^ into its slot with no rounding of its own, so the slot IS the gradient the update saw.
    Its norm must be clipnorm: each element carries one rounding of the multiplication by the factor (u), the factor the 2u of its
    bound (tests/test_keras_optimizers_cpu.py) -- |norm - clipnorm| <= 3u clipnorm, + 1u of slack as everywhere."""
    from dlwp_amd import training as T
    _env(monkeypatch, 'eager')
    c = f32(1e-3)
    d = _build(cnn2_layers(CS, hidden=8), time_dim=2, seed=3, optimizer=T.SGD(lr=1.0, momentum=0.0, clipnorm=c))
    _weights_of(d.model, np.random.default_rng(30))
    tr = d.model._trainer
    x, y = _batches(63, 1)[0]
    d.model.train_on_batch(x, y)
    torch.cuda.synchronize()
    g = tr.flat_grads.cpu().numpy().astype(np.float64)
    raw = float(np.sqrt((g * g).sum()))
    assert raw > 100 * c
    seen = tr.opt_state[0].cpu().numpy().astype(np.float64)
    norm = float(np.sqrt((seen * seen).sum()))
    print('\nMEASURED clipped model step: raw norm %.6g, clipnorm %.6g, norm of the seen gradient %.9g (error / bound %.3f)'
          % (raw, c, norm, abs(norm - c) / (4 * U * c)))
    assert abs(norm - c) <= 4 * U * c
    # the loss table in the tail of the exchange buffer is not part of the norm
    assert float(tr._clip_out[1].item()) == pytest.approx(raw, rel=1e-6)
    # without clipnorm the same step moves the weights by the raw gradient
    d2 = _build(cnn2_layers(CS, hidden=8), time_dim=2, seed=3, optimizer=T.SGD(lr=1.0, momentum=0.0))
    _weights_of(d2.model, np.random.default_rng(30))
    d2.model.train_on_batch(x, y)
    assert float(d2.model._trainer.opt_state[0].double().norm().item()) == pytest.approx(raw, rel=1e-6)


@pytest.mark.parametrize('name,fmt', [('adadelta', 'npz'), ('adadelta', 'keras'), ('adam_amsgrad', 'npz'), ('adam_amsgrad', 'keras'),
                                      ('nadam', 'npz')])
def test_save_load_continue_gives_the_bits_of_the_uninterrupted_run(monkeypatch, tmp_path, name, fmt):
    """3 eager steps, save (this package's npz archive / Keras HDF5), load, 3 more: weights, every slot and `iterations` are those
    of the uninterrupted eager run, bit for bit.  amsgrad-Adam's HDF5 file holds real vhat arrays in place of the (1,)
    placeholders; Nadam's m_schedule rides in the npz archive only (a Keras file re-starts it at 1, as Keras does)."""
    from dlwp_amd import hdf5_lite, serialization
    _env(monkeypatch, 'eager')
    batches = _batches(64, 6)
    whole = _model(name)
    for x, y in batches:
        whole.model.train_on_batch(x, y)
    part = _model(name)
    for x, y in batches[:3]:
        part.model.train_on_batch(x, y)
    path = str(tmp_path / ('ckpt.' + fmt))
    part.model.save(path, format=fmt)
    n_par = len(part.model._trainer.entries)
    if fmt == 'keras':
        f = hdf5_lite.File(path)
        names = [n.decode() for n in np.asarray(f['optimizer_weights'].attrs['weight_names']).reshape(-1)]
        cls = type(part.model.optimizer).__name__
        assert names[0] == '%s/iterations:0' % cls and len(names) == 1 + part.model.optimizer.n_slots() * n_par
        shapes = [tuple(e[4]) for e in part.model._trainer.entries]
        assert [tuple(np.asarray(f['optimizer_weights'][nm][...]).shape) for nm in names[1:]] == \
            shapes * part.model.optimizer.n_slots()
    again = serialization.load_model_file(path)
    opt = again.optimizer
    assert type(opt) is type(part.model.optimizer) and vars(opt) == vars(part.model.optimizer) and opt.iterations == 3
    for a, b in zip(part.model._trainer.opt_state, again._trainer.opt_state):
        assert torch.equal(a, b)
    for x, y in batches[3:]:
        again.train_on_batch(x, y)
    torch.cuda.synchronize()
    assert opt.iterations == whole.model.optimizer.iterations == 6
    assert len(again._trainer.opt_state) == len(whole.model._trainer.opt_state) == opt.n_slots()
    for a, b in zip(whole.model.get_weights(), again.get_weights()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in zip(whole.model._trainer.opt_state, again._trainer.opt_state):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    if name == 'nadam':
        assert opt.m_schedule == whole.model.optimizer.m_schedule
