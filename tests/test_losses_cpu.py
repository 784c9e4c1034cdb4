"""The Keras regression losses and metrics beyond 'mse' / 'mae' (mae, mape, msle, logcosh as losses; anomaly_correlation and the
package's loss objects as metrics; DLWP.custom.LatitudeWeightedLoss): name resolution, log names, the class's latitude weights,
model files and the loss-table column mapping -- everything that needs no GPU."""
import os

import numpy as np
import pytest
import torch

from dlwp_amd import custom as C
from dlwp_amd import layers as L
from dlwp_amd import serialization, training
from dlwp_amd.engine import Model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def small_net(outputs=1):
    x0 = L.Input(shape=(2, 8, 12))
    outs = [L.Conv2D(2, 3, padding='same', data_format='channels_first', name='out%d' % k)(x0) for k in range(outputs)]
    return Model(inputs=x0, outputs=outs if outputs > 1 else outs[0], device=torch.device('cpu'))


def test_loss_names_and_aliases_resolve_to_the_kernel_kinds():
    import dlwp_amd.compat  # noqa: F401
    import keras.losses
    import keras.metrics
    table = {0: ('mse', 'MSE', 'mean_squared_error'), 1: ('mae', 'MAE', 'mean_absolute_error'),
             2: ('mape', 'MAPE', 'mean_absolute_percentage_error'), 3: ('msle', 'MSLE', 'mean_squared_logarithmic_error'),
             4: ('logcosh',)}
    for kind, names in table.items():
        for nm in names:
            assert C.loss_kind(nm) == kind
            assert C.loss_kind(getattr(keras.losses, nm)) == kind
            assert getattr(keras.metrics, nm) is getattr(keras.losses, nm)
        assert getattr(keras.losses, names[-1]).__name__ == C.KIND_NAMES[kind]
    assert training._loss_name('mse') == 'mse' and training._loss_name(keras.losses.mean_squared_error) == 'mse'
    assert training._loss_name('mae') == 'elementwise' and training._loss_name(training.logcosh) == 'elementwise'
    assert training._loss_name(C.acc_loss) == 'custom'
    with pytest.raises(NotImplementedError):
        training._loss_name('cosine_proximity')
    with pytest.raises(NotImplementedError):
        small_net().compile('adam', loss='mse', metrics=['cosine_proximity'])


def test_metric_names_follow_keras_single_and_multi_output():
    m = small_net()
    m.compile('adam', loss='mae', metrics=['logcosh', 'MAPE', C.anomaly_correlation, 'mse', 'mean_squared_logarithmic_error',
                                           C.acc_loss])
    assert m.metrics_names == ['loss', 'logcosh', 'mean_absolute_percentage_error', 'anomaly_correlation',
                               'mean_squared_error', 'mean_squared_logarithmic_error', 'acc_loss']
    m2 = small_net(2)
    m2.compile('adam', loss='logcosh', metrics=['mae', C.anomaly_correlation], loss_weights=[1.0, 0.5])
    assert m2.metrics_names == ['loss', 'out0_loss', 'out1_loss', 'out0_mean_absolute_error', 'out0_anomaly_correlation',
                                'out1_mean_absolute_error', 'out1_anomaly_correlation']
    # only today's metrics: the table keeps its 7 columns
    m3 = small_net()
    m3.compile('adam', loss='mse', metrics=['mae'])
    assert m3._trainer.n_cols == 7 and m3._trainer._metric_mask == 0
    m3.compile('adam', loss=C.acc_loss, metrics=['mae', 'mse'])
    assert m3._trainer.n_cols == 7


def test_latitude_weighted_loss_class_weights_and_refusals():
    lats = np.linspace(-88.5, 88.5, 60)
    r = np.deg2rad(lats)
    cos = C.LatitudeWeightedLoss('mae', lats)
    np.testing.assert_allclose(cos.row_weights, np.cos(r), rtol=1e-6, atol=1e-7)
    mid = C.LatitudeWeightedLoss(training.logcosh, lats, weighting='midlatitude')
    np.testing.assert_allclose(mid.row_weights, np.cos(r) - 0.25 * np.sin(2 * r), rtol=1e-6, atol=1e-6)
    # the function form keeps its own formula
    np.testing.assert_allclose(C.latitude_weights(lats, 'midlatitude'), np.cos(r) + 0.5 * np.sin(2 * r) ** 2, rtol=1e-6, atol=1e-6)
    assert cos.__name__ == mid.__name__ == 'latitude_weighted_loss'
    assert (cos.kind, cos.inner) == (0, 1) and (mid.kind, mid.inner) == (0, 4)
    mse = C.LatitudeWeightedLoss('mse', lats)
    assert (mse.kind, mse.inner) == (0, 0)
    acc = C.LatitudeWeightedLoss(C.anomaly_correlation_loss(), lats)
    assert (acc.kind, acc.regularize, acc.inner) == (1, 1, 0)
    with pytest.raises(NotImplementedError, match='channel'):
        C.LatitudeWeightedLoss('mae', lats, data_format='channels_first')
    with pytest.raises(ValueError):
        C.LatitudeWeightedLoss('mae', lats, weighting='polar')
    with pytest.raises(NotImplementedError):
        C.LatitudeWeightedLoss('cosine_proximity', lats)
    # the function over the new kinds: literal weighting, inner kind recorded
    f = C.latitude_weighted_loss('msle', lats, output_shape=(2, 60, 12))
    assert (f.kind, f.inner, f.__name__) == (0, 3, 'lat_loss')
    np.testing.assert_array_equal(f.row_weights, C.latitude_weights(lats))
    assert (C.lat_loss.kind, C.lat_loss.inner) == (0, 0)


def test_loss_spec_round_trips_npz_and_keras_and_old_spec_dicts_load(tmp_path):
    lats = np.linspace(-60, 60, 8)
    for loss in (C.LatitudeWeightedLoss('mape', lats, weighting='midlatitude'), C.latitude_weighted_loss('logcosh', lats),
                 C.latitude_weighted_loss(None, lats)):
        for fmt in ('npz', 'keras'):
            net = small_net()
            net.compile('adam', loss=loss, metrics=['logcosh', C.anomaly_correlation])
            path = str(tmp_path / ('m.' + fmt))
            net.save(path, format=fmt)
            m2 = serialization.load_model_file(path, device=torch.device('cpu'))
            got = m2.loss
            assert isinstance(got, C.LossSpec)
            assert (got.kind, got.inner, got.regularize, got.scale, got.__name__) == \
                (loss.kind, loss.inner, loss.regularize, loss.scale, loss.__name__)
            np.testing.assert_array_equal(got.row_weights, loss.row_weights)
            assert m2.metrics_names == ['loss', 'logcosh', 'anomaly_correlation']
    # a spec dict as the earlier code writes it (no 'inner'): kind 0 stays the latitude-weighted mse
    cfg = serialization._loss_config(C.latitude_weighted_loss(None, lats))
    assert 'inner' not in cfg['spec']
    assert 'inner' not in serialization._loss_config(C.anomaly_correlation_loss())['spec']
    assert serialization._loss_config(C.latitude_weighted_loss('mae', lats))['spec']['inner'] == 1
    net = small_net()
    net.compile('adam', loss=C.latitude_weighted_loss(None, lats), metrics=['mae'])
    path = str(tmp_path / 'old.npz')
    net.save(path, format='npz')
    m2 = serialization.load_model_file(path, device=torch.device('cpu'))
    assert (m2.loss.kind, m2.loss.inner) == (0, 0) and m2.metrics_names == ['loss', 'mean_absolute_error']
    # a plain Keras-name loss goes into training_config by name
    net.compile('adam', loss='mean_absolute_percentage_error', metrics=['msle'])
    path = str(tmp_path / 'plain.keras')
    net.save(path, format='keras')
    m3 = serialization.load_model_file(path, device=torch.device('cpu'))
    assert m3.loss == 'mean_absolute_percentage_error' and m3.metrics_names == ['loss', 'mean_squared_logarithmic_error']


@pytest.mark.parametrize('loss,metrics,names', [
    ('logcosh', 'mape', ['loss', 'mean_absolute_percentage_error']),
    ('MAE', 'logcosh', ['loss', 'logcosh']),
    ('msle', 'anomaly_correlation', ['loss', 'anomaly_correlation']),
])
def test_training_config_of_a_keras_file_names_the_new_losses(tmp_path, loss, metrics, names):
    src = open(os.path.join(GOLDEN, 'keras_sequential.h5'), 'rb').read()
    old = b'"loss": "mse", "metrics": ["mae"], "sample_weight_mode": null, "loss_weights": null'    # (same length: blanks pad)
    new = ('"loss":"%s","metrics":["%s"]' % (loss, metrics)).encode()
    assert src.count(old) == 1 and len(new) <= len(old)
    path = str(tmp_path / 'patched.h5')
    with open(path, 'wb') as fh:
        fh.write(src.replace(old, new + b' ' * (len(old) - len(new))))
    m = serialization.load_model_file(path)
    assert m.loss == loss and m.metrics_names == names
    assert type(m.optimizer).__name__ == 'Adam'


def test_load_model_resolves_the_reference_custom_objects(tmp_path):
    import pickle
    from dlwp_amd import util
    from dlwp_amd.model import DLWPNeuralNet
    base = os.path.join(str(tmp_path), 'ref_model')
    d = DLWPNeuralNet(is_convolutional=True, is_recurrent=False, time_dim=1, scaler_type=None, scale_targets=False)
    with open(base + '.pkl', 'wb') as fh:
        pickle.dump(d, fh)
    net = small_net()
    net.compile('adam', loss='mae', metrics=[C.anomaly_correlation, C.acc_loss])
    net.save(base + '.keras', format='keras')
    d2 = util.load_model(base)
    # anomaly_correlation by name; 'acc_loss' through DLWP.custom's objects, as the reference's load_model registers them
    assert d2.model.metrics_names == ['loss', 'anomaly_correlation', 'acc_loss']
    assert d2.model.loss == 'mae'


def test_report_maps_the_loss_table_columns():
    net = small_net()
    net.compile('adam', loss='mae', metrics=['mae', 'logcosh', C.anomaly_correlation, 'mse', C.latitude_weighted_loss('mape')])
    tr = net._trainer
    # loss 'mae' fills column 0 only: the pass holds mse (7), mae (8), logcosh (9), then the ACC sums (10-12); the spec: 13
    assert tr.n_cols == 14 and tr._metric_mask == 0b10011 | 0x20
    v = np.arange(1.0, 15.0)[None, :]
    out = tr._report_from(v, reg=0.0)
    acc = v[0, 7] - v[0, 10] / np.sqrt(v[0, 11] * v[0, 12])
    assert out == pytest.approx([1.0, 9.0, 10.0, acc, 8.0, 14.0])
    # loss 'mse': mse / mae stay in columns 1 / 2, the pass holds what is left
    net.compile('adam', loss='mse', metrics=['msle', 'mae', C.anomaly_correlation])
    tr = net._trainer
    assert tr.n_cols == 11
    v = np.arange(1.0, 12.0)[None, :]
    acc = v[0, 1] - v[0, 8] / np.sqrt(v[0, 9] * v[0, 10])
    assert tr._report_from(v, reg=0.0) == pytest.approx([2.0, 8.0, 3.0, acc])
    # two outputs with loss weights
    m2 = small_net(2)
    m2.compile('adam', loss='logcosh', metrics=['mape'], loss_weights=[1.0, 0.5])
    v = np.array([[1.0] + [0] * 6 + [3.0], [2.0] + [0] * 6 + [5.0]])
    assert m2._trainer._report_from(v, reg=0.0) == pytest.approx([2.0, 1.0, 2.0, 3.0, 5.0])


def test_anomaly_correlation_metric_and_whole_batch_logging():
    net = small_net()
    net.compile('adam', loss='mae', metrics=[C.anomaly_correlation])
    assert net._trainer._batch_stat            # epoch logs average per-batch values, as Keras does
    net.compile('adam', loss='mae', metrics=['logcosh'])
    assert not net._trainer._batch_stat
    with pytest.raises(NotImplementedError):
        C.anomaly_correlation(torch.zeros(4), torch.zeros(4), regularize_mean='global')
