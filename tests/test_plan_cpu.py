"""The planner on the host (dlwp_amd/plan.py): which lowering a layer gets (the order of plan._LOWERINGS), the order buffers are
numbered in, the redirect of a launch into a model's output slot, the builder's helpers and the refusals' messages.  Training
plans only, or facts no epilogue fold changes: every test holds with and without the built library."""
import pytest
import torch

from dlwp_amd import layers as L
from dlwp_amd import plan as P
from dlwp_amd.engine import Model

CF = {'data_format': 'channels_first'}
CPU = torch.device('cpu')


def X():
    return L.Input(shape=(4, 16, 24))


def conv(t, f=8, k=3, **kw):
    return L.Conv2D(f, k, **dict(CF, **dict({'padding': 'same'}, **kw)))(t)


def kinds(plan):
    return [op.kind for op in plan.ops]


# -- dispatch order --------------------------------------------------------------------------------------------------------------------- #
def test_bilinear_upsampling_is_a_launch_and_nearest_is_not():
    x = X()
    m = Model(inputs=x, outputs=conv(L.UpSampling2D(2, interpolation='bilinear', **CF)(x)), device=CPU)
    assert kinds(m.plan) == ['bilinear', 'conv'] == kinds(m.infer_plan)
    x = X()
    m = Model(inputs=x, outputs=conv(L.UpSampling2D(2, **CF)(x)), device=CPU)
    for plan in (m.plan, m.infer_plan):           # (3 taps behind a halo of 1 reach 3 source pixels: nothing to restate)
        assert kinds(plan) == ['conv'] and plan.ops[0].src_mode == P.SRC_UPSAMPLE2 and plan.ops[0].xs == (4, 16, 24)


def test_separable_depthwise_and_strided_convolutions_get_their_own_lowerings():
    x = X()
    assert kinds(Model(inputs=x, outputs=L.SeparableConv2D(8, 3, **CF)(x), device=CPU).plan) == ['dwconv', 'pwconv']
    x = X()
    assert kinds(Model(inputs=x, outputs=L.DepthwiseConv2D(3, **CF)(x), device=CPU).plan) == ['dwconv']
    x = X()
    m = Model(inputs=x, outputs=conv(x, strides=2), device=CPU)
    assert kinds(m.plan) == ['sphasew', 's2dp', 'conv'] == kinds(m.infer_plan)
    x = X()
    assert kinds(Model(inputs=x, outputs=L.Conv2DTranspose(8, 3, strides=2, **CF)(x), device=CPU).plan) == ['tphasew', 'conv', 'd2sc']


# -- buffer order ----------------------------------------------------------------------------------------------------------------------- #
def test_the_destination_is_numbered_in_front_of_the_phase_temporary():
    x = X()         # 3 taps behind a top / left halo of 2 reach 2 source pixels: the layer runs on phase kernels
    t = L.ZeroPadding2D(((2, 0), (2, 0)), **CF)(L.UpSampling2D(2, **CF)(x))
    plan = Model(inputs=x, outputs=conv(conv(t, padding='valid')), device=CPU).plan
    assert kinds(plan) == ['phasew', 'conv', 'd2s', 'conv']
    assert plan.ops[1].dst == plan.ops[2].src and 0 <= plan.ops[2].dst < plan.ops[2].src
    x = X()
    plan = Model(inputs=x, outputs=conv(L.Conv2DTranspose(8, 4, strides=2, padding='same', **CF)(x)), device=CPU).plan
    assert kinds(plan) == ['tphasew', 'conv', 'd2sc', 'conv']
    assert plan.ops[1].dst == plan.ops[2].src and 0 <= plan.ops[2].dst < plan.ops[2].src


# -- output redirect -------------------------------------------------------------------------------------------------------------------- #
def test_a_convolution_behind_a_reshape_writes_the_output_slot_itself():
    x = X()
    plan = Model(inputs=x, outputs=L.Reshape((2, 4, 16, 24))(conv(x)), device=CPU).plan
    assert kinds(plan) == ['conv'] and plan.ops[0].dst == P.OUT(0) and plan.output_store == [(8, 16, 24)]


def test_a_later_reader_follows_the_redirected_convolution_into_the_slot():
    x = X()
    c = conv(x)
    plan = Model(inputs=x, outputs=[L.Reshape((2, 4, 16, 24))(c), conv(c, f=2)], device=CPU).plan
    assert kinds(plan) == ['conv', 'conv'] and plan.ops[0].dst == P.OUT(0)
    assert (plan.ops[1].src, plan.ops[1].dst) == (P.OUT(0), P.OUT(1))


def test_a_tensor_named_as_two_outputs_is_copied_into_the_second_slot():
    x = X()
    c = conv(x)
    plan = Model(inputs=x, outputs=[c, c], device=CPU).plan
    assert kinds(plan) == ['conv', 'copy']
    assert (plan.ops[0].dst, plan.ops[1].src, plan.ops[1].dst) == (P.OUT(0), P.OUT(0), P.OUT(1))
    assert plan.output_store == [(8, 16, 24), (8, 16, 24)]


# -- the builder's helpers -------------------------------------------------------------------------------------------------------------- #
def test_out_or_new_records_the_stored_shape_of_an_output_slot_only():
    x = X()
    b = P._PlanBuilder([x], [conv(x), conv(x)], False, True, False, True, False)
    assert b.out_or_new([], (2, 3, 4)) == 0 and b.plan.buffers == [(2, 3, 4)] and b.plan.output_store == [None, None]
    assert b.out_or_new([1], (5, 6, 7)) == P.OUT(1) and b.plan.buffers == [(2, 3, 4)] and b.plan.output_store == [None, (5, 6, 7)]


def test_whole_extracts_a_channel_window_with_one_copy():
    x = X()
    b = P._PlanBuilder([x], [conv(x)], False, True, False, True, False)
    v = b.whole(P.View(P.STATE_IN, 1, 2, 4, 16, 24))
    assert kinds(b.plan) == ['copy'] and b.plan.buffers == [(2, 16, 24)]
    op = b.plan.ops[0]
    assert (op.src, op.dst, op.in_c_off, op.in_c_total, op.out_c_off, op.out_c_total) == (P.STATE_IN, 0, 1, 4, 0, 2)
    assert v.full and (v.buf, v.c, v.h, v.w) == (0, 2, 16, 24)
    assert b.whole(v) is v and len(b.plan.ops) == 1                      # a whole buffer is left alone


# -- refusals --------------------------------------------------------------------------------------------------------------------------- #
def test_refusals_keep_their_messages():
    x = X()
    with pytest.raises(NotImplementedError, match='^exactly one model input is supported$'):
        P.build_plan([x, X()], [conv(x)])
    with pytest.raises(ValueError, match='^an input / output transform belongs to inference plans: training data is prepared on the host$'):
        P.build_plan([x], [conv(x)], transform=(True, False))
    up = L.Conv2DTranspose(4, 2, strides=2, name='up', **CF)
    with pytest.raises(NotImplementedError, match='^up: a Conv2DTranspose layer applied more than once is not implemented$'):
        P.build_plan([x], [up(up(x))])
    from dlwp_amd.custom import PeriodicPadding2D
    wrap = L.KTensor((4, 50, 24), PeriodicPadding2D((17, 0), name='wrap', **CF), [x])     # (the layer's own shape check is passed by)
    with pytest.raises(ValueError, match='^wrap: periodic row padding exceeds the input height 16$'):
        P.build_plan([x], [wrap])

    class Odd(L.Layer):
        pass
    with pytest.raises(NotImplementedError, match=r'^layer odd \(Odd\) has no HIP lowering$'):
        P.build_plan([x], [Odd(name='odd')(x)])
