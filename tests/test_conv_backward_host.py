"""The host side of the conv backward without a device: the weight-gradient problem record of the five layer kinds, the argument lists of the
four weight-gradient entry points (a recording hook in place of the library call), and what one conv layer's backward launches in which order
(recorders in place of conv_wgrad / conv_dgrad_into).  The expectations are written out from the code this replaced: four copies of the backward
(ConvFn, the up and the skip conv of UpCatFn, the rank-1 skip of BnActFn) and five copies of the argument list."""
import ctypes
import itertools
import types

import pytest
import torch

from reconvat_amd import _lib, ops

B, H, W, CIN, COUT = 2, 4, 6, 3, 5


@pytest.fixture
def setcell():
    """setcell(cell, value): cell[0] = value until the end of the test (the package's switches are one-element lists)"""
    undo = []

    def set_(cell, value):
        undo.append((cell, cell[0]))
        cell[0] = value
    yield set_
    for cell, old in reversed(undo):
        cell[0] = old


def _layer(kind):
    x = torch.zeros(B, H, W, 8)[..., :CIN]                       # a channel slice: pixel stride 8
    ho, wo = {'down': (H // 2, W // 2), 'up': (2 * H, 2 * W)}.get(kind, (H, W))
    return x, torch.zeros(B, ho, wo, COUT)


#          mode taps  U   uld hu  wu  ca   V   vld hv wv cb  bb s_a s_b flip
GEOM = {
    'c3':   (0, 9, 'x', 8, 4, 6, 3, 'dy', 5, 4, 6, 5, 2, 9, 27, 0),
    't3':   (0, 9, 'x', 8, 4, 6, 3, 'dy', 5, 4, 6, 5, 2, 45, 9, 1),
    'c1':   (1, 1, 'x', 8, 4, 6, 3, 'dy', 5, 4, 6, 5, 2, 1, 3, 0),
    'down': (2, 4, 'x', 8, 4, 6, 3, 'dy', 5, 2, 3, 5, 2, 4, 12, 0),
    'up':   (2, 4, 'dy', 5, 8, 12, 5, 'x', 8, 4, 6, 3, 2, 4, 20, 0),
}


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('kind', list(GEOM))
def test_problem_record_of_the_five_layer_kinds(kind, bf16):
    x, dy = _layer(kind)
    p = ops._wgrad_geom(kind, x, dy, bf16)
    want = list(GEOM[kind])
    if bf16 and kind in ('c3', 't3'):
        want[0] |= 0x100                                         # bf16 operands: the 3x3 kernels only
    named = {'x': x, 'dy': dy}
    assert p._fields == ('mode', 'taps', 'u', 'uld', 'hu', 'wu', 'ca', 'v', 'vld', 'hv', 'wv', 'cb', 'bb', 's_a', 's_b', 'flip')
    assert p.u is named[want[2]] and p.v is named[want[7]]
    assert tuple(p._replace(u=None, v=None)) == tuple(want[:2] + [None] + want[3:7] + [None] + want[8:])
    assert p.plan_key == (p.taps, p.bb, p.hv, p.ca, p.cb) and p.tune_key == (p.taps, p.bb, p.hv, p.wv, p.ca, p.cb)
    assert p.head() == (p.mode, p.u.data_ptr(), p.uld, p.hu, p.wu, p.ca, p.v.data_ptr(), p.vld, p.hv, p.wv, p.cb, p.bb)
    # segments of one launch: the same numbers, the operands anywhere
    assert p.same_geometry(ops._wgrad_geom(kind, x.clone(), dy.clone(), bf16)._replace(uld=p.uld, vld=p.vld))
    for field in ('mode', 'uld', 'hu', 'wu', 'ca', 'vld', 'hv', 'wv', 'cb', 'bb', 's_a', 's_b', 'flip'):
        assert not p.same_geometry(p._replace(**{field: getattr(p, field) + 1})), field


# --------------------------------------------------------------------------------------------
# the argument lists
# --------------------------------------------------------------------------------------------
class _Table:
    def __init__(self):
        self.n, self.keep = 0, []

    def slot(self):
        return 0x7AB00 + self.n


STREAM = types.SimpleNamespace(cuda_stream=0x5EED)


@pytest.fixture
def launches(monkeypatch, setcell):
    """[(entry point, arguments, segment pointers)] of every library call made through _lib.invoke; the call itself is not made."""
    seen = []

    def hook(name, args, fn):
        segs = None
        if name.endswith('_seg'):
            segs = [list((ctypes.c_void_p * args[1]).from_address(a)) for a in args[2:4]]
        seen.append((name, args, segs))
        return 1 if 'deferred' in name else 0
    setcell(_lib.HOOK, hook)
    monkeypatch.setattr(ops, 'AUTOTUNE', False)
    setcell(ops.DETERMINISTIC, False)
    return seen


def _check_signature(name, args):
    types_ = _lib.SIGNATURES[name][1]
    assert len(args) == len(types_), name
    for i, (a, t) in enumerate(zip(args, types_)):
        assert (a is None or type(a) is int) if t is _lib.P else type(a) is int, (name, i, a)


def test_weight_gradient_argument_lists(launches):
    lib = _lib.load()
    cin, cout = 16, 32
    xs = [torch.zeros(B, H, W, cin) for _ in range(3)]
    dys = [torch.zeros(B, H, W, cout) for _ in range(3)]
    dw, db = torch.zeros(cout, cin, 3, 3), torch.zeros(cout)
    probs = [ops._wgrad_geom('c3', x, dy) for x, dy in zip(xs, dys)]
    X, DY, DW, DB, ST = xs[0].data_ptr(), dys[0].data_ptr(), dw.data_ptr(), db.data_ptr(), STREAM.cuda_stream
    nb1, nb3 = lib.rv_conv_wgrad_workspace_bytes(9, B, H, cin, cout), lib.rv_conv_wgrad_workspace_bytes(9, 3 * B, H, cin, cout)
    tab = _Table()

    assert ops._wgrad_launch(probs[:1], dw, db, 1, STREAM) is True           # no deferral context: immediate
    assert ops._wgrad_launch(probs[:1], dw, None, 0, STREAM) is True         # (no bias gradient, not accumulating)
    assert ops._wgrad_launch(probs, dw, db, 1, STREAM) is True
    with ops.deferred_wgrad_reductions() as pend:
        pend.tables[ST] = tab
        assert ops._wgrad_launch(probs[:1], dw, db, 1, STREAM) is True
        assert ops._wgrad_launch(probs, dw, db, 1, STREAM) is True
        assert tab.n == 2 and [t.numel() * 4 for t in tab.keep] == [nb1, nb3]
        assert ops._wgrad_launch(probs[:1], dw, db, 0, STREAM) is True       # not accumulating: never deferred
    assert len(launches) == 6
    for name, args, _ in launches:
        _check_signature(name, args)
    ws = [a[{'rv_conv_wgrad': 18, 'rv_conv_wgrad_deferred': 17, 'rv_conv_wgrad_seg': 19, 'rv_conv_wgrad_deferred_seg': 18}[n]] for n, a, _ in launches]
    assert all(type(p_) is int and p_ for p_ in ws) and ws[3:5] == [t.data_ptr() for t in tab.keep]
    seg_ptrs = [[x.data_ptr() for x in xs], [dy.data_ptr() for dy in dys]]
    assert [(n, a) for n, a, _ in launches] == [
        ('rv_conv_wgrad', (0, X, 16, 4, 6, 16, DY, 32, 4, 6, 32, 2, DW, 9, 144, 0, DB, 1, ws[0], nb1, ST)),
        ('rv_conv_wgrad', (0, X, 16, 4, 6, 16, DY, 32, 4, 6, 32, 2, DW, 9, 144, 0, None, 0, ws[1], nb1, ST)),
        ('rv_conv_wgrad_seg', (0, 3, launches[2][1][2], launches[2][1][3], 16, 4, 6, 16, 32, 4, 6, 32, 2, DW, 9, 144, 0, DB, 1, ws[2], nb3, ST)),
        ('rv_conv_wgrad_deferred', (0, X, 16, 4, 6, 16, DY, 32, 4, 6, 32, 2, DW, 9, 144, 0, DB, ws[3], nb1, 0x7AB00, ST)),
        ('rv_conv_wgrad_deferred_seg', (0, 3, launches[4][1][2], launches[4][1][3], 16, 4, 6, 16, 32, 4, 6, 32, 2, DW, 9, 144, 0, DB, ws[4], nb3, 0x7AB01, ST)),
        ('rv_conv_wgrad', (0, X, 16, 4, 6, 16, DY, 32, 4, 6, 32, 2, DW, 9, 144, 0, DB, 0, ws[5], nb1, ST)),
    ]
    assert launches[2][2] == seg_ptrs and launches[4][2] == seg_ptrs


def test_when_a_weight_gradient_is_deferred(launches, setcell):
    """Inside deferred_wgrad_reductions: accumulating launches, but not in deterministic mode and never the 1 -> many 3x3 layer; segments of
    different geometry are refused before anything is launched, and a refused segmented launch is reported, not raised."""
    def names(cin, cout, acc=1, kind='c3'):
        del launches[:]
        x, dy = torch.zeros(B, H, W, cin), torch.zeros(B, H, W, cout)
        with ops.deferred_wgrad_reductions() as pend:
            pend.tables[STREAM.cuda_stream] = _Table()
            ops._wgrad_launch([ops._wgrad_geom(kind, x, dy)], torch.zeros(cout * cin * 9), torch.zeros(cout), acc, STREAM)
        return [n for n, _, _ in launches]
    assert names(16, 32) == ['rv_conv_wgrad_deferred'] and names(16, 32, acc=0) == ['rv_conv_wgrad']
    assert names(1, 32) == ['rv_conv_wgrad'] and names(1, 16) == ['rv_conv_wgrad_deferred'] and names(1, 32, kind='c1') == ['rv_conv_wgrad_deferred']
    setcell(ops.DETERMINISTIC, True)
    assert names(16, 32) == ['rv_conv_wgrad']
    setcell(ops.DETERMINISTIC, False)
    del launches[:]
    a, b = ops._wgrad_geom('c3', torch.zeros(B, H, W, 16), torch.zeros(B, H, W, 32)), ops._wgrad_geom('c3', torch.zeros(B, H + 1, W, 16), torch.zeros(B, H + 1, W, 32))
    assert ops._wgrad_launch([a, b], torch.zeros(32 * 16 * 9), None, 1, STREAM) is False and launches == []
    setcell(_lib.HOOK, lambda name, args, fn: 3)            # the library refuses
    assert ops._wgrad_launch([a, a], torch.zeros(32 * 16 * 9), None, 1, STREAM) is False
    with pytest.raises(RuntimeError, match='rv_conv_wgrad failed'):
        ops._wgrad_launch([a], torch.zeros(32 * 16 * 9), None, 1, STREAM)


def test_merged_items_may_be_records_or_tuples(launches, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: STREAM)
    w, gw, gb = torch.zeros(32, 16, 3, 3), torch.zeros(32, 16, 3, 3), torch.zeros(32)
    pairs = [(torch.zeros(B, H, W, 16), torch.zeros(B, H, W, 32)) for _ in range(2)]
    items = [ops.WgradItem('c3', x, dy, w, gw, gb, False, STREAM) for x, dy in pairs]
    assert ops.conv_wgrad_merged(items) is True and ops.conv_wgrad_merged([tuple(it) for it in items]) is True
    assert ops.conv_wgrad_merged(items[:1]) is False                         # one pass: the caller launches it
    same = lambda a: a[:2] + a[4:19] + a[20:]             # noqa: E731 -- (all but the segment tables and the workspace, allocated per launch)
    assert [n for n, _, _ in launches] == ['rv_conv_wgrad_seg'] * 2 and same(launches[0][1]) == same(launches[1][1])
    assert launches[0][1][13] == gw.data_ptr() and launches[0][1][17] == gb.data_ptr()


# --------------------------------------------------------------------------------------------
# one conv layer's backward
# --------------------------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    calls = []

    def conv_wgrad(kind, x, dy, w, want_bias=True, dw_acc=None, db_acc=None, bf16=False, colsum=None):
        calls.append(('wgrad', kind, want_bias, dw_acc, db_acc, bf16, colsum))
        return (None, None) if dw_acc is not None else ('dw', 'db' if want_bias else None)

    def conv_dgrad_into(kind, dy, w, dx, bn_link=None, accumulate=False, bf16=False, sum_ws=None):
        calls.append(('dgrad', kind, dx, bn_link, accumulate, bf16, sum_ws))
    monkeypatch.setattr(ops, 'conv_wgrad', conv_wgrad)
    monkeypatch.setattr(ops, 'conv_dgrad_into', conv_dgrad_into)
    return calls


def _params(allocated):
    """(weight, bias) leaves; allocated: which of them have a .grad buffer ('', 'w', 'wb')"""
    w, b = torch.zeros(COUT, CIN, 1, 1, requires_grad=True), torch.zeros(COUT, requires_grad=True)
    if 'w' in allocated:
        w.grad = torch.zeros_like(w)
    if 'b' in allocated:
        b.grad = torch.zeros_like(b)
    return w, b


@pytest.mark.parametrize('wgrad_first', [True, False])
@pytest.mark.parametrize('consumer', [None, 'first', 'second'])
def test_conv_backward_calls_order_and_results(recorded, setcell, wgrad_first, consumer):
    """Every (need_x, need_w, need_b) x direct_param_grads off / on with no, the weight's, both .grad buffers -- for one position of the layer among the consumers of
    a GradShare and one order of the halves.  From the replaced copies: the parameter gradients go straight into .grad iff the weight has a buffer and the bias has one
    or no bias gradient is wanted (else both are returned); the first consumer of a GradShare writes and returns its buffer, a later one accumulates and returns None;
    the weight gradient runs first iff WGRAD_FIRST."""
    setcell(ops.WGRAD_FIRST, wgrad_first)
    x, dy = torch.zeros(B, H, W, CIN), torch.zeros(B, H, W, COUT)
    for need_x, need_w, need_b, (direct, allocated) in itertools.product((False, True), (False, True), (False, True),
                                                                         ((False, 'wb'), (True, ''), (True, 'w'), (True, 'wb'))):
        del recorded[:]
        w, b = _params(allocated)
        share = None if consumer is None else ops.GradShare()
        if consumer == 'second':
            share.buf = torch.zeros(B, H, W, CIN)
        held = share.buf if share is not None else None
        setcell(ops._DIRECT, direct)
        dx, dw, db = ops._conv_backward('c1', x, dy, w, (w, b), need_x, need_w, need_b, xshape=(B, H, W, CIN), share=share, bf16=True)
        in_place = direct and 'w' in allocated and ('b' in allocated or not need_b)
        want = []
        if need_w:
            want.append(('wgrad', 'c1', need_b, w.grad if in_place else None, b.grad if in_place else None, True, None))
        if need_x:
            want.append(('dgrad', 'c1', dx if consumer != 'second' else held, None, consumer == 'second', True, None))
        assert recorded == (want if wgrad_first else want[::-1]), (need_x, need_w, need_b, direct, allocated)
        assert (dw, db) == (('dw', 'db' if need_b else None) if need_w and not in_place else (None, None))
        if not need_x or consumer == 'second':
            assert dx is None
        else:
            assert tuple(dx.shape) == (B, H, W, CIN) and (share is None or share.buf is dx)


def test_conv_backward_links(recorded, monkeypatch, setcell):
    """bn_in owns the input-gradient kernel's epilogue (no GradShare, no column sums of dx); dx_colsum is filled in a final graph only (need_w); dy_colsum
    travels to the weight gradient and is released; the wgrad_first argument overrides the knob."""
    setcell(ops.WGRAD_FIRST, True)
    monkeypatch.setattr(ops, 'bn_ws_doubles', lambda c: 2 * c)
    x, dy = torch.zeros(B, H, W, CIN), torch.zeros(B, H, W, COUT)
    w, b = _params('')
    kw = dict(xshape=(B, H, W, CIN))
    bn, share, link, dyl = ops.BnLink(), ops.GradShare(), ops.ColsumLink(), ops.ColsumLink()
    dx, _, _ = ops._conv_backward('c3', x, dy, w, (w, b), True, True, True, share=share, bn_in=bn, dx_colsum=link, **kw)
    assert share.buf is None and link.sums is None and recorded[1] == ('dgrad', 'c3', dx, bn, False, False, None)
    del recorded[:]
    dx, _, _ = ops._conv_backward('c3', x, dy, w, (w, b), True, True, True, dx_colsum=link, **kw)
    assert link.c == CIN and link.sums.numel() == 2 * CIN and recorded[1] == ('dgrad', 'c3', dx, None, False, False, link.sums)
    link.sums = None
    ops._conv_backward('c3', x, dy, w, (w, b), True, False, False, dx_colsum=link, **kw)          # weights not live: no column sums
    assert link.sums is None
    del recorded[:]
    dyl.sums, dyl.c = torch.zeros(4), COUT
    ops._conv_backward('up', x, dy, w, (w, b), True, True, True, dy_colsum=dyl, wgrad_first=False, **kw)
    assert [c[0] for c in recorded] == ['dgrad', 'wgrad'] and recorded[1][6] is dyl and dyl.sums is None


@pytest.mark.parametrize('wgrad_first', [True, False])
@pytest.mark.parametrize('allocated,in_place', [('wb', True), ('w', False), ('', False)])
def test_upcat_backward_interleaves_two_layers(recorded, monkeypatch, setcell, wgrad_first, allocated, in_place):
    """UpCatFn: both weight gradients (up, then skip) before both input gradients (up, then skip), or the reverse; the bias gradients are always
    computed, so a weight with a .grad buffer whose bias has none gets BOTH gradients returned (the rule of ConvFn with need_b = True)."""
    setcell(ops.WGRAD_FIRST, wgrad_first)
    setcell(ops._DIRECT, True)
    cu, cs = 4, 3
    wu, bu = _params(allocated)
    wsk, bsk = _params(allocated)
    share = ops.GradShare()
    ctx = types.SimpleNamespace(saved_tensors=('x', 's', wu, wsk), cu=cu, params=(wu, bu, wsk, bsk), shapes=((B, H, W, 7), (B, 2 * H, 2 * W, 2)), share=share,
                                dy_colsum=None, live=True, needs_input_grad=(True, True, False, True, True, False, False, False, False))
    monkeypatch.setitem(ops.BF16, 'bwd', True)
    out = ops.UpCatFn.backward(ctx, torch.zeros(B, 2 * H, 2 * W, cu + cs))
    acc = lambda p: p.grad if in_place else None          # noqa: E731
    weights = [('wgrad', 'up', True, acc(wu), acc(bu), False, None), ('wgrad', 'c3', True, acc(wsk), acc(bsk), True, None)]
    inputs = [('dgrad', 'up', out[0], None, False, False, None), ('dgrad', 'c3', out[3], None, False, True, None)]
    assert recorded == (weights + inputs if wgrad_first else inputs + weights)
    assert tuple(out[0].shape) == (B, H, W, 7) and out[3] is share.buf and out[6:] == (None, None, None)
    assert (out[1], out[2], out[4], out[5]) == ((None,) * 4 if in_place else ('dw', 'db', 'dw', 'db'))
