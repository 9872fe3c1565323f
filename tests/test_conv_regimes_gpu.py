"""rv_conv_fwd outside the persistent 3x3 and Winograd families, through the C ABI, at every launch regime of tests/conv_cases.py: the
integer problem against the int64 convolution with `==`, the float problem against float64 under the derived per-element bound, inputs
in NaN-padded buffers, destinations in buffers whose padding must come back bit-unchanged, the fused and the trailing BatchNorm
statistics against float64 sums of the device's own output; the bit identities the kernels document (a forced tile repeats, every
(NT, MT) equals (1, 1), the pack table equals the per-entry packs, conv_small_k equals conv_cin12_k, the fused statistics do not
change `out`) and the argument refusals.  Every measured ratio error / bound is appended to conv_errors.jsonl, next to
gemm_errors.jsonl."""
import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu

NAN = float('nan')
QUICK = [n for n in cc.RUN_CASES if n not in cc.GRID_STRIDE_CASES]
TILED = [n for n in cc.RUN_CASES if n.split()[0] in ('direct', 'splitk') and cc.CASES[n]['algo'] & 0xff != 0x11]
ARG_NAMES = ['mode', 'in', 'in_ld', 'B', 'H', 'W', 'Cin', 'out', 'out_ld', 'Ho', 'Wo', 'Cout', 'wpack', 'bias', 'accumulate', 'algo', 'bn_sums', 'bn_z',
             'bn_z_ld', 'bn_coef', 'bn_slope', 'stream']
INPUTS = ('in', 'w', 'bias', 'z', 'coef')


def _lib():
    from reconvat_amd import _lib
    return _lib


def _bits(t):
    return t.detach().cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def upload(dev, pr):
    """fresh device copies of the problem's buffers, and the weights packed by rv_pack_weights into a NaN-filled buffer of the size the ABI names"""
    d = {k: pr[k + '_buf'].to(dev) if k + '_buf' in pr else None for k in INPUTS + ('out', 'sums')}
    assert all(t is None or t.data_ptr() % 256 == 0 for t in d.values())         # the float offsets of conv_cases.py decide every alignment
    lib = _lib()
    args = pr['pack_args']
    taps, kdim, ndim = args[:3]
    n = cc.pack_floats(args)                                         # (a forced plain layout: taps * kdim * ndim, which the ABI's size query does not know)
    assert args[7] and cc.frag_R(kdim) or lib.load().rv_packed_weight_floats(taps, kdim, ndim) == n
    d['wpack'] = torch.full((n + cc.GUARD,), NAN, device=dev)
    lib.call('rv_pack_weights', d['w'].data_ptr(), d['wpack'].data_ptr(), *args, lib.stream())
    if pr['case']['stats']:
        assert lib.load().rv_bn_workspace_bytes(pr['case']['cout']) == 8 * cc.RV_BN_NREP * 2 * pr['case']['cout']
    return d


def _at(t, off):
    return None if t is None else t.data_ptr() + 4 * off


def conv_args(pr, d, **kw):
    """the arguments of rv_conv_fwd for the problem on the buffers `d`; kw replaces arguments by name"""
    c = pr['case']
    z = c['stats'] == 'z'
    a = [c['mode'], _at(d['in'], pr['in_at']), pr['in_ld'], c['B'], c['H'], c['W'], c['cin'], _at(d['out'], pr['out_at']), pr['out_ld'], c['Ho'], c['Wo'],
         c['cout'], d['wpack'].data_ptr(), _at(d['bias'], pr.get('bias_at', 0)), c['acc'], c['algo'], None if d['sums'] is None else d['sums'].data_ptr(),
         _at(d['z'], pr['z_at']) if z else None, pr['z_ld'] if z else 0, _at(d['coef'], pr['coef_at']) if z else None, c['slope'] if z else 0.0, _lib().stream()]
    for k, v in kw.items():
        a[ARG_NAMES.index(k)] = v
    return tuple(a)


def collect(pr, d):
    """after the launch: inputs untouched, the padding of the destination intact -> (out [B, Ho, Wo, Cout] on the CPU, the statistics workspace)"""
    torch.cuda.synchronize()
    for k in INPUTS:
        assert d[k] is None or torch.equal(_bits(d[k]), _bits(pr[k + '_buf'])), 'rv_conv_fwd wrote into ' + k
    assert bool(torch.isnan(d['wpack'][-cc.GUARD:]).all().item()), 'rv_pack_weights wrote behind the packed buffer'
    out_buf = d['out'].cpu()
    assert cc.padding_intact(pr, out_buf), 'rv_conv_fwd wrote into the padding of out'
    return cc.live(pr, out_buf).clone(), None if d['sums'] is None else d['sums'].cpu()


def run(dev, pr, **kw):
    d = upload(dev, pr)
    _lib().call('rv_conv_fwd', *conv_args(pr, d, **kw))
    return collect(pr, d)


def variant(case, tag, **kw):
    """the same problem (same seed, same logical tensors) with other strides, offsets or options"""
    return dict(case, name=case['name'] + ' / ' + tag, regime={}, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# every case, both problems
# ---------------------------------------------------------------------------------------------------------------------
def _run_case(dev, name, kind):
    pr = cc.problem(cc.CASES[name], kind)
    out, sums = run(dev, pr)
    ratio = cc.compare(pr, out)
    print(name, kind, ratio)
    cc.check('rv_conv_fwd ' + kind, name, 'out', ratio, log=True)
    if sums is not None:
        cc.check('rv_conv_fwd ' + kind, name, 'stats', cc.stats_ratio(pr, out, sums), log=True)


@pytest.mark.parametrize('kind', ['int', 'float'])
@pytest.mark.parametrize('name', QUICK)
def test_conv_case(dev, name, kind):
    _run_case(dev, name, kind)


@pytest.mark.parametrize('kind', ['int', 'float'])
@pytest.mark.parametrize('name', cc.GRID_STRIDE_CASES)
def test_conv_small_grid_stride(dev, name, kind):
    """513 x 513 pixels: more workgroups than the cap, a second pass for the first few of them"""
    _run_case(dev, name, kind)


# ---------------------------------------------------------------------------------------------------------------------
# bit identities (the float problem)
# ---------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('name', [n for n in QUICK if n.startswith('direct') and n.endswith('S plain')])
def test_forced_tile_repeats_bit_for_bit(dev, name):
    pr = cc.problem(cc.CASES[name], 'float')
    assert same_bits(run(dev, pr)[0], run(dev, pr)[0])


@pytest.mark.parametrize('name', TILED)
def test_every_tile_equals_1x1(dev, name):
    """each output element is one k-ordered chain of MFMAs (0x5NM: four of them, added in wave order), whatever tile its lane sits in"""
    pr = cc.problem(cc.CASES[name], 'float')
    assert same_bits(run(dev, pr)[0], run(dev, pr, algo=(pr['case']['algo'] & 0xf00) | 0x11)[0])


@pytest.mark.parametrize('form', cc.RV_CIN12)
def test_fallback_small_k_equals_cin12(dev, form):
    """both start the accumulator at the bias and add the taps by fmaf in (ky, kx, ci) order"""
    for tail in ('big', 'big sums', '1x1 sums', '64 px'):
        case = cc.CASES['small fallback %d->%d %s' % (form + (tail,))]
        fast = variant(case, 'aligned', bias_off=0, in_pad=0)
        assert cc.case_regime(case)['kernel'] == 'small_k' and cc.case_regime(fast)['kernel'] == 'cin12'
        for kind in ('int', 'float'):
            slow_out, _ = run(dev, cc.problem(case, kind))
            fast_out, sums = run(dev, cc.problem(fast, kind))
            assert same_bits(slow_out, fast_out), (case['name'], kind)
            if sums is not None:
                cc.check('conv_cin12_k ' + kind, fast['name'], 'stats', cc.stats_ratio(cc.problem(fast, kind), fast_out, sums), log=True)


@pytest.mark.parametrize('form', cc.RV_CIN12)
def test_cin12_statistics_do_not_change_out(dev, form):
    for tail in ('big sums', 'big z', 'H2 sums', 'H4 z_ld+4'):
        case = cc.CASES['cin12 %d->%d %s' % (form + (tail,))]
        pr = cc.problem(case, 'float')
        assert same_bits(run(dev, pr)[0], run(dev, cc.problem(variant(case, 'no statistics', stats=None), 'float'))[0]), case['name']


@pytest.mark.parametrize('kind', ['int', 'float'])
def test_pack_table_equals_the_per_entry_packs(dev, kind):
    """one buffer for all entries, NaN between and behind them: the table launch and the per-entry launches leave the same bits everywhere, and (the integer
    problem, weights that are multiples of 4) the bits of the mirror, Winograd section included"""
    lib = _lib()
    entries = [cc.pack_entry(i, kind) for i in range(len(cc.PACK_TABLE))]
    sizes = [cc.pack_floats(a) for _, a in entries]
    offs = [sum(sizes[:i]) + 4 * i for i in range(len(sizes))]
    total_floats = offs[-1] + sizes[-1] + 4
    ws = [w.to(dev) for w, _ in entries]
    one = torch.full((total_floats,), NAN, device=dev)
    for w, (_, a), off in zip(ws, entries, offs):
        lib.call('rv_pack_weights', w.data_ptr(), one.data_ptr() + 4 * off, *a, lib.stream())
    tab = torch.full((total_floats,), NAN, device=dev)
    host = torch.zeros(len(entries) * lib.load().rv_pack_table_entry_bytes(), dtype=torch.uint8)
    blocks = 0
    for i, (w, (_, a), off) in enumerate(zip(ws, entries, offs)):
        blocks = lib.invoke('rv_pack_table_fill', host.data_ptr(), i, w.data_ptr(), tab.data_ptr() + 4 * off, *a)
        assert blocks == sum(cc.cdiv(s, 256) for s in sizes[:i + 1]), lib.last_error()
    table = host.to(dev)
    lib.call('rv_pack_table_run', table.data_ptr(), len(entries), blocks, lib.stream())
    torch.cuda.synchronize()
    assert same_bits(tab, one)
    got = tab.cpu()
    for (w, a), off, n, e in zip(entries, offs, sizes, cc.PACK_TABLE):
        assert bool(torch.isnan(got[off + n:off + n + 4]).all().item()), e[0]
        if kind == 'int':
            assert torch.equal(got[off:off + n], cc.pack_mirror(w, *a)), e[0]
        else:
            taps, kdim, ndim = a[:3]
            assert torch.equal(cc.unpack_mirror(got[off:off + n], taps, kdim, ndim, a[7]), cc.logical_weights(w, *a[:7])), e[0]
    assert lib.invoke('rv_pack_table_run', table.data_ptr(), 0, blocks, lib.stream()) != 0 and lib.invoke('rv_pack_table_run', table.data_ptr(), 3, 0, lib.stream()) != 0


def test_pack_arguments_are_the_ones_ops_passes(dev):
    from reconvat_amd import ops
    for kind, shape in (('c3', (5, 3, 3, 3)), ('t3', (3, 5, 3, 3)), ('c1', (5, 3, 1, 1)), ('c1', (16, 1, 1, 1)), ('c3', (16, 8, 3, 3)),
                        ('up', (16, 32, 2, 2)), ('down', (32, 16, 2, 2)), ('c3', (2, 8, 3, 3))):
        w = torch.zeros(shape, device=dev)
        cin, cout = ops._channels(kind, w)
        for which in ('fwd', 'dgrad'):
            assert ops._pack_make(kind, w, which)[1] == cc.pack_args_of(kind, which, cin, cout), (kind, which)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: non-zero, a message, the destinations untouched
# ---------------------------------------------------------------------------------------------------------------------
def _refused(d, args, what):
    lib = _lib()
    before = {k: _bits(d[k]).clone() for k in ('out', 'sums') if d[k] is not None}
    rc = lib.invoke('rv_conv_fwd', *args)
    torch.cuda.synchronize()
    assert rc != 0, (what, rc)
    assert lib.last_error(), what
    for k, b in before.items():
        assert torch.equal(_bits(d[k]), b), (what, k)


@pytest.mark.parametrize('name', cc.REFUSED_CASES)
def test_refused_case(dev, name):
    pr = cc.problem(cc.CASES[name], 'float')
    d = upload(dev, pr)
    _refused(d, conv_args(pr, d), name)


def test_conv_refusals(dev):
    for name, tries in (
            ('direct m1 16->32 L sums', (('mode 4', {'mode': 4}), ('mode -1', {'mode': -1}), ('mode 1 with Ho = H - 1', {'Ho': 8}), ('mode 0 with Wo = W + 1', {'mode': 0, 'Wo': 32}),
                                         ('mode 2 with Ho = H', {'mode': 2}), ('mode 3 with Ho = H', {'mode': 3}), ('mode 3 with Wo = 2 W + 2', {'mode': 3, 'Ho': 18, 'Wo': 64}),
                                         ('in 4 bytes off', {'in': 'in+1'}), ('no small kernel for 16 -> 2 in mode 1', {'Cout': 2}),
                                         ('no small kernel for 4 -> 32', {'Cin': 4}), ('mode 3 with Cout = 24', {'mode': 3, 'Ho': 18, 'Wo': 62, 'Cout': 24}))),
            ('direct m3 16->16 S z', (('bn_z without bn_sums', {'bn_sums': None}), ('bn_z without bn_coef', {'bn_coef': None}), ('mode 3 with Ho = 2 H + 2', {'Ho': 12}))),
            ('direct m0 8->16 S plain', (('in 8 bytes off at R = 2', {'in': 'in+1'}), ('in_ld odd at R = 2', {'in_ld': 9}), ('a tile that does not divide ntile_n', {'algo': 0x121}),
                                         ('MT = 3', {'algo': 0x113}), ('NT = 0', {'algo': 0x101})))):
        pr = cc.problem(cc.CASES[name], 'float')
        d = upload(dev, pr)
        ok = conv_args(pr, d)
        for what, kw in tries:
            if kw.get('in') == 'in+1':
                kw = dict(kw, **{'in': ok[1] + 4})
            _refused(d, conv_args(pr, d, **kw), what)
        # ... and the same buffers still serve the accepted call
        _lib().call('rv_conv_fwd', *ok)
        out, sums = collect(pr, d)
        cc.check('rv_conv_fwd after refusals', name, 'out', cc.compare(pr, out))
        if sums is not None:
            cc.check('rv_conv_fwd after refusals', name, 'stats', cc.stats_ratio(pr, out, sums))
