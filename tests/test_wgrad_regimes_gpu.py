"""The weight gradient through the C ABI (rv_conv_wgrad, rv_conv_wgrad_seg, rv_conv_wgrad_deferred, rv_conv_wgrad_deferred_seg,
rv_wgrad_reduce_table) at every launch regime of tests/wgrad_cases.py: the integer problem against the int64 reference with `==`, the float
problem against float64 under the derived per-element bound, U and V in NaN buffers (segments scattered over a heap), dw and dbias in
buffers whose padding must come back bit-unchanged, a NaN workspace with a guard behind it; the bit identities the code gives (a call
repeats, segments equal the contiguous launch, the sliced 1 -> 48 call equals its three slices, a one-entry table equals the immediate call,
a refused Winograd plan equals the direct plan of the same rows per workgroup) and the argument refusals.  Every case sets its plan in the
process-wide tuning table before it launches and resets it to (0, 0) afterwards.  Every measured ratio error / bound is appended to
wgrad_errors.jsonl, next to conv_errors.jsonl."""
import ctypes

import pytest
import torch

import wgrad_cases as wc

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = wc.GUARD
ARGS = ['mode', 'U', 'u_ld', 'Hu', 'Wu', 'Ca', 'V', 'v_ld', 'Hv', 'Wv', 'Cb', 'B', 'dw', 's_a', 's_b', 'flip', 'dbias', 'accumulate', 'workspace', 'workspace_bytes',
        'stream']
ARGS_SEG = ['mode', 'nseg', 'Useg', 'Vseg', 'u_ld', 'Hu', 'Wu', 'Ca', 'v_ld', 'Hv', 'Wv', 'Cb', 'Bseg', 'dw', 's_a', 's_b', 'flip', 'dbias', 'accumulate', 'workspace',
            'workspace_bytes', 'stream']


def _lib():
    from reconvat_amd import _lib
    return _lib


def _bits(t):
    return t.detach().cpu().view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def variant(case, tag, **kw):
    """the same problem (same seed, same logical tensors) with other strides, offsets, plans or options"""
    return dict(case, name=case['name'] + ' / ' + tag, regime={}, **kw)


class Planned:
    """the case's plan in the tuning table for the duration of the block; (0, 0) afterwards"""

    def __init__(self, case, tune=None):
        self.key, self.tune = wc.case_key(case), case['tune'] if tune is None else tune

    def __enter__(self):
        assert _lib().load().rv_conv_wgrad_set_plan(*self.key, *self.tune) == 0, _lib().last_error()

    def __exit__(self, *exc):
        assert _lib().load().rv_conv_wgrad_set_plan(*self.key, 0, 0) == 0


def upload(dev, pr):
    d = {k: pr[k + '_buf'].to(dev) for k in ('u', 'v', 'dw', 'db')}
    assert all(t.data_ptr() % 256 == 0 for t in d.values())          # the float offsets of wgrad_cases.py decide every alignment
    return d


def make_workspace(dev, case):
    """(inside Planned) a NaN workspace of the size the ABI names -- which is the mirror's -- at the case's offset, PAD_BITS behind it"""
    c = case
    taps = wc.TAPS[c['mode']]
    nbytes = _lib().load().rv_conv_wgrad_workspace_bytes(taps, c['B'], c['Hv'], c['Ca'], c['Cb'])
    assert nbytes == wc.case_regime(c)['workspace_bytes'] == wc.workspace_bytes(taps, c['B'], c['Hv'], c['Ca'], c['Cb'], c['tune']), c['name']
    ws = torch.full((c['ws_off'] + nbytes // 4 + GUARD,), NAN, device=dev)
    ws[c['ws_off'] + nbytes // 4:].view(torch.int32).fill_(wc.PAD_BITS)
    assert ws.data_ptr() % 256 == 0
    return ws, nbytes


def guard_intact(ws):
    return bool((_bits(ws[-GUARD:]) == wc.PAD_BITS).all().item())


def call_args(pr, d, ws, nbytes, entry=None, **kw):
    """-> (entry point, arguments, objects to keep alive) for the problem on the buffers `d`; kw replaces arguments by name"""
    c = pr['case']
    s_a, s_b, flip = pr['layout']
    nseg = kw.pop('nseg', c['nseg'])
    seg = kw.pop('seg', nseg != 1)
    a = {'mode': c['mode'] | (wc.BF16 if c['bf'] else 0), 'U': d['u'].data_ptr() + 4 * pr['u_at'][0], 'u_ld': pr['u_ld'], 'Hu': c['Hu'], 'Wu': c['Wu'], 'Ca': c['Ca'],
         'V': d['v'].data_ptr() + 4 * pr['v_at'][0], 'v_ld': pr['v_ld'], 'Hv': c['Hv'], 'Wv': c['Wv'], 'Cb': c['Cb'], 'B': c['B'], 'dw': d['dw'].data_ptr() + 4 * GUARD,
         's_a': s_a, 's_b': s_b, 'flip': flip, 'dbias': d['db'].data_ptr() + 4 * GUARD if c['bias'] else None, 'accumulate': c['acc'],
         'workspace': ws.data_ptr() + 4 * c['ws_off'], 'workspace_bytes': nbytes, 'stream': _lib().stream(), 'nseg': nseg, 'Bseg': c['B'] // max(nseg, 1) if nseg else c['B']}
    us = (ctypes.c_void_p * 4)(*[d['u'].data_ptr() + 4 * pr['u_at'][min(s, c['nseg'] - 1)] for s in range(4)])
    vs = (ctypes.c_void_p * 4)(*[d['v'].data_ptr() + 4 * pr['v_at'][min(s, c['nseg'] - 1)] for s in range(4)])
    a['Useg'], a['Vseg'] = ctypes.addressof(us), ctypes.addressof(vs)
    a.update(kw)
    names = list(ARGS_SEG if seg else ARGS)
    fn = 'rv_conv_wgrad_seg' if seg else 'rv_conv_wgrad'
    if entry is not None:
        names.remove('accumulate')
        names.insert(names.index('stream'), 'entry')
        a['entry'] = entry
        fn = 'rv_conv_wgrad_deferred_seg' if seg else 'rv_conv_wgrad_deferred'
    return fn, tuple(a[n] for n in names), (us, vs)


def collect(pr, d, ws):
    """after the launch: inputs untouched, the padding of the destinations and the guard of the workspace intact -> (G [taps, Ca, Cb], db [Cb]) on the CPU"""
    torch.cuda.synchronize()
    for k in ('u', 'v'):
        assert same_bits(d[k], pr[k + '_buf']), 'the weight gradient wrote into ' + k
    assert guard_intact(ws), 'the weight gradient wrote behind its workspace'
    dw, db = d['dw'].cpu(), d['db'].cpu()
    assert wc.padding_intact(pr, dw, db), 'the weight gradient wrote into the padding of dw or dbias'
    G, b = wc.live(pr, dw, db)
    return G.clone(), b.clone()


def run_table(dev, host, count, blocks):
    """finalize the host table, copy it to the device, run every reduction in one launch"""
    lib = _lib()
    total = lib.load().rv_wgrad_table_finalize(host.data_ptr(), count)
    assert total == sum(blocks)
    table = host.to(dev)
    lib.call('rv_wgrad_reduce_table', table.data_ptr(), count, total, lib.stream())
    torch.cuda.synchronize()
    return table


def run(dev, pr, tune=None, **kw):
    """one case through its entry point (a deferred case: a one-entry table) -> (G, db)"""
    lib = _lib()
    c = pr['case']
    d = upload(dev, pr)
    with Planned(c, tune):
        ws, nbytes = make_workspace(dev, c) if tune is None else make_workspace(dev, dict(c, tune=tune))
        if c['defer']:
            host = torch.zeros(wc.ENTRY_BYTES, dtype=torch.uint8)
            fn, args, keep = call_args(pr, d, ws, nbytes, entry=host.data_ptr(), **kw)
            blocks = lib.invoke(fn, *args)
            assert blocks == wc.case_regime(c)['reduce_blocks'], (blocks, lib.last_error())
            assert host[wc.ENTRY_EL_AT:wc.ENTRY_EL_AT + 8].view(torch.int32).tolist() == list(wc.case_regime(c)['reduce'])
            run_table(dev, host, 1, [blocks])
        else:
            fn, args, keep = call_args(pr, d, ws, nbytes, **kw)
            lib.call(fn, *args)
    return collect(pr, d, ws)


# ---------------------------------------------------------------------------------------------------------------------
# every case, both problems
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['int', 'float'])
@pytest.mark.parametrize('name', wc.RUN_CASES)
def test_wgrad_case(dev, name, kind):
    pr = wc.problem(wc.CASES[name], kind)
    G, db = run(dev, pr)
    rg, rb = wc.compare(pr, G, db)
    print(name, kind, wc.case_regime(wc.CASES[name])['kernel'], rg, rb)
    where = '%s %s' % (wc.case_regime(wc.CASES[name])['kernel'], kind)
    try:
        wc.check(where, name, 'dw', rg, log=True)
    finally:
        wc.check(where, name, 'dbias', rb, log=True)


# ---------------------------------------------------------------------------------------------------------------------
# the deferred table: seven entries of every body, two of them onto one destination, one launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['int', 'float'])
def test_wgrad_reduce_table(dev, kind):
    lib = _lib()
    names = wc.TABLE_CASES
    host = torch.zeros(len(names) * wc.ENTRY_BYTES, dtype=torch.uint8)
    held, blocks, times = {}, [], {n: names.count(n) for n in names}
    for i, n in enumerate(names):
        c = wc.CASES[n]
        pr = wc.problem(c, kind)
        if n not in held:
            held[n] = (pr, upload(dev, pr), [])
        d = held[n][1]
        with Planned(c):
            ws, nbytes = make_workspace(dev, c)                        # (one workspace per entry: they stay untouched until the table has run)
            fn, args, keep = call_args(pr, d, ws, nbytes, entry=host.data_ptr() + i * wc.ENTRY_BYTES)
            blocks.append(lib.invoke(fn, *args))
            assert blocks[-1] == wc.case_regime(c)['reduce_blocks'], (n, blocks[-1], lib.last_error())
        held[n][2].append(ws)
    run_table(dev, host, len(names), blocks)
    for n, (pr, d, wss) in held.items():
        for ws in wss[1:]:
            assert guard_intact(ws)
        G, db = collect(pr, d, wss[0])
        ref, k = wc.reference(pr), times[n]
        start = (pr['dw0'].double(), pr['db0'].double()) if pr['case']['acc'] else (0.0, 0.0)
        wantG, wantb = start[0] + k * (ref['G'] - start[0]), start[1] + k * (ref['db'] - start[1])
        zero = kind == 'int'
        rg = wc.err_ratio(G, wantG, k * ref['G_bound'] * (0 if zero else 1))
        rb = wc.err_ratio(db, wantb, k * ref['db_bound'] * (0 if zero else 1)) if pr['case']['bias'] else 0.0
        wc.check('table ' + kind, n, 'dw', rg, log=True)
        wc.check('table ' + kind, n, 'dbias', rb, log=True)
    assert lib.invoke('rv_wgrad_reduce_table', None, 3, 5, lib.stream()) != 0 and lib.invoke('rv_wgrad_reduce_table', None, 0, 5, lib.stream()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# bit identities (the float problem), each read off csrc/conv.hip
# ---------------------------------------------------------------------------------------------------------------------
REPEATS = ['mfma m0 8->16 nw8', 'mfma m2 32->24 nw8', 'wino 16->32', 'bf16 24->8 nw4', 'sw1 big', 'sw2 3 strips', 'cin1 big', 'small 1x1 1->16', 'part wgs32', 'sliced 1->48']


@pytest.mark.parametrize('name', REPEATS)
def test_immediate_call_repeats_bit_for_bit(dev, name):
    """one partial per workgroup (wave), a fixed tree in the reduction: no atomics on the immediate path"""
    pr = wc.problem(wc.CASES[name], 'float')
    a, b = run(dev, pr), run(dev, pr)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize('name', [n for n in wc.RUN_CASES if wc.CASES[n]['nseg'] > 1 and not wc.CASES[n]['defer']])
def test_segments_equal_the_contiguous_launch(dev, name):
    """the same plan (its key holds nseg * Bseg), the same rows per workgroup in the same order: only the base pointer of a row differs"""
    case = wc.CASES[name]
    a = run(dev, wc.problem(case, 'float'))
    b = run(dev, wc.problem(variant(case, 'contiguous', nseg=1), 'float'))
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


def test_one_segment_through_the_segmented_entry(dev):
    case = wc.CASES['mfma m0 16->32 nw8']
    pr = wc.problem(case, 'float')
    a, b = run(dev, pr), run(dev, pr, seg=True)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize('name', ['sliced 1->48', 'sliced 1->32 v_ld+1'])
def test_sliced_call_equals_its_slices(dev, name):
    """conv_wgrad_impl calls itself on V + c0, dw + c0 * s_b, dbias + c0 with Cb = 16, one slice after the other through the same workspace"""
    lib = _lib()
    case = wc.CASES[name]
    for kind in ('int', 'float'):
        pr = wc.problem(case, kind)
        want = run(dev, pr)
        d = upload(dev, pr)
        with Planned(case):
            ws, nbytes = make_workspace(dev, case)
            s_b = pr['layout'][1]
            for c0 in range(0, case['Cb'], 16):
                _, args, keep = call_args(pr, d, ws, nbytes)
                args = dict(zip(ARGS, args))
                args.update(V=args['V'] + 4 * c0, Cb=16, dw=args['dw'] + 4 * c0 * s_b, dbias=args['dbias'] + 4 * c0)
                lib.call('rv_conv_wgrad', *[args[n] for n in ARGS])
        got = collect(pr, d, ws)
        assert same_bits(want[0], got[0]) and same_bits(want[1], got[1]), kind


ONE_ENTRY = ['mfma m1 24->8 nw4', 'wino 8->16', 'sw1 big', 'cin1 big', 'part 256', 'chan 36->40 m1']


@pytest.mark.parametrize('name', ONE_ENTRY)
def test_one_entry_table_equals_the_immediate_call(dev, name):
    """the same partial sums through the same body (same el, same vec4) and one fp32 atomic onto a zeroed destination: 0 + s = s.  (The 1 024-element
    form of the table has no immediate twin: it meets the bound, see the deferred cases.)"""
    case = variant(wc.CASES[name], 'start from zero', acc=0, defer=False)
    twin = variant(case, 'deferred', defer=True)
    assert wc.case_regime(case)['reduce'] == wc.case_regime(twin)['reduce']
    a, b = run(dev, wc.problem(case, 'float')), run(dev, wc.problem(twin, 'float'))
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize('name,twin_tune', [('part 3x15 wgs32 nw24', (8, 32)), ('wino bf16 3x14', (8, 32))])
def test_refused_winograd_plan_equals_the_direct_plan(dev, name, twin_tune):
    """nw = 24 on an odd Hv plans in rows like nw = 8; with the bf16 bit it plans 21 row pairs, runs the direct kernel on 2 rows per workgroup -- what
    nw = 8 at wgs = 32 plans for the 42 rows.  (The 132-pixel row that does not fit the ring has no such twin: no wgs gives 8 rows in runs of 2.)"""
    case = wc.CASES[name]
    ra, rb = wc.case_regime(case), wc.case_regime(case, tune=twin_tune)
    assert (ra['kernel'], ra['rows_per_wave'], ra['nparts'], ra['nw']) == (rb['kernel'], rb['rows_per_wave'], rb['nparts'], rb['nw'])
    pr = wc.problem(case, 'float')
    a, b = run(dev, pr), run(dev, pr, tune=twin_tune)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# refusals: non-zero, a message, destinations and workspace untouched, nothing launched
# ---------------------------------------------------------------------------------------------------------------------
def _refused(d, ws, fn, args, what):
    lib = _lib()
    before = {k: _bits(t).clone() for k, t in (('dw', d['dw']), ('db', d['db']), ('ws', ws))}
    rc = lib.invoke(fn, *args)
    torch.cuda.synchronize()
    assert rc < 0, (what, rc)
    assert lib.last_error(), what
    for k, t in (('dw', d['dw']), ('db', d['db']), ('ws', ws)):
        assert torch.equal(_bits(t), before[k]), (what, k)


@pytest.mark.parametrize('name', wc.REFUSED_CASES)
def test_refused_case(dev, name):
    case = wc.CASES[name]
    pr = wc.problem(case, 'float')
    d = upload(dev, pr)
    with Planned(case):
        nbytes = max(_lib().load().rv_conv_wgrad_workspace_bytes(wc.TAPS[case['mode']], case['B'], case['Hv'], case['Ca'], case['Cb']), 64)
        ws = torch.full((nbytes // 4 + GUARD,), NAN, device=dev)
        host = torch.zeros(wc.ENTRY_BYTES, dtype=torch.uint8)
        fn, args, keep = call_args(pr, d, ws, nbytes, entry=host.data_ptr() if case['defer'] else None)
        _refused(d, ws, fn, args, name)


def test_wgrad_refusals(dev):
    lib = _lib()
    for nw, wgs in ((3, 0), (8, 31), (8, 4097)):
        assert lib.load().rv_conv_wgrad_set_plan(9, 2, 6, 16, 32, nw, wgs) != 0
    host = torch.zeros(wc.ENTRY_BYTES, dtype=torch.uint8)
    for name, tries in (
            ('mfma m0 16->32 nw8', (('mode 3', {'mode': 3}), ('mode -1', {'mode': -1}), ('workspace one float short', {'workspace_bytes': -4}),
                                    ('mode 0 with Hu = Hv + 1', {'Hu': 7}), ('mode 0 with Wu = Wv - 1', {'Wu': 4}), ('mode 2 on the same grid', {'mode': 2}),
                                    ('u_ld = Ca + 2', {'u_ld': 18}), ('v_ld = Cb + 1', {'v_ld': 33}), ('U 4 bytes off', {'U': 4}), ('V 8 bytes off', {'V': 8}),
                                    ('Ca = 14', {'Ca': 14}), ('Cb = 30', {'Cb': 30}), ('u_ld below Ca', {'u_ld': 12}),
                                    ('nseg 0', {'seg': True, 'nseg': 0}), ('nseg 5', {'seg': True, 'nseg': 5}), ('null entry', {'entry': 0}),
                                    ('null entry, segmented', {'entry': 0, 'seg': True}), ('deferred nseg 5', {'entry': host.data_ptr(), 'seg': True, 'nseg': 5}))),
            ('seg3x1 m1 24->8', (('a segment 4 bytes off', {'Vseg': 'off'}),)),
            ('mfma m2 8->16 nw4', (('mode 2 with Hu = 2 Hv + 2', {'Hu': 14}), ('mode 2 with Wu = 2 Wv - 1', {'Wu': 9}))),
            ('sw1 big', (('two segments of a small-channel layer', {'seg': True, 'nseg': 2, 'Bseg': 1}), ('mode 1 for 8 -> 1', {'mode': 1}))),
            ('sliced 1->48', (('two segments of the sliced layer', {'seg': True, 'nseg': 2, 'Bseg': 1}), ('the sliced layer deferred', {'entry': host.data_ptr()})))):
        case = wc.CASES[name]
        pr = wc.problem(case, 'float')
        d = upload(dev, pr)
        with Planned(case):
            ws, nbytes = make_workspace(dev, case)
            for what, kw in tries:
                kw = dict(kw)
                entry = kw.pop('entry', None)
                if kw.get('workspace_bytes') == -4:
                    kw['workspace_bytes'] = nbytes - 4
                _, ok, keep = call_args(pr, d, ws, nbytes)
                for k in ('U', 'V'):
                    if isinstance(kw.get(k), int):
                        kw[k] = dict(zip(ARGS, ok))[k] + kw[k]
                if kw.get('Vseg') == 'off':
                    bad = (ctypes.c_void_p * 4)(*[d['v'].data_ptr() + 4 * pr['v_at'][min(s, case['nseg'] - 1)] + (4 if s == 1 else 0) for s in range(4)])
                    kw['Vseg'] = ctypes.addressof(bad)
                if entry == 0:
                    fn, args, keep = call_args(pr, d, ws, nbytes, entry=host.data_ptr(), **kw)
                    args = tuple(None if (i == len(args) - 2) else v for i, v in enumerate(args))
                else:
                    fn, args, keep = call_args(pr, d, ws, nbytes, entry=entry, **kw)
                _refused(d, ws, fn, args, what)
            # ... and the same buffers still serve the accepted call
            if not case['defer']:
                fn, args, keep = call_args(pr, d, ws, nbytes)
                lib.call(fn, *args)
        rg, rb = wc.compare(pr, *collect(pr, d, ws))
        wc.check('after refusals', name, 'dw', rg)
        wc.check('after refusals', name, 'dbias', rb)
