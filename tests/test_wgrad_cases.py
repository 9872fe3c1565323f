"""CPU checks of tests/wgrad_cases.py: every case sits in the launch regime it is labelled with, the cases together reach every regime and
every template instantiation of the weight-gradient kernels of csrc/conv.hip within 40 keys of the tuning table, the mirror's workspace
sizes and table prefixes equal the built library's, the reference equals torch's autograd for the five layer kinds, the integer problem is
exact in float32 (Winograd transforms included), torch's float32 weight gradient alone meets the derived bounds the GPU test applies (no
case is born failing), a single dropped term misses them by 10x on some case of every kernel and mode, and emulated kernel faults are caught
by the comparison the GPU test uses."""
import numpy as np
import pytest
import torch

import wgrad_cases as wc

ALL = list(wc.CASES)
RUN = wc.RUN_CASES


@pytest.mark.parametrize('name', ALL)
def test_case_reaches_its_regime(name):
    case = wc.CASES[name]
    reg = wc.case_regime(case)
    if case['refusal']:
        assert reg == {'refused': case['refusal']}
        return
    assert case['regime'], 'a case without a label'
    assert reg['refused'] is None, reg
    for k, v in case['regime'].items():
        assert reg[k] == v, (k, reg[k], v)


def test_case_table_covers_the_regimes():
    regs = {n: wc.case_regime(wc.CASES[n]) for n in RUN}
    R = list(regs.values())
    C = [wc.CASES[n] for n in RUN]

    def sel(**kv):
        return [(c, r) for c, r in zip(C, R) if all(r.get(k) == v for k, v in kv.items())]
    forms = {r['form'] for r in R}
    tiles = [(1, 1), (1, 2), (2, 1), (2, 2)]
    # every template instantiation
    assert {f for f in forms if f[0] == 'mfma'} == {('mfma', m, ta, tb, nw) for m in (0, 1, 2) for ta, tb in tiles for nw in (4, 8)}
    assert {f for f in forms if f[0] == 'wino'} == {('wino', ta, tb) for ta, tb in tiles}
    assert {f for f in forms if f[0] == 'mfma_bf'} == {('mfma_bf', 0, ta, tb, nw) for ta, tb in tiles for nw in (4, 8)}
    assert {f for f in forms if f[0] == 'small'} == {('small', m, a, b) for m, a, b in wc.RV_WS}
    assert {f[0] for f in forms} == {'mfma', 'wino', 'mfma_bf', 'small', 'sw1', 'sw2', 'cin1'}
    for kern, form in (('sw1', ('small', 0, 8, 1)), ('sw2', ('small', 0, 8, 2)), ('cin1', ('small', 0, 1, 16))):
        assert sel(kernel=kern) and any(r['fallback'] for _, r in sel(form=form)), kern                 # each strip kernel also in its flat fallback
    assert {r['fallback'] for r in R} == {None, 'u', 'u_ld', 'v', 'v_ld', 'tiny'}
    assert {r['reduce'] for c, r in zip(C, R) if not c['defer']} == set(wc.REDUCE_IMM)
    assert {r['reduce'] for c, r in zip(C, R) if c['defer']} == set(wc.REDUCE_TAB)
    assert {regs[n]['reduce'] for n in wc.TABLE_CASES} == set(wc.REDUCE_TAB) and len(wc.TABLE_CASES) >= 5 and len(set(wc.TABLE_CASES)) < len(wc.TABLE_CASES)
    for el in (64, 16):
        assert {r['el_why'] for r in R if r['el'] == el} == {'nel', 'parts'}, el
    assert {(r['reduce_unrolled'], r['reduce_tail']) for r in R if not r['vec4']} >= {(True, True), (False, True), (True, False)}
    assert {(r['reduce_unrolled'], r['reduce_tail']) for r in R if r['vec4']} >= {(True, True), (False, True)}
    assert any(r['vec4'] == 0 and r['el'] >= 16 and not r['small'] for r in R), 'a misaligned workspace behind an MFMA kernel'
    # channel groups
    m = [(c, r) for c, r in zip(C, R) if not r['small']]
    assert {c['Ca'] for c, _ in m} >= {8, 16, 24, 32, 48, 20, 36} and {c['Cb'] for c, _ in m} >= {8, 16, 24, 32, 48, 12, 40}
    assert any(r['tie'] for _, r in m) and any(r['padded_a'] and r['nga'] > 1 for _, r in m) and any(r['padded_b'] and r['ngb'] > 1 for _, r in m)
    assert any(r['nga'] * r['ngb'] == 9 for _, r in m) and all(a != b for a, b in wc.TILE_OF)       # a transposed index shows
    # the partition, for the direct and the Winograd kernel
    for kern in ('mfma', 'wino'):
        k = [r for _, r in sel(kernel=kern)]
        flags = set().union(*[r['parts'] for r in k])
        assert flags >= {'mid_image', 'cross_image', 'cross_segment', 'ragged_last', 'prefetch'}, (kern, flags)
        assert max(r['images_spanned'] for r in k) >= 3 and any(r['want'] > r['nparts'] for r in k) and any(r['rows_per_wave'] > 1 for r in k), kern
    assert any('one_part' in r['parts'] for _, r in sel(kernel='mfma'))
    assert {256, 260} <= {r['nparts'] for _, r in sel(kernel='mfma')} and {c['tune'][1] for c, _ in m} >= {0, 32, 4096}
    assert any(c['Hv'] == 1 and r['images_spanned'] == 3 for c, r in m) and any(c['Hv'] == 2 and r['images_spanned'] == 3 for c, r in m)
    # widths
    d = sel(kernel='mfma')
    assert {c['Wv'] for c, _ in d} >= {1, 3, 4, 5, 37} and any(r['ksteps_unequal'] for _, r in d) and {r['last_kstep_partial'] for _, r in d} == {True, False}
    b = sel(kernel='mfma_bf')
    assert any(c['Wv'] > 16 * r['NXG'] for c, r in b) and {r['NXG'] for _, r in b} == {4, 8}
    # mode 2: the down and up geometries
    assert {(c['Hu'] - 2 * c['Hv'], c['Wu'] - 2 * c['Wv']) for c, r in d if r['mode'] == 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # Winograd
    w = sel(kernel='wino')
    assert {c['Hv'] for c, _ in w} >= {2, 4, 6} and {r['odd_width'] for _, r in w} == {True, False}
    assert {r['u_pieces'] for _, r in w} >= {1, 2, 3} and {r['v_pieces'] for _, r in w} >= {1, 3}
    assert any(c['tune'][0] == 24 and c['Hv'] % 2 and not r['wino_planned'] for c, r in d)
    assert {r['wino_refused'] for r in R} == {None, 'lds', 'bf16'}
    lds = sel(wino_refused='lds')[0][1]
    assert lds['kernel'] == 'mfma' and lds['nparts'] * lds['pstride'] * 4 <= lds['workspace_bytes'] and lds['lds'] <= wc.LDS_MAX
    # the generic staging loop of wgrad_wino_k (more than MAXP * NW pieces per row) cannot be reached: such a row does not fit the LDS
    for ta, tb in tiles:
        for wv in range(1, 700):
            s = wc.wino_sizes(ta, tb, wv)
            assert not (s['generic_loop'] and s['lds'] <= wc.LDS_MAX), (ta, tb, wv)
    # the strip kernels
    for kern in ('sw1', 'sw2', 'cin1'):
        k = [r for _, r in sel(kernel=kern)]
        assert k, kern
    s = [r for r in R if r['kernel'] in ('sw1', 'sw2', 'cin1')]
    assert any(r['last_strip_cols'] == 1 and r['nstrip'] > 1 for r in s) and any(1 < r['last_strip_cols'] < 16 for r in s)
    assert any(r['last_band_rows'] == 1 and r['nband'] > 1 for r in s) and any(r['h_short'] for r in s) and any(r['rows_doubled'] for r in s)
    assert any(r['nparts'] % 4 for r in s) and {r['sliced'] for r in R} == {0, 2, 3}
    for kern in ('sw2', 'cin1'):
        assert any(r['rows_doubled'] for _, r in sel(kernel=kern)), kern
    f = [r for r in R if r['kernel'] == 'small']
    assert any(r['empty_partials'] for r in f) and any(r['idle_waves'] for r in f) and {r['uvec'] for r in f} == {True, False} and {r['vvec'] for r in f} == {True, False}
    # operands and destinations on every kernel
    for kern in ('mfma', 'wino', 'mfma_bf'):
        cs = [c for c, _ in sel(kernel=kern)]
        assert any(c['u_pad'] == 4 for c in cs) and any(c['v_pad'] == 8 for c in cs) and any(not c['bias'] for c in cs) and any(c['acc'] for c in cs), kern
        assert {c['layout'] for c in cs} == set(wc.LAYOUTS) and any(c['nseg'] > 1 for c in cs) and any(c['defer'] for c in cs), kern
    for kern in ('small', 'sw1', 'sw2', 'cin1'):
        cs = [c for c, _ in sel(kernel=kern)]
        assert any(c['acc'] for c in cs) and any(not c['bias'] for c in cs), kern
    sg = [(c, r) for c, r in zip(C, R) if c['nseg'] > 1]
    assert {c['nseg'] for c, _ in sg} == {2, 3, 4} and {c['B'] // c['nseg'] for c, _ in sg} == {1, 2} and {r['kernel'] for _, r in sg} == {'mfma', 'wino', 'mfma_bf'}
    assert any(c['defer'] for c, _ in sg)
    # the older operator test at its default plan: one row per workgroup, no ring reuse, no image boundary inside a part -- which is why this table exists
    r0 = wc.regime(0, 2, 24, 57, 32, 24, 57, 32)
    assert r0['kernel'] == 'mfma' and r0['rows_per_wave'] == 1 and not r0['parts'] & {'prefetch', 'cross_image', 'ragged_last'}


def test_the_cases_use_at_most_40_plan_keys():
    """rv_conv_wgrad_set_plan's table holds 256 keys for the whole process and is never emptied"""
    keys = {wc.case_key(wc.CASES[n]) for n in RUN}
    assert len(keys) <= 40, len(keys)


def test_mirror_by_hand():
    """values worked out from csrc/conv.hip by hand, so that an edit of the mirror itself shows"""
    p = wc.plan(9, 8, 114, 48, 48)
    assert (p['TA'], p['TB'], p['nga'], p['ngb'], p['want'], p['rows_per_wave'], p['nparts']) == (1, 1, 3, 3, 28, 33, 28)
    p = wc.plan(9, 2, 6, 24, 8)
    assert (p['TA'], p['TB'], p['tie']) == (2, 1, True)
    p = wc.plan(9, 3, 14, 8, 16, (24, 32))
    assert (p['wino'], p['units'], p['rows_per_wave'], p['nparts'], p['nw']) == (True, 21, 1, 21, 8)
    assert wc.plan(9, 3, 15, 8, 16, (24, 32))['wino'] is False and wc.plan(4, 2, 6, 8, 16, (24, 0))['wino'] is False
    assert wc.plan(1, 2, 17, 1, 16)['small'] and not wc.plan(1, 2, 6, 8, 16)['small'] and wc.plan(9, 1, 5000, 8, 1)['nparts'] == 4096
    assert wc.sliced(9, 1, 48) and wc.sliced(9, 1, 32) and not wc.sliced(9, 1, 16) and not wc.sliced(9, 1, 24) and not wc.sliced(1, 1, 48)
    assert wc.workspace_bytes(9, 1, 33, 1, 48) == 33 * 160 * 4
    s = wc.wino_sizes(2, 2, 132)
    assert (s['WT4'], s['UPp'], s['VPp'], s['lds']) == (68, 144, 136, 180224)
    s = wc.direct_sizes(0, 2, 2, 8, 132, False)
    assert (s['Wv4'], s['UP'], s['lds'], s['NH'], s['NXG']) == (132, 134, 102400, 2, 4)
    s = wc.direct_sizes(2, 1, 1, 4, 5, False)
    assert (s['Wv4'], s['UP'], s['NXG'], s['ksteps']) == (8, 16, 4, [1, 1, 0, 0])
    r = wc.reduce_regime(1168, 256, 1168, 0, False)
    assert (r['el'], r['vec4'], r['reduce_unrolled'], r['reduce_tail']) == (4, 0, True, False)
    r = wc.reduce_regime(13000, 12, 13000, 0, True)
    assert (r['el'], r['vec4'], r['reduce_blocks']) == (1024, 1, 13)
    assert wc.reduce_regime(13000, 12, 13000, 1, True)['reduce'] == (16, 0)
    assert wc.table_prefix([3, 1, 5]) == ([0, 3, 4], 9) and [wc.table_lookup([0, 3, 4], b) for b in range(9)] == [0, 0, 0, 1, 2, 2, 2, 2, 2]
    assert wc.regime(0, 1, 4, 5, 8, 4, 4, 16) == {'refused': 'geometry'} and wc.regime(2, 1, 10, 8, 8, 4, 4, 16) == {'refused': 'geometry'}
    assert wc.regime(3, 1, 4, 4, 8, 4, 4, 16) == {'refused': 'mode'}


def test_mirror_against_the_built_library():
    """rv_conv_wgrad_workspace_bytes under every plan the cases set, rv_wgrad_table_entry_bytes and rv_wgrad_table_finalize: none needs a device"""
    from reconvat_amd import _lib
    lib = _lib.load()
    for n in RUN:
        c = wc.CASES[n]
        key, taps = wc.case_key(c), wc.TAPS[c['mode']]
        try:
            assert lib.rv_conv_wgrad_set_plan(*key, *c['tune']) == 0
            assert lib.rv_conv_wgrad_workspace_bytes(taps, c['B'], c['Hv'], c['Ca'], c['Cb']) == wc.workspace_bytes(taps, c['B'], c['Hv'], c['Ca'], c['Cb'], c['tune']), n
            assert wc.case_regime(c)['workspace_bytes'] == wc.workspace_bytes(taps, c['B'], c['Hv'], c['Ca'], c['Cb'], c['tune']), n
        finally:
            assert lib.rv_conv_wgrad_set_plan(*key, 0, 0) == 0
        assert lib.rv_conv_wgrad_workspace_bytes(taps, c['B'], c['Hv'], c['Ca'], c['Cb']) == wc.workspace_bytes(taps, c['B'], c['Hv'], c['Ca'], c['Cb']), n
    for nw, wgs in ((3, 0), (16, 0), (8, 31), (8, 4097), (-4, 0)):
        assert lib.rv_conv_wgrad_set_plan(9, 2, 6, 8, 16, nw, wgs) != 0
    assert lib.rv_wgrad_table_entry_bytes() == wc.ENTRY_BYTES
    counts = [wc.case_regime(wc.CASES[n])['reduce_blocks'] for n in wc.TABLE_CASES]
    tab = np.zeros(len(counts) * wc.ENTRY_BYTES, dtype=np.uint8)
    blk = tab[wc.ENTRY_BLOCK0_AT:].view(np.int64)[::wc.ENTRY_BYTES // 8]
    blk[:] = counts
    prefix, total = wc.table_prefix(counts)
    assert lib.rv_wgrad_table_finalize(tab.ctypes.data, len(counts)) == total
    assert list(blk) == prefix and not tab.view(np.int64).reshape(-1, wc.ENTRY_BYTES // 8)[:, :wc.ENTRY_BLOCK0_AT // 8].any()
    # every workgroup of the table finds its entry, the first and the last block of each included
    for i, (p0, n) in enumerate(zip(prefix, counts)):
        assert wc.table_lookup(prefix, p0) == i and wc.table_lookup(prefix, p0 + n - 1) == i


def _scatter(G, s_a, s_b, flip, size):
    taps, Ca, Cb = G.shape
    t_, a_, b_ = torch.arange(taps).view(-1, 1, 1), torch.arange(Ca).view(1, -1, 1), torch.arange(Cb).view(1, 1, -1)
    out = torch.zeros(size, dtype=G.dtype)
    out[(a_ * s_a + b_ * s_b + ((taps - 1 - t_) if flip else t_)).reshape(-1)] = G.reshape(-1)
    return out


@pytest.mark.parametrize('kind', ['c3', 't3', 'c1', 'down', 'up'])
def test_reference_against_torch_autograd(kind):
    """the five layer kinds with the (mode, U, V, s_a, s_b, flip) ops._wgrad_geom passes (the function itself, on the CPU tensors)"""
    from reconvat_amd import ops
    g = torch.Generator().manual_seed(5)
    B, H, W, cin, cout = 2, 5, 7, 3, 4
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    mk = {'c3': lambda: torch.nn.Conv2d(cin, cout, 3, padding=1), 't3': lambda: torch.nn.ConvTranspose2d(cin, cout, 3, padding=1),
          'c1': lambda: torch.nn.Conv2d(cin, cout, 1), 'down': lambda: torch.nn.Conv2d(cin, cout, 2, stride=2),
          'up': lambda: torch.nn.ConvTranspose2d(cin, cout, 2, stride=2, output_padding=(1, 0))}[kind]
    layer = mk().double()
    y = layer(x)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    xn, dyn = x.permute(0, 2, 3, 1).contiguous(), dy.permute(0, 2, 3, 1).contiguous()
    p = ops._wgrad_geom(kind, xn, dyn)
    mode, Uu, Vv, s_a, s_b, flip = p.mode, p.u, p.v, p.s_a, p.s_b, p.flip
    assert p.taps == wc.TAPS[mode] and (Uu is dyn and Vv is xn if kind == 'up' else Uu is xn and Vv is dyn)
    assert (p.bb, p.hu, p.wu, p.ca, p.uld) == (*Uu.shape, Uu.shape[3]) and (p.bb, p.hv, p.wv, p.cb, p.vld) == (*Vv.shape, Vv.shape[3])
    G, db, N = wc.wgrad_ref(mode, Uu, Vv)
    got = _scatter(G, s_a, s_b, flip, layer.weight.numel())
    assert torch.allclose(got, layer.weight.grad.reshape(-1), rtol=1e-12, atol=1e-12)
    if kind != 'up':
        assert torch.allclose(db, layer.bias.grad, rtol=1e-12, atol=1e-12)
        Gt, dbt = wc.torch_wgrad(mode, Uu, Vv)
        assert torch.allclose(G, Gt, rtol=1e-12, atol=1e-12) and torch.allclose(db, dbt, rtol=1e-12, atol=1e-12)
    assert int(N.max()) == Vv.shape[0] * Vv.shape[1] * Vv.shape[2] and (mode != 0 or int(N[0]) == B * (H - 1) * (W - 1))
    if mode == 0:                                                    # the Winograd identity in float64
        Hh = H - 1
        assert torch.allclose(wc.wino_wgrad(Uu[:, :Hh], Vv[:, :Hh]), wc.wgrad_ref(0, Uu[:, :Hh], Vv[:, :Hh])[0], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('name', RUN)
def test_integer_problem_is_exact_in_float32(name):
    """the float32 emulation along the mirror's partition (the Winograd regime: through the kernel's transforms) equals the int64 reference, every
    intermediate below 2^24; the same emulation of the float problem meets the bound"""
    case = wc.CASES[name]
    pr = wc.problem(case, 'int')
    G, db = wc.emulate(pr)
    assert wc.compare(pr, G, db) == (0.0, 0.0)
    ref = wc.reference(pr)
    big = wc.wgrad_ref(case['mode'], pr['Uu'].double().abs(), pr['Vv'].double().abs())[0].max().item()
    if wc.case_regime(case)['kernel'] == 'wino':
        big = wc.wino_wgrad(pr['Uu'].double(), pr['Vv'].double(), absolute=True).max().item()
    assert big + 3 < 2 ** 24 and ref['G'].abs().max().item() < 2 ** 24
    pf = wc.problem(case, 'float')
    rg, rb = wc.compare(pf, *wc.emulate(pf))
    assert rg <= 1.0 and rb <= 1.0, (rg, rb)


@pytest.mark.parametrize('name', RUN)
def test_torch_float32_meets_the_bound(name):
    case = wc.CASES[name]
    pr = wc.problem(case, 'float')
    Uu, Vv = pr['Uu'], pr['Vv']
    if wc.case_regime(case)['kernel'] == 'mfma_bf':
        Uu, Vv = wc.bf16_round(Uu), wc.bf16_round(Vv)
    G, _ = wc.torch_wgrad(case['mode'], Uu, Vv)
    db = pr['Vv'].reshape(-1, case['Cb']).sum(0)
    if case['acc']:
        G, db = G + pr['dw0'], db + pr['db0']
    rg, rb = wc.compare(pr, G, db)
    assert rg <= 1.0 and rb <= 1.0, (rg, rb)


def test_a_dropped_term_misses_the_bound_by_10x_somewhere_on_every_kernel_and_mode():
    best = {}
    for n in RUN:
        c = wc.CASES[n]
        r = wc.case_regime(c)
        k = (r['kernel'], r['mode'])
        if c['B'] * c['Hv'] * c['Wv'] <= 700:
            best[k] = max(best.get(k, 0.0), wc.dropped_term_margin(wc.problem(c, 'float')))
    want = {('mfma', 0), ('mfma', 1), ('mfma', 2), ('wino', 0), ('mfma_bf', 0), ('small', 0), ('small', 1), ('sw1', 0), ('sw2', 0), ('cin1', 0)}
    assert set(best) >= want
    for k in want:
        assert best[k] >= 10.0, (k, best[k])


@pytest.mark.parametrize('fault', wc.FAULTS)
def test_emulated_faults_are_caught(fault):
    """every case the fault applies to fails the integer comparison; at least one also fails the float bound"""
    hit, float_hit = 0, 0
    for n in RUN:
        c = wc.CASES[n]
        if c['B'] * c['Hv'] * c['Wv'] > 1200 or not wc.fault_applies(wc.problem(c, 'int'), fault):
            continue
        pr = wc.problem(c, 'int')
        assert max(wc.compare(pr, *wc.emulate(pr, fault))) > 1.0, n
        pf = wc.problem(c, 'float')
        float_hit += max(wc.compare(pf, *wc.emulate(pf, fault))) > 1.0
        hit += 1
    assert hit >= 1 and float_hit >= 1, (fault, hit, float_hit)
