"""CPU checks of tests/conv_cases.py: every case sits in the launch regime it is labelled with, the cases together reach every regime
and every template instantiation of the direct and small-channel kernels of csrc/conv.hip, the mirror's packed sizes equal the built
library's and its packing round-trips, the reference equals torch's convolutions for the pack arguments of every layer kind, torch's
float32 CPU convolution alone meets the derived bound the GPU test applies (no case is born failing), and emulated kernel faults are
caught by the comparison the GPU test uses."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc

ALL = list(cc.CASES)
RUN = cc.RUN_CASES


def _in_regime(launch, regime):
    for k, v in regime.items():
        assert launch[k] == v, (k, launch[k], v, launch)


@pytest.mark.parametrize('name', ALL)
def test_case_reaches_its_regime(name):
    case = cc.CASES[name]
    reg = cc.case_regime(case)
    if case['refusal']:
        assert reg == {'refused': case['refusal']}
        return
    assert case['regime'], 'a case without a label'
    assert reg['refused'] is None, reg
    _in_regime(reg, case['regime'])


def test_case_table_covers_the_regimes():
    regs = {n: cc.case_regime(cc.CASES[n]) for n in RUN}
    R = list(regs.values())

    def have(**kv):
        return any(all(r.get(k) == v for k, v in kv.items()) for r in R)

    def values(key, **kv):
        out = []
        for r in R:
            if key in r and all(r.get(k) == v for k, v in kv.items()) and r[key] not in out:
                out.append(r[key])
        return out
    assert set(values('kernel')) == {'mfma', 'mfma_ks4', 'narrow', 'cin12', 'small_k'}
    # every instantiation: RV_CASE for both fragment widths of every mode, RV_CASEK, RV_NARROW, the three conv_cin12_k forms, RV_SMALL
    forms = values('form', kernel='mfma')
    for mode in range(4):
        assert {(nt, mt) for m, _, nt, mt in forms if m == mode} == set(cc.RV_CASE), mode
        assert {r for m, r, _, _ in forms if m == mode} == {2, 4}, mode
        for r_ in (2, 4):
            assert {mt for m, r, _, mt in forms if (m, r) == (mode, r_)} == {1, 2, 4} and len({nt for m, r, nt, _ in forms if (m, r) == (mode, r_)}) >= 2
    formsk = values('form', kernel='mfma_ks4')
    for mode in (1, 2, 3):
        assert {(nt, mt) for m, _, nt, mt in formsk if m == mode} == set(cc.RV_CASEK), mode
    assert set(values('form', kernel='narrow')) == set(cc.RV_NARROW)
    assert set(values('form', kernel='cin12')) == set(cc.RV_CIN12)
    assert set(values('form', kernel='small_k')) == {(ci, co, 3, 3) for ci, co in cc.RV_SMALL[0]} | {(ci, co, 1, 1) for ci, co in cc.RV_SMALL[1]}
    # the fallbacks behind the fast small-channel kernels, each reason, each instantiation behind them
    assert set(values('fallback')) == {None, 'in_ld', 'in', 'bias', 'bn_z', 'bn_coef'}
    for ci, co in cc.RV_NARROW + cc.RV_CIN12:
        assert any(r.get('form') == (ci, co, 3, 3) and r['fallback'] for r in R), (ci, co)
    # the direct kernel
    m = [r for r in R if r['kernel'] == 'mfma']
    for mode in range(4):
        mm = [r for r in m if r['form'][0] == mode]
        assert {r['npix'] for r in mm} >= {1, 558} and any(r['npix'] in cc.UPS.values() for r in mm), mode
        assert {r['xcd'] for r in mm} == {True, False} and {r['idle_waves'] for r in mm} >= {1, 2, 3}, mode
        assert any(r['partial_tile'] for r in mm) and any(r['idle_tiles'] > 0 for r in mm)
        assert any(r['forced'] for r in mm) and sum(r['degenerate'] and not r['forced'] for r in mm) >= 2, mode
        want = {'vec', 'scalar'} if mode == 3 else {'vec', 'scalar', 'tail', 'skip'}
        assert set().union(*[r['stores'] for r in mm]) == want, mode
    assert any(not r['forced'] and not r['degenerate'] and cc.cdiv(r['ntiles'], 1) * r['ntile_n'] >= 2048 for r in m), 'a default where the score decides'
    assert {(r['pad_row'], r['pad_col']) for r in m if r['form'][0] == 3} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(not r['partial_tile'] and r['idle_waves'] == 0 and r['idle_tiles'] == 0 for r in m), 'a grid of whole tiles and whole workgroups'
    assert {r['stats'] for r in m} == {None, 'bn_stats', 'bn_bwd_stats'}
    # the split-K form
    k = [r for r in R if r['kernel'] == 'mfma_ks4']
    assert {r['nsteps'] for r in k} >= {4, 5, 8} and {r['ragged'] for r in k} == {True, False} and {r['mid_tap'] for r in k} == {True, False}
    assert {tuple(r['deal']) for r in k} == {(0,), (0, 1), (0, 1, 2, 3)} and {r['npix'] for r in k} >= {70, 558}
    assert any(cc.CASES[n]['acc'] for n in RUN if regs[n]['kernel'] == 'mfma_ks4') and any(cc.CASES[n]['out_pad'] for n in RUN if regs[n]['kernel'] == 'mfma_ks4')
    # strips and bands
    for kern in ('narrow', 'cin12'):
        s = [r for r in R if r['kernel'] == kern]
        for form in {r['form'] for r in s}:
            f = [r for r in s if r['form'] == form]
            assert any(r['nstrip'] > 1 and r['last_strip_cols'] == 1 for r in f) and any(r['nband'] > 1 and r['last_band_rows'] == 1 for r in f), form
            assert {r['h_short'] for r in f} == {True, False}, form
        assert {r['store'] for r in s} == ({'scalar'} if kern == 'narrow' else {'vec', 'scalar'})
    c12 = [r for r in R if r['kernel'] == 'cin12']
    for form in cc.RV_CIN12:
        f = [r for r in c12 if r['form'] == form]
        assert {r['stats_kind'] for r in f} == {None, 'fwd', 'bn_z'} and {r['z_past_band'] for r in f if r['stats_kind'] == 'bn_z'} == {True, False}, form
        assert {r['last_band_rows'] for r in f if r['h_short']} == {1, 2, 4}, form
    z = [cc.CASES[n] for n in RUN if regs[n]['kernel'] == 'cin12' and cc.CASES[n]['stats'] == 'z']
    assert {c['z_pad'] for c in z} == {0, 4} and all(c['slope'] == 0.01 for c in z)
    # conv_small_k
    s = [r for r in R if r['kernel'] == 'small_k']
    assert set().union(*[r['store'] for r in s]) == {'transpose', 'vec', 'scalar'}
    tr = [r for r in s if r['TPP'] == 1 and r['CPT'] % 4 == 0]
    for form in {r['form'] for r in tr}:
        f = [frozenset(r['store']) for r in tr if r['form'] == form]
        assert {frozenset({'transpose', 'vec'}), frozenset({'vec'}), frozenset({'scalar'})} <= set(f), form
    assert any(r['store'] == {'transpose'} and not r['ragged_wave'] for r in tr)
    assert {r['fold'] for r in s} == {None, 'shuffle', 'lds'} and {r['WREG'] for r in s} == {True, False} and {r['TPP'] for r in s} == {1, 4}
    assert {r['cap'] for r in s if r['passes'] == 2} == {1024, 4096} and {r['passes'] for r in s} == {1, 2}
    assert {r['stats'] for r in s} >= {None, 'fused', 'bn_bwd_stats'}
    # destinations: accumulate, no bias, padded strides on every kernel
    for kern in ('mfma', 'mfma_ks4', 'narrow', 'cin12', 'small_k'):
        cs = [cc.CASES[n] for n in RUN if regs[n]['kernel'] == kern]
        assert any(c['acc'] for c in cs) and any(not c['bias'] for c in cs) and any(c['out_pad'] for c in cs) and any(not c['acc'] and c['bias'] for c in cs), kern
        assert any(c['in_pad'] for c in cs) or kern == 'mfma_ks4', kern
    # the largest shape the older operator test runs (B = 2 at 9 x 21) stays below nine workgroups, on dense 16-byte stores -- which is why this table exists
    r0 = cc.conv_regime(1, 2, 9, 21, 16, 9, 21, 32)
    assert r0['tile'] == (1, 1) and r0['grid'] == (6, 2) and not r0['xcd'] and r0['stores'] == {'vec'}
    r0 = cc.conv_regime(1, 2, 5, 7, 16, 5, 7, 32)
    assert r0['degenerate'] and r0['tile'] == (2, 4) and r0['grid'] == (1, 1)


def test_mirror_by_hand():
    """values worked out from csrc/conv.hip by hand, so that an edit of the mirror itself shows"""
    assert cc.frag_R(32) == 4 and cc.frag_R(24) == 2 and cc.frag_R(2) == 0 and cc.frag_R(48) == 4
    assert cc.packed_weight_floats(9, 16, 32) == 25 * 1 * 2 * 256 and cc.packed_weight_floats(4, 24, 16) == 4 * 3 * 1 * 128
    assert cc.packed_weight_floats(9, 1, 16) == 144 and cc.packed_weight_floats(1, 16, 18) == 512
    assert cc.small_cpt(1, 16, 9) == 16 and cc.small_cpt(1, 16, 1) == 4 and cc.small_cpt(16, 1, 9) == 1 and cc.small_cpt(8, 2, 9) == 2
    assert cc.choose_tiles(5, 3)[:2] == (3, 4) and cc.choose_tiles(5, 3)[2] == 0          # every score 0: the first candidate
    assert cc.choose_tiles(260, 12)[:2] == (2, 1)                                         # 5016 against 5016 of (1, 2): the earlier candidate
    assert cc.choose_tiles(100000, 4)[:2] == (4, 4)
    r = cc.conv_regime(3, 2, 5, 7, 16, 11, 15, 16, algo=0x111)
    assert (r['P'], r['npix'], r['ntile_n'], r['grid'], r['idle_waves']) == ((6, 8), 96, 4, (2, 4), 2)
    r = cc.conv_regime(1, 2, 9, 31, 80, 9, 31, 64, algo=0x521)
    assert (r['nsteps'], r['slices'], r['grid'], r['f'], r['K']) == (5, [(0, 1), (1, 2), (2, 3), (3, 5)], (35, 2), 4, 80)
    r = cc.conv_regime(0, 1, 513, 513, 1, 513, 513, 16, bias_off=1, stats='sums')
    assert (r['nblk_wanted'], r['nblk'], r['second_pass_wgs'], r['fallback']) == (1029, 1024, 5, 'bias')
    assert cc.conv_regime(0, 2, 17, 65, 1, 17, 65, 16, in_ld=2)['kernel'] == 'cin12'      # no alignment is asked of a one-channel input
    assert cc.conv_regime(1, 1, 4, 4, 8, 4, 4, 1) == {'refused': 'no small kernel'}
    assert cc.conv_regime(1, 1, 4, 4, 16, 4, 4, 16, in_off=1) == {'refused': 'in alignment'}
    assert cc.conv_regime(3, 1, 4, 4, 16, 8, 8, 24) == {'refused': 'scatter Cout'}
    assert cc.conv_regime(2, 1, 5, 5, 16, 3, 3, 16) == {'refused': 'size'} and cc.conv_regime(3, 1, 4, 4, 16, 10, 8, 16) == {'refused': 'size'}


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def built():
    from reconvat_amd import build
    return ctypes.CDLL(build.build())


def _pack_shapes():
    shapes = {cc.case_pack_args(cc.CASES[n])[:3] for n in RUN} | {(e[1], e[2], e[3]) for e in cc.PACK_TABLE}
    return sorted(shapes)


def test_packed_weight_floats_equals_the_library(built):
    fn = built.rv_packed_weight_floats
    fn.restype = ctypes.c_long
    for taps, kdim, ndim in _pack_shapes():
        assert fn(taps, kdim, ndim) == cc.packed_weight_floats(taps, kdim, ndim), (taps, kdim, ndim)


def test_pack_table_layout_equals_the_library(built):
    """rv_pack_table_fill is host arithmetic on host memory: made-up (never dereferenced) pointers, the running workgroup count back"""
    I, L, P = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    built.rv_pack_table_entry_bytes.restype = L
    built.rv_pack_table_fill.restype = L
    built.rv_pack_table_fill.argtypes = [P, I, P, P, I, I, I, L, L, I, I, I]
    host = torch.zeros(len(cc.PACK_TABLE) * built.rv_pack_table_entry_bytes(), dtype=torch.uint8)
    total = 0
    for i in range(len(cc.PACK_TABLE)):
        _, args = cc.pack_entry(i)
        total += cc.cdiv(cc.pack_floats(args), 256)
        assert built.rv_pack_table_fill(host.data_ptr(), i, 4096, 4096, *args) == total, cc.PACK_TABLE[i][0]
    assert built.rv_pack_table_fill(host.data_ptr(), 0, 4096, 4096, 1, 1, 16, 1, 1, 0, 4, 0) == -1     # the plain layout has no scatter form


def test_pack_table_has_every_entry_kind():
    kinds = [(cc.frag_R(k) if not plain else 0, cc.wino_packed(t, k) and not sc, bool(fl), bool(sc), n % 16 != 0) for _, t, k, n, _, fl, sc, plain in cc.PACK_TABLE]
    assert any(r == 4 and w for r, w, _, _, _ in kinds) and any(r == 2 for r, _, _, _, _ in kinds) and any(r == 0 for r, _, _, _, _ in kinds)
    assert any(f for _, _, f, _, _ in kinds) and any(s for _, _, _, s, _ in kinds) and any(r and o for r, _, _, _, o in kinds)
    assert {e[4] for e in cc.PACK_TABLE} == {'kn', 'nk'}


@pytest.mark.parametrize('i', range(len(cc.PACK_TABLE)))
def test_pack_mirror_round_trips(i):
    for kind in ('int', 'float'):
        w, args = cc.pack_entry(i, kind)
        packed = cc.pack_mirror(w, *args)
        assert packed.numel() == cc.pack_floats(args)
        taps, kdim, ndim, *_ = args
        assert torch.equal(cc.unpack_mirror(packed, taps, kdim, ndim, args[7]), cc.logical_weights(w, *args[:7]))
    if cc.wino_packed(args[0], args[1]) and not args[6]:             # the Winograd section: A^T (U . d) A with d = e_centre gives back the centre tap ...
        w, args = cc.pack_entry(i, 'int')
        taps, kdim, ndim = args[:3]
        n_tap = cc.packed_weight_floats(taps, kdim, ndim) * 9 // 25
        Uw = cc.unpack_mirror(cc.pack_mirror(w, *args)[n_tap:], 16, kdim, ndim, 0).view(4, 4, kdim, ndim).double()
        g = cc.logical_weights(w, *args[:7]).view(3, 3, kdim, ndim).double()
        # ... and its four corners are the four corner taps, its (1, 1) element the sum of all nine over 4
        assert torch.equal(Uw[0, 0], g[0, 0]) and torch.equal(Uw[0, 3], g[0, 2]) and torch.equal(Uw[3, 0], g[2, 0]) and torch.equal(Uw[3, 3], g[2, 2])
        assert torch.equal(Uw[1, 1], g.sum((0, 1)) / 4)
        assert torch.equal(Uw, Uw.float().double()), 'multiples of 4: the transform is exact in float32'


# ---------------------------------------------------------------------------------------------------------------------
# the reference against torch, for the pack arguments ops._pack_make passes
# ---------------------------------------------------------------------------------------------------------------------
_FWD_MODE = {'c3': 0, 't3': 0, 'c1': 1, 'down': 2, 'up': 3}          # reconvat_amd/ops.py
_DGRAD_MODE = {'c3': 0, 't3': 0, 'c1': 1, 'down': 3, 'up': 2}


@pytest.mark.parametrize('kind', list(_FWD_MODE))
def test_reference_equals_torch_for_every_layer_kind(kind):
    g = cc._gen(99, len(kind), ord(kind[0]))
    cin, cout, B = 3, 5, 2
    for H, W, up in ((5, 7, (1, 1)), (4, 6, (0, 1)), (1, 1, (1, 0))):
        if kind == 'down':
            H, W = 2 * H + up[0], 2 * W + up[1]                      # odd sizes: the last row / column is never read
        x = cc._draw(g, 'float', B, cin, H, W).double().requires_grad_()
        b = cc._draw(g, 'float', cout).double()
        k = {'c3': 3, 't3': 3, 'c1': 1, 'down': 2, 'up': 2}[kind]
        w = cc._draw(g, 'float', *((cin, cout, k, k) if kind in ('t3', 'up') else (cout, cin, k, k))).double()
        if kind in ('c3', 'c1'):
            y = F.conv2d(x, w, b, padding=k // 2)
        elif kind == 't3':
            y = F.conv_transpose2d(x, w, b, padding=1)
        elif kind == 'down':
            y = F.conv2d(x, w, b, stride=2)
        else:
            y = F.conv_transpose2d(x, w, b, stride=2, output_padding=up)
        dy = cc._draw(g, 'float', *y.shape).double()
        dx, = torch.autograd.grad(y, x, dy)
        Ho, Wo = y.shape[2:]
        a = cc.pack_args_of(kind, 'fwd', cin, cout)
        got = cc.conv_ref(_FWD_MODE[kind], x.detach().permute(0, 2, 3, 1), cc.logical_weights(w.reshape(-1), *a[:7]), b, Ho, Wo, cout)
        assert (got - y.detach().permute(0, 2, 3, 1)).abs().max().item() < 1e-12, (kind, 'fwd')
        assert cc.out_size(_FWD_MODE[kind], H, W, up) == (Ho, Wo)
        a = cc.pack_args_of(kind, 'dgrad', cin, cout)
        got = cc.conv_ref(_DGRAD_MODE[kind], dy.permute(0, 2, 3, 1), cc.logical_weights(w.reshape(-1), *a[:7]), None, H, W, cin)
        assert (got - dx.permute(0, 2, 3, 1)).abs().max().item() < 1e-12, (kind, 'dgrad')
        # ... and torch_conv, the float32 stand-in of the checks below, is the same function of (mode, Wm)
        for mode, inp, ww, oh, ow, co in ((_FWD_MODE[kind], x.detach(), cc.pack_args_of(kind, 'fwd', cin, cout), Ho, Wo, cout),
                                          (_DGRAD_MODE[kind], dy, cc.pack_args_of(kind, 'dgrad', cin, cout), H, W, cin)):
            Wm = cc.logical_weights(w.reshape(-1), *ww[:7])
            xn = inp.permute(0, 2, 3, 1)
            assert (cc.torch_conv(mode, xn, Wm, None, oh, ow, co) - cc.conv_ref(mode, xn, Wm, None, oh, ow, co)).abs().max().item() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# per-case checks, group by group (the first two words of a case's name); the two 513 x 513 cases form a group of their own
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = {}
for _n in RUN:
    GROUPS.setdefault(' '.join(_n.split()[:2]), []).append(_n)


@pytest.mark.parametrize('group', list(GROUPS))
def test_integer_problem_is_exact_in_float32(group):
    for name in GROUPS[group]:
        pr = cc.problem(cc.CASES[name], 'int')
        for t in (pr['x'], pr['w_buf'], pr['bias'], pr['out0']):
            assert t is None or bool(((t.abs() >= 1) & (t.abs() <= 3) & (t == t.round())).all().item())
        ref = cc.reference(pr)
        assert ref['mag'].max().item() < 2 ** 24, name               # the sum of the magnitudes bounds every partial sum, in any order
        assert cc.compare(pr, cc.emulate(pr)) == 0.0, name


@pytest.mark.parametrize('group', list(GROUPS))
def test_float32_reference_meets_the_bound(group):
    """torch's float32 CPU convolution, and the taps added one by one in float32, under the comparison of the GPU test"""
    for name in GROUPS[group]:
        c = cc.CASES[name]
        pr = cc.problem(c, 'float')
        out = cc.torch_conv(c['mode'], pr['x'], pr['Wm'], pr['bias'], c['Ho'], c['Wo'], c['cout'])
        if c['acc']:
            out = out + pr['out0']
        cc.check('cpu-f32 torch', name, 'out', cc.compare(pr, out))
        cc.check('cpu-f32 taps', name, 'out', cc.compare(pr, cc.emulate(pr)))
        if c['stats']:                                               # float32 column sums of the float32 result meet the statistics tolerance
            y = out.reshape(-1, c['cout'])
            want, terms = cc.stats_reference(pr, out)
            if c['stats'] == 'sums':
                got = torch.stack([y.sum(0), (y * y).sum(0)]).double()
                cc.check('cpu-f32 sums', name, 'stats', cc.err_ratio(got, want, cc.TOL_COLSUM * terms))


FAULTS = ('clamp_tap', 'last_strip', 'last_band', 'pad_row', 'no_accumulate', 'drop_slice', 'quad_shift')
# faults that replace a value by the prefill, or leave a start value of magnitude >= 0.5 out, move EVERY affected element by >= 100 bounds; the others
# change a sum by a random-sign sum of terms, which can be small on single elements: there at least half of the affected elements move by >= 100 bounds
_EVERY = ('pad_row', 'no_accumulate', 'quad_shift')


@pytest.mark.parametrize('fault', FAULTS)
def test_emulated_faults_are_caught(fault):
    hit = 0
    for name in RUN:
        if name in cc.GRID_STRIDE_CASES and fault != 'quad_shift':
            continue
        c = cc.CASES[name]
        prf = cc.problem(c, 'float')
        region = cc.fault_region(prf, fault)
        if region is None:
            continue
        if fault in ('last_strip', 'last_band') and c['acc']:
            every = False                                            # the start value stays: the element moves by the conv's own value
        else:
            every = fault in _EVERY or fault in ('last_strip', 'last_band')
        hit += 1
        ref = cc.reference(prf)
        r = cc.ratio_map(cc.emulate(prf, fault), ref['out'], ref['bound'])
        assert r[~region].max().item() <= 1.0 if (~region).any() else True, (name, fault)
        moved = r[region]
        if every:
            # a value of magnitude >= 0.5 (or a NaN) against a bound of at most 1.01 (K + 3) U (K + 2): a hundredfold up to K = 285, and by
            # what that expression leaves for the two longer chains of the table (48 -> 1: K = 432, 44-fold; 3x3 64 channels: K = 576, 25-fold)
            K = cc.case_regime(c)['K']
            floor = 100 if K <= 285 else 0.5 / (1.01 * (K + 3) * (K + 2) * cc.U)
            assert moved.min().item() >= floor, (name, fault, moved.min().item())
        else:
            assert moved.max().item() >= 100 and (moved.median().item() >= 100 or moved.numel() < 8), (name, fault, moved.median().item())
        pri = cc.problem(c, 'int')
        assert cc.compare(pri, cc.emulate(pri, fault)) > 1.0, (name, fault, 'int')
    assert hit >= 2 or fault == 'quad_shift' and hit == 1, (fault, hit)


def test_a_dropped_statistics_replica_is_caught():
    hit = 0
    for name in RUN:
        c = cc.CASES[name]
        if c['stats'] != 'sums' or cc.case_regime(c)['kernel'] != 'cin12':
            continue
        for kind in ('int', 'float'):
            pr = cc.problem(c, kind)
            out = cc.emulate(pr)
            assert cc.stats_ratio(pr, out, cc.replica_sums(pr, out)) <= 1.0, (name, kind)
            assert cc.stats_ratio(pr, out, cc.replica_sums(pr, out, drop=0)) >= 100, (name, kind)
            ws = cc.replica_sums(pr, out)
            ws[-1] = 0.0                                             # a write behind the workspace
            assert cc.stats_ratio(pr, out, ws) == float('inf')
        hit += 1
    assert hit >= 6
