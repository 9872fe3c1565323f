"""CPU checks of tests/band_cases.py: every case sits in the launch regime it is labelled with, the cases together reach every value of every
key of the mirror and every instance of conv3x3_lds_k the host can launch, every tile the search can select has an instance, torch's float32
CPU convolution alone meets the bound the GPU test applies, and emulated faults of the kernel -- each of them one line of conv3x3_lds_k
reverted or gone wrong -- miss the bound, or the `==`, on every case they apply to."""
import pytest
import torch

import band_cases as bc
import conv_cases as cc

ALL = list(bc.CASES)
RUN = bc.RUN_CASES
BAND = bc.BAND_CASES


@pytest.mark.parametrize('name', ALL)
def test_case_reaches_its_regime(name):
    case = bc.CASES[name]
    reg = cc.case_regime(case)
    if case['refusal']:
        assert reg == {'refused': case['refusal']}
        return
    assert case['regime'], 'a case without a label'
    assert reg['refused'] is None, reg
    for k, v in case['regime'].items():
        assert reg[k] == v, (k, reg[k], v)


def test_case_table_covers_the_regimes():
    regs = {n: cc.case_regime(bc.CASES[n]) for n in BAND}
    R = list(regs.values())

    def values(key, **kv):
        return {r[key] for r in R if all(r[k] == v for k, v in kv.items())}

    def cases(**kv):
        return [bc.CASES[n] for n in BAND if all(regs[n][k] == v for k, v in kv.items())]
    # every instance the host can launch at R = 4, the shipped ones and more at R = 2, bf16 at every NW
    for nw in (4, 8, 12, 16):
        assert {(nt, mt) for r, w, nt, mt, bf in values('form') if (r, w, bf) == (4, nw, False)} == set(bc.REACHABLE[nw]), nw
        r2 = {(nt, mt) for r, w, nt, mt, bf in values('form') if (r, w) == (2, nw)}
        assert r2 >= {(nt, mt) for w, nt, mt in bc.R2_SHIPPED if w == nw} and len(r2) >= 2 and r2 <= set(bc.REACHABLE[nw]), nw
        assert any(bf for r, w, nt, mt, bf in values('form') if w == nw), nw
    assert sum(len(v) for v in bc.REACHABLE.values()) == 55 and set(bc.RV_L3[16]) - set(bc.REACHABLE[16]) == {(2, 8), (3, 4), (4, 4)}
    # the launch
    assert values('th_from') == {'force_th', 'H', 'slots'} and values('wgs_per_cu') == {1, 2} and values('forced') == {True, False}
    assert values('nsplit') >= {1, 2, 4} and values('xcd') == {True, False} and values('nchunk', R=2) == {1, 3} and values('nchunk', R=4) == {1, 2, 3}
    assert values('short_last_run') == {True, False} and values('run_crosses_image') == {True, False}
    persistent = [r for r in R if r['bands_per_wg'] >= 3 and r['run_crosses_image'] and r['short_last_run'] and r['xcd']]
    assert {r['weights'] for r in persistent} == {'once', 'per_unit'} and {r['stats'] for r in persistent} == {None, 'fwd', 'bn_z'} and any(r['bf'] for r in persistent)
    assert any(r['nchunk'] == 3 for r in persistent)
    # staging
    for r_ in (2, 4):
        assert values('row_tail', R=r_) == {True, False} and values('weights', R=r_) == {'once', 'per_unit'}, r_
        assert {bc.CASES[n]['W'] for n in BAND if regs[n]['R'] == r_} >= {1, 7, 15, 16, 17, 33}
    assert values('PPI') == {16, 32} and values('w_half_instr') == {True, False}
    assert values('overflow_loop', NW=4) == {True, False} and values('idle_stagers', NW=16) == {True, False} and values('planned_only') == {True, False}
    assert any(r['planned_only'] and not r['idle_stagers'] for r in R) and len(values('TW')) >= 4
    # bands and tiles
    assert values('short_last_band') == {True, False} and 1 in values('last_band_rows', short_last_band=True) and values('one_band_image') == {True, False}
    assert values('H1') == {True, False} and values('partial_tile') == {True, False} and values('tile_spans_rows') == {True, False}
    assert any(r['idle_tile_slots'] == 0 for r in R) and any(r['idle_tile_slots'] > 0 for r in R) and all(r['idle_tile_slots'] >= 0 for r in R)
    assert any(r['idle_waves'] == 0 for r in R) and any(r['idle_waves'] > 0 for r in R)
    assert any(r['ntile'][0] != r['ntile'][1] for r in R)
    # epilogue
    assert set().union(*[r['stores'] for r in R]) == {'vec', 'tail', 'scalar', 'skip'}
    assert set().union(*[r['z_load'] for r in R if r['z_load']]) == {'vec', 'scalar_ld', 'scalar_tail'}
    assert values('stats') == {None, 'fwd', 'bn_z'} and any(r['replicas'] == set(range(8)) for r in R) and any(r['replicas'] == {0} for r in R)
    for nw in (4, 8, 12, 16):
        assert values('stats', NW=nw) == {None, 'fwd', 'bn_z'}, nw
        exact = [n for n in BAND if regs[n]['NW'] == nw and regs[n]['stats'] == 'fwd'
                 and cc.stats_reference(cc.problem(bc.CASES[n], 'int'), cc.reference(cc.problem(bc.CASES[n], 'int'))['out'])[1].max().item() < 2 ** 24]
        assert exact, nw
    multi = [regs[n] for n in BAND if regs[n]['bands_per_wg'] > 1 and regs[n]['run_crosses_image']]
    assert {r['stats'] for r in multi} == {None, 'fwd', 'bn_z'} and any(r['z_load'] == {'vec', 'scalar_tail'} for r in multi) and any(r['z_load'] == {'scalar_ld'} for r in multi)
    assert {c['z_pad'] for c in cases(stats='bn_z')} >= {0, 4}
    # destinations and inputs, per R
    for r_ in (2, 4):
        cs = cases(R=r_)
        assert any(c['acc'] for c in cs) and any(not c['bias'] for c in cs) and {c['out_pad'] for c in cs} >= {0, 1, 4} and any(c['in_pad'] == 4 * r_ for c in cs), r_
        assert {c['cout'] for c in cs} >= {6, 18, 24}, r_
    assert any(c['in_pad'] == 2 for c in cases(R=2)) and any(c['in_off'] == 2 for c in cases(R=2)), 'a 16-byte DMA from an 8-byte-aligned pixel'
    for nw in (4, 8, 12, 16):
        assert any(r['bands_per_wg'] > 1 and r['run_crosses_image'] for r in R if r['NW'] == nw), nw
    assert {cc.case_pack_args(bc.CASES[n])[5] for n in BAND} == {0, 1}, 'flipped packs: the input gradient'
    # an accumulating case whose workgroups run several bands with a partial tile each and a short last band: a store past the band's pixels would be added twice
    assert any(bc.CASES[n]['acc'] and regs[n]['partial_tile'] and regs[n]['short_last_band'] and regs[n]['bands_per_wg'] > 1 for n in BAND)
    # bf16: per NW, two chunks, ignored at R = 2
    assert values('bf', R=2) == {False} and any(bc.CASES[n]['algo'] & bc.BF16_BIT for n in BAND if regs[n]['R'] == 2)
    assert {r['nchunk'] for r in R if r['bf']} >= {1, 2}
    # the default
    d = [regs[n] for n in bc.DEFAULT_CASES]
    assert len({(r['tile'], r['TH'], r['wgs_per_cu']) for r in d}) >= 4 and {bc.CASES[n]['algo'] & 3 for n in bc.DEFAULT_CASES} == {0, 2}
    assert any(r['score'] == 0 for r in d) and any(r['score'] > 0 for r in d)
    fell = [cc.case_regime(bc.CASES[n]) for n in RUN if n not in BAND]
    assert len(fell) == 1 and fell[0]['kernel'] == 'mfma' and fell[0]['fell_through'] and bc.CASES[[n for n in RUN if n not in BAND][0]]['W'] > 512
    # refusals
    assert {bc.CASES[n]['refusal'].split(': ')[1] for n in bc.REFUSED_CASES} == {'ntile_n % NT', 'nothing fits', 'accumulator budget', 'force_th', 'lds',
                                                                                 'row wider than the tile slots'}
    # the older operator tests: B = 3 at 6 x 10 and smaller, dense, one band per image and workgroup -- which is why this table exists
    r0 = cc.conv_regime(0, 3, 6, 10, 16, 6, 10, 32, algo=0x212)
    assert r0['bands_per_wg'] == 1 and r0['one_band_image'] and not r0['xcd'] and r0['stores'] == {'vec'}


def test_every_selectable_tile_has_an_instance():
    """a tile the search selects without an RV_L3 instance would be a silent fall-through to the direct kernel (default) or a refusal nobody asked for
    (forced): every candidate that passes the budget has one, whatever W and H make of the scores ..."""
    for nw in (4, 8, 12, 16):
        for nt in (1, 2, 3, 4):
            for mt in bc.MTS[nw]:
                assert not bc.budget_ok(nw, nt, mt) or (nt, mt) in bc.RV_L3[nw], (nw, nt, mt)
    # ... and the search itself, over ntile_n 1 .. 8, W 1 .. 600 and H on both sides of every cap
    for ntile_n in range(1, 9):
        for W in range(1, 601):
            for H, B, R, nchunk in ((1, 1, 4, 1), (3, 2, 2, 3), (9, 8, 4, 2), (40, 1, 4, 6), (640, 8, 2, 1)):
                best, _ = bc.search(R, 4, ntile_n, nchunk, B, H, W)
                if best is None:
                    assert W > 512 or bc.lds_bytes(R, 1, 1, W, nchunk) > bc.LDS_CAP, (ntile_n, W, H)
                else:
                    assert (best['NT'], best['MTW']) in bc.RV_L3[4] and best['lds'] <= bc.LDS_CAP and 1 <= best['TH'] <= H


def test_mirror_by_hand():
    """values worked out from csrc/conv.hip and conv_band.h by hand, so that an edit of the mirror itself shows"""
    assert bc.lds_bytes(4, 1, 1, 7, 1) == (2 * 3 * 9 * 16 + 2304) * 4 == 12672 and bc.lds_bytes(4, 1, 17, 57, 2) == 161920 > bc.LDS_CAP
    assert [bc.xcd_remap(b, 8) for b in range(8)] == list(range(8)) and [bc.xcd_remap(b, 9) for b in range(9)] == [0, 2, 3, 4, 5, 6, 7, 8, 1]
    assert sorted(bc.xcd_remap(b, 176) for b in range(176)) == list(range(176))
    r = bc.band_regime(2, 65, 7, 16, 64, algo=0x1311)                 # 130 bands, four n-splits on 256 slots: 64 workgroups -> runs of 3 -> 44 of them
    assert (r['NW'], r['tile'], r['TH'], r['lds_bytes'], r['wgs_per_cu'], r['nbands'], r['total_bands'], r['nsplit'], r['bands_per_wg'], r['grid']) == \
        (8, (1, 1), 1, 12672, 1, 65, 130, 4, 3, 176)
    assert r['runs'][21] == (63, 66) and r['runs'][-1] == (129, 130) and r['run_crosses_image'] and r['short_last_run'] and r['xcd']
    assert (r['PPI'], r['ipr'], r['nx'], r['NWF'], r['TW'], r['ntile'], r['idle_tile_slots'], r['idle_waves'], r['K']) == (16, 1, 3, 9, 2, (1, 1), 7, 7, 144)
    r = bc.band_regime(2, 65, 7, 16, 16)                              # the default: (1, 8) 0, (1, 4) 0, (1, 2) 1 x 116, (1, 1) 3 x 100
    assert (r['tile'], r['TH'], r['th_from'], r['wgs_per_cu'], r['score'], r['grid'], r['bands_per_wg']) == ((1, 1), 9, 'slots', 2, 300, 16, 1)
    r = bc.band_regime(2, 3, 33, 8, 16, algo=0x312)                   # R = 2: 32 pixels and two fragments per DMA instruction, 9 fragments: the fifth is half masked
    assert (r['PPI'], r['ipr'], r['row_tail'], r['NWF'], r['TW'], r['w_half_instr'], r['TH'], r['nx']) == (32, 2, True, 5, 1, True, 3, 10)
    assert bc.band_regime(1, 17, 57, 32, 64, algo=0x318) == {'refused': 'forced tile: lds'}
    assert bc.band_regime(1, 17, 57, 32, 64, algo=0x348) == {'refused': 'forced tile: accumulator budget'}
    assert bc.band_regime(1, 1, 513, 8, 16)['kernel'] == 'mfma' and bc.band_regime(1, 1, 512, 8, 16)['tile'] == (1, 8)
    assert bc.band_regime(2, 5, 7, 8, 16, algo=0x311 | bc.BF16_BIT)['bf'] is False and bc.band_regime(2, 5, 7, 16, 16, algo=0x311 | bc.BF16_BIT)['bf'] is True
    assert bc.band_regime(2, 5, 7, 8, 16, in_ld=9) == {'refused': 'in alignment'} and bc.band_regime(2, 5, 7, 8, 16, in_ld=10)['R'] == 2
    assert bc.forced(12, 3, 3, 3, bf=1) == 0x103733 and bc.forced(8, 1, 1, 1) == 0x1311


# ---------------------------------------------------------------------------------------------------------------------
# per-case checks, group by group (the first word of a case's name)
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = {}
for _n in BAND:
    GROUPS.setdefault(' '.join(_n.split()[:2]) if _n.startswith('R') else _n.split()[0], []).append(_n)


@pytest.mark.parametrize('group', list(GROUPS))
def test_integer_problem_is_exact_in_float32(group):
    for name in GROUPS[group]:
        pr = cc.problem(bc.CASES[name], 'int')
        assert cc.reference(pr)['mag'].max().item() < 2 ** 24, name   # the sum of the magnitudes bounds every partial sum, in any order
        assert torch.equal(cc.bf16_round(pr['x']), pr['x']) and torch.equal(cc.bf16_round(pr['Wm']), pr['Wm'])
        assert cc.compare(pr, bc.emulate(pr)) == 0.0, name


@pytest.mark.parametrize('group', list(GROUPS))
def test_float32_reference_meets_the_bound(group):
    """torch's float32 CPU convolution (of the bf16-rounded operands under bit 20), and the taps added one by one in float32, under the comparison of the GPU test"""
    for name in GROUPS[group]:
        c = bc.CASES[name]
        pr = cc.problem(c, 'float')
        x, Wm = bc.operands(pr)
        out = cc.torch_conv(0, x, Wm, pr['bias'], c['H'], c['W'], c['cout'])
        if c['acc']:
            out = out + pr['out0']
        cc.check('cpu-f32 torch', name, 'out', cc.compare(pr, out))
        cc.check('cpu-f32 taps', name, 'out', cc.compare(pr, bc.emulate(pr)))
        if c['stats']:
            for kind in ('int', 'float'):
                p = cc.problem(c, kind)
                o = bc.emulate(p)
                cc.check('cpu-f32 replicas', name, 'stats', cc.stats_ratio(p, o, bc.replica_sums(p, o)))


def test_bf16_rounding_is_seen():
    """the float32 result of the unrounded operands misses the bf16 reference: a kernel that ignored bit 20 (or a reference that did) would show"""
    for name in BAND:
        c = bc.CASES[name]
        if cc.case_regime(c)['bf']:
            pr = cc.problem(c, 'float')
            out = cc.torch_conv(0, pr['x'], pr['Wm'], pr['bias'], c['H'], c['W'], c['cout']) + (pr['out0'] if c['acc'] else 0)
            # two roundings of up to 2^-9 on each of K random-sign terms of magnitude ~0.56 move an element by some 0.002 sqrt(K), the bound is
            # 1.01 (2K + 3) 2^-24 x 0.56 K: the ratio falls like K^-1.5, from some 14 on a typical element at K = 144 to 3 at K = 432
            assert cc.compare(pr, out) > 3, name


# faults that leave the prefill, or a start value of magnitude >= 0.5 out, move EVERY affected element; the others change a sum by a random-sign sum of
# terms, small on single elements: there at least half of the affected elements move by >= 100 bounds (halo_neighbour: NaN on the outer rows, which counts)
_EVERY = ('partial_tile', 'no_accumulate')


@pytest.mark.parametrize('fault', bc.FAULTS)
def test_emulated_faults_are_caught(fault):
    hit = 0
    for name in BAND:
        c = bc.CASES[name]
        prf = cc.problem(c, 'float')
        region = bc.fault_region(prf, fault)
        if region is None:
            continue
        hit += 1
        ref = cc.reference(prf)
        r = cc.ratio_map(bc.emulate(prf, fault), ref['out'], ref['bound'])
        assert r[~region].max().item() <= 1.0 if (~region).any() else True, (name, fault)
        moved = r[region]
        if fault in _EVERY and not (fault == 'partial_tile' and c['acc']):
            # a value of magnitude >= 0.5 (or the NaN prefill) against a bound of at most 1.01 (2K + 3) U (K + 2), K <= 432
            assert moved.min().item() >= 20, (name, fault, moved.min().item())
        else:
            assert moved.max().item() >= 100 and (moved.median().item() >= 100 or moved.numel() < 8), (name, fault, moved.median().item())
        pri = cc.problem(c, 'int')
        assert cc.compare(pri, bc.emulate(pri, fault)) > 1.0, (name, fault, 'int')
    assert hit >= (3 if fault == 'second_weight_buffer' else 7), (fault, hit)


def test_a_dropped_workgroup_of_statistics_is_caught():
    hit = 0
    for name in BAND:
        c = bc.CASES[name]
        if not c['stats']:
            continue
        reg = cc.case_regime(c)
        for kind in ('int', 'float'):
            pr = cc.problem(c, kind)
            out = bc.emulate(pr)
            for drop in {0, reg['grid'] // 2, reg['grid'] - 1}:
                assert cc.stats_ratio(pr, out, bc.replica_sums(pr, out, drop=drop)) >= 100, (name, kind, drop)
            ws = bc.replica_sums(pr, out)
            ws[-1] = 0.0                                             # a write behind the workspace
            assert cc.stats_ratio(pr, out, ws) == float('inf')
        hit += 1
    assert hit >= 20
